"""GPU: the hybrid association probabilities (the partial mode of kbest_cluster.hip, kbest_clustered_partial_batch_f64_dev,
kbest_hybrid_probs_batch_f64, the hybridProb shim) against the numpy restatement of tests/hybrid_check.py -- exact clusters by
subset sums, open clusters by the pinned CPU oracle's assignmentProb on the sub-block -- never against the kernel's own output.
Columns of answered clusters: the bits of clustered_probs (where it answers the frame) and 1e-12 absolute against the restatement;
columns of open clusters: 1e-9 absolute against the restatement, the project's tolerance for weights against the oracle;
sub-blocks, row lists and descriptors: equal, bit for bit."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import cluster_check as cc
import hybrid_check as hc
import probabilisticsemslam_amd as pk
from probabilisticsemslam_amd import workloads as wl
from test_gpu_permanent import bits, dense_frame

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    e = pk.KBestEngine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def restated(F, nL, nM, side, k, max_exact, condition=True):
    """Raw scene frames and the restatement of every frame: (frames, [(probs, method, opens, info, maxCluster, label)]).
    Computed once; nobody changes it."""
    frames = wl.scene_frames(F, nL, nM, side)
    return frames, [hc.hybrid_probs(f, nL, nM, k, condition=condition, max_exact=max_exact) for f in frames]


def open_columns(want, nM):
    mask = np.zeros(nM, bool)
    for o in want[2]:
        mask[o["cols"]] = True
    return mask


def check_against_restatement(eng, shape, k, max_exact):
    """hybrid_probs on the raw scene frames of `shape` against the restatement; returns (out, method, want)."""
    F, nL, nM, _ = shape
    frames, want = restated(*shape, k, max_exact)
    out, method, nOpen, maxc = eng.hybrid_probs(frames, [nL] * F, [nM] * F, k, condition=True, max_exact=max_exact)
    plain, _, info, _ = eng.clustered_probs(frames, [nL] * F, [nM] * F, condition=True)
    worst_open = worst_ans = worst_sum = 0.0
    for b, w in enumerate(want):
        assert method[b] == w[1] and nOpen[b] == len(w[2]) and maxc[b] == w[4], (b, method[b], w[1], nOpen[b], len(w[2]))
        op = open_columns(w, nM)
        if not w[2]:
            assert method[b] == 0 and info[b] > 0 and np.array_equal(bits(out[b]), bits(plain[b])), b
        if info[b] > 0:  # the plain entry answers the frame: the answered clusters' columns are its bits
            assert np.array_equal(bits(out[b][~op]), bits(plain[b][~op])), b
        worst_ans = max(worst_ans, np.abs(out[b][~op] - w[0][~op]).max() if (~op).any() else 0.0)
        worst_open = max(worst_open, np.abs(out[b][op] - w[0][op]).max() if op.any() else 0.0)
        worst_sum = max(worst_sum, np.abs(out[b].sum(axis=1) - 1.0).max())
    print(f"{shape} max_exact {max_exact} k {k}: methods {method.tolist()}, open {nOpen.tolist()}; answered columns vs restatement "
          f"{worst_ans:.3g}, open columns vs restatement {worst_open:.3g} (1e-12 expected), columns - 1 {worst_sum:.3g}")
    assert worst_ans <= 1e-12 and worst_open <= 1e-9 and worst_sum <= 1e-12
    return out, method, plain, want


# ---- 1. a lowered cap: open clusters whose truth is known ---------------------------------------------------------------------
def test_lowered_cap_against_restatement_and_truth(eng):
    out, method, plain, want = check_against_restatement(eng, (24, 20, 10, 12), 1000, 4)
    assert sum(1 for w in want if w[2]) == 20
    complete = [b for b, w in enumerate(want) if w[1] == 1]
    assert len(complete) >= 4  # (the restatement itself: a condition of the test)
    worst = max(np.abs(out[b] - plain[b]).max() for b in complete)
    print(f"complete enumerations {complete}: vs clustered_probs {worst:.3g}")
    assert worst <= 1e-9


# ---- 2. what the partial kernel hands out ----------------------------------------------------------------------------------------
def partial_run(eng, frames, max_exact, condition, maxRawRow=None, maxCol=None):
    """The device entry on a stream of the caller's, every output pre-filled with a sentinel.  frames: [(block, nL, nM)]."""
    import torch
    blocks, nLs, nMs = [f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames]
    B = len(frames)
    sizes = np.array([(l + m) * m for l, m in zip(nLs, nMs)], np.int64)
    psizes = np.array([m * (l + 1) for l, m in zip(nLs, nMs)], np.int64)
    coff = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    poff = np.concatenate([[0], np.cumsum(psizes)[:-1]]).astype(np.int64)
    maxRawRow = max(l + m for l, m in zip(nLs, nMs)) if maxRawRow is None else maxRawRow
    maxCol = max(nMs) if maxCol is None else maxCol
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_cost, d_coff, d_poff = t(np.concatenate(blocks)), t(coff), t(poff)
    d_nL, d_nM = t(np.asarray(nLs, np.int32)), t(np.asarray(nMs, np.int32))
    d_probs = torch.full((int(psizes.sum()),), -5.0, dtype=torch.float64, device=dev)
    d_sub = torch.full((int(sizes.sum()),), -7.0, dtype=torch.float64, device=dev)
    d_lp = torch.full((B,), -5.0, dtype=torch.float64, device=dev)
    ints = lambda *shape: torch.full(shape, -77, dtype=torch.int32, device=dev)  # noqa: E731
    d_info, d_maxc, d_nopen, d_lab = ints(B), ints(B), ints(B), ints(B, maxCol)
    d_desc, d_rows = ints(B, maxCol, 4), ints(B, maxRawRow)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    eng.clustered_partial_dev(B, maxRawRow, maxCol, d_nL, d_nM, d_cost, d_coff, d_probs, d_poff, d_nopen, d_desc, maxCol, d_rows,
                              maxRawRow, d_sub, max_exact=max_exact, d_logPerm=d_lp, d_info=d_info, d_maxCluster=d_maxc,
                              d_label=d_lab, labelStride=maxCol, condition=condition, stream=s.cuda_stream)
    s.synchronize()
    hp, hs = d_probs.cpu().numpy(), d_sub.cpu().numpy()
    return dict(probs=[hp[poff[b]: poff[b] + psizes[b]].reshape(nMs[b], nLs[b] + 1) for b in range(B)],
                sub=[hs[coff[b]: coff[b] + sizes[b]] for b in range(B)], logPerm=d_lp.cpu().numpy(), info=d_info.cpu().numpy(),
                maxc=d_maxc.cpu().numpy(), nOpen=d_nopen.cpu().numpy(), label=d_lab.cpu().numpy(), desc=d_desc.cpu().numpy(),
                rows=d_rows.cpu().numpy())


def check_handed_out(got, b, want, nM):
    """Frame b of a partial_run against its restatement: descriptors, row lists and sub-blocks bit for bit, nothing else written."""
    opens = want[2]
    assert got["nOpen"][b] == len(opens) and got["info"][b] == want[3] and got["maxc"][b] == want[4], b
    np.testing.assert_array_equal(got["label"][b][:nM], want[5], err_msg=str(b))
    sub_at = row_at = 0
    for j, o in enumerate(opens):
        assert got["desc"][b, j].tolist() == [o["root"], o["m"], o["nL"], o["R"]], (b, j)
        n = o["block"].size
        assert np.array_equal(bits(got["sub"][b][sub_at: sub_at + n]), bits(o["block"])), (b, j)
        np.testing.assert_array_equal(got["rows"][b, row_at: row_at + o["nL"]], o["rows"], err_msg=str((b, j)))
        sub_at += n
        row_at += o["nL"]
        assert not got["probs"][b][o["cols"]].any(), (b, j)  # the columns of open clusters stay 0.0
    assert (got["sub"][b][sub_at:] == -7.0).all() and (got["rows"][b, row_at:] == -77).all(), b
    assert (got["desc"][b, len(opens):] == -77).all(), b


@pytest.mark.parametrize("condition", [False, True])
def test_partial_kernel_hands_out_the_restatements_sub_problems(eng, condition):
    import oracle_lib as ol
    F, nL, nM = 24, 20, 10
    raw, want_raw = restated(F, nL, nM, 12, 1000, 4)
    if condition:
        frames, want = [(f, nL, nM) for f in raw], want_raw
    else:  # the conditioned blocks, handed over as they are
        frames, want = [], []
        for f in raw:
            cond, idx = ol.condition_costs(f, nL + nM, nM)
            frames.append((cond, len(idx) - nM, nM))
            want.append(hc.hybrid_probs(cond, len(idx) - nM, nM, 1000, max_exact=4))
    got = partial_run(eng, frames, 4, condition)
    plain, lp, _, _ = eng.clustered_probs([f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames], condition=condition)
    seen = 0
    for b, w in enumerate(want):
        check_handed_out(got, b, w, nM)
        op = open_columns(w, nM)
        seen += len(w[2])
        assert np.array_equal(bits(got["probs"][b][~op]), bits(plain[b][~op])), b
        if not w[2]:
            assert bits(got["logPerm"][b]) == bits(lp[b]), b
    assert seen >= 20
    # a frame beyond the launch's bounds is left alone, its neighbours are not
    small = partial_run(eng, [frames[0], (dense_frame(40, 12, 3), 28, 12), frames[1]], 4, condition, maxRawRow=30, maxCol=10)
    assert small["info"][1] == -1 and small["nOpen"][1] == 0 and (small["probs"][1] == -5.0).all() and (small["sub"][1] == -7.0).all()
    check_handed_out(small, 0, want[0], nM)
    check_handed_out(small, 2, want[1], nM)


# ---- 3. real oversized clusters -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,frame,cluster,others", [((2, 60, 40, 30), 1, (17, 23), 8), ((6, 200, 128, 60), 5, (20, 26), 49)])
def test_real_oversized_clusters(eng, shape, frame, cluster, others):
    out, method, plain, want = check_against_restatement(eng, shape, 200, 16)
    assert [b for b, w in enumerate(want) if w[2]] == [frame]  # (the restatement itself: a condition of the test)
    (o,) = want[frame][2]
    assert (o["m"], o["nL"]) == cluster and want[frame][3] == others + 1
    assert method[frame] == 2 and method.tolist().count(0) == shape[0] - 1


# ---- 4. invariance ------------------------------------------------------------------------------------------------------------------
def test_invariance_over_batches_and_caps(eng):
    rng = np.random.default_rng(77)
    others = []
    for i in range(96):
        nM = 1 + i % 12
        nL = int(rng.integers(0, 41))
        others.append((rng.random((nL + nM) * nM) * 10.0, nL, nM))
    nL, nM, k = 40, 24, 200
    f = wl.scene_frames(8, nL, nM, 24)[7]  # (clusters of 5 and 9 columns: both open at 4, one at 8, none at 16)
    x = (f, nL, nM)

    def run(batch, max_exact):
        out, method, nOpen, _ = eng.hybrid_probs([q[0] for q in batch], [q[1] for q in batch], [q[2] for q in batch], k,
                                                 condition=True, max_exact=max_exact)
        return out, method, nOpen

    wants = {me: hc.hybrid_probs(f, nL, nM, k, condition=True, max_exact=me) for me in (4, 8, 16)}
    assert [len(wants[me][2]) for me in (4, 8, 16)] == [2, 1, 0]
    alone = {}
    for me in (4, 8, 16):
        a = run([x], me)
        first = run([x] + others, me)
        last = run(others + [x], me)
        op = open_columns(wants[me], nM)
        assert a[1][0] == first[1][0] == last[1][-1] == wants[me][1] and a[2][0] == first[2][0] == last[2][-1] == len(wants[me][2])
        for name, got in (("first", first[0][0]), ("last", last[0][-1])):
            assert np.array_equal(bits(a[0][0][~op]), bits(got[~op])), (me, name)
            assert np.abs(a[0][0][op] - got[op]).max(initial=0.0) <= 1e-12, (me, name)
        np.testing.assert_allclose(a[0][0][~op], wants[me][0][~op], rtol=0, atol=1e-12)
        np.testing.assert_allclose(a[0][0][op], wants[me][0][op], rtol=0, atol=1e-9)
        alone[me] = (a[0][0], op)
    for lo, hi in ((4, 8), (8, 16), (4, 16)):  # a cluster answered under both caps: the same bits
        both = ~alone[lo][1] & ~alone[hi][1]
        assert both.any() and np.array_equal(bits(alone[lo][0][both]), bits(alone[hi][0][both])), (lo, hi)


# ---- 5. edges -----------------------------------------------------------------------------------------------------------------------
def flat(blk):
    return np.ascontiguousarray(np.asarray(blk, dtype=np.float64).T).reshape(-1)


def test_open_cluster_without_an_assignment(eng):
    inf = np.inf
    same_row = flat([[1.0, 2.0], [inf, inf], [inf, inf], [inf, inf]])  # nL = 2, nM = 2: both columns can only take row 0
    good = dense_frame(9, 3, 6)
    out, method, nOpen, maxc = eng.hybrid_probs([good, same_row, good], [6, 2, 6], [3, 2, 3], 50, max_exact=1)
    assert hc.hybrid_probs(same_row, 2, 2, 50, max_exact=1)[1] == -2
    assert method[1] == -2 and not out[1].any() and not np.isnan(out[1]).any() and maxc[1] == 2
    want = hc.hybrid_probs(good, 6, 3, 50, max_exact=1)
    assert method[0] == method[2] == want[1] and nOpen[0] == len(want[2]) == 1
    np.testing.assert_allclose(out[0], want[0], rtol=0, atol=1e-9)
    assert np.array_equal(bits(out[0]), bits(out[2]))
    # an answered cluster with Z = 0 beside an open one: infeasible, nothing open
    lone = np.full((5, 3), inf)  # nL = 2, nM = 3: columns 0 and 1 share rows 0 and 1, column 2 has no finite entry at all
    lone[0, 0], lone[1, 0], lone[0, 1], lone[1, 1] = 1.0, 2.0, 2.5, 1.5
    (p,), method, nOpen, _ = eng.hybrid_probs([flat(lone)], [2], [3], 50, max_exact=1)
    assert hc.hybrid_probs(flat(lone), 2, 3, 50, max_exact=1)[1] == -2
    assert method[0] == -2 and nOpen[0] == 0 and not p.any()


def test_slot_cap_opens_instead_of_refusing(eng):
    nL, nM, k = 20, 10, 300
    blk = dense_frame(nL + nM, nM, 31)  # one cluster of ten columns and thirty rows: layers of (30 + 2) 2^10 8 bytes
    cap = 32 * 1024 * 8 - 8
    try:
        eng.set_clustered_slot_cap(cap)
        _, _, info, _ = eng.clustered_probs([blk], [nL], [nM])
        (p,), method, nOpen, maxc = eng.hybrid_probs([blk], [nL], [nM], k)
    finally:
        eng.set_clustered_slot_cap(0)
    want = hc.hybrid_probs(blk, nL, nM, k, slot_bytes=cap)
    assert info[0] == -3 and len(want[2]) == 1 and want[2][0]["m"] == 10
    assert nOpen[0] == 1 and method[0] == want[1] == 2 and maxc[0] == 10
    print(f"slot cap: vs restatement {np.abs(p - want[0]).max():.3g}")
    np.testing.assert_allclose(p, want[0], rtol=0, atol=1e-9)
    (q,), method, nOpen, _ = eng.hybrid_probs([blk], [nL], [nM], k)  # the cap is gone: exact again
    assert method[0] == 0 and nOpen[0] == 0
    np.testing.assert_allclose(q, cc.clustered_probs(blk, nL, nM)[0], rtol=0, atol=1e-12)


def test_layout_refusal_bad_arguments_and_empty_batch(eng):
    inf = np.inf
    odd = flat([[inf, inf, 1.0], [1.0, 1.5, inf], [2.0, 1.0, inf], [1.0, 3.0, inf]])  # nL = 1, nM = 3: three rows >= nL on two columns
    good = dense_frame(9, 3, 6)
    out, method, nOpen, _ = eng.hybrid_probs([good, odd, good], [6, 1, 6], [3, 3, 3], 20, max_exact=1)
    assert hc.hybrid_probs(odd, 1, 3, 20, max_exact=1)[1] == -1
    assert method[1] == -1 and nOpen[1] == 0 and not out[1].any()
    assert method[0] == method[2] == 2 and np.array_equal(bits(out[0]), bits(out[2]))
    with pytest.raises(RuntimeError, match="refused"):
        pk.hybridProb(wide_odd_frame(), 1, 19, 20)  # (the module function has max_exact 16: a 17-column cluster)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    nLa, nMa, off = np.array([6], np.int32), np.array([3], np.int32), np.zeros(1, np.int64)
    probs, meth = np.zeros(3 * 7), np.zeros(1, np.int32)
    for bad in (-1, 17):
        rc = eng.lib.kbest_hybrid_probs_batch_f64(eng.ctx, 1, vp(nLa), vp(nMa), vp(good), vp(off), 0, 20, bad, vp(probs), vp(off),
                                                  vp(meth), None, None)
        assert rc == -2  # KBEST_ERR_BAD_ARG
    with pytest.raises(pk.KBestError):
        eng.hybrid_probs([good], [6], [3], 0)  # k < 1
    assert eng.lib.kbest_hybrid_probs_batch_f64(eng.ctx, 0, None, None, None, None, 0, 20, 0, None, None, None, None, None) == 0
    out, method, nOpen, maxc = eng.hybrid_probs([], [], [], 20)
    assert out == [] and method.size == 0
    (again,), method, _, _ = eng.hybrid_probs([good], [6], [3], 20)  # the context still answers
    assert method[0] == 0
    np.testing.assert_allclose(again, cc.clustered_probs(good, 6, 3)[0], rtol=0, atol=1e-12)


def wide_odd_frame():
    """nL = 1, nM = 19: columns 0 .. 16 share the miss rows 1 .. 18 -- eighteen rows >= nL on seventeen columns."""
    rng = np.random.default_rng(5)
    blk = np.full((20, 19), np.inf)
    blk[1:19, :17] = rng.random((18, 17)) * 10.0
    blk[0, 17] = 1.0
    blk[19, 18] = 1.0
    return flat(blk)


def test_cpp_shim_and_module_function(eng, tmp_path):
    exe = str(tmp_path / "shim_hybrid")
    libdir = os.path.join(ROOT, "probabilisticsemslam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_hybrid.cpp"), "-o", exe,
                           "-L", libdir, "-l:libkbest_amd.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
                           "-L/opt/rocm/lib", "-lamdhip64"])
    dense, nL, nM, k = dense_frame(20, 17, 17), 3, 17, 50  # one cluster of seventeen columns: open at the cap of 16

    def write(name, blk, l, m):
        path = tmp_path / name
        path.write_text(f"{l} {m}\n" + "\n".join("inf" if np.isinf(v) else float.hex(float(v)) for v in blk) + "\n")
        return str(path)

    lines = subprocess.check_output([exe, str(k), write("dense.txt", dense, nL, nM), write("odd.txt", wide_odd_frame(), 1, 19)],
                                    text=True).splitlines()
    want = hc.hybrid_probs(dense, nL, nM, k)
    assert want[1] == 2 and len(want[2]) == 1
    (got,), method, nOpen, _ = eng.hybrid_probs([dense], [nL], [nM], k)  # the C entry: the same doubles
    assert method[0] == 2 and nOpen[0] == 1
    np.testing.assert_allclose(got, want[0], rtol=0, atol=1e-9)
    assert len(lines) == nM + 1
    for c in range(nM):
        tok = lines[c].split()
        assert tok[:2] == ["p", str(c)]
        assert np.array_equal(bits(np.array([float.fromhex(v) for v in tok[2:]])), bits(got[c])), c
    assert lines[-1].startswith("hybridProb: runtime_error") and "refused" in lines[-1]
    np.testing.assert_array_equal(pk.hybridProb(dense, nL, nM, k), got)  # the package-level wrapper
