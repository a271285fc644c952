"""GPU: the big-cluster tier (kbest_bigcluster.hip, kbest_bigcluster_probs_f64_dev, kbest_hybrid_exact_probs_batch_f64, the
hybridExactProb shim) -- exact association probabilities of clusters of 17 .. 20 measurements, one cluster over the whole chip --
against the numpy restatement of tests/bigcluster_check.py and against the project's other exact tiers, never against its own
output.  Tolerances: 1e-12 absolute on probabilities (sums of non-negative terms in a fixed order; the project's tiers agree to
below 1e-15), 1e-12 relative on logPerm; everything that does not go through the new tier: equal bits."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import bigcluster_check as bc
import probabilisticsemslam_amd as pk
from probabilisticsemslam_amd import workloads as wl
from test_gpu_permanent import bits, dense_frame

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -2  # KBEST_ERR_BAD_ARG


@pytest.fixture(scope="module")
def eng():
    e = pk.KBestEngine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def scene(F, nL, nM, side):
    return wl.scene_frames(F, nL, nM, side)


@functools.lru_cache(maxsize=None)
def restated(shape, index, **kw):
    """The restatement of frame `index` of scene(*shape), conditioned while loading.  Computed once; nobody changes it."""
    _, nL, nM, _ = shape
    return bc.hybrid_exact_probs(scene(*shape)[index], nL, nM, condition=True, **kw)


def big_columns(want, nM):
    mask = np.zeros(nM, bool)
    for o in want[2]:
        if o["big"]:
            mask[o["cols"]] = True
    return mask


SMALL = (24, 20, 10, 12)
MID = (75, 60, 40, 30)
WIDE = (6, 200, 128, 60)


# ---- 1. smallest shapes, tier against tier -------------------------------------------------------------------------------------------
def test_small_clusters_against_the_plain_tiers(eng):
    F, nL, nM, _ = SMALL
    frames = scene(*SMALL)
    out, method, nOpen, nBig, maxc, lp = eng.hybrid_exact_probs(frames, [nL] * F, [nM] * F, 0, condition=True, max_exact=1, max_big=16)
    plain, plp, info, pmaxc = eng.clustered_probs(frames, [nL] * F, [nM] * F, condition=True)
    worst = worst_lp = 0.0
    sizes = set()
    for b in range(F):
        want = restated(SMALL, b, max_exact=1, max_big=16)
        sizes |= {o["m"] for o in want[2]}
        assert nBig[b] == want[3] and nOpen[b] == len(want[2]) and maxc[b] == pmaxc[b], b
        if info[b] > 0:
            assert method[b] == 0, b
            worst = max(worst, np.abs(out[b] - plain[b]).max())
            worst_lp = max(worst_lp, abs(lp[b] - plp[b]) / max(1.0, abs(plp[b])))
    print(f"clusters of {sorted(sizes)} columns through the big-cluster tier: vs clustered_probs {worst:.3g}, logPerm {worst_lp:.3g}")
    assert (info > 0).sum() >= 20 and min(sizes) == 2 and max(sizes) >= 8 and nBig.sum() >= 20
    assert worst <= 1e-12 and worst_lp <= 1e-12


# ---- 2. / 3. just beyond 16, and at the cap --------------------------------------------------------------------------------------------
def check_big_frame(eng, shape, index, cluster):
    _, nL, nM, _ = shape
    f = scene(*shape)[index]
    want = restated(shape, index)
    (o,) = [o for o in want[2] if o["big"]]
    assert (o["m"], o["R"]) == cluster and want[1] == 0 and want[3] == 1  # (the restatement itself: a condition of the test)
    (p,), method, nOpen, nBig, maxc, lp = eng.hybrid_exact_probs([f], [nL], [nM], 0, condition=True)
    (h,), hmethod, hOpen, hmaxc = eng.hybrid_probs([f], [nL], [nM], 200, condition=True)
    big = big_columns(want, nM)
    err = np.abs(p[big] - want[0][big]).max()
    sums = np.abs(p.sum(axis=1) - 1.0).max()
    print(f"{shape[1:]} frame {index}, cluster {cluster}: big columns vs restatement {err:.3g}, columns - 1 {sums:.3g}, "
          f"logPerm {lp[0]!r} vs {want[5]!r}; hybrid_probs(k = 200) is off by {np.abs(h - p).max():.3g}")
    assert method[0] == 0 and nBig[0] == 1 and nOpen[0] == hOpen[0] == 1 and maxc[0] == hmaxc[0] == cluster[0]
    assert big.sum() == cluster[0] and err <= 1e-12 and sums <= 1e-12
    assert np.array_equal(bits(p[~big]), bits(h[~big]))
    assert abs(lp[0] - want[5]) <= 1e-12 * max(1.0, abs(want[5]))
    return p


@pytest.mark.parametrize("index,cluster", [(1, (17, 40)), (38, (18, 43))])
def test_just_beyond_sixteen(eng, index, cluster):
    check_big_frame(eng, MID, index, cluster)


def test_at_the_cap_of_twenty(eng):
    check_big_frame(eng, WIDE, 5, (20, 46))


# ---- 4. beyond the cap -----------------------------------------------------------------------------------------------------------------
def same_as_hybrid(eng, frames, nLs, nMs, k, **kw):
    out, method, nOpen, nBig, maxc, _ = eng.hybrid_exact_probs(frames, nLs, nMs, k, condition=True, **kw)
    kw.pop("max_big", None)
    h, hmethod, hOpen, hmaxc = eng.hybrid_probs(frames, nLs, nMs, k, condition=True, **kw)
    assert not nBig.any()
    np.testing.assert_array_equal(method, hmethod)
    np.testing.assert_array_equal(nOpen, hOpen)
    np.testing.assert_array_equal(maxc, hmaxc)
    for b in range(len(frames)):
        assert np.array_equal(bits(out[b]), bits(h[b])), b
    return out, method


def test_beyond_twenty(eng):
    _, nL, nM, _ = MID
    f = scene(*MID)[74]  # (a cluster of 23 measurements)
    (p,), method, nOpen, nBig, maxc, lp = eng.hybrid_exact_probs([f], [nL], [nM], 0, condition=True)
    assert method[0] == -1 and not p.any() and np.isnan(lp[0]) and nBig[0] == 0 and maxc[0] == 23
    _, method = same_as_hybrid(eng, [f], [nL], [nM], 200)
    assert method[0] == 2


# ---- 5. range ----------------------------------------------------------------------------------------------------------------------------
def test_products_below_the_normal_doubles(eng):
    nL, nM = 21, 19
    rng = np.random.default_rng(11)
    blk = np.full((nL + nM, nM), np.inf)
    blk[:20, :18] = 38.0 + 3.9 * rng.random((20, 18))  # products of 18 entries: about e^-720
    blk[20, 18] = 0.0
    low = blk.copy()
    low[:20, :18] -= 38.0
    flat = lambda a: np.ascontiguousarray(a.T).reshape(-1)  # noqa: E731
    out, method, nOpen, nBig, maxc, lp = eng.hybrid_exact_probs([flat(blk), flat(low)], [nL] * 2, [nM] * 2, 0)
    err = np.abs(out[0] - out[1]).max()
    print(f"costs 38 higher: probabilities differ by {err:.3g}, logPerm {lp[0]!r} vs {lp[1]!r} - 684")
    assert method.tolist() == [0, 0] and nBig.tolist() == [1, 1] and maxc.tolist() == [18, 18]
    assert err <= 1e-12 and np.abs(out[0].sum(axis=1) - 1.0).max() <= 1e-12
    assert np.isfinite(lp).all() and abs(lp[0] - (lp[1] - 18 * 38.0)) <= 1e-12 * abs(lp[0])
    want = bc.hybrid_exact_probs(flat(low), nL, nM)
    assert want[1] == 0 and np.abs(out[1] - want[0]).max() <= 1e-12 and abs(lp[1] - want[5]) <= 1e-12 * max(1.0, abs(want[5]))


# ---- 6. the same bits everywhere ---------------------------------------------------------------------------------------------------------
def test_same_bits_in_any_batch_and_under_any_cap(eng):
    _, nL, nM, _ = MID
    frames = scene(*MID)
    x = (frames[1], nL, nM)
    rng = np.random.default_rng(7)
    others = [(frames[38], nL, nM)]  # (a cluster of 18 measurements: shares the launches)
    for i in range(31):
        m = 1 + i % 12
        l = int(rng.integers(0, 30))
        others.append((rng.random((l + m) * m) * 10.0, l, m))

    def run(batch, k=0):
        return eng.hybrid_exact_probs([q[0] for q in batch], [q[1] for q in batch], [q[2] for q in batch], k, condition=True)

    alone = run([x])
    first = run([x] + others)
    last = run(others + [x])
    assert alone[1][0] == first[1][0] == last[1][-1] == 0 and alone[3][0] == first[3][0] == last[3][-1] == 1
    assert first[3][1] == 1  # (frame 38 went through the tier beside it)
    assert np.array_equal(bits(alone[0][0]), bits(first[0][0])) and np.array_equal(bits(alone[0][0]), bits(last[0][-1]))
    assert bits(alone[5][0]) == bits(first[5][0]) == bits(last[5][-1])
    want = restated(MID, 1)
    (o,) = [o for o in want[2] if o["big"]]
    (o38,) = [q for q in restated(MID, 38)[2] if q["big"]]
    need, need38 = bc.layers_bytes(o["m"], o["nL"]), bc.layers_bytes(o38["m"], o38["nL"])
    try:
        eng.set_bigcluster_work_cap(max(need, need38))  # one cluster at a time
        one = run([x] + others)
        eng.set_bigcluster_work_cap(need - 8)  # below this cluster's need
        (p,), method, nOpen, nBig, _, lp = run([x])
        assert method[0] == -1 and not p.any() and nBig[0] == 0 and np.isnan(lp[0])
        same_as_hybrid(eng, [x[0]], [nL], [nM], 200)
    finally:
        eng.set_bigcluster_work_cap(0)
    assert one[1][0] == 0 and one[3][0] == 1 and one[3][1] == 1
    assert np.array_equal(bits(alone[0][0]), bits(one[0][0])) and bits(alone[5][0]) == bits(one[5][0])

    # the device entry on a stream of the caller's: the bits of the host entry, nothing else written
    import torch
    dev = torch.device("cuda", 0)
    m, cL = o["m"], o["nL"]
    pad = 64
    sub = np.concatenate([np.full(pad, -7.0), o["block"], np.full(pad, -7.0)])
    d_sub = torch.from_numpy(sub).to(dev)
    d_probs = torch.full((2 * pad + m * (cL + 1),), -5.0, dtype=torch.float64, device=dev)
    d_logZ = torch.full((3,), -5.0, dtype=torch.float64, device=dev)
    d_info = torch.full((3,), -77, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    eng.bigcluster_probs_dev([m], [cL], [pad], [pad], d_sub, d_probs, d_logZ[1:], d_info[1:], stream=s.cuda_stream)
    s.synchronize()
    hp, hz, hi = d_probs.cpu().numpy(), d_logZ.cpu().numpy(), d_info.cpu().numpy()
    assert (hp[:pad] == -5.0).all() and (hp[-pad:] == -5.0).all() and np.array_equal(d_sub.cpu().numpy(), sub)
    assert hz[0] == hz[2] == -5.0 and hi.tolist() == [-77, 1, -77] and np.isfinite(hz[1])
    q = hp[pad:-pad].reshape(m, cL + 1)
    got = alone[0][0]
    assert np.array_equal(bits(q[:, :cL]), bits(got[np.ix_(o["cols"], o["rows"])]))
    assert np.array_equal(bits(q[:, cL]), bits(got[o["cols"], nL]))
    assert np.abs(q - o["probs"]).max() <= 1e-12 and abs(hz[1] - o["logZ"]) <= 1e-12 * abs(o["logZ"])
    try:  # ... and under a cap below its need: -3, its outputs untouched
        eng.set_bigcluster_work_cap(need - 8)
        d_probs.fill_(-5.0)
        d_logZ.fill_(-5.0)
        eng.bigcluster_probs_dev([m], [cL], [pad], [pad], d_sub, d_probs, d_logZ[1:], d_info[1:], stream=s.cuda_stream, reserve=False)
        s.synchronize()
    finally:
        eng.set_bigcluster_work_cap(0)
    assert d_info.cpu().tolist() == [-77, -3, -77] and (d_probs.cpu().numpy() == -5.0).all() and (d_logZ.cpu().numpy() == -5.0).all()


# ---- 7. edges ------------------------------------------------------------------------------------------------------------------------------
def flat(blk):
    return np.ascontiguousarray(np.asarray(blk, dtype=np.float64).T).reshape(-1)


def test_without_the_tier_it_is_hybrid_probs(eng):
    F, nL, nM, _ = SMALL
    out, method = same_as_hybrid(eng, scene(*SMALL), [nL] * F, [nM] * F, 50, max_exact=1, max_big=0)
    assert (method > 0).sum() >= 20


def test_infeasible_bad_arguments_and_empty_batch(eng):
    inf = np.inf
    same_row = flat([[1.0, 2.0], [inf, inf], [inf, inf], [inf, inf]])  # nL = 2, nM = 2: both columns can only take row 0
    good = dense_frame(9, 3, 6)
    out, method, nOpen, nBig, maxc, lp = eng.hybrid_exact_probs([good, same_row, good], [6, 2, 6], [3, 2, 3], 0, max_exact=1)
    assert bc.hybrid_exact_probs(same_row, 2, 2, max_exact=1)[1] == -2
    assert method[1] == -2 and not out[1].any() and nBig[1] == 0 and maxc[1] == 2 and lp[1] == -inf
    want = bc.hybrid_exact_probs(good, 6, 3, max_exact=1)
    assert method[0] == method[2] == 0 and nBig[0] == nBig[2] == want[3] == 1
    assert np.abs(out[0] - want[0]).max() <= 1e-12 and np.array_equal(bits(out[0]), bits(out[2]))
    assert abs(lp[0] - want[5]) <= 1e-12 * max(1.0, abs(want[5]))
    out0 = out[0]
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    nLa, nMa, off = np.array([6], np.int32), np.array([3], np.int32), np.zeros(1, np.int64)
    probs, meth = np.zeros(3 * 7), np.zeros(1, np.int32)
    for k, max_exact, max_big in ((0, 16, -1), (0, 16, 21), (0, 17, 20), (-1, 16, 20)):
        rc = eng.lib.kbest_hybrid_exact_probs_batch_f64(eng.ctx, 1, vp(nLa), vp(nMa), vp(good), vp(off), 0, k, max_exact, max_big,
                                                        vp(probs), vp(off), None, vp(meth), None, None, None)
        assert rc == BAD_ARG, (k, max_exact, max_big)
    for m in (0, 21):
        one = np.array([m], np.int32)
        rc = eng.lib.kbest_bigcluster_probs_f64_dev(eng.ctx, 1, vp(one), vp(nLa), vp(off), vp(off), C.c_void_p(8), C.c_void_p(8), None,
                                                    None, None)
        assert rc == BAD_ARG, m
    assert eng.lib.kbest_hybrid_exact_probs_batch_f64(eng.ctx, 0, None, None, None, None, 0, 0, 16, 20, None, None, None, None, None,
                                                      None, None) == 0
    out, method, nOpen, nBig, maxc, lp = eng.hybrid_exact_probs([], [], [], 0)
    assert out == [] and method.size == 0 and lp.size == 0
    (again,), method, _, nBig, _, _ = eng.hybrid_exact_probs([good], [6], [3], 0, max_exact=1)  # the context still answers
    assert method[0] == 0 and nBig[0] == 1 and np.array_equal(bits(again), bits(out0))


def test_cpp_shim_and_module_function(eng, tmp_path):
    exe = str(tmp_path / "shim_bigcluster")
    libdir = os.path.join(ROOT, "probabilisticsemslam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_bigcluster.cpp"), "-o", exe,
                           "-L", libdir, "-l:libkbest_amd.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
                           "-L/opt/rocm/lib", "-lamdhip64"])
    dense, nL, nM = dense_frame(20, 17, 17), 3, 17  # one cluster of seventeen columns
    wide = dense_frame(24, 21, 5)                   # ... and one of twenty-one: refused with k = 0

    def write(name, blk, l, m):
        path = tmp_path / name
        path.write_text(f"{l} {m}\n" + "\n".join("inf" if np.isinf(v) else float.hex(float(v)) for v in blk) + "\n")
        return str(path)

    lines = subprocess.check_output([exe, "0", write("dense.txt", dense, nL, nM), write("wide.txt", wide, 3, 21)],
                                    text=True).splitlines()
    want = bc.hybrid_exact_probs(dense, nL, nM)
    assert want[1] == 0 and want[3] == 1
    (got,), method, nOpen, nBig, _, _ = eng.hybrid_exact_probs([dense], [nL], [nM], 0)  # the C entry: the same doubles
    assert method[0] == 0 and nBig[0] == 1
    np.testing.assert_allclose(got, want[0], rtol=0, atol=1e-12)
    assert len(lines) == nM + 1
    for c in range(nM):
        tok = lines[c].split()
        assert tok[:2] == ["p", str(c)]
        assert np.array_equal(bits(np.array([float.fromhex(v) for v in tok[2:]])), bits(got[c])), c
    assert lines[-1].startswith("hybridExactProb: runtime_error") and "refused" in lines[-1]
    np.testing.assert_array_equal(pk.hybridExactProb(dense, nL, nM, 0), got)  # the package-level wrapper
    with pytest.raises(RuntimeError, match="refused"):
        pk.hybridExactProb(wide, 3, 21, 0)
