"""GPU: the frontier tier (kbest_frontier.hip, kbest_frontier_probs_f64_dev, kbest_hybrid_frontier_probs_batch_f64, the
hybridFrontierProb shim) -- exact association probabilities of sparse clusters of up to 64 measurements, one workgroup per cluster
in one launch -- against the Python restatement of tests/frontier_check.py (dicts keyed by full column masks: no index maps),
against the plain subset sums and against the big-cluster tier, never against its own output.  Tolerances: 1e-12 absolute on
probabilities (sums of non-negative terms in a fixed order), 1e-12 relative on log Z / logPerm; everything that does not go
through the new tier: equal bits."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import frontier_check as fc
import permanent_check as pc
import probabilisticsemslam_amd as pk
from probabilisticsemslam_amd import workloads as wl
from test_gpu_permanent import bits, dense_frame

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, NOT_RESERVED = -2, -6  # KBEST_ERR_BAD_ARG, KBEST_ERR_NOT_RESERVED
SMALL = (200, 40, 24, 24)
MID = (200, 60, 40, 30)
WIDE = (64, 200, 128, 60)
PAD, UNTOUCHED = 64, -5.0
INF = np.inf
flat = fc.flat


@pytest.fixture(scope="module")
def eng():
    e = pk.KBestEngine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def scene(F, nL, nM, side):
    return wl.scene_frames(F, nL, nM, side)


@functools.lru_cache(maxsize=None)
def restated(shape, index, condition=True):
    """The restatement of frame `index` of scene(*shape).  Computed once; nobody changes it."""
    _, nL, nM, _ = shape
    return fc.hybrid_frontier_probs(scene(*shape)[index], nL, nM, condition=condition)


def scene_cluster(shape, index, cluster):
    """(block, nL_k, m) of the one open cluster of that frame, and its dict."""
    (o,) = restated(shape, index)[2]
    assert (o["m"], o["R"]) == cluster and o["tier"] == "frontier"
    return (o["block"], o["nL"], o["m"]), o


@functools.lru_cache(maxsize=None)
def restated_cluster(name):
    return fc.frontier_cluster(*fc.edge_clusters()[name])


def run_dev(eng, blocks, stream=None, reserve=True):
    """kbest_frontier_probs_f64_dev on the blocks [(flat, nL_k, m)], sentinels between and around everything.  Returns one
    (probs [m, nL_k + 1], logZ, info, width) per block; probs and logZ keep UNTOUCHED where nothing was written."""
    dev = torch.device("cuda", 0)
    sub, subOff, probOff, at = [np.full(PAD, -7.0)], [], [], PAD
    pat = PAD
    for blk, l, m in blocks:
        subOff.append(at)
        sub += [np.asarray(blk, dtype=np.float64), np.full(PAD, -7.0)]
        at += len(blk) + PAD
        probOff.append(pat)
        pat += m * (l + 1) + PAD
    sub = np.concatenate(sub)
    n = len(blocks)
    d_sub = torch.from_numpy(sub).to(dev)
    d_probs = torch.full((pat,), UNTOUCHED, dtype=torch.float64, device=dev)
    d_logZ = torch.full((n + 2,), UNTOUCHED, dtype=torch.float64, device=dev)
    d_int = torch.full((2, n + 2), -77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    eng.frontier_probs_dev([b[2] for b in blocks], [b[1] for b in blocks], subOff, probOff, d_sub, d_probs, d_logZ[1:], d_int[0, 1:],
                           d_int[1, 1:], stream=stream, reserve=reserve)
    torch.cuda.synchronize()
    hp, hz, hi = d_probs.cpu().numpy(), d_logZ.cpu().numpy(), d_int.cpu().numpy()
    assert np.array_equal(d_sub.cpu().numpy(), sub)
    assert hz[0] == hz[-1] == UNTOUCHED and hi[:, 0].tolist() == hi[:, -1].tolist() == [-77, -77]
    out, end = [], 0
    for j, (blk, l, m) in enumerate(blocks):
        assert (hp[end:probOff[j]] == UNTOUCHED).all(), j
        end = probOff[j] + m * (l + 1)
        out.append((hp[probOff[j]:end].reshape(m, l + 1).copy(), float(hz[1 + j]), int(hi[0, 1 + j]), int(hi[1, 1 + j])))
    assert (hp[end:] == UNTOUCHED).all()
    return out


def check_against(got, want, name):
    p, lz, info, W = got
    wp, wlz, winfo, wW = want
    assert (info, W) == (winfo, wW), (name, info, W, winfo, wW)
    err = np.abs(p - wp).max()
    print(f"{name}: W {W}, probabilities vs restatement {err:.3g}, log Z {lz!r} vs {wlz!r}")
    assert err <= 1e-12 and abs(lz - wlz) <= 1e-12 * max(1.0, abs(wlz)), name
    return err


# ---- 1. the smallest shapes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one_by_one", "two_by_one", "fewer_states_than_a_wave", "more_states_than_the_workgroup",
                                  "opens_and_closes_in_one_row", "band_of_24", "more_rows_than_lanes"])
def test_smallest_shapes_against_the_restatement(eng, name):
    blk = fc.edge_clusters()[name]
    want = restated_cluster(name)
    assert want[2] == 1  # (the restatement itself: a condition of the test)
    A, _, _ = fc.scaled_block(*blk)
    steps, W, _ = fc.greedy_plan(fc.row_masks(A), blk[2])
    if name == "more_states_than_the_workgroup":
        assert W == 12
    if name == "fewer_states_than_a_wave":
        assert W < 6
    if name == "opens_and_closes_in_one_row":
        assert any(s["new"] & s["closing"] and s["phi"] for s in steps)
    if name == "band_of_24":
        assert W <= 3 and blk[2] == 24
    if name == "more_rows_than_lanes":
        assert len(steps) > 256
    (got,) = run_dev(eng, [blk])
    check_against(got, want, name)
    assert np.abs(got[0].sum(axis=1) - 1.0).max() <= 1e-12  # sum_r w[r][c] = Z for every column
    if name == "one_by_one":
        assert got[0].tolist() == [[1.0]] and got[1] == -1.5


def test_width_sixteen_is_answered_and_seventeen_is_not(eng):
    blk = fc.edge_clusters()["width_16"]
    X = np.asarray(blk[0]).reshape(16, 18).T
    w, Z = pc.subset_sums(np.where(np.isfinite(X), np.exp(-X), 0.0))
    want = pc.fold(w, Z, 2)
    got, wide = run_dev(eng, [blk, fc.edge_clusters()["width_17"]])
    err = np.abs(got[0] - want).max()
    print(f"two rows over 16 columns: W {got[3]}, vs subset_sums {err:.3g}, log Z {got[1]!r} vs {np.log(Z)!r}")
    assert got[2:] == (1, 16) and err <= 1e-12 and abs(got[1] - np.log(Z)) <= 1e-12 * max(1.0, abs(np.log(Z)))
    assert wide[2:] == (fc.REFUSED_WIDTH, 17) and (wide[0] == UNTOUCHED).all() and wide[1] == UNTOUCHED
    assert restated_cluster("width_17")[2:] == (fc.REFUSED_WIDTH, 17) and restated_cluster("width_16")[2:] == (1, 16)


def test_a_lowered_slot_refuses(eng):
    blk = fc.edge_clusters()["band_of_24"]
    A, _, _ = fc.scaled_block(*blk)
    need = fc.layers_bytes(fc.row_masks(A), blk[2])
    try:
        eng.set_frontier_slot(need - 8)
        (low,) = run_dev(eng, [blk])
        eng.set_frontier_slot(need)
        (fits,) = run_dev(eng, [blk])
    finally:
        eng.set_frontier_slot(0)
    assert low[2] == fc.REFUSED_SLOT and (low[0] == UNTOUCHED).all() and low[1] == UNTOUCHED and low[3] == restated_cluster("band_of_24")[3]
    check_against(fits, restated_cluster("band_of_24"), "band_of_24 in a slot of exactly its layers")


def test_columns_that_share_their_only_row(eng):
    (got,) = run_dev(eng, [fc.edge_clusters()["same_only_row"]])
    assert restated_cluster("same_only_row")[2] == 0
    assert got[2] == 0 and not got[0].any() and got[1] == -INF and got[3] == 2


# ---- 2. the scene clusters -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,index,cluster", [(MID, 1, (17, 40)), (MID, 38, (18, 43)), (WIDE, 5, (20, 46))])
def test_against_the_big_cluster_tier(eng, shape, index, cluster):
    blk, o = scene_cluster(shape, index, cluster)
    (got,) = run_dev(eng, [blk])
    dev = torch.device("cuda", 0)
    m, cL = blk[2], blk[1]
    d_sub = torch.from_numpy(np.asarray(blk[0])).to(dev)
    d_probs = torch.zeros(m * (cL + 1), dtype=torch.float64, device=dev)
    d_logZ = torch.zeros(1, dtype=torch.float64, device=dev)
    d_info = torch.zeros(1, dtype=torch.int32, device=dev)
    eng.bigcluster_probs_dev([m], [cL], [0], [0], d_sub, d_probs, d_logZ, d_info)
    torch.cuda.synchronize()
    big, bigZ = d_probs.cpu().numpy().reshape(m, cL + 1), float(d_logZ.cpu()[0])
    err = np.abs(got[0] - big).max()
    print(f"cluster {cluster}: W {got[3]}, vs the big-cluster tier {err:.3g}, log Z {got[1]!r} vs {bigZ!r}")
    assert int(d_info.cpu()[0]) == 1 and got[2] == 1 and got[3] == o["W"]
    assert err <= 1e-12 and abs(got[1] - bigZ) <= 1e-12 * max(1.0, abs(bigZ))


@pytest.mark.parametrize("shape,index,cluster", [(WIDE, 54, (22, 51)), (WIDE, 8, (23, 61)), (MID, 89, (25, 58))])
def test_beyond_twenty_against_the_restatement(eng, shape, index, cluster):
    blk, o = scene_cluster(shape, index, cluster)
    (got,) = run_dev(eng, [blk])
    check_against(got, (o["probs"], o["logZ"], 1, o["W"]), f"cluster {cluster}")
    assert np.abs(got[0].sum(axis=1) - 1.0).max() <= 1e-12


# ---- 3. the same bits everywhere -------------------------------------------------------------------------------------------------------
def test_same_bits_alone_in_a_batch_and_under_a_cap(eng):
    names = list(fc.edge_clusters())
    mixed = [fc.edge_clusters()[n] for n in names] + [scene_cluster(MID, 1, (17, 40))[0], scene_cluster(WIDE, 8, (23, 61))[0],
                                               scene_cluster(MID, 89, (25, 58))[0]]
    alone = [run_dev(eng, [b])[0] for b in mixed]
    batch = run_dev(eng, mixed)
    back = run_dev(eng, mixed[::-1])[::-1]
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    mine = run_dev(eng, mixed, stream=s.cuda_stream)  # (a stream of the caller's)
    many = run_dev(eng, (mixed * 11)[:131])  # more clusters than one launch takes
    try:
        eng.set_frontier_work_cap(fc.SLOT)  # one slot: one cluster at a time
        one = run_dev(eng, mixed, reserve=False)
    finally:
        eng.set_frontier_work_cap(0)
    for j, a in enumerate(alone):
        for other in (batch[j], back[j], mine[j], one[j], many[j], many[j + len(mixed) * ((130 - j) // len(mixed))]):
            assert a[2:] == other[2:], j
            assert np.array_equal(bits(a[0]), bits(other[0])) and bits(a[1]) == bits(other[1]), j
    assert sorted({a[2] for a in alone}) == [fc.REFUSED_WIDTH, 0, 1]
    for n, a in zip(names, alone):
        assert a[2:] == restated_cluster(n)[2:], n


# ---- 4. the host entry -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,extra", [(SMALL, (125, 154)), (MID, (1, 38, 89, 126, 157)), (WIDE, (54,))])
def test_hybrid_frontier_probs_with_k_zero(eng, shape, extra):
    """The first 16 frames of the family and the frames that hold its oversized clusters, conditioned while loading."""
    _, nL, nM, _ = shape
    index = sorted(set(range(16)) | set(extra))
    frames = [scene(*shape)[b] for b in index]
    n = len(frames)
    out, method, nOpen, nBig, maxc, lp, nFr = eng.hybrid_frontier_probs(frames, [nL] * n, [nM] * n, 0, condition=True)
    plain, _, info, _ = eng.clustered_probs(frames, [nL] * n, [nM] * n, condition=True)
    h, _, _, _ = eng.hybrid_probs(frames, [nL] * n, [nM] * n, 200, condition=True)
    worst = worst_lp = 0.0
    sizes = []
    for j, b in enumerate(index):
        want = restated(shape, b)
        assert (method[j], nFr[j], nBig[j], maxc[j], nOpen[j]) == (want[1], want[3], want[4], want[5], len(want[2])), b
        assert want[1] == 0 and want[4] == 0  # (k = 0 answers every frame: a condition of the test)
        worst_lp = max(worst_lp, abs(lp[j] - want[6]) / max(1.0, abs(want[6])))
        openc = np.zeros(nM, bool)
        for o in want[2]:
            openc[o["cols"]] = True
            sizes.append(o["m"])
        if not want[2]:
            assert info[j] > 0 and np.array_equal(bits(out[j]), bits(plain[j])), b
        else:  # the partial kernel's columns: hybrid_probs has their bits whatever it does with the open ones
            assert np.array_equal(bits(out[j][~openc]), bits(h[j][~openc])), b
            worst = max(worst, np.abs(out[j][openc] - want[0][openc]).max())
            assert np.abs(out[j].sum(axis=1) - 1.0).max() <= 1e-12, b
    print(f"{shape[1:]}: clusters of {sorted(sizes)} through the frontier tier: open columns {worst:.3g}, logPerm {worst_lp:.3g}")
    assert len(sizes) >= len(extra) and nFr.sum() == len(sizes)
    assert worst <= 1e-12 and worst_lp <= 1e-12


def test_without_the_tier_it_is_hybrid_exact_probs(eng):
    _, nL, nM, _ = MID
    index = list(range(16)) + [38, 74, 89]  # (74: a cluster of 23, 89: one of 25)
    frames = [scene(*MID)[b] for b in index]
    n = len(frames)
    for k in (0, 200):
        a = eng.hybrid_frontier_probs(frames, [nL] * n, [nM] * n, k, condition=True, max_width=0)
        b = eng.hybrid_exact_probs(frames, [nL] * n, [nM] * n, k, condition=True)
        assert not a[6].any()
        for x, y in zip(a[1:5], b[1:5]):
            np.testing.assert_array_equal(x, y)
        assert np.array_equal(bits(a[5]), bits(b[5]))
        for j in range(n):
            assert np.array_equal(bits(a[0][j]), bits(b[0][j])), (k, index[j])
        assert (b[1] == -1).sum() == (2 if k == 0 else 0) and b[3].sum() >= 2
    # a width below the cluster's: the big-cluster tier takes the 18 columns of frame 38 (W = 10), nothing takes the 25 of frame 89
    few = [scene(*MID)[38], scene(*MID)[89]]
    out, method, nOpen, nBig, maxc, lp, nFr = eng.hybrid_frontier_probs(few, [nL] * 2, [nM] * 2, 0, condition=True, max_width=8)
    assert restated(MID, 38)[2][0]["W"] == 10 and restated(MID, 89)[2][0]["W"] == 9
    ex = eng.hybrid_exact_probs(few, [nL] * 2, [nM] * 2, 0, condition=True)
    assert method.tolist() == [0, -1] and nBig.tolist() == [1, 0] and nFr.tolist() == [0, 0]
    assert np.array_equal(bits(out[0]), bits(ex[0][0])) and not out[1].any() and np.isnan(lp[1])


# ---- 5. edges ------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_not_reserved_and_empty_batch(eng):
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    good = dense_frame(9, 3, 6)
    nLa, nMa, off = np.array([6], np.int32), np.array([3], np.int32), np.zeros(1, np.int64)
    probs, meth = np.zeros(3 * 7), np.zeros(1, np.int32)
    for k, max_exact, max_big, max_width in ((0, 16, 20, -1), (0, 16, 20, 17), (0, 16, 21, 16), (0, 17, 20, 16), (-1, 16, 20, 16)):
        rc = eng.lib.kbest_hybrid_frontier_probs_batch_f64(eng.ctx, 1, vp(nLa), vp(nMa), vp(good), vp(off), 0, k, max_exact, max_big,
                                                           max_width, vp(probs), vp(off), None, vp(meth), None, None, None, None)
        assert rc == BAD_ARG, (k, max_exact, max_big, max_width)
    for m in (0, 65):
        one = np.array([m], np.int32)
        rc = eng.lib.kbest_frontier_probs_f64_dev(eng.ctx, 1, vp(one), vp(nLa), vp(off), vp(off), C.c_void_p(8), C.c_void_p(8), None,
                                                  None, None, None)
        assert rc == BAD_ARG, m
    assert eng.lib.kbest_reserve_frontier(eng.ctx, 1, 65, 70) == BAD_ARG
    fresh = pk.KBestEngine(0)
    try:  # the asynchronous entry allocates nothing
        one = np.array([3], np.int32)
        rc = fresh.lib.kbest_frontier_probs_f64_dev(fresh.ctx, 1, vp(one), vp(nLa), vp(off), vp(off), C.c_void_p(8), C.c_void_p(8), None,
                                                    None, None, None)
        assert rc == NOT_RESERVED
    finally:
        fresh.close()
    assert eng.lib.kbest_hybrid_frontier_probs_batch_f64(eng.ctx, 0, None, None, None, None, 0, 0, 16, 20, 16, None, None, None, None,
                                                         None, None, None, None) == 0
    out, method, nOpen, nBig, maxc, lp, nFr = eng.hybrid_frontier_probs([], [], [], 0)
    assert out == [] and method.size == 0 and nFr.size == 0
    # a dense cluster has no narrow order: its 17 columns go on to the big-cluster tier, its 21 refuse the frame
    dense, wide = dense_frame(20, 17, 17), dense_frame(24, 21, 5)
    out, method, nOpen, nBig, maxc, lp, nFr = eng.hybrid_frontier_probs([dense, wide, good], [3, 3, 6], [17, 21, 3], 0)
    ex = eng.hybrid_exact_probs([dense, wide, good], [3, 3, 6], [17, 21, 3], 0)
    assert method.tolist() == [0, -1, 0] and nBig.tolist() == [1, 0, 0] and nFr.tolist() == [0, 0, 0]
    for j in range(3):
        assert np.array_equal(bits(out[j]), bits(ex[0][j]))
    assert np.array_equal(bits(lp), bits(ex[5]))


def test_cpp_shim_and_module_function(eng, tmp_path):
    exe = str(tmp_path / "shim_frontier")
    libdir = os.path.join(ROOT, "probabilisticsemslam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_frontier.cpp"), "-o", exe,
                           "-L", libdir, "-l:libkbest_amd.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
                           "-L/opt/rocm/lib", "-lamdhip64"])
    _, nL, nM, _ = MID
    frame = scene(*MID)[89]          # raw: a cluster of twenty-five measurements
    wide = dense_frame(24, 21, 5)    # ... and a dense one of twenty-one: refused with k = 0

    def write(name, blk, l, m):
        path = tmp_path / name
        path.write_text(f"{l} {m}\n" + "\n".join("inf" if np.isinf(v) else float.hex(float(v)) for v in blk) + "\n")
        return str(path)

    lines = subprocess.check_output([exe, "0", write("scene.txt", frame, nL, nM), write("wide.txt", wide, 3, 21)],
                                    text=True).splitlines()
    want = restated(MID, 89, condition=False)
    assert want[1] == 0 and want[3] == 1 and want[5] == 25
    (got,), method, nOpen, nBig, _, lp, nFr = eng.hybrid_frontier_probs([frame], [nL], [nM], 0)  # the C entry: the same doubles
    assert method[0] == 0 and nFr[0] == 1 and nBig[0] == 0
    np.testing.assert_allclose(got, want[0], rtol=0, atol=1e-12)
    assert abs(lp[0] - want[6]) <= 1e-12 * max(1.0, abs(want[6]))
    assert len(lines) == nM + 1
    for c in range(nM):
        tok = lines[c].split()
        assert tok[:2] == ["p", str(c)]
        assert np.array_equal(bits(np.array([float.fromhex(v) for v in tok[2:]])), bits(got[c])), c
    assert lines[-1].startswith("hybridFrontierProb: runtime_error") and "refused" in lines[-1]
    np.testing.assert_array_equal(pk.hybridFrontierProb(frame, nL, nM, 0), got)  # the package-level wrapper
    with pytest.raises(RuntimeError, match="refused"):
        pk.hybridFrontierProb(wide, 3, 21, 0)
    with pytest.raises(RuntimeError, match="refused"):  # (what the frame got before this tier)
        pk.hybridExactProb(frame, nL, nM, 0)
