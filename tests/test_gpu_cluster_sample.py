"""GPU: joint associations drawn from the exact posterior by gated clusters (kbest_cluster_sample.hip,
kbest_clustered_sample_assoc_batch_f64[_dev], the clusterSampleAssoc shim) against the numpy restatement of
tests/cluster_sample_check.py -- never against the kernel's own output.  The draws are compared for EXACT equality: the two sides
differ by the last bits of exp (about 1e-15 relative), so every case first asserts that the smallest relative margin of its
restatement, min |T - boundary| / tot over every decision, is at least 1e-10; then assign exactly and logProb within 1e-12."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import cluster_check as cc
import cluster_sample_check as cs
import oracle_lib as ol
import probabilisticsemslam_amd as pk
import sample_check as sc
from probabilisticsemslam_amd import workloads as wl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_MARGIN = 1e-10


@pytest.fixture(scope="module")
def eng():
    e = pk.KBestEngine(0)
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def check(got_assign, got_logp, want, n=None, lo=0):
    """One frame's draws lo .. lo+n-1 against the restatement: the margin first, then assign exactly and logProb within 1e-12."""
    n = len(got_assign) if n is None else n
    assert want.margin >= MIN_MARGIN, want.margin
    assert got_assign.dtype == np.int32 and got_assign.shape == want.assign[lo: lo + n].shape
    assert np.array_equal(got_assign, want.assign[lo: lo + n])
    assert np.abs(got_logp - want.logp[lo: lo + n]).max() <= 1e-12


def cross_check(eng, frames, nLs, nMs, condition, logPerm, info, maxc):
    """logPerm and maxCluster carry the bits of clustered_probs on every answered frame; info is its info."""
    _, lp, inf, mc = eng.clustered_probs(frames, nLs, nMs, condition=condition)
    assert np.array_equal(info, inf) and np.array_equal(maxc, mc)
    ans = inf > 0
    assert np.array_equal(bits(logPerm)[ans], bits(lp)[ans])


def run_scene(eng, shape, n, condition=False):
    F, nL, nM, side = shape
    frames = wl.scene_frames(F, nL, nM, side)
    want = cs.scene_draws(F, nL, nM, side, n, condition)
    asg, lp, logPerm, info, maxc = eng.clustered_sample_assoc(frames, [nL] * F, [nM] * F, n, seed=sc.SEED, condition=condition)
    print(f"{F} x {nL}+{nM} (side {side}): clusters {[w.info for w in want]}, largest {[w.maxc for w in want]}, "
          f"smallest margin {min(w.margin for w in want):.3g}")
    for b in range(F):
        check(asg[b], lp[b], want[b])
        assert info[b] == want[b].info and maxc[b] == want[b].maxc and abs(logPerm[b] - want[b].logperm) <= 1e-12 * max(1.0, abs(want[b].logperm))
    cross_check(eng, frames, [nL] * F, [nM] * F, condition, logPerm, info, maxc)
    return frames, asg, lp


# ---- 1. the small tier only; the same decisions as the whole-frame entry ----------------------------------------------------------
@pytest.mark.parametrize("condition", [False, True])
def test_small_tier_equals_sample_assoc(eng, condition):
    F, nL, nM = 6, 20, 10
    frames, asg, lp = run_scene(eng, (F, nL, nM, 12.0), 1024, condition)
    whole, whole_lp, _ = eng.sample_assoc(frames, [nL] * F, [nM] * F, 1024, seed=sc.SEED, condition=condition)  # (frame b: key b)
    for b in range(F):
        assert np.array_equal(asg[b], whole[b]), b
        assert np.abs(lp[b] - whole_lp[b]).max() <= 1e-12
    if condition:  # condition = 1 on the raw block against condition = 0 on its conditioned block: the same bits
        for b in (0, 3):
            blk, idx = ol.condition_costs(frames[b], nL + nM, nM)
            (a0,), (l0,), _, _, _ = eng.clustered_sample_assoc([blk], [len(idx) - nM], [nM], 1024, seed=sc.SEED, frame_key=[b])
            assert np.array_equal(np.asarray(idx)[a0], asg[b]) and np.array_equal(bits(l0), bits(lp[b]))


# ---- 2. beyond 16 measurements -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,n", [((6, 40, 24, 24.0), 512), ((4, 60, 40, 30.0), 256)])
def test_beyond_sixteen_measurements(eng, shape, n):
    """24 measurements: 8 to 12 clusters, small and workgroup tier mixed in label order.  40 measurements: frame 1 holds a cluster
    of 14 measurements and 34 rows -- the workgroup tier with 4.4 MB of layers in the work space -- beside one of 7 whose layers stay
    in the arena."""
    run_scene(eng, shape, n)
    if shape[2] == 40:
        assert cs.scene_draws(*shape, n)[1].maxc == 14


def test_assembled_frame(eng):
    f, nL, nM, parts, want = cs.assembled_draws(1024)
    (asg,), (lp,), logPerm, info, maxc = eng.clustered_sample_assoc([f], [nL], [nM], 1024, seed=sc.SEED, frame_key=[0])
    check(asg, lp, want)
    assert info[0] == 3 and maxc[0] == 6 and abs(logPerm[0] - want.logperm) <= 1e-12
    cross_check(eng, [f], [nL], [nM], False, logPerm, info, maxc)


# ---- 3. one cluster in the workgroup tier: the draws of the whole-frame restatement -------------------------------------------------
@pytest.mark.parametrize("which", ["12x8", "20x12", "20x13"])
def test_single_cluster_workgroup_tier(eng, which):
    """One dense cluster: the draws of sample_check.sample_assoc.  12 x 8: the entries and all 12 layers (24 KiB) in the LDS arena;
    20 x 12: the entries in the arena, the 640 KiB of layers in the work space; 20 x 13 (sample_check.wide_frame): 1.3 MB of
    layers there."""
    f, nL, nM, key, want = {"12x8": lambda: sc.dense_draws(12, 8, 813, 256), "20x12": lambda: sc.dense_draws(20, 12, 1213, 256),
                            "20x13": sc.wide_frame}[which]()
    print(f"{which}: margin {want.margin:.3g}")
    (asg,), (lp,), logPerm, info, maxc = eng.clustered_sample_assoc([f], [nL], [nM], want.n, seed=sc.SEED, frame_key=[key])
    check(asg, lp, want)
    assert info[0] == 1 and maxc[0] == nM and abs(logPerm[0] - np.log(want.Z)) <= 1e-12
    cross_check(eng, [f], [nL], [nM], False, logPerm, info, maxc)


# ---- 4. draw counts and continuation -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_draws():
    f = wl.scene_frames(1, 40, 24, 24.0)[0]
    f.setflags(write=False)
    return f, cs.clustered_sample_assoc(f, 40, 24, 5000, seed=sc.SEED, frame_key=0)


@pytest.mark.parametrize("n", [1, 63, 5000])
def test_sample_counts(eng, n):
    """Fewer than a wave, not a multiple of it, more than the workgroup: draws 0 .. n-1 of the same sequence."""
    f, want = long_draws()
    (asg,), (lp,), _, info, _ = eng.clustered_sample_assoc([f], [40], [24], n, seed=sc.SEED, frame_key=[0])
    check(asg, lp, want, n)
    assert info[0] == want.info


def test_sample_base_continues(eng):
    f, want = long_draws()
    (asg,), (lp,), _, _, _ = eng.clustered_sample_assoc([f], [40], [24], 904, seed=sc.SEED, frame_key=[0], sample_base=4096)
    check(asg, lp, want, 904, lo=4096)
    with pytest.raises(pk.KBestError):  # sampleBase + nSample <= 2^32
        eng.clustered_sample_assoc([f], [40], [24], 2, sample_base=2 ** 32 - 1)
    with pytest.raises(pk.KBestError):
        eng.clustered_sample_assoc([f], [40], [24], 0)


# ---- 5. batch independence, bitwise ------------------------------------------------------------------------------------------------
def test_batch_independence_bitwise(eng):
    rng = np.random.default_rng(2024)
    others, oL, oM = [], [], []
    for i in range(39):
        nM = 1 + i % 12
        nL = int(rng.integers(0, 41))
        others.append(rng.random((nL + nM) * nM) * 10.0)
        oL.append(nL)
        oM.append(nM)
    okeys = [int(k) for k in rng.integers(0, 2 ** 63, 39)]
    x = wl.scene_frames(5, 40, 24, 24.0)[4]
    key, n = 0xDEADBEEF12345, 300  # (a key beyond 32 bits: both words of the counter)
    want = cs.clustered_sample_assoc(x, 40, 24, n, seed=7, frame_key=key)
    (alone,), (alone_lp,), alone_perm, alone_info, _ = eng.clustered_sample_assoc([x], [40], [24], n, seed=7, frame_key=[key])
    check(alone, alone_lp, want)
    assert alone_info[0] == want.info
    blocks, nLs, nMs, keys = [x] + others, [40] + oL, [24] + oM, [key] + okeys
    first = eng.clustered_sample_assoc(blocks, nLs, nMs, n, seed=7, frame_key=keys)
    last = eng.clustered_sample_assoc(blocks[::-1], nLs[::-1], nMs[::-1], n, seed=7, frame_key=keys[::-1])
    slot = 64 * 16 * 8 + ((64 + 2) << 16) * 8  # work space of one frame in flight (kbest_c.h)
    need = max(((len(p.gidx) + 2) << len(p.cols)) * 8 for p in cs.cluster_parts(x, 40, 24)[0])
    try:
        eng.set_clustered_work_cap(slot + 64)
        capped = eng.clustered_sample_assoc(blocks, nLs, nMs, n, seed=7, frame_key=keys)
        assert eng.last_clustered_grid() == 1  # the cap took effect: one workgroup takes the 40 frames in turn
        eng.set_clustered_work_cap(0)
        eng.set_clustered_slot_cap(need)  # exactly enough for this frame (its dense neighbours of 12 columns are refused)
        slotted = eng.clustered_sample_assoc(blocks, nLs, nMs, n, seed=7, frame_key=keys)
        assert slotted[3][0] == want.info and (slotted[3][1:] == -3).any()
    finally:
        eng.set_clustered_work_cap(0)
        eng.set_clustered_slot_cap(0)
    for name, got, at in (("first", first, 0), ("reversed", last, 39), ("one frame in flight", capped, 0), ("slot cap", slotted, 0)):
        assert np.array_equal(got[0][at], alone), name
        assert np.array_equal(bits(got[1][at]), bits(alone_lp)) and bits(got[2][at]) == bits(alone_perm[0]), name
    # a neighbour in the mixed batch is right as well (12 columns, one dense cluster: the workgroup tier)
    b = 12
    wb = sc.Draws(*sc.sample_assoc(others[b - 1], oL[b - 1], oM[b - 1], n, seed=7, frame_key=okeys[b - 1]), n)
    check(first[0][b], first[1][b], wb)


# ---- 6. refusals and infeasible frames -----------------------------------------------------------------------------------------------
def test_slot_cap_refuses_one_frame(eng):
    shape, n = (4, 60, 40, 30.0), 256
    frames, want = wl.scene_frames(*shape), cs.scene_draws(*shape, n)
    need = max(((len(p.gidx) + 2) << len(p.cols)) * 8 for p in cs.cluster_parts(frames[1], 60, 40)[0])
    assert want[1].maxc == 14 and need >= (14 + 2) << 14 << 3
    try:
        eng.set_clustered_slot_cap(need - 8)  # just below the layers of the cluster of 14 measurements
        asg, lp, logPerm, info, maxc = eng.clustered_sample_assoc(frames, [60] * 4, [40] * 4, n, seed=sc.SEED)
    finally:
        eng.set_clustered_slot_cap(0)
    assert info.tolist() == [want[0].info, -3, want[2].info, want[3].info] and maxc[1] == 14
    assert (asg[1] == -1).all() and np.isnan(lp[1]).all() and np.isnan(logPerm[1])
    low = cs.clustered_sample_assoc(frames[1], 60, 40, 4, seed=sc.SEED, frame_key=1, slot_bytes=need - 8)
    assert low.info == -3 and (low.assign == -1).all()
    for b in (0, 2, 3):
        check(asg[b], lp[b], want[b])


def test_refusal_is_per_frame(eng):
    dense = wl.dense_batch(1, 20, 17, 17)[0] * 10.0
    frames, want = wl.scene_frames(2, 20, 10, 12.0), cs.scene_draws(6, 20, 10, 12.0, 1024)
    asg, lp, logPerm, info, maxc = eng.clustered_sample_assoc([frames[0], dense, frames[1]], [20, 3, 20], [10, 17, 10], 200,
                                                              seed=sc.SEED, frame_key=[0, 5, 1])
    assert info[1] == -2 and maxc[1] == 17 and (asg[1] == -1).all() and np.isnan(lp[1]).all() and np.isnan(logPerm[1])
    for at, b in ((0, 0), (2, 1)):
        check(asg[at], lp[at], want[b], 200)
        assert info[at] == want[b].info
    # 129 columns: the call is refused, and the context still answers
    with pytest.raises(pk.KBestError, match="128"):
        eng.clustered_sample_assoc([wl.dense_batch(1, 140, 129, 129)[0] * 10.0], [11], [129], 4)
    (again,), _, _, _, _ = eng.clustered_sample_assoc([frames[0]], [20], [10], 200, seed=sc.SEED, frame_key=[0])
    assert np.array_equal(again, asg[0])


def test_empty_column_gives_no_draw(eng):
    """The LAST column without a finite entry: the clusters before it have been walked when its Z_k = 0 turns up."""
    frames, want = wl.scene_frames(1, 20, 10, 12.0), cs.scene_draws(6, 20, 10, 12.0, 1024)
    bad = np.array(frames[0])
    bad[9 * 30:] = np.inf
    for condition in (False, True):
        asg, lp, logPerm, info, maxc = eng.clustered_sample_assoc([frames[0], bad, frames[0]], [20] * 3, [10] * 3, 200, seed=sc.SEED,
                                                                  condition=condition, frame_key=[0, 1, 0])
        assert info[1] == 0 and logPerm[1] == -np.inf and (asg[1] == -1).all() and np.isnan(lp[1]).all()
        assert info[0] > 0 and np.array_equal(asg[0], asg[2]) and np.array_equal(bits(lp[0]), bits(lp[2]))
        if not condition:
            check(asg[0], lp[0], want[0], 200)
    r = cs.clustered_sample_assoc(bad, 20, 10, 4)
    assert r.info == 0 and r.logperm == -np.inf


def dev_batch(blocks, nLs, nMs, n, keys=None, sentinel=-9):
    """The frames on the device as the _dev entry takes them; outputs prefilled with a sentinel."""
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    sizes = np.array([(l + m) * m for l, m in zip(nLs, nMs)], np.int64)
    coff = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    aoff = np.concatenate([[0], np.cumsum(np.asarray(nMs, np.int64) * n)[:-1]]).astype(np.int64)
    loff = np.arange(len(blocks), dtype=np.int64) * n
    B = len(blocks)
    return dict(B=B, d_nL=t(np.asarray(nLs, np.int32)), d_nM=t(np.asarray(nMs, np.int32)), d_cost=t(np.concatenate(blocks)),
                d_coff=t(coff), d_aoff=t(aoff), d_loff=t(loff), aoff=aoff, loff=loff,
                d_key=None if keys is None else t(np.asarray(keys, np.uint64).view(np.int64)),
                d_asg=torch.full((int(sum(nMs)) * n,), sentinel, dtype=torch.int32, device=dev),
                d_lp=torch.full((B * n,), float(sentinel), dtype=torch.float64, device=dev),
                d_logperm=torch.full((B,), float(sentinel), dtype=torch.float64, device=dev),
                d_info=torch.full((B,), sentinel, dtype=torch.int32, device=dev),
                d_maxc=torch.full((B,), sentinel, dtype=torch.int32, device=dev))


def test_frame_beyond_the_launch_bounds_is_left_alone(eng):
    import torch
    small, nL, nM, _, want = sc.dense_draws(9, 3, 6, 200)
    big = wl.dense_batch(1, 12, 5, 77)[0] * 10.0  # 5 columns and 12 rows in a launch sized for 3 and 9
    d = dev_batch([small, big, small], [nL, 7, nL], [nM, 5, nM], 200, keys=[0, 1, 0])
    eng.clustered_sample_assoc_dev(3, 9, 3, d["d_nL"], d["d_nM"], d["d_cost"], d["d_coff"], 200, d["d_asg"], d["d_aoff"], d["d_lp"],
                                   d["d_loff"], d["d_logperm"], d["d_info"], d["d_maxc"], seed=sc.SEED, d_frameKey=d["d_key"])
    torch.cuda.synchronize()
    asg, lp = d["d_asg"].cpu().numpy(), d["d_lp"].cpu().numpy()
    info, maxc, logperm = d["d_info"].cpu().numpy(), d["d_maxc"].cpu().numpy(), d["d_logperm"].cpu().numpy()
    assert info.tolist() == [1, -1, 1] and maxc[1] == -9 and logperm[1] == -9.0
    assert (asg[d["aoff"][1]: d["aoff"][2]] == -9).all() and (lp[200:400] == -9.0).all()
    for b in (0, 2):
        check(asg[d["aoff"][b]: d["aoff"][b] + 200 * nM].reshape(200, nM), lp[200 * b: 200 * b + 200], want)
        assert abs(logperm[b] - np.log(want.Z)) <= 1e-12 and maxc[b] == 3


# ---- 7. the device entry -------------------------------------------------------------------------------------------------------------
def test_dev_entry_reservation_and_stream():
    import torch
    e = pk.KBestEngine(0)  # a context of its own: nothing reserved yet
    try:
        f, want = long_draws()
        nL, nM, n = 40, 24, 600
        d1, d2 = dev_batch([f], [nL], [nM], 100, keys=[0]), dev_batch([f], [nL], [nM], n - 100, keys=[0])
        args = lambda d, ns, base, s: (e.ctx, 1, nL + nM, nM, C.c_void_p(d["d_nL"].data_ptr()), C.c_void_p(d["d_nM"].data_ptr()),  # noqa: E731
                                       C.c_void_p(d["d_cost"].data_ptr()), C.c_void_p(d["d_coff"].data_ptr()), 0, ns, sc.SEED, base,
                                       C.c_void_p(d["d_key"].data_ptr()), C.c_void_p(d["d_asg"].data_ptr()),
                                       C.c_void_p(d["d_aoff"].data_ptr()), C.c_void_p(d["d_lp"].data_ptr()),
                                       C.c_void_p(d["d_loff"].data_ptr()), C.c_void_p(d["d_logperm"].data_ptr()),
                                       C.c_void_p(d["d_info"].data_ptr()), C.c_void_p(d["d_maxc"].data_ptr()), s)
        assert e.lib.kbest_clustered_sample_assoc_batch_f64_dev(*args(d1, 100, 0, None)) == -6  # KBEST_ERR_NOT_RESERVED
        assert b"kbest_reserve_clustered_sample" in e.lib.kbest_last_error(e.ctx)
        e.reserve_clustered_sample(1, nL + nM, nM)
        s = torch.cuda.Stream(device=torch.device("cuda", 0))
        torch.cuda.synchronize()
        # two launches on the caller's stream, no synchronise in between: the second continues the first's sequence
        assert e.lib.kbest_clustered_sample_assoc_batch_f64_dev(*args(d1, 100, 0, C.c_void_p(s.cuda_stream))) == 0
        assert e.lib.kbest_clustered_sample_assoc_batch_f64_dev(*args(d2, n - 100, 100, C.c_void_p(s.cuda_stream))) == 0
        s.synchronize()
        check(d1["d_asg"].cpu().numpy().reshape(100, nM), d1["d_lp"].cpu().numpy(), want, 100)
        check(d2["d_asg"].cpu().numpy().reshape(n - 100, nM), d2["d_lp"].cpu().numpy(), want, n - 100, lo=100)
        assert bits(d1["d_logperm"].cpu().numpy()[0]) == bits(d2["d_logperm"].cpu().numpy()[0])
        assert d1["d_info"].cpu().numpy()[0] == want.info == d2["d_info"].cpu().numpy()[0]
    finally:
        e.close()


# ---- 8. the shim ---------------------------------------------------------------------------------------------------------------------
def test_cpp_shim_cluster_sample(eng, tmp_path):
    exe = str(tmp_path / "shim_cluster_sample")
    libdir = os.path.join(ROOT, "probabilisticsemslam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_cluster_sample.cpp"), "-o", exe,
                           "-L", libdir, "-l:libkbest_amd.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
                           "-L/opt/rocm/lib", "-lamdhip64"])
    f, want = long_draws()  # 40 + 24, frame key 0: the shim's
    nL, nM = 40, 24
    path = tmp_path / "frame.txt"
    path.write_text(f"{nL} {nM}\n" + "\n".join(float.hex(float(v)) for v in f) + "\n")
    lines = subprocess.check_output([exe, str(path), "200", str(sc.SEED)], text=True).splitlines()
    assert len(lines) == 201 and want.margin >= MIN_MARGIN
    got = np.array([[int(v) for v in ln.split()[2:]] for ln in lines[:200]])
    assert [ln.split()[:2] for ln in lines[:200]] == [["s", str(s)] for s in range(200)]
    assert np.array_equal(got, want.assign[:200])
    assert lines[-1].startswith("empty column: runtime_error")
    # the package-level wrapper
    assert np.array_equal(pk.clusterSampleAssoc(f, nL, nM, 200, sc.SEED), want.assign[:200])
    bad = np.array(f)
    bad[:nL + nM] = np.inf
    with pytest.raises(RuntimeError, match="no consistent association"):
        pk.clusterSampleAssoc(bad, nL, nM, 1)
    with pytest.raises(RuntimeError, match="17 measurements"):
        pk.clusterSampleAssoc(wl.dense_batch(1, 20, 17, 17)[0] * 10.0, 3, 17, 1)
