"""GPU: joint associations drawn from the exact posterior (kbest_sample.hip, kbest_sample_assoc_batch_f64[_dev], the sampleAssoc
shim) against the numpy restatement of tests/sample_check.py -- never against the kernel's own output.  The draws are compared for
EXACT equality: the two sides differ by the last bits of exp (about 1e-15 relative), so every case first asserts that the smallest
relative margin of its restatement, min |T - boundary| / tot over every decision, is at least 1e-10."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

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


# ---- 1. every layer in LDS (mode 0) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sc.FRAME_SETS)
def test_frame_sets_in_lds(eng, shape):
    F, nL, nM = shape
    frames = wl.kitti_like_frames(F, nL=nL, nM=nM)
    want = sc.reference_draws(F, nL, nM)
    asg, lp, perm = eng.sample_assoc(frames, [nL] * F, [nM] * F, sc.N_DRAWS, seed=sc.SEED, condition=True)  # (frame b: key b)
    _, perm_exact = eng.permanent_probs(frames, [nL] * F, [nM] * F, condition=True)
    print(f"{F} x {nL + nM}x{nM}: smallest margin {min(w.margin for w in want):.3g}")
    for b in range(F):
        check(asg[b], lp[b], want[b])
    assert np.array_equal(bits(perm), bits(perm_exact))
    lone, lone_lp, _ = eng.sample_assoc(frames[F - 1:], [nL], [nM], sc.N_DRAWS, seed=sc.SEED, condition=True, frame_key=[F - 1])
    assert np.array_equal(lone[0], asg[F - 1]) and np.array_equal(bits(lone_lp[0]), bits(lp[F - 1]))


# ---- 2. the layers in the work space (modes 1 and 2), more rows than threads --------------------------------------------------------
@pytest.mark.parametrize("nR,nM,n", [(20, 12, 256), (20, 13, 256), (20, 16, 64), (304, 4, 512)])
def test_layers_outside_lds(eng, nR, nM, n):
    """12 columns: the two sweep layers fill the LDS a frame may take, the F layers go to the work space (mode 1); 13: a layer no
    longer fits LDS (mode 2); 4 + 16: 10 MB of layers; 300 + 4: more active rows than the workgroup has threads (64), layers of
    304 rows outside LDS."""
    f, nL, _, key, want = sc.dense_draws(nR, nM, 100 * nM + 13, n)
    print(f"{nR}x{nM}: margin {want.margin:.3g}")
    (asg,), (lp,), perm = eng.sample_assoc([f], [nL], [nM], n, seed=sc.SEED, frame_key=[key])
    check(asg, lp, want)
    _, perm_exact = eng.permanent_probs([f], [nL], [nM])
    assert bits(perm[0]) == bits(perm_exact[0]) and abs(perm[0] - want.Z) <= 1e-12 * want.Z


# ---- 3. sample counts and sampleBase ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 5000])
def test_sample_counts(eng, n):
    """Fewer than a wave, not a multiple of it, more than the workgroup: draws 0 .. n-1 of the same sequence."""
    F, nL, nM = sc.FRAME_SETS[1]
    frames = wl.kitti_like_frames(F, nL=nL, nM=nM)
    want = sc.reference_draws(F, nL, nM, 5000)
    asg, lp, _ = eng.sample_assoc(frames, [nL] * F, [nM] * F, n, seed=sc.SEED, condition=True)
    for b in range(F):
        check(asg[b], lp[b], want[b], n)


def test_sample_base_continues(eng):
    F, nL, nM = sc.FRAME_SETS[1]
    frames = wl.kitti_like_frames(F, nL=nL, nM=nM)
    want = sc.reference_draws(F, nL, nM, 5000)
    asg, lp, _ = eng.sample_assoc(frames, [nL] * F, [nM] * F, 904, seed=sc.SEED, condition=True, sample_base=4096)
    for b in range(F):
        check(asg[b], lp[b], want[b], 904, lo=4096)
    with pytest.raises(pk.KBestError):  # sampleBase + nSample <= 2^32
        eng.sample_assoc(frames, [nL] * F, [nM] * F, 2, sample_base=2 ** 32 - 1)
    with pytest.raises(pk.KBestError):
        eng.sample_assoc(frames, [nL] * F, [nM] * F, 0)


# ---- 4. batch independence, bitwise ----------------------------------------------------------------------------------------------
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
    x = wl.kitti_like_frames(3, nL=20, nM=10, seed=4242)[2]
    key, n = 0xDEADBEEF12345, 300  # (a key beyond 32 bits: both words of the counter)
    want = sc.Draws(*sc.sample_assoc(x, 20, 10, n, seed=7, condition=True, frame_key=key), n)
    (alone,), (alone_lp,), alone_perm = eng.sample_assoc([x], [20], [10], n, seed=7, condition=True, frame_key=[key])
    check(alone, alone_lp, want)
    blocks, nLs, nMs, keys = [x] + others, [20] + oL, [10] + oM, [key] + okeys
    first = eng.sample_assoc(blocks, nLs, nMs, n, seed=7, condition=True, frame_key=keys)
    last = eng.sample_assoc(blocks[::-1], nLs[::-1], nMs[::-1], n, seed=7, condition=True, frame_key=keys[::-1])
    maxR, maxC = max(l + m for l, m in zip(nLs, nMs)), max(nMs)
    slot = (maxR * maxC + ((maxR + 2) << maxC)) * 8  # work space of one frame in flight (kbest_c.h)
    eng.set_permanent_work_cap(slot + 64)
    try:
        capped = eng.sample_assoc(blocks, nLs, nMs, n, seed=7, condition=True, frame_key=keys)
        eng.permanent_probs(blocks, nLs, nMs, condition=True)
        assert eng.last_permanent_grid() == 1  # the cap took effect on this shape: one workgroup takes the 40 frames in turn
    finally:
        eng.set_permanent_work_cap(0)
    for name, got, at in (("first", first, 0), ("reversed", last, 39), ("one frame in flight", capped, 0)):
        assert np.array_equal(got[0][at], alone), name
        assert np.array_equal(bits(got[1][at]), bits(alone_lp)) and bits(got[2][at]) == bits(alone_perm[0]), name
    # a neighbour in the mixed batch is right as well (12 columns, not conditioned by the caller: condition = 1 on a dense block)
    b = 12
    wb = sc.Draws(*sc.sample_assoc(others[b - 1], oL[b - 1], oM[b - 1], n, seed=7, condition=True, frame_key=okeys[b - 1]), n)
    check(first[0][b], first[1][b], wb)


# ---- 5. degenerate frames ---------------------------------------------------------------------------------------------------------
def test_empty_column_gives_no_draw(eng):
    cost = wl.dense_batch(1, 9, 3, 5)[0] * 10.0
    cost[9:18] = np.inf  # column 1 without a finite entry
    good, nL, nM, _, want = sc.dense_draws(9, 3, 6, 200)
    for condition in (False, True):
        asg, lp, perm = eng.sample_assoc([good, cost, good], [6] * 3, [3] * 3, 200, seed=sc.SEED, condition=condition, frame_key=[0, 1, 0])
        assert perm[1] == 0.0 and (asg[1] == -1).all() and np.isnan(lp[1]).all()
        assert perm[0] > 0.0 and np.array_equal(asg[0], asg[2]) and np.array_equal(bits(lp[0]), bits(lp[2]))
        if not condition:
            check(asg[0], lp[0], want)


def dev_batch(blocks, nLs, nMs, n, keys=None, sentinel=-9):
    """The frames on the device as the _dev entry takes them; outputs prefilled with a sentinel."""
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    sizes = np.array([(l + m) * m for l, m in zip(nLs, nMs)], np.int64)
    coff = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    aoff = np.concatenate([[0], np.cumsum(np.asarray(nMs, np.int64) * n)[:-1]]).astype(np.int64)
    loff = np.arange(len(blocks), dtype=np.int64) * n
    return dict(B=len(blocks), d_nL=t(np.asarray(nLs, np.int32)), d_nM=t(np.asarray(nMs, np.int32)), d_cost=t(np.concatenate(blocks)),
                d_coff=t(coff), d_aoff=t(aoff), d_loff=t(loff), aoff=aoff, loff=loff,
                d_key=None if keys is None else t(np.asarray(keys, np.uint64).view(np.int64)),
                d_asg=torch.full((int(sum(nMs)) * n,), sentinel, dtype=torch.int32, device=dev),
                d_lp=torch.full((len(blocks) * n,), float(sentinel), dtype=torch.float64, device=dev),
                d_perm=torch.full((len(blocks),), float(sentinel), dtype=torch.float64, device=dev))


def test_frame_beyond_the_launch_bounds_is_left_alone(eng):
    import torch
    small, nL, nM, _, want = sc.dense_draws(9, 3, 6, 200)
    big = wl.dense_batch(1, 12, 5, 77)[0] * 10.0  # 5 columns and 12 rows in a launch sized for 3 and 9
    d = dev_batch([small, big, small], [nL, 7, nL], [nM, 5, nM], 200, keys=[0, 1, 0])
    eng.sample_assoc_dev(3, 9, 3, d["d_nL"], d["d_nM"], d["d_cost"], d["d_coff"], 200, d["d_asg"], d["d_aoff"], d["d_lp"], d["d_loff"],
                         d["d_perm"], seed=sc.SEED, d_frameKey=d["d_key"])
    torch.cuda.synchronize()
    asg, lp, perm = d["d_asg"].cpu().numpy(), d["d_lp"].cpu().numpy(), d["d_perm"].cpu().numpy()
    assert perm[1] == 0.0 and (asg[d["aoff"][1]: d["aoff"][2]] == -9).all() and (lp[200:400] == -9.0).all()
    for b in (0, 2):
        check(asg[d["aoff"][b]: d["aoff"][b] + 200 * nM].reshape(200, nM), lp[200 * b: 200 * b + 200], want)
        assert abs(perm[b] - want.Z) <= 1e-12 * want.Z


# ---- 6. the device entry ------------------------------------------------------------------------------------------------------------
def test_dev_entry_reservation_and_stream():
    import torch
    e = pk.KBestEngine(0)  # a context of its own: nothing reserved yet
    try:
        f, nL, nM, key, want = sc.wide_frame()  # 13 columns: the layers need the work space
        n = want.n
        d1, d2 = dev_batch([f], [nL], [nM], 100, keys=[key]), dev_batch([f], [nL], [nM], n - 100, keys=[key])
        args = lambda d, ns, base, s: (e.ctx, 1, nL + nM, nM, C.c_void_p(d["d_nL"].data_ptr()), C.c_void_p(d["d_nM"].data_ptr()),  # noqa: E731
                                       C.c_void_p(d["d_cost"].data_ptr()), C.c_void_p(d["d_coff"].data_ptr()), 0, ns, sc.SEED, base,
                                       C.c_void_p(d["d_key"].data_ptr()), C.c_void_p(d["d_asg"].data_ptr()),
                                       C.c_void_p(d["d_aoff"].data_ptr()), C.c_void_p(d["d_lp"].data_ptr()),
                                       C.c_void_p(d["d_loff"].data_ptr()), C.c_void_p(d["d_perm"].data_ptr()), s)
        assert e.lib.kbest_sample_assoc_batch_f64_dev(*args(d1, 100, 0, None)) == -6  # KBEST_ERR_NOT_RESERVED
        assert b"kbest_reserve_sample" in e.lib.kbest_last_error(e.ctx)
        e.reserve_sample(1, nL + nM, nM)
        s = torch.cuda.Stream(device=torch.device("cuda", 0))
        torch.cuda.synchronize()
        # two launches on the caller's stream, no synchronise in between: the second continues the first's sequence
        assert e.lib.kbest_sample_assoc_batch_f64_dev(*args(d1, 100, 0, C.c_void_p(s.cuda_stream))) == 0
        assert e.lib.kbest_sample_assoc_batch_f64_dev(*args(d2, n - 100, 100, C.c_void_p(s.cuda_stream))) == 0
        s.synchronize()
        check(d1["d_asg"].cpu().numpy().reshape(100, nM), d1["d_lp"].cpu().numpy(), want, 100)
        check(d2["d_asg"].cpu().numpy().reshape(n - 100, nM), d2["d_lp"].cpu().numpy(), want, n - 100, lo=100)
        assert bits(d1["d_perm"].cpu().numpy()[0]) == bits(d2["d_perm"].cpu().numpy()[0])
        # 17 measurements: unsupported, by the entry and by the wrapper; the context still answers
        assert e.lib.kbest_sample_assoc_batch_f64_dev(e.ctx, 1, 20, 17, *args(d1, 100, 0, None)[4:]) == -3  # KBEST_ERR_UNSUPPORTED
        assert b"16" in e.lib.kbest_last_error(e.ctx)
        with pytest.raises(pk.KBestError):
            e.sample_assoc([wl.dense_batch(1, 20, 17, 17)[0] * 10.0], [3], [17], 4)
        (asg,), (lp,), _ = e.sample_assoc([f], [nL], [nM], 50, seed=sc.SEED, frame_key=[key])
        check(asg, lp, want, 50)
    finally:
        e.close()


# ---- 7. the shim ------------------------------------------------------------------------------------------------------------------
def test_cpp_shim_sample(eng, tmp_path):
    exe = str(tmp_path / "shim_sample")
    libdir = os.path.join(ROOT, "probabilisticsemslam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_sample.cpp"), "-o", exe,
                           "-L", libdir, "-l:libkbest_amd.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
                           "-L/opt/rocm/lib", "-lamdhip64"])
    f, nL, nM, key, want = sc.dense_draws(9, 3, 6, 200)  # (frame key 0: the shim's)
    path = tmp_path / "frame.txt"
    path.write_text(f"{nL} {nM}\n" + "\n".join(float.hex(float(v)) for v in f) + "\n")
    lines = subprocess.check_output([exe, str(path), "200", str(sc.SEED)], text=True).splitlines()
    assert len(lines) == 201 and want.margin >= MIN_MARGIN
    got = np.array([[int(v) for v in ln.split()[2:]] for ln in lines[:200]])
    assert [ln.split()[:2] for ln in lines[:200]] == [["s", str(s)] for s in range(200)]
    assert np.array_equal(got, want.assign)
    assert lines[-1].startswith("empty column: runtime_error")
    # the package-level wrapper
    assert np.array_equal(pk.sampleAssoc(f, nL, nM, 200, sc.SEED), want.assign)
    bad = np.array(f)
    bad[:9] = np.inf
    with pytest.raises(RuntimeError):
        pk.sampleAssoc(bad, nL, nM, 1)
