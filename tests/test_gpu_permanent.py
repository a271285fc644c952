"""GPU: the exact association probabilities (kbest_perm.hip, kbest_permanent_probs_batch_f64[_dev], the permanentProb shim)
against the permutation sum and the numpy restatement of tests/permanent_check.py -- never against the kernel's own output."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import permanent_check as pc
import probabilisticsemslam_amd as pk
from probabilisticsemslam_amd import workloads as wl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME_SETS = ((40, 6, 3), (20, 5, 4), (6, 6, 5))  # (frames, nL, nM) of kitti_like_frames: small enough to enumerate


@pytest.fixture(scope="module")
def eng():
    e = pk.KBestEngine(0)
    yield e
    e.close()


def conditioned_sets():
    blocks, cLs, nMs = [], [], []
    for F, nL, nM in FRAME_SETS:
        for f in wl.kitti_like_frames(F, nL=nL, nM=nM):
            cond, idx = ol.condition_costs(f, nL + nM, nM)
            blocks.append(cond)
            cLs.append(len(idx) - nM)
            nMs.append(nM)
    return blocks, cLs, nMs


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def dense_frame(nR, nM, seed):
    return wl.dense_batch(1, nR, nM, seed)[0] * 10.0


# ---- 1. truth at enumerable size ---------------------------------------------------------------------------------------------
def test_truth_at_enumerable_size(eng):
    blocks, cLs, nMs = conditioned_sets()
    out, perm = eng.permanent_probs(blocks, cLs, nMs, condition=False)
    worst = worst_bf = worst_z = 0.0
    want, Zs = [], []
    for blk, cL, nM in zip(blocks, cLs, nMs):
        w, Z = pc.permutation_sum(blk, cL, nM)
        want.append(w)
        Zs.append(Z)
    # the engine's own exhaustive enumeration, frame set by frame set (k: every assignment of the set's largest frame, at most
    # bruteForceProb's own cap of 20 000, assignment.cpp:868)
    bf = []
    lo = 0
    for F, nL, nM in FRAME_SETS:
        k = min(20000, int(np.prod(np.arange(nL + 1, nL + nM + 1))))
        o, _ = eng.weights(blocks[lo: lo + F], cLs[lo: lo + F], nMs[lo: lo + F], k, brute_force=True)
        bf += o
        lo += F
    for b in range(len(blocks)):
        worst = max(worst, np.abs(out[b] - want[b]).max())
        worst_bf = max(worst_bf, np.abs(out[b] - bf[b]).max())
        worst_z = max(worst_z, abs(perm[b] - Zs[b]) / Zs[b])
    print(f"engine vs permutation sum {worst:.3g}, perm rel {worst_z:.3g}, vs the engine's brute force {worst_bf:.3g}")
    for b in range(len(blocks)):
        np.testing.assert_allclose(out[b], want[b], rtol=0, atol=1e-12, err_msg=str(b))
        np.testing.assert_allclose(perm[b], Zs[b], rtol=1e-12, atol=0, err_msg=str(b))
        np.testing.assert_allclose(out[b], bf[b], rtol=0, atol=1e-12, err_msg=str(b))


# ---- 2. production size ------------------------------------------------------------------------------------------------------
def test_production_size_conditioned_batch(eng):
    F, nL, nM = 1000, 20, 10
    nR = nL + nM
    frames = wl.kitti_like_frames(F, nL=nL, nM=nM)
    out, perm = eng.permanent_probs(frames, [nL] * F, [nM] * F, condition=True)
    worst = worst_row = 0.0
    for b, f in enumerate(frames):
        p = out[b]
        cond, idx = ol.condition_costs(f, nR, nM)
        assert not np.isnan(p).any() and (p >= 0.0).all(), b
        worst_row = max(worst_row, np.abs(p.sum(axis=1) - 1.0).max())
        dropped = np.setdiff1d(np.arange(nL), np.asarray(idx, dtype=np.int64))
        assert (p[:, dropped] == 0.0).all(), b  # exactly 0.0
        if b % 8 == 0:
            cp, Z = pc.permanent_probs(cond, len(idx) - nM, nM)
            want = pc.scatter_back(cp, idx, nL, nM)
            worst = max(worst, np.abs(p - want).max())
            assert abs(perm[b] - Z) <= 1e-12 * Z, b
    print(f"1000 x 30x10 conditioned: every 8th frame vs helper {worst:.3g}, rows - 1 {worst_row:.3g}")
    assert worst <= 1e-12 and worst_row <= 1e-12


# ---- 3. toProbs is the project's toProbs --------------------------------------------------------------------------------------
def test_to_probs_is_the_projects(eng):
    frames = wl.kitti_like_frames(20, nL=20, nM=10, seed=77)
    blocks, cLs = [], []
    for f in frames:
        cond, idx = ol.condition_costs(f, 30, 10)
        blocks.append(cond)
        cLs.append(len(idx) - 10)
    out, _ = eng.permanent_probs(blocks, cLs, [10] * 20)
    worst = 0.0
    for b in range(20):
        a = eng.to_probs(blocks[b])
        want, _ = pc.permanent_probs(blocks[b], cLs[b], 10, a=a)
        worst = max(worst, np.abs(out[b] - want).max())
    print(f"helper on engine.to_probs vs engine.permanent_probs {worst:.3g}")
    assert worst <= 1e-12
    # the gate is strict (assignment.cpp:536): min + 42 > c
    mn = 1.5
    cost = np.array([mn, mn + 41.9999, mn + 42.0, mn + 50.0, 3.0, 4.0, 5.0, 6.0])  # 4 x 2, nL = 2
    (p,), _ = eng.permanent_probs([cost], [2], [2])
    want, _ = pc.permanent_probs(cost, 2, 2)
    assert p[0, 1] > 0.0 and p[0, 2] == 0.0
    np.testing.assert_allclose(p, want, rtol=0, atol=1e-12)
    # (rows 2 and 3 each: a 4 x 2 frame with nL = 4 rows of landmarks keeps them apart)
    cost6 = np.concatenate([cost[:4], [np.inf, np.inf], cost[4:], [np.inf, np.inf]])  # 6 x 2, nL = 4
    (p,), _ = eng.permanent_probs([cost6], [4], [2])
    assert p[0, 1] > 0.0 and p[0, 2] == 0.0 and p[0, 3] == 0.0


# ---- 4. batch independence, bitwise -------------------------------------------------------------------------------------------
def test_batch_independence_bitwise(eng):
    import torch
    rng = np.random.default_rng(2024)
    others, oL, oM = [], [], []
    for i in range(256):
        nM = 1 + i % 12
        nL = int(rng.integers(0, 41))
        others.append(rng.random((nL + nM) * nM) * 10.0)
        oL.append(nL)
        oM.append(nM)
    x = wl.kitti_like_frames(3, nL=20, nM=10, seed=4242)[2]
    xc, idx = ol.condition_costs(x, 30, 10)
    xL, xM = len(idx) - 10, 10
    (alone,), perm_alone = eng.permanent_probs([xc], [xL], [xM])
    first, perm_first = eng.permanent_probs([xc] + others, [xL] + oL, [xM] + oM)
    last, perm_last = eng.permanent_probs(others + [xc], oL + [xL], oM + [xM])
    # the device entry on a stream of the caller's, x in the middle of the batch
    blocks, nLs, nMs = others[:100] + [xc] + others[100:], oL[:100] + [xL] + oL[100:], oM[:100] + [xM] + oM[100:]
    B = len(blocks)
    sizes = np.array([(l + m) * m for l, m in zip(nLs, nMs)], np.int64)
    psizes = np.array([m * (l + 1) for l, m in zip(nLs, nMs)], np.int64)
    coff = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    poff = np.concatenate([[0], np.cumsum(psizes)[:-1]]).astype(np.int64)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_cost, d_coff, d_poff = t(np.concatenate(blocks)), t(coff), t(poff)
    d_nL, d_nM = t(np.asarray(nLs, np.int32)), t(np.asarray(nMs, np.int32))
    d_probs = torch.full((int(psizes.sum()),), -1.0, dtype=torch.float64, device=dev)
    d_perm = torch.full((B,), -1.0, dtype=torch.float64, device=dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    eng.permanent_probs_dev(B, max(l + m for l, m in zip(nLs, nMs)), max(nMs), d_nL, d_nM, d_cost, d_coff, d_probs, d_poff, d_perm,
                            condition=False, stream=s.cuda_stream)
    s.synchronize()
    hp, hperm = d_probs.cpu().numpy(), d_perm.cpu().numpy()
    mid = hp[poff[100]: poff[100] + psizes[100]].reshape(xM, xL + 1)
    for name, got, pm in (("first", first[0], perm_first[0]), ("last", last[-1], perm_last[-1]), ("dev", mid, hperm[100])):
        assert np.array_equal(bits(alone), bits(got)), name
        assert bits(perm_alone[0]) == bits(pm), name
    # the answer itself is right, and so are its neighbours in the mixed batch
    want, Z = pc.permanent_probs(xc, xL, xM)
    np.testing.assert_allclose(alone, want, rtol=0, atol=1e-12)
    for b in (1, 12, 60, 255):
        wb, _ = pc.permanent_probs(others[b - 1], oL[b - 1], oM[b - 1])
        np.testing.assert_allclose(first[b], wb, rtol=0, atol=1e-12, err_msg=str(b))


# ---- 5. edges ---------------------------------------------------------------------------------------------------------------------
def test_single_column_and_no_landmarks(eng):
    col = np.array([0.5, 43.0, 2.0, 10.0, 7.0])  # nL = 4, nM = 1
    (p,), perm = eng.permanent_probs([col], [4], [1])
    w = np.where(col.min() + 42.0 > col, np.exp(col.min() - col), 0.0)
    np.testing.assert_allclose(p[0], w / w.sum(), rtol=1e-13, atol=0)
    np.testing.assert_allclose(perm[0], w.sum(), rtol=1e-13)
    cost = dense_frame(4, 4, 99)  # nL = 0: every measurement is unassigned with certainty
    (p,), perm = eng.permanent_probs([cost], [0], [4])
    assert p.shape == (4, 1)
    np.testing.assert_allclose(p, np.ones((4, 1)), rtol=0, atol=1e-12)
    np.testing.assert_allclose(perm[0], pc.permanent_probs(cost, 0, 4)[1], rtol=1e-12)


def test_empty_column_gives_zeros(eng):
    cost = dense_frame(9, 3, 5)
    cost[9:18] = np.inf
    good = dense_frame(9, 3, 6)
    for condition in (False, True):
        out, perm = eng.permanent_probs([good, cost, good], [6] * 3, [3] * 3, condition=condition)
        assert perm[1] == 0.0 and not out[1].any() and not np.isnan(out[1]).any()
        assert perm[0] > 0.0 and np.array_equal(bits(out[0]), bits(out[2]))
    # fewer usable rows than columns
    few = np.full(12, np.inf)
    few[0] = few[4] = few[8] = 1.0  # 4 x 3, only row 0 is finite
    (p,), perm = eng.permanent_probs([few], [1], [3])
    assert perm[0] == 0.0 and not p.any()


@pytest.mark.parametrize("nM", [13, 16])
def test_hbm_layers(eng, nM):
    cost = dense_frame(20, nM, 1300 + nM)
    (p,), perm = eng.permanent_probs([cost], [20 - nM], [nM])
    want, Z = pc.permanent_probs(cost, 20 - nM, nM)
    print(f"nM = {nM}: vs helper {np.abs(p - want).max():.3g}, perm rel {abs(perm[0] - Z) / Z:.3g}")
    np.testing.assert_allclose(p, want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(perm[0], Z, rtol=1e-12)


def test_seventeen_columns_unsupported(eng):
    cost = dense_frame(20, 17, 17)
    nL, nM, off = np.array([3], np.int32), np.array([17], np.int32), np.zeros(1, np.int64)
    probs, perm = np.zeros(17 * 4), np.zeros(1)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = eng.lib.kbest_permanent_probs_batch_f64(eng.ctx, 1, vp(nL), vp(nM), vp(cost), vp(off), 0, vp(probs), vp(off), vp(perm))
    assert rc == -3  # KBEST_ERR_UNSUPPORTED
    assert b"16" in eng.lib.kbest_last_error(eng.ctx)
    with pytest.raises(pk.KBestError):
        eng.permanent_probs([cost], [3], [17])
    # the context still answers
    f = wl.kitti_like_frames(1, nL=6, nM=3)[0]
    cond, idx = ol.condition_costs(f, 9, 3)
    (p,), _ = eng.permanent_probs([cond], [len(idx) - 3], [3])
    np.testing.assert_allclose(p, pc.permutation_sum(cond, len(idx) - 3, 3)[0], rtol=0, atol=1e-12)


def test_chunked_batch_equals_unchunked(eng):
    nR, nM, B = 18, 14, 7
    blocks = [dense_frame(nR, nM, 1400 + i) for i in range(B)]
    whole, perm_whole = eng.permanent_probs(blocks, [nR - nM] * B, [nM] * B)
    assert eng.last_permanent_grid() == B  # every frame in flight at once
    slot = (nR * nM + ((nR + 2) << nM)) * 8  # work space of one frame in flight (kbest_c.h)
    eng.set_permanent_work_cap(2 * slot + 64)  # two frames in flight: chunks of two
    try:
        chunked, perm_chunked = eng.permanent_probs(blocks, [nR - nM] * B, [nM] * B)
        assert eng.last_permanent_grid() == 2  # the cap took effect: two workgroups took the seven frames in turn
    finally:
        eng.set_permanent_work_cap(0)
    for b in range(B):
        assert np.array_equal(bits(whole[b]), bits(chunked[b])), b
    assert np.array_equal(bits(perm_whole), bits(perm_chunked))
    want, _ = pc.permanent_probs(blocks[B - 1], nR - nM, nM)
    np.testing.assert_allclose(chunked[B - 1], want, rtol=0, atol=1e-12)


# ---- 6. the shim ------------------------------------------------------------------------------------------------------------------
def test_cpp_shim_permanent(eng, tmp_path):
    exe = str(tmp_path / "shim_permanent")
    libdir = os.path.join(ROOT, "probabilisticsemslam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_permanent.cpp"), "-o", exe,
                           "-L", libdir, "-l:libkbest_amd.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
                           "-L/opt/rocm/lib", "-lamdhip64"])
    f = wl.kitti_like_frames(1, nL=8, nM=4)[0]
    cond, idx = ol.condition_costs(f, 12, 4)
    nL, nM = len(idx) - 4, 4
    path = tmp_path / "frame.txt"
    path.write_text(f"{nL} {nM}\n" + "\n".join("inf" if np.isinf(v) else float.hex(float(v)) for v in cond) + "\n")
    lines = subprocess.check_output([exe, str(path)], text=True).splitlines()
    (want,), _ = eng.permanent_probs([cond], [nL], [nM])  # the C entry: the same doubles
    truth, _ = pc.permutation_sum(cond, nL, nM)
    np.testing.assert_allclose(want, truth, rtol=0, atol=1e-12)
    assert len(lines) == 3 * nM + 1
    for opt in range(3):
        for c in range(nM):
            tok = lines[opt * nM + c].split()
            assert tok[:3] == ["p", str(opt), str(c)]
            got = np.array([float.fromhex(v) for v in tok[3:]])
            assert np.array_equal(bits(got), bits(want[c])), (opt, c)
    assert lines[-1].startswith("permOpt 3: runtime_error")
    # the package-level wrapper
    np.testing.assert_array_equal(pk.permanentProb(cond, nL, nM, 1), want)
    with pytest.raises(RuntimeError):
        pk.permanentProb(cond, nL, nM, 3)


# ---- 7. convergence: the reason for the feature -------------------------------------------------------------------------------
def test_kbest_converges_to_exact(eng):
    F, nL, nM = 64, 20, 10
    frames = wl.kitti_like_frames(F, nL=nL, nM=nM)
    exact, _ = eng.permanent_probs(frames, [nL] * F, [nM] * F, condition=True)
    err = {}
    for k in (200, 1000):
        p, _ = eng.weights(frames, [nL] * F, [nM] * F, k, condition=True)
        err[k] = np.array([np.abs(p[b] - exact[b]).max() for b in range(F)])
    ok = int((err[1000] <= err[200]).sum())
    print(f"max |assoc_probs(k) - exact| on 64 frames 30x10: k = 200 median {np.median(err[200]):.3g} max {err[200].max():.3g}; "
          f"k = 1000 median {np.median(err[1000]):.3g} max {err[1000].max():.3g}; non-increasing on {ok} of {F}")
    assert ok >= 60
    small = wl.kitti_like_frames(40, nL=6, nM=3)
    exact, _ = eng.permanent_probs(small, [6] * 40, [3] * 40, condition=True)
    p, _ = eng.weights(small, [6] * 40, [3] * 40, 200, condition=True)  # exhaustive there
    worst = max(np.abs(p[b] - exact[b]).max() for b in range(40))
    print(f"6x3 frames, k = 200 vs exact: {worst:.3g}")
    assert worst < 1e-12
