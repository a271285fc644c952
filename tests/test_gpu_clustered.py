"""GPU: the clustered exact association probabilities (kbest_cluster.hip, kbest_clustered_probs_batch_f64[_dev], the clusterProb
shim, exact_or_belief_probs) against the permutation sum and the numpy restatement of tests/cluster_check.py -- never against the
kernel's own output.  Probabilities 1e-12 absolute; logPerm 1e-12 x (number of clusters) absolute; info, maxCluster and labels
equal."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import cluster_check as cc
import oracle_lib as ol
import permanent_check as pc
import probabilisticsemslam_amd as pk
from probabilisticsemslam_amd import workloads as wl
from test_gpu_permanent import FRAME_SETS, bits, conditioned_sets, dense_frame

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    e = pk.KBestEngine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def scene_truth(F, nL, nM, side):
    """Raw scene frames and, per frame, the restatement on the conditioned block scattered back: (frames, [(probs, logPerm, info,
    maxCluster, label)]).  Computed once; nobody changes it."""
    frames = wl.scene_frames(F, nL, nM, side)
    want = []
    for f in frames:
        cond, idx = ol.condition_costs(f, nL + nM, nM)
        p, lp, info, maxc, lab = cc.clustered_probs(cond, len(idx) - nM, nM)
        want.append((pc.scatter_back(p, idx, nL, nM), lp, info, maxc, lab))
    return frames, want


def conditioned(frames, nL, nM):
    out = []
    for f in frames:
        cond, idx = ol.condition_costs(f, nL + nM, nM)
        out.append((cond, len(idx) - nM, nM))
    return out


def device_run(eng, frames, maxRawRow=None, maxCol=None, condition=False, fill=-5.0, stream=True):
    """The device entry on a stream of the caller's.  frames: [(block, nL, nM)].  Returns (probs list, logPerm, info, maxCluster,
    label [B, maxCol])."""
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
    d_probs = torch.full((int(psizes.sum()),), fill, dtype=torch.float64, device=dev)
    d_lp = torch.full((B,), fill, dtype=torch.float64, device=dev)
    d_info = torch.full((B,), -77, dtype=torch.int32, device=dev)
    d_maxc = torch.full((B,), -77, dtype=torch.int32, device=dev)
    d_lab = torch.full((B, maxCol), -77, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(device=dev) if stream else None
    torch.cuda.synchronize()
    eng.clustered_probs_dev(B, maxRawRow, maxCol, d_nL, d_nM, d_cost, d_coff, d_probs, d_poff, d_lp, d_info, d_maxc, d_lab, maxCol,
                            condition=condition, stream=s.cuda_stream if s else None)
    if s:
        s.synchronize()
    else:
        torch.cuda.synchronize()
    hp = d_probs.cpu().numpy()
    out = [hp[poff[b]: poff[b] + psizes[b]].reshape(nMs[b], nLs[b] + 1) for b in range(B)]
    return out, d_lp.cpu().numpy(), d_info.cpu().numpy(), d_maxc.cpu().numpy(), d_lab.cpu().numpy()


# ---- 1. truth at enumerable size ---------------------------------------------------------------------------------------------
def test_truth_at_enumerable_size(eng):
    blocks, cLs, nMs = conditioned_sets()
    assert len(blocks) == sum(F for F, _, _ in FRAME_SETS)
    for shape in ((5, 4, 5), (6, 5, 6)):
        for cond, cL, nM in conditioned(wl.scene_frames(40, *shape), shape[0], shape[1]):
            blocks.append(cond)
            cLs.append(cL)
            nMs.append(nM)
    out, lp, info, maxc = eng.clustered_probs(blocks, cLs, nMs)
    exact, perm = eng.permanent_probs(blocks, cLs, nMs)
    worst = worst_e = worst_z = 0.0
    split = 0
    for b, (blk, cL, nM) in enumerate(zip(blocks, cLs, nMs)):
        want, Z = pc.permutation_sum(blk, cL, nM)
        _, _, winfo, wmaxc, _ = cc.clustered_probs(blk, cL, nM)
        assert info[b] == winfo and maxc[b] == wmaxc and info[b] > 0, b
        split += info[b] > 1
        worst = max(worst, np.abs(out[b] - want).max())
        worst_e = max(worst_e, np.abs(out[b] - exact[b]).max())
        worst_z = max(worst_z, abs(lp[b] - np.log(Z)) / info[b], abs(lp[b] - np.log(perm[b])) / info[b])
    print(f"{len(blocks)} frames ({split} split): vs permutation sum {worst:.3g}, vs permanent_probs {worst_e:.3g}, "
          f"logPerm per cluster {worst_z:.3g}")
    assert worst <= 1e-12 and worst_e <= 1e-12 and worst_z <= 1e-12
    assert split >= 14  # (8 and 6 of the two scene sets)


# ---- 2. single cluster -------------------------------------------------------------------------------------------------------
def test_single_cluster_c5(eng):
    F, nL, nM = 64, 20, 10
    frames = wl.kitti_like_frames(F, nL=nL, nM=nM)
    out, lp, info, maxc = eng.clustered_probs(frames, [nL] * F, [nM] * F, condition=True)
    exact, perm = eng.permanent_probs(frames, [nL] * F, [nM] * F, condition=True)
    worst = worst_z = 0.0
    for b, f in enumerate(frames):
        cond, idx = ol.condition_costs(f, nL + nM, nM)
        A = np.asarray(pc.to_probs(cond)).reshape(nM, len(idx)).T
        clusters, _ = cc.clusters_of(A)
        assert info[b] == len(clusters) and maxc[b] == max(len(c) for c, _ in clusters), b
        dropped = np.setdiff1d(np.arange(nL), np.asarray(idx, dtype=np.int64))
        assert (out[b][:, dropped] == 0.0).all(), b  # exactly 0.0
        worst = max(worst, np.abs(out[b] - exact[b]).max())
        worst_z = max(worst_z, abs(lp[b] - np.log(perm[b])) / info[b])
    print(f"64 x 30x10 conditioned: vs permanent_probs {worst:.3g}, logPerm per cluster {worst_z:.3g}; "
          f"single cluster on {(info == 1).sum()} frames")
    assert worst <= 1e-12 and worst_z <= 1e-12
    assert (info == 1).sum() >= 50  # (55 by the restatement)


# ---- 3. beyond 16 measurements -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,refused,biggest", [((24, 40, 24, 24), {}, 15), ((16, 60, 40, 30), {1: 17}, 17),
                                                   ((6, 200, 128, 60), {5: 20}, 20), ((2, 896, 128, 127), {}, 7)])
def test_beyond_sixteen_measurements(eng, shape, refused, biggest):
    F, nL, nM, _ = shape
    frames, want = scene_truth(*shape)
    out, lp, info, maxc, lab = eng.clustered_probs(frames, [nL] * F, [nM] * F, condition=True, labels=True)
    assert {b: w[3] for b, w in enumerate(want) if w[2] < 0} == refused  # (the restatement itself: a condition of the test)
    assert max(w[3] for w in want) == biggest
    worst = worst_z = worst_row = 0.0
    for b, (wp, wlp, winfo, wmaxc, wlab) in enumerate(want):
        assert info[b] == winfo and maxc[b] == wmaxc, (b, info[b], winfo, maxc[b], wmaxc)
        np.testing.assert_array_equal(lab[b], wlab, err_msg=str(b))
        if b in refused:
            assert info[b] == -2 and maxc[b] == refused[b] and not out[b].any() and np.isnan(lp[b]), b
            continue
        worst = max(worst, np.abs(out[b] - wp).max())
        worst_z = max(worst_z, abs(lp[b] - wlp) / winfo)
        worst_row = max(worst_row, np.abs(out[b].sum(axis=1) - 1.0).max())
    print(f"{shape}: vs restatement {worst:.3g}, logPerm per cluster {worst_z:.3g}, rows - 1 {worst_row:.3g}, "
          f"clusters {info.tolist()}, largest {maxc.tolist()}")
    assert worst <= 1e-12 and worst_z <= 1e-12 and worst_row <= 1e-12


# ---- 4. the assembled frame ---------------------------------------------------------------------------------------------------
def test_assembled_frame_against_the_exact_entry(eng):
    big, nL, nM, parts = cc.assembled_frame()
    (p,), lp, info, maxc, lab = eng.clustered_probs([big], [nL], [nM], labels=True)
    assert info[0] == 3 and maxc[0] == 6
    np.testing.assert_array_equal(lab[0], np.arange(18) % 3)
    exact, perm = eng.permanent_probs([q[0] for q in parts], [q[1] for q in parts], [q[2] for q in parts])
    worst = 0.0
    for q, (_, cL, m) in enumerate(parts):
        got = np.zeros((m, cL + 1))
        got[:, :cL] = p[q::3, q:nL:3]
        got[:, cL] = p[q::3, nL]
        worst = max(worst, np.abs(got - exact[q]).max())
    print(f"assembled 36 x 18 frame vs permanent_probs on its parts {worst:.3g}")
    assert worst <= 1e-12
    assert abs(lp[0] - np.log(perm).sum()) <= 3e-12
    assert abs(p.sum() - 18.0) <= 1e-11


# ---- 5. refusal is per frame ---------------------------------------------------------------------------------------------------
def test_refusal_is_per_frame(eng):
    dense = dense_frame(20, 17, 17)
    (g0, l0, m0), (g1, l1, m1) = conditioned(wl.scene_frames(2, 20, 10, 12), 20, 10)
    out, lp, info, maxc = eng.clustered_probs([g0, dense, g1], [l0, 3, l1], [m0, 17, m1])  # (returns: KBEST_OK)
    assert info[1] == -2 and maxc[1] == 17 and not out[1].any() and np.isnan(lp[1])
    for got, glp, (blk, cL, nM) in ((out[0], lp[0], (g0, l0, m0)), (out[2], lp[2], (g1, l1, m1))):
        (alone,), lpa, ia, _ = eng.clustered_probs([blk], [cL], [nM])
        assert ia[0] > 0 and np.array_equal(bits(alone), bits(got)) and bits(lpa[0]) == bits(glp)
        np.testing.assert_allclose(alone, cc.clustered_probs(blk, cL, nM)[0], rtol=0, atol=1e-12)
    # 129 columns: the call is refused, and the context still answers
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    cost = wl.dense_batch(1, 140, 129, 129)[0] * 10.0
    nL, nM, off = np.array([11], np.int32), np.array([129], np.int32), np.zeros(1, np.int64)
    probs = np.zeros(129 * 12)
    rc = eng.lib.kbest_clustered_probs_batch_f64(eng.ctx, 1, vp(nL), vp(nM), vp(cost), vp(off), 0, vp(probs), vp(off), None, None,
                                                 None, None, 0)
    assert rc == -3  # KBEST_ERR_UNSUPPORTED
    assert b"128" in eng.lib.kbest_last_error(eng.ctx)
    with pytest.raises(pk.KBestError, match="1024"):  # 1 025 rows
        eng.clustered_probs([np.zeros(1025 * 2)], [1023], [2])
    (again,), _, _, _ = eng.clustered_probs([g0], [l0], [m0])
    assert np.array_equal(bits(again), bits(out[0]))


def test_frame_beyond_the_launch_bounds_and_reserve(eng):
    a = (dense_frame(9, 3, 21), 6, 3)
    wide = (dense_frame(9, 5, 22), 4, 5)
    tall = (dense_frame(12, 3, 23), 9, 3)
    out, lp, info, maxc, lab = device_run(eng, [a, wide, tall, a], maxRawRow=9, maxCol=3)
    assert info[1] == -1 and info[2] == -1 and info[0] == 1 and info[3] == 1
    assert (out[1] == -5.0).all() and (out[2] == -5.0).all() and maxc[1] == -77  # untouched
    np.testing.assert_allclose(out[0], pc.permanent_probs(*a)[0], rtol=0, atol=1e-12)
    assert np.array_equal(bits(out[0]), bits(out[3]))
    fresh = pk.KBestEngine(0)  # the device entry never allocates
    try:
        import torch
        z = torch.zeros(64, dtype=torch.float64, device="cuda:0")
        zi = torch.zeros(8, dtype=torch.int64, device="cuda:0")
        with pytest.raises(pk.KBestError, match="kbest_reserve_clustered"):
            fresh.clustered_probs_dev(1, 9, 3, zi, zi, z, zi, z, zi, reserve=False)
    finally:
        fresh.close()


# ---- 6. batch independence, bitwise ---------------------------------------------------------------------------------------------
def test_batch_independence_bitwise(eng):
    rng = np.random.default_rng(2024)
    others = []
    for i in range(256):
        nM = 1 + i % 12
        nL = int(rng.integers(0, 41))
        others.append((rng.random((nL + nM) * nM) * 10.0, nL, nM))
    frames, want = scene_truth(24, 40, 24, 24)
    xc, idx = ol.condition_costs(frames[10], 64, 24)  # (the frame whose largest cluster has 15 columns: layers in HBM)
    x = (xc, len(idx) - 24, 24)

    def run(batch):
        out, lp, info, maxc, lab = eng.clustered_probs([f[0] for f in batch], [f[1] for f in batch], [f[2] for f in batch],
                                                       labels=True)
        return out, lp, info, lab

    alone = run([x])
    first = run([x] + others)
    last = run(others + [x])
    dout, dlp, dinfo, _, dlab = device_run(eng, others[:100] + [x] + others[100:])
    assert alone[2][0] == want[10][2] > 0
    for name, got, glp, glab in (("first", first[0][0], first[1][0], first[3][0]), ("last", last[0][-1], last[1][-1], last[3][-1]),
                                 ("dev", dout[100], dlp[100], dlab[100])):
        assert np.array_equal(bits(alone[0][0]), bits(got)), name
        assert bits(alone[1][0]) == bits(glp), name
        np.testing.assert_array_equal(alone[3][0], glab[:24], err_msg=name)
    # the answer itself is right, and so are its neighbours in the mixed batch
    np.testing.assert_allclose(alone[0][0], cc.clustered_probs(*x)[0], rtol=0, atol=1e-12)
    for b in (1, 12, 60, 255):
        wb, _ = pc.permanent_probs(*others[b - 1])
        np.testing.assert_allclose(first[0][b], wb, rtol=0, atol=1e-12, err_msg=str(b))
        assert first[2][b] == 1


# ---- 7. caps ----------------------------------------------------------------------------------------------------------------------
def test_caps(eng):
    frames, want = scene_truth(24, 40, 24, 24)
    sel = [8, 9, 10, 11, 12, 13]
    batch, nLs, nMs = [frames[b] for b in sel], [40] * 6, [24] * 6
    whole = eng.clustered_probs(batch, nLs, nMs, condition=True, labels=True)
    assert eng.last_clustered_grid() == 6  # every frame in flight at once
    slot = 64 * 16 * 8 + ((64 + 2) << 16) * 8  # work space of one frame in flight (kbest_c.h)
    need = max(((len(rows) + 2) << len(cols)) * 8 for cols, rows in
               cc.clusters_of(np.asarray(pc.to_probs(ol.condition_costs(frames[10], 64, 24)[0])).reshape(24, -1).T)[0])
    assert need == (36 + 2) * (1 << 15) * 8
    try:
        eng.set_clustered_work_cap(2 * slot + 64)  # two frames in flight
        capped = eng.clustered_probs(batch, nLs, nMs, condition=True, labels=True)
        assert eng.last_clustered_grid() == 2
        for b in range(6):
            assert np.array_equal(bits(whole[0][b]), bits(capped[0][b])), b
        assert np.array_equal(bits(whole[1]), bits(capped[1])) and np.array_equal(whole[2], capped[2])
        np.testing.assert_array_equal(whole[4], capped[4])
        eng.set_clustered_work_cap(0)
        eng.set_clustered_slot_cap(need)  # exactly enough: nothing is refused
        exact = eng.clustered_probs(batch, nLs, nMs, condition=True)
        assert (exact[2] > 0).all()
        eng.set_clustered_slot_cap(need - 8)  # just below the largest cluster of frame 10
        low = eng.clustered_probs(batch, nLs, nMs, condition=True, labels=True)
    finally:
        eng.set_clustered_work_cap(0)
        eng.set_clustered_slot_cap(0)
    assert low[2].tolist() == [whole[2][0], whole[2][1], -3, whole[2][3], whole[2][4], whole[2][5]]
    assert not low[0][2].any() and np.isnan(low[1][2]) and low[3][2] == 15
    np.testing.assert_array_equal(low[4], whole[4])
    for b in (0, 1, 3, 4, 5):
        assert np.array_equal(bits(whole[0][b]), bits(low[0][b])) and bits(whole[1][b]) == bits(low[1][b]), b
        assert np.array_equal(bits(whole[0][b]), bits(exact[0][b])), b
    for j, b in enumerate(sel):  # and the answers are right
        np.testing.assert_allclose(whole[0][j], want[b][0], rtol=0, atol=1e-12)


# ---- 8. edges ---------------------------------------------------------------------------------------------------------------------
def test_single_column_and_no_landmarks(eng):
    col = np.array([0.5, 43.0, 2.0, 10.0, 7.0])  # nL = 4, nM = 1
    (p,), lp, info, maxc = eng.clustered_probs([col], [4], [1])
    w = np.where(col.min() + 42.0 > col, np.exp(col.min() - col), 0.0)
    np.testing.assert_allclose(p[0], w / w.sum(), rtol=1e-13, atol=0)
    assert info[0] == 1 and maxc[0] == 1 and abs(lp[0] - np.log(w.sum())) <= 1e-12
    diag = np.full(16, np.inf)  # nL = 0: every measurement has its miss row only -- all singletons, unassigned with certainty
    diag[::5] = [10.0, 3.0, 7.5, 10.0]
    (p,), lp, info, maxc, lab = eng.clustered_probs([diag], [0], [4], labels=True)
    assert p.shape == (4, 1) and (p == 1.0).all() and info[0] == 4 and maxc[0] == 1
    np.testing.assert_array_equal(lab[0], np.arange(4))
    np.testing.assert_allclose(lp[0], cc.clustered_probs(diag, 0, 4)[1], rtol=0, atol=4e-12)
    cost = dense_frame(4, 4, 99)  # nL = 0, one cluster of four
    (p,), lp, info, _ = eng.clustered_probs([cost], [0], [4])
    np.testing.assert_allclose(p, np.ones((4, 1)), rtol=0, atol=1e-12)
    assert info[0] == 1 and abs(lp[0] - np.log(pc.permanent_probs(cost, 0, 4)[1])) <= 1e-12


def test_infeasible_frames_give_zeros(eng):
    cost = dense_frame(9, 3, 5)
    cost[9:18] = np.inf  # an empty column
    good = dense_frame(9, 3, 6)
    for condition in (False, True):
        out, lp, info, maxc = eng.clustered_probs([good, cost, good], [6] * 3, [3] * 3, condition=condition)
        assert info[1] == 0 and lp[1] == -np.inf and not out[1].any() and not np.isnan(out[1]).any()
        assert info[0] == 1 and np.array_equal(bits(out[0]), bits(out[2]))
    forced = np.full(8, np.inf)  # 4 x 2: both columns can only take row 0
    forced[0] = forced[4] = 1.0
    (p,), lp, info, maxc = eng.clustered_probs([forced], [2], [2])
    assert info[0] == 0 and lp[0] == -np.inf and not p.any() and not np.isnan(p).any() and maxc[0] == 2
    # an infeasible cluster beside feasible ones: the whole frame is zeros
    two = np.full((5, 3), np.inf)  # nL = 2, nM = 3: columns 0 and 1 share their only row, column 2 is fine
    two[0, 0] = two[0, 1] = 1.0
    two[1, 2], two[4, 2] = 2.0, 10.0
    two = np.ascontiguousarray(two.T).reshape(-1)
    (p,), lp, info, maxc = eng.clustered_probs([two], [2], [3])
    assert info[0] == 0 and lp[0] == -np.inf and not p.any()
    assert cc.clustered_probs(two, 2, 3)[2] == 0


def test_strict_gate_decides_membership(eng):
    mn = 1.5

    def frame(x):  # nL = 1, nM = 2: row 0 joins the two columns iff x passes the gate
        return np.array([mn, 5.0, np.inf, x, np.inf, 6.0])

    out, lp, info, maxc, lab = eng.clustered_probs([frame(mn + 41.9999), frame(mn + 42.0)], [1, 1], [2, 2], labels=True)
    assert lab.tolist() == [[0, 0], [0, 1]] and info.tolist() == [1, 2] and maxc.tolist() == [2, 1]
    for b, x in enumerate((mn + 41.9999, mn + 42.0)):
        want, wlp, winfo, _, wlab = cc.clustered_probs(frame(x), 1, 2)
        assert winfo == info[b] and wlab.tolist() == lab[b].tolist()
        np.testing.assert_allclose(out[b], want, rtol=0, atol=1e-12)
        assert abs(lp[b] - wlp) <= 1e-12 * winfo
    assert out[0][1, 0] > 0.0 and out[1][1, 0] == 0.0 and out[1][1, 1] == 1.0


# ---- 9. the shim and the wrappers -------------------------------------------------------------------------------------------------
def test_cpp_shim_cluster(eng, tmp_path):
    exe = str(tmp_path / "shim_cluster")
    libdir = os.path.join(ROOT, "probabilisticsemslam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_cluster.cpp"), "-o", exe,
                           "-L", libdir, "-l:libkbest_amd.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
                           "-L/opt/rocm/lib", "-lamdhip64"])
    (cond, nL, nM), = conditioned(wl.scene_frames(1, 20, 10, 12), 20, 10)
    dense = dense_frame(20, 17, 17)

    def write(name, blk, l, m):
        path = tmp_path / name
        path.write_text(f"{l} {m}\n" + "\n".join("inf" if np.isinf(v) else float.hex(float(v)) for v in blk) + "\n")
        return str(path)

    lines = subprocess.check_output([exe, write("frame.txt", cond, nL, nM), write("dense.txt", dense, 3, 17)], text=True).splitlines()
    (want,), _, info, _ = eng.clustered_probs([cond], [nL], [nM])  # the C entry: the same doubles
    np.testing.assert_allclose(want, cc.clustered_probs(cond, nL, nM)[0], rtol=0, atol=1e-12)
    assert info[0] > 1 and len(lines) == nM + 1
    for c in range(nM):
        tok = lines[c].split()
        assert tok[:2] == ["p", str(c)]
        got = np.array([float.fromhex(v) for v in tok[2:]])
        assert np.array_equal(bits(got), bits(want[c])), c
    assert lines[-1].startswith("clusterProb: runtime_error") and "17" in lines[-1]
    np.testing.assert_array_equal(pk.clusterProb(cond, nL, nM), want)  # the package-level wrapper
    with pytest.raises(RuntimeError, match="17"):
        pk.clusterProb(dense, 3, 17)


# ---- 10. exact where possible, belief propagation elsewhere -----------------------------------------------------------------------
def test_exact_or_belief_probs(eng):
    F, nL, nM = 16, 60, 40
    frames, want = scene_truth(16, 60, 40, 30)
    out, method = eng.exact_or_belief_probs(frames, [nL] * F, [nM] * F, condition=True)
    exact, _, info, _ = eng.clustered_probs(frames, [nL] * F, [nM] * F, condition=True)
    (bp,), iters, _ = eng.belief_probs([frames[1]], [nL], [nM], condition=True)
    assert method.tolist() == [0] + [1] + [0] * 14 and iters[0] > 0
    for b in range(F):
        assert np.array_equal(bits(out[b]), bits(bp if b == 1 else exact[b])), b
    assert np.abs(out[1].sum(axis=1) - 1.0).max() <= 1e-9
