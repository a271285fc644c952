"""CPU: the numpy restatement of the clustered exact association probabilities (tests/cluster_check.py) against the whole-frame
subset sums and the permutation sum of tests/permanent_check.py; the scene generator's pins; the library exports clusterProb and
its C entries; without a GPU they fail loudly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cluster_check as cc
import oracle_lib as ol
import permanent_check as pc
import probabilisticsemslam_amd as pk
from probabilisticsemslam_amd import workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pk.lib_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "probabilisticsemslam_amd", "csrc")])
    return pk.load_library()


def conditioned_scene(F, nL, nM, side):
    out = []
    for f in wl.scene_frames(F, nL, nM, side):
        cond, idx = ol.condition_costs(f, nL + nM, nM)
        out.append((cond, len(idx) - nM, nM))
    return out


@pytest.mark.parametrize("shape,split", [((12, 8, 8), 8), ((20, 10, 12), 35)])
def test_restatement_against_whole_frame_subset_sums(shape, split):
    worst = worst_z = worst_row = 0.0
    multi = 0
    for cond, cL, nM in conditioned_scene(40, *shape):
        p, lp, info, maxc, lab = cc.clustered_probs(cond, cL, nM)
        want, Z = pc.permanent_probs(cond, cL, nM)
        assert info > 0 and maxc <= nM
        multi += info > 1
        worst = max(worst, np.abs(p - want).max())
        worst_z = max(worst_z, abs(lp - np.log(Z)))
        worst_row = max(worst_row, np.abs(p.sum(axis=1) - 1.0).max())
    print(f"{shape}: clustered vs whole-frame {worst:.3g}, logPerm {worst_z:.3g}, rows - 1 {worst_row:.3g}, {multi} of 40 split")
    assert worst <= 1e-12 and worst_z <= 1e-12 * nM and worst_row <= 1e-12
    assert multi == split


@pytest.mark.parametrize("shape,split", [((5, 4, 5), 8), ((6, 5, 6), 6)])
def test_restatement_against_permutation_sum(shape, split):
    worst = 0.0
    multi = 0
    for cond, cL, nM in conditioned_scene(40, *shape):
        p, lp, info, _, _ = cc.clustered_probs(cond, cL, nM)
        want, Z = pc.permutation_sum(cond, cL, nM)
        multi += info > 1
        worst = max(worst, np.abs(p - want).max())
        assert abs(lp - np.log(Z)) <= 1e-12 * info
    print(f"{shape}: clustered vs permutation sum {worst:.3g}, {multi} of 40 split")
    assert worst <= 1e-12
    assert multi == split


def test_labels_against_transitive_closure():
    frames = conditioned_scene(20, 20, 10, 12) + conditioned_scene(6, 40, 24, 24) + [cc.assembled_frame()[:3]]
    for cond, cL, nM in frames:
        A = np.asarray(pc.to_probs(cond)).reshape(nM, cL + nM).T > 0.0
        adj = (A.T.astype(np.int64) @ A.astype(np.int64)) > 0
        adj |= np.eye(nM, dtype=bool)
        for _ in range(nM):  # transitive closure of the boolean column adjacency
            adj = (adj.astype(np.int64) @ adj.astype(np.int64)) > 0
        want = np.array([np.flatnonzero(adj[c])[0] for c in range(nM)], dtype=np.int32)
        np.testing.assert_array_equal(cc.labels_of(A.astype(np.float64)), want)


def test_assembled_frame_gives_its_parts():
    big, nL, nM, parts = cc.assembled_frame()
    p, lp, info, maxc, lab = cc.clustered_probs(big, nL, nM)
    assert info == 3 and maxc == 6
    np.testing.assert_array_equal(lab, np.arange(18) % 3)
    worst = 0.0
    lps = 0.0
    for q, (blk, cL, m) in enumerate(parts):
        want, Z = pc.permanent_probs(blk, cL, m)
        got = np.zeros((m, cL + 1))
        got[:, :cL] = p[q::3, q:nL:3]
        got[:, cL] = p[q::3, nL]
        worst = max(worst, np.abs(got - want).max())
        lps += np.log(Z)
        others = np.ones(nL + 1, bool)  # nothing of another part's landmarks
        others[q:nL:3] = False
        others[nL] = False
        assert not p[q::3][:, others].any()
    print(f"assembled 36 x 18 frame vs its three parts {worst:.3g}")
    assert worst <= 1e-12 and abs(lp - lps) <= 3e-12


def test_refusals_of_the_restatement():
    cost = wl.dense_batch(1, 20, 17, 17)[0] * 10.0
    p, lp, info, maxc, _ = cc.clustered_probs(cost, 3, 17)
    assert info == cc.REFUSED_SIZE and maxc == 17 and np.isnan(lp) and not p.any()
    (cond, cL, nM), = conditioned_scene(1, 20, 10, 12)
    _, _, info, _, _ = cc.clustered_probs(cond, cL, nM, slot_bytes=64)
    assert info == cc.REFUSED_SLOT
    empty = wl.dense_batch(1, 9, 3, 5)[0] * 10.0
    empty[9:18] = np.inf
    p, lp, info, _, _ = cc.clustered_probs(empty, 6, 3)
    assert info == 0 and lp == -np.inf and not p.any()


def test_scene_generator_pins():
    f = wl.scene_frames(3, 20, 10, 12)[0]
    assert f.shape == (300,) and abs(f[np.isfinite(f)].sum() - 34724.1659447) <= 1e-6
    g = wl.scene_frames(2, 5, 4, 5)[0]
    assert abs(g[np.isfinite(g)].sum() - 536.078418871) <= 1e-8
    np.testing.assert_array_equal(wl.scene_frames(1, 20, 10, 12)[0], f)  # the first frames do not depend on F
    blk = f.reshape(10, 30).T
    assert np.isfinite(blk[:20]).all() and (np.diag(blk[20:]) == 10.0).all() and np.isinf(blk[20:]).sum() == 90
    with pytest.raises(ValueError):
        wl.scene_frames(1, 4, 5, 5)


def test_library_exports_clustered_entries(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pk.lib_path()], text=True)
    assert "_Z11clusterProbRKSt6vectorIdSaIdEEmm" in out
    raw = C.CDLL(pk.lib_path())
    for sym in ("kbest_clustered_probs_batch_f64", "kbest_clustered_probs_batch_f64_dev", "kbest_reserve_clustered",
                "kbest_set_clustered_slot_cap", "kbest_set_clustered_work_cap", "kbest_last_clustered_grid"):
        assert hasattr(raw, sym), sym
    assert callable(pk.clusterProb)
    for name in ("clustered_probs", "clustered_probs_dev", "reserve_clustered", "set_clustered_slot_cap", "set_clustered_work_cap",
                 "last_clustered_grid", "exact_or_belief_probs"):
        assert hasattr(pk.KBestEngine, name), name


def test_clustered_without_gpu_fails_loudly(lib):
    if lib.kbest_device_count() > 0:
        return  # (a GPU is present: tests/test_gpu_clustered.py has the rest)
    with pytest.raises(pk.KBestError):
        pk.clusterProb(np.random.rand(12), 2, 3)
