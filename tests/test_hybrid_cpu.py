"""CPU: the numpy restatement of the hybrid association probabilities (tests/hybrid_check.py) against the clustered restatement
(tests/cluster_check.py) where every cluster can be answered exactly, and against whole-frame assignmentProb of the pinned CPU
oracle; the library exports hybridProb and its C entries; without a GPU they fail loudly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cluster_check as cc
import hybrid_check as hc
import oracle_lib as ol
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


@pytest.mark.parametrize("shape", [(12, 8, 8), (20, 10, 12)])
def test_nothing_open_is_the_clustered_restatement(shape):
    for cond, cL, nM in conditioned_scene(12, *shape):
        p, method, opens, info, maxc, lab = hc.hybrid_probs(cond, cL, nM, 200)
        wp, _, winfo, wmaxc, wlab = cc.clustered_probs(cond, cL, nM)
        assert winfo > 0 and method == 0 and not opens and info == winfo and maxc == wmaxc
        np.testing.assert_array_equal(lab, wlab)
        assert np.array_equal(p.view(np.int64), wp.view(np.int64))  # exactly


def test_condition_while_loading_is_the_conditioned_block():
    nL, nM = 20, 10
    for f in wl.scene_frames(6, nL, nM, 12):
        cond, idx = ol.condition_costs(f, nL + nM, nM)
        cL = len(idx) - nM
        p, method, opens, _, _, _ = hc.hybrid_probs(f, nL, nM, 300, condition=True, max_exact=4)
        q, qmethod, qopens, _, _, _ = hc.hybrid_probs(cond, cL, nM, 300, max_exact=4)
        assert method == qmethod and len(opens) == len(qopens)
        for o, w in zip(opens, qopens):  # the same sub-blocks, bit for bit: conditionCosts only drops rows no cluster holds
            assert (o["m"], o["nL"], o["nf"]) == (w["m"], w["nL"], w["nf"])
            assert np.array_equal(o["block"].view(np.int64), w["block"].view(np.int64))
            np.testing.assert_array_equal(o["rows"], np.asarray(idx)[w["rows"]])
        back = np.zeros((nM, nL + 1))
        back[:, np.asarray(idx[:cL], dtype=np.int64)] = q[:, :cL]
        back[:, nL] = q[:, cL]
        np.testing.assert_array_equal(p, back)


def test_lowered_cap_on_small_scene():
    k = 1000
    opened = complete = 0
    worst = 0.0
    for cond, cL, nM in conditioned_scene(24, 20, 10, 12):
        p, method, opens, info, _, _ = hc.hybrid_probs(cond, cL, nM, k, max_exact=4)
        exact, _, winfo, _, _ = cc.clustered_probs(cond, cL, nM)
        assert winfo > 0 and info == winfo and len(opens) <= 2
        assert all(o["m"] > 4 and o["block"].size == (o["nL"] + o["m"]) * o["m"] for o in opens)
        if not opens:
            assert method == 0
            continue
        opened += 1
        assert method == (1 if all(o["nf"] < k for o in opens) else 2)
        assert np.abs(p.sum(axis=1) - 1.0).max() <= 1e-12
        if method == 1:  # everything within the cutoff was weighed: what is left out weighs below e^-42 each
            complete += 1
            worst = max(worst, np.abs(p - exact).max())
    print(f"(20, 10, 12) x 24, max_exact 4, k {k}: {opened} frames with an open cluster, {complete} complete, worst {worst:.3g}")
    assert opened == 20 and complete == 4
    assert worst <= 1e-12


def test_closer_than_whole_frame_kbest():
    k = 200
    mine, whole = [], []
    for cond, cL, nM in conditioned_scene(60, 40, 24, 24):
        p, method, opens, _, _, _ = hc.hybrid_probs(cond, cL, nM, k, max_exact=8)
        if not opens:
            continue
        exact, _, winfo, _, _ = cc.clustered_probs(cond, cL, nM)
        assert winfo > 0 and method in (1, 2)
        mine.append(np.abs(p - exact).max())
        whole.append(np.abs(ol.assignment_prob(cond, cL, nM, k)[0] - exact).max())
    print(f"(40, 24, 24) x 60, max_exact 8, k {k}: {len(mine)} open frames; per-cluster k-best median {np.median(mine):.3g} "
          f"p95 {np.percentile(mine, 95):.3g} max {max(mine):.3g}; whole-frame median {np.median(whole):.3g} "
          f"p95 {np.percentile(whole, 95):.3g} max {max(whole):.3g}")
    assert len(mine) == 17
    assert np.median(mine) < np.median(whole)


def test_refusal_and_infeasible_of_the_restatement():
    inf = np.inf
    # three rows >= nL on two columns: not the reference's layout
    blk = np.array([[inf, inf, 1.0], [1.0, 1.5, inf], [2.0, 1.0, inf], [1.0, 3.0, inf]])  # nL = 1, nM = 3: rows 1 .. 3 are >= nL
    p, method, opens, info, _, _ = hc.hybrid_probs(np.ascontiguousarray(blk.T).reshape(-1), 1, 3, 10, max_exact=1)
    assert method == -1 and info == -2 and not opens and not p.any()
    # two columns whose only finite entry is the same row: the open cluster has no assignment
    blk = np.array([[1.0, 2.0], [inf, inf], [inf, inf], [inf, inf]])  # nL = 2, nM = 2
    p, method, opens, _, _, _ = hc.hybrid_probs(np.ascontiguousarray(blk.T).reshape(-1), 2, 2, 10, max_exact=1)
    assert method == -2 and len(opens) == 1 and opens[0]["nf"] == 0 and not p.any()


def test_library_exports_hybrid_entries(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pk.lib_path()], text=True)
    assert "_Z10hybridProbRKSt6vectorIdSaIdEEmmm" in out
    raw = C.CDLL(pk.lib_path())
    for sym in ("kbest_clustered_partial_batch_f64_dev", "kbest_hybrid_probs_batch_f64"):
        assert hasattr(raw, sym), sym
    assert callable(pk.hybridProb)
    for name in ("hybrid_probs", "clustered_partial_dev"):
        assert hasattr(pk.KBestEngine, name), name


def test_hybrid_without_gpu_fails_loudly(lib):
    if lib.kbest_device_count() > 0:
        return  # (a GPU is present: tests/test_gpu_hybrid.py has the rest)
    with pytest.raises(pk.KBestError):
        pk.hybridProb(np.random.rand(12), 2, 3, 10)
