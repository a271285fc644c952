"""CPU: the numpy restatement of the belief-propagation association probabilities (tests/lbp_check.py) against the exact
marginals of tests/permanent_check.py; the library exports beliefProb and its C entries; without a GPU they fail loudly."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import lbp_check as lc
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


def conflict_free_frame(rng, nL, nM):
    """Every landmark is plausible for ONE measurement only (and every measurement has its miss row): the columns are independent."""
    nR = nL + nM
    cost = np.full(nR * nM, np.inf)
    for r in range(nL):
        cost[int(rng.integers(0, nM)) * nR + r] = rng.random() * 12.0
    for c in range(nM):
        cost[c * nR + nL + c] = 10.0
    return cost


def test_exclusive_sums_have_no_subtraction():
    x = np.array([[1.0, np.inf, 0.0], [2.0, 3.0, 0.0], [4.0, 5.0, 0.0]])
    s = lc.exclusive_sums(x, 0)
    assert not np.isnan(s).any()
    np.testing.assert_array_equal(s[:, 0], [6.0, 5.0, 3.0])
    np.testing.assert_array_equal(s[:, 1], [8.0, np.inf, np.inf])  # the forced entry's own sum stays finite
    np.testing.assert_array_equal(lc.exclusive_sums(x, 1)[1], [3.0, 2.0, 5.0])
    np.testing.assert_array_equal(lc.exclusive_sums(np.ones((1, 3)), 0), np.zeros((1, 3)))


def test_single_column_is_the_normalised_column():
    rng = np.random.default_rng(11)
    for nL in (0, 1, 4, 40):
        col = rng.random(nL + 1) * 50.0  # the last row is the miss
        p, iters, resid = lc.belief_probs(col, nL, 1)
        w = pc.to_probs(col)
        np.testing.assert_allclose(p[0], w / w.sum(), rtol=0, atol=1e-15)
        assert iters == 1 and resid == 0.0


def test_conflict_free_frames_are_exact():
    rng = np.random.default_rng(12)
    worst = 0.0
    for nL, nM in ((6, 3), (12, 5), (20, 10), (30, 12)):
        for _ in range(10):
            cost = conflict_free_frame(rng, nL, nM)
            p, iters, _ = lc.belief_probs(cost, nL, nM)
            worst = max(worst, np.abs(p - lc.exact_probs(cost, nL, nM)).max())
            assert iters == 1
    print(f"conflict-free frames vs exact {worst:.3g}")
    assert worst <= 1e-12


def test_c5_quality_beats_k200():
    truth = json.load(open(os.path.join(ROOT, "profiles", "exact_truth_c5.json")))
    k200 = truth["shapes"]["30x10"]["k"]["200"]["median"]
    err, its = [], []
    for f in wl.kitti_like_frames(200, nL=20, nM=10):
        cond, idx = ol.condition_costs(f, 30, 10)
        cL = len(idx) - 10
        p, iters, resid = lc.belief_probs(cond, cL, 10)
        assert iters > 0 and resid <= 1e-12
        assert np.abs(p.sum(axis=1) - 1.0).max() <= 1e-12
        err.append(np.abs(p - lc.exact_probs(cond, cL, 10)).max())
        its.append(iters)
    err = np.array(err)
    print(f"200 C5 frames vs exact: median {np.median(err):.4g} p95 {np.quantile(err, 0.95):.3g} max {err.max():.3g} "
          f"frames > 0.1: {(err > 0.1).sum()}; sweeps median {np.median(its):.0f} max {max(its)}; k = 200 median {k200:.3g}")
    assert np.median(err) < k200


def test_crowded_family_converges():
    rng = np.random.default_rng(5)
    its = []
    for _ in range(10):
        cost = lc.crowded_frame(rng)
        p, iters, resid = lc.belief_probs(cost, 8, 8, tol=1e-12, max_iter=10000)
        assert 0 < iters < 10000 and resid <= 1e-12
        assert np.abs(p.sum(axis=1) - 1.0).max() <= 1e-12
        its.append(iters)
    print(f"crowded 8+8 frames: sweeps {min(its)} .. {max(its)}")


def test_infeasible_frames_give_zeros():
    cost = wl.dense_batch(1, 9, 3, 5)[0] * 10.0
    cost[9:18] = np.inf  # a column without a finite entry
    p, iters, _ = lc.belief_probs(cost, 6, 3)
    assert iters == lc.INFEASIBLE and not p.any()
    forced = np.full(8, np.inf)  # 4 x 2: both columns can only take row 0
    forced[0] = forced[4] = 1.0
    p, iters, _ = lc.belief_probs(forced, 2, 2)
    assert iters == lc.INFEASIBLE and not p.any() and not np.isnan(p).any()


def test_library_exports_belief_entries(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pk.lib_path()], text=True)
    assert "_Z10beliefProbRKSt6vectorIdSaIdEEmm" in out
    raw = C.CDLL(pk.lib_path())
    for sym in ("kbest_belief_probs_batch_f64", "kbest_belief_probs_batch_f64_dev", "kbest_reserve_belief",
                "kbest_set_belief_lds_limit"):
        assert hasattr(raw, sym), sym
    assert callable(pk.beliefProb) and hasattr(pk.KBestEngine, "belief_probs") and hasattr(pk.KBestEngine, "belief_probs_dev")


def test_belief_without_gpu_fails_loudly(lib):
    if lib.kbest_device_count() > 0:
        return  # (a GPU is present: tests/test_gpu_lbp.py has the rest)
    with pytest.raises(pk.KBestError):
        pk.beliefProb(np.random.rand(12), 2, 3)
