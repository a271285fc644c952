"""CPU: the numpy restatement of the exact association probabilities (tests/permanent_check.py) against the permutation sum
and the oracle's bruteForceProb; the library exports permanentProb and its C entries; without a GPU they fail loudly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import permanent_check as pc
import probabilisticsemslam_amd as pk
from probabilisticsemslam_amd import workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME_SETS = ((40, 6, 3), (20, 5, 4), (6, 6, 5))  # (frames, nL, nM) of kitti_like_frames: small enough to enumerate


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pk.lib_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "probabilisticsemslam_amd", "csrc")])
    return pk.load_library()


def conditioned_sets():
    for F, nL, nM in FRAME_SETS:
        for f in wl.kitti_like_frames(F, nL=nL, nM=nM):
            cond, idx = ol.condition_costs(f, nL + nM, nM)
            yield cond, len(idx) - nM, nM


def test_subset_sums_equal_permutation_sum_and_brute_force():
    worst_p = worst_b = worst_row = 0.0
    for cond, cL, nM in conditioned_sets():
        p, Z = pc.permanent_probs(cond, cL, nM)
        pp, Zp = pc.permutation_sum(cond, cL, nM)
        pb, _, _ = ol.brute_force_prob(cond, cL, nM)
        worst_p = max(worst_p, np.abs(p - pp).max())
        worst_b = max(worst_b, np.abs(p - pb).max())
        worst_row = max(worst_row, np.abs(p.sum(axis=1) - 1.0).max())
        np.testing.assert_allclose(Z, Zp, rtol=1e-12)
    print(f"subset sums vs permutation sum {worst_p:.3g}, vs brute_force_prob {worst_b:.3g}, rows - 1 {worst_row:.3g}")
    assert worst_p <= 1e-12 and worst_b <= 1e-12 and worst_row <= 1e-12


def test_helper_on_dense_frames_rows_sum_to_one():
    # dense 20-row frames with costs in [0, 10): every subset is populated
    for nM in (12, 13):
        cost = wl.dense_batch(1, 20, nM, 0x5EED0000 + nM)[0] * 10.0
        p, Z = pc.permanent_probs(cost, 20 - nM, nM)
        assert Z > 0.0 and np.abs(p.sum(axis=1) - 1.0).max() <= 1e-12


def test_helper_gate_and_empty_column():
    nL, nM = 2, 2
    cost = np.array([1.0, 1.0 + 41.9999, 1.0 + 42.0, 51.0, 2.0, 3.0, 4.0, 5.0])
    a = pc.to_probs(cost)
    assert a[0] == 1.0 and a[1] > 0.0 and a[2] == 0.0 and a[3] == 0.0  # 42 > c - min is strict (assignment.cpp:536)
    p, Z = pc.permanent_probs(cost, nL, nM)
    assert p[0, 1] > 0.0 and p[0, 2] == 0.0
    cost[4:] = np.inf
    p, Z = pc.permanent_probs(cost, nL, nM)
    assert Z == 0.0 and not p.any()


def test_library_exports_permanent_entries(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pk.lib_path()], text=True)
    assert "_Z13permanentProbSt6vectorIdSaIdEEmmi" in out  # assignment.h:13, by value
    raw = C.CDLL(pk.lib_path())
    for sym in ("kbest_permanent_probs_batch_f64", "kbest_permanent_probs_batch_f64_dev", "kbest_reserve_permanent"):
        assert hasattr(raw, sym), sym


def test_permanent_without_gpu_fails_loudly(lib):
    if lib.kbest_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(pk.KBestError):
        pk.permanentProb(np.random.rand(12), 2, 3, 1)
