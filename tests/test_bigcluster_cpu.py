"""CPU: the numpy restatement of the big-cluster tier (tests/bigcluster_check.py) against the clustered restatement where both
answer, its invariance under a shift of a cluster's costs, the sizes of the oversized clusters the GPU tests rely on; the library
exports hybridExactProb and its C entries; without a GPU they fail loudly."""
import functools
import os
import subprocess

import numpy as np
import pytest

import bigcluster_check as bc
import cluster_check as cc
import hybrid_check as hc
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


@functools.lru_cache(maxsize=None)
def conditioned_scene(F, nL, nM, side):
    out = []
    for f in wl.scene_frames(F, nL, nM, side):
        cond, idx = ol.condition_costs(f, nL + nM, nM)
        out.append((cond, len(idx) - nM, nM))
    return out


def test_nothing_big_is_the_clustered_restatement():
    """Frames whose clusters all fit the plain tiers: with the default caps nothing is open and the answer is cluster_check's;
    with max_exact = 1 every cluster of 2 .. 10 columns goes through the column-scaled sums instead and agrees within 1e-12."""
    seen = 0
    for cond, cL, nM in conditioned_scene(24, 20, 10, 12):
        wp, wlp, winfo, wmaxc, _ = cc.clustered_probs(cond, cL, nM)
        assert winfo > 0
        p, method, opens, nbig, maxc, lp = bc.hybrid_exact_probs(cond, cL, nM)
        assert method == 0 and not opens and nbig == 0 and maxc == wmaxc
        assert np.array_equal(p.view(np.int64), wp.view(np.int64)) and lp == wlp
        p, method, opens, nbig, maxc, lp = bc.hybrid_exact_probs(cond, cL, nM, max_exact=1, max_big=16)
        assert method == 0 and nbig == len(opens) and all(o["big"] and 2 <= o["m"] <= 10 for o in opens)
        seen += nbig
        assert np.abs(p - wp).max() <= 1e-12 and abs(lp - wlp) <= 1e-12 * max(1.0, abs(wlp))
    assert seen >= 20


def test_scaled_sums_are_the_plain_sums():
    rng = np.random.default_rng(3)
    a = rng.random((9, 6)) * (rng.random((9, 6)) < 0.6)
    w, Z = bc.scaled_subset_sums(a)
    pw, pZ = pc.subset_sums(a)
    np.testing.assert_allclose(w, pw, rtol=1e-13, atol=0)
    assert abs(Z - pZ) <= 1e-13 * pZ


def test_shift_of_a_clusters_costs():
    """x -> x + s inside one cluster: the probabilities stay (1e-12), log Z in the units exp(-x) moves by -m s -- also where the
    unscaled product of m entries would leave the doubles (s = 40: e^-40m)."""
    opens = []
    for cond, cL, nM in conditioned_scene(24, 20, 10, 12):
        opens += bc.hybrid_exact_probs(cond, cL, nM, max_exact=4, max_big=16)[2]
    opens = [o for o in opens if o["big"]][:8]
    assert len(opens) == 8
    for o in opens:
        p, lz, info = bc.big_cluster(o["block"], o["nL"], o["m"])
        assert info == 1
        for s in (-3.25, 40.0):
            q, lzs, infos = bc.big_cluster(o["block"] + s, o["nL"], o["m"])
            assert infos == 1 and np.abs(p - q).max() <= 1e-12
            assert abs((lzs - lz) + o["m"] * s) <= 1e-12 * max(1.0, abs(lzs))


def largest_cluster(frame, nL, nM):
    _, A = hc.gated_block(frame, nL, nM, condition=True)
    clusters, _ = cc.clusters_of(A)
    cols, rows = max(clusters, key=lambda cr: len(cr[0]))
    return len(cols), len(rows)


def test_oversized_clusters_the_gpu_tests_rely_on():
    small = wl.scene_frames(75, 60, 40, 30)
    assert largest_cluster(small[1], 60, 40) == (17, 40)
    assert largest_cluster(small[38], 60, 40) == (18, 43)
    assert largest_cluster(small[74], 60, 40) == (23, 53)
    assert largest_cluster(wl.scene_frames(6, 200, 128, 60)[5], 200, 128) == (20, 46)
    assert bc.layers_bytes(20, 26) == 49 * (1 << 20) * 8 <= bc.WORK_CAP


def test_edges_of_the_restatement():
    inf = np.inf
    flat = lambda blk: np.ascontiguousarray(np.asarray(blk, dtype=np.float64).T).reshape(-1)  # noqa: E731
    same_row = flat([[1.0, 2.0], [inf, inf], [inf, inf], [inf, inf]])  # nL = 2, nM = 2: both columns can only take row 0
    p, method, opens, nbig, _, lp = bc.hybrid_exact_probs(same_row, 2, 2, max_exact=1)
    assert method == -2 and not p.any() and nbig == 0 and lp == -inf
    # beyond max_big: refused with k = 0, hybrid_check's answer with k >= 1
    cond, cL, nM = conditioned_scene(24, 20, 10, 12)[0]
    p, method, opens, nbig, _, lp = bc.hybrid_exact_probs(cond, cL, nM, k=0, max_exact=1, max_big=2)
    assert any(o["m"] > 2 for o in opens) and method == -1 and not p.any() and np.isnan(lp)
    p, method, opens, nbig, _, _ = bc.hybrid_exact_probs(cond, cL, nM, k=50, max_exact=1, max_big=0)
    want = hc.hybrid_probs(cond, cL, nM, 50, max_exact=1)
    assert nbig == 0 and method == want[1] and np.array_equal(p.view(np.int64), want[0].view(np.int64))


def test_library_exports_bigcluster_entries(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pk.lib_path()], text=True)
    assert "_Z15hybridExactProbRKSt6vectorIdSaIdEEmmm" in out
    from probabilisticsemslam_amd import engine
    for sym in ("kbest_reserve_bigcluster", "kbest_set_bigcluster_work_cap", "kbest_bigcluster_probs_f64_dev",
                "kbest_hybrid_exact_probs_batch_f64"):
        assert sym in engine.C_ABI_SYMBOLS and f" T {sym}\n" in out and hasattr(lib, sym), sym
    assert callable(pk.hybridExactProb)
    for name in ("hybrid_exact_probs", "bigcluster_probs_dev", "reserve_bigcluster", "set_bigcluster_work_cap"):
        assert callable(getattr(pk.KBestEngine, name)), name
    header = open(os.path.join(ROOT, "include", "kbest_c.h")).read()
    assert "#define KBEST_BIGCLUSTER_MAX_SIZE 20" in header and "KBEST_BIGCLUSTER_WORK_CAP ((size_t)1 << 30)" in header
    assert engine.KBEST_BIGCLUSTER_MAX_SIZE == bc.MAX_BIG == 20


def test_bigcluster_without_gpu_fails_loudly(lib):
    if lib.kbest_device_count() > 0:
        return  # (a GPU is present: tests/test_gpu_bigcluster.py has the rest)
    with pytest.raises(pk.KBestError):
        pk.hybridExactProb(np.random.rand(12), 2, 3, 10)
