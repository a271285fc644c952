"""CPU: the tall frames of tests/tall_lib.py before any GPU run.  The project's float64 restatements (permanent_check,
cluster_check, sample_check, cluster_sample_check) against the long-double truth, with every tolerance tests/test_gpu_tall.py puts
on the kernels -- so the reference alone meets them -- and every case on the side of its seam that its name says."""
import os

import numpy as np
import pytest

import cluster_check as cc
import permanent_check as pc
import tall_lib as tl

MIN_MARGIN = 1e-10   # tests/test_gpu_sample.py: a restatement whose smallest relative margin is above it draws the kernel's joints
N_DRAWS = 4096


# ---- 1. every case sits where its name says ------------------------------------------------------------------------------------------
def test_dense_cases_sit_at_their_seams():
    for nR, nM in tl.DENSE:
        assert tl.supported(nR, nM, 16)
        if (nR, nM) in tl.DENSE_MODES:
            assert tl.perm_modes(nR, nM) == tl.DENSE_MODES[(nR, nM)], (nR, nM, tl.perm_modes(nR, nM))
        assert (nR > tl.perm_threads(nM)) == ((nR, nM) not in tl.ROWS_WITHIN_THREADS), (nR, nM)
    assert [tl.perm_threads(m) for m in (3, 8, 10, 12)] == [64, 64, 256, 1024]
    assert {m for ms in tl.DENSE_MODES.values() for m in ms} == {0, 1, 2}
    assert max(nR for nR, _ in tl.DENSE) == tl.MAX_ROWS and any(nR > 64 and nR % 64 for nR, _ in tl.DENSE)
    assert set(tl.SAMPLED) <= set(tl.DENSE)
    # the mixed batch of the GPU test: sized by its tallest and its widest frame
    assert tl.perm_modes(1024, 4) == (1, 1) and tl.perm_modes(6, 3) == (0, 0)


def test_cluster_cases_sit_at_their_seams():
    for name, rows, cols in (("edges_low", 605, 12), ("edges_high", 93, 30)):
        spec = tl.CLUSTERED[name]
        f = tl.tall_clusters(spec)
        assert (f.nL + f.nM, f.nM) == (rows, cols)
        assert [tl.cl_small(m, R) for m, R in spec] == [True, False] * 3, name
        assert all(R2 == R1 + 1 and m1 == m2 for (m1, R1), (m2, R2) in zip(spec[::2], spec[1::2]))
        assert all(tl.cl_placement(m, R) == "arena" for m, R in spec)
    assert {m for m, _ in tl.EDGES_LOW + tl.EDGES_HIGH} == {1, 2, 3, 4, 5, 6} and not tl.cl_small(7, 7)
    assert {tl.cl_threads(m) for m, _ in tl.EDGES_LOW} == {64}  # nsub of 2, 4 or 8 under 64 threads and four subsets a thread
    want = {"ga": "ga", "slot": "slot", "slot33": "slot", "column": "arena"}
    for name, place in want.items():
        ((m, R),) = tl.PLACEMENTS[name]
        f = tl.tall_clusters(tl.PLACEMENTS[name])
        assert not tl.cl_small(m, R) and tl.cl_placement(m, R) == place, name
        assert tl.cl_layer_bytes(m, R) <= cc.SLOT_CAP and tl.supported(f.nL + f.nM, f.nM, 128), name
    assert tl.cl_layer_bytes(10, 1000) > 8.2e6 and 33e6 < tl.cl_layer_bytes(12, 1010) < cc.SLOT_CAP
    f = tl.tall_clusters(tl.PLACEMENTS["column"])
    assert (f.nL, f.nM) == (1023, 1) and len(f.clusters[0][1]) == 1024


def test_generated_blocks():
    """Every finite entry lies within the gate of the block's smallest one (every row is active); the generator's clusters are the
    blocks of the matrix; the restatement's labelling finds them."""
    for nR, nM in tl.DENSE:
        f = tl.tall_dense(nR, nM)
        assert f.block.shape == (nR * nM,) and f.block.max() < f.block.min() + pc.GATE and (pc.to_probs(f.block) > 0.0).all()
    for name, spec in tl.CLUSTERED.items():
        f = tl.tall_clusters(spec)
        A = tl.matrix(pc.to_probs(f.block), f.nL, f.nM)
        mask = np.zeros(A.shape, bool)
        for cols, rows in f.clusters:
            mask[np.ix_(rows[: len(rows) - len(cols)], cols)] = True
            mask[rows[len(rows) - len(cols):], cols] = True
        assert np.array_equal(A > 0.0, mask), name
        found, lab = cc.clusters_of(A)
        assert np.array_equal(lab, tl.labels_of(f)) and len(found) == len(f.clusters), name
        for (c1, r1), (c2, r2) in zip(found, f.clusters):
            assert np.array_equal(c1, c2) and np.array_equal(r1, r2), name


# ---- 2. the float64 restatements against the long-double truth --------------------------------------------------------------------------
@pytest.mark.parametrize("nR,nM", tl.DENSE)
def test_permanent_restatement_on_dense(nR, nM):
    f, t = tl.tall_dense(nR, nM), tl.true_dense(nR, nM)
    probs, Z = pc.permanent_probs(f.block, f.nL, f.nM)
    err = tl.check_probs(probs, t, (nR, nM))
    tl.check_probs(t.probs, t, (nR, nM))  # (the truth itself: columns sum to 1)
    print(f"{nR}x{nM}: restatement vs long double {err:.3g}, Z rel {abs(Z - float(t.Z)) / float(t.Z):.3g}")
    assert abs(Z - float(t.Z)) <= tl.TOL * float(t.Z)
    tl.close(float(np.log(Z)), t.logperm, (nR, nM))


@pytest.mark.parametrize("name", list(tl.CLUSTERED))
def test_clustered_restatement(name):
    f = tl.tall_clusters(tl.CLUSTERED[name])
    probs, logperm, info, maxc, lab = cc.clustered_probs(f.block, f.nL, f.nM)
    err = tl.check_clustered(name, probs, logperm, info, maxc, lab)
    print(f"{name}: restatement vs long double {err:.3g}, logPerm {logperm!r} vs {tl.true_clusters(name).logperm!r}")


def test_conditioned_restatement():
    import oracle_lib as ol
    f = tl.tall_conditioned()
    t, idx = tl.true_conditioned()
    cond, idx2 = ol.condition_costs(f.block, f.nL + f.nM, f.nM)
    cL = len(idx2) - f.nM
    assert idx.max() == 1023 and cL >= 6 and idx[:cL].max() > 512  # raw rows the u16 tables and the scatter must carry
    p, Z = pc.permanent_probs(cond, cL, f.nM)
    err = tl.check_probs(pc.scatter_back(p, idx2, f.nL, f.nM), t, "conditioned")
    print(f"1018+6 conditioned: {cL} landmarks kept, restatement vs long double {err:.3g}")
    assert abs(Z - float(t.Z)) <= tl.TOL * float(t.Z)


# ---- 3. the draws -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nR,nM", list(tl.SAMPLED))
def test_dense_draws(nR, nM):
    """The margin rule of tests/test_gpu_sample.py on 4 096 draws (the GPU test compares the first 512 or 64 of them), each
    draw's logProb against the long-double log-probability of its joint, the marginals of the 4 096 draws against the truth."""
    n = N_DRAWS
    f, t, d = tl.tall_dense(nR, nM), tl.true_dense(nR, nM), tl.dense_draws(nR, nM, n)
    assert n >= tl.SAMPLED[(nR, nM)]
    print(f"{nR}x{nM}: {n} draws, smallest margin {d.margin:.3g}")
    assert d.margin >= MIN_MARGIN
    assert abs(d.Z - float(t.Z)) <= tl.TOL * float(t.Z)
    err = tl.check_draws(f, t.probs, np.log(t.Z), d.assign, d.logp, (nR, nM), rel=True)
    print(f"{nR}x{nM}: logProb vs long double {err:.3g}")


@pytest.mark.parametrize("name", tl.CLUSTER_SAMPLED)
def test_clustered_draws(name):
    n = N_DRAWS
    f, t, d = tl.tall_clusters(tl.CLUSTERED[name]), tl.true_clusters(name), tl.cluster_draws(name, n)
    print(f"{name}: {n} draws, smallest margin {d.margin:.3g}")
    assert d.margin >= MIN_MARGIN and d.info == len(f.clusters) and d.maxc == max(len(c) for c, _ in f.clusters)
    tl.close(d.logperm, t.logperm, name)
    err = tl.check_draws(f, t.probs, t.logperm, d.assign, d.logp, name, rel=True)
    print(f"{name}: logProb vs long double {err:.3g}")


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_a_frame_of_1025_rows_is_refused_by_the_restated_bounds():
    assert tl.supported(1024, 16, 16) and not tl.supported(1025, 2, 16) and not tl.supported(1025, 2, 128)
    assert not tl.supported(20, 17, 16) and tl.supported(20, 17, 128)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kbest_c.h")).read()
    assert "#define KBEST_MAX_DIM_WIDE 1024" in header


# ---- 5. the checker bites ---------------------------------------------------------------------------------------------------------------------
def test_the_checker_notices_a_wrong_truth_and_a_wrong_count():
    """One entry of the truth moved by 1e-11, and the expected number of clusters swapped with another case's: the checker that
    passes the restatement above must fail both."""
    name = "edges_low"
    f = tl.tall_clusters(tl.CLUSTERED[name])
    probs, logperm, info, maxc, lab = cc.clustered_probs(f.block, f.nL, f.nM)
    tl.check_clustered(name, probs, logperm, info, maxc, lab)
    with pytest.raises(AssertionError):
        tl.check_clustered(name, probs, logperm, info, maxc, lab, truth=tl.cluster_truth(f, perturb=(5, 200, 1e-11)))
    with pytest.raises(AssertionError):
        tl.check_clustered(name, probs, logperm, info, maxc, lab, want_info=len(tl.PLACEMENTS["ga"]))
    wrong = np.array(lab)
    wrong[1] = 0  # column 1 is a cluster of its own
    with pytest.raises(AssertionError):
        tl.check_clustered(name, probs, logperm, info, maxc, wrong)
    t = tl.true_dense(65, 3)
    off = t.probs.copy()
    off[1, 7] += 1e-11
    with pytest.raises(AssertionError):
        tl.check_probs(off, t, "65x3")
