"""GPU: the exact tiers on tall frames -- up to the 1 024 rows include/kbest_c.h promises -- against the long-double truth of
tests/tall_lib.py, never against the kernel's own output: kbest_perm.hip and kbest_sample.hip with more rows than threads, more
than one chunk of 64 rows in the compactions and every LDS mode; kbest_cluster.hip and kbest_cluster_sample.hip on either side of
the row boundary between the wave and the workgroup tier for every m, and in the three placements of the workgroup tier's layers.
tests/test_tall_cpu.py shows that every case sits at its seam and that the restatements meet the same tolerances: 1e-12 absolute on
probabilities, 1e-12 relative on perm and logPerm, columns summing to 1 within 1e-12; draws exactly the restatement's (its margin
asserted first) with logProb within 1e-12 of the long-double log-probability."""
import numpy as np
import pytest

import probabilisticsemslam_amd as pk
import tall_lib as tl

pytestmark = pytest.mark.gpu

MIN_MARGIN = 1e-10


@pytest.fixture(scope="module")
def eng():
    e = pk.KBestEngine(0)
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- 1. permanent_probs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nR,nM", tl.DENSE)
def test_permanent_probs_dense(eng, nR, nM):
    f, t = tl.tall_dense(nR, nM), tl.true_dense(nR, nM)
    (p,), perm = eng.permanent_probs([f.block], [f.nL], [f.nM])
    err = tl.check_probs(p, t, (nR, nM))
    rel = abs(perm[0] - float(t.Z)) / float(t.Z)
    print(f"{nR}x{nM}: vs long double {err:.3g}, perm rel {rel:.3g}")
    assert rel <= tl.TOL
    tl.close(float(np.log(perm[0])), t.logperm, (nR, nM))


def test_permanent_probs_conditioned_raw_rows_to_1023(eng):
    f = tl.tall_conditioned()
    t, idx = tl.true_conditioned()
    (p,), perm = eng.permanent_probs([f.block], [f.nL], [f.nM], condition=True)
    err = tl.check_probs(p, t, "conditioned")
    dropped = np.setdiff1d(np.arange(f.nL), idx)
    assert (p[:, dropped] == 0.0).all()  # exactly 0.0
    print(f"1018+6 conditioned: vs long double {err:.3g}, perm rel {abs(perm[0] - float(t.Z)) / float(t.Z):.3g}")
    assert abs(perm[0] - float(t.Z)) <= tl.TOL * float(t.Z)


def test_permanent_probs_mixed_batch_bitwise(eng):
    """65 x 3 and 1 024 x 4 with a 6 x 3 frame in one launch (sized 1 024 x 4: mode 1) against each frame alone (modes 0, 1, 0)."""
    frames = [tl.tall_dense(65, 3), tl.tall_dense(1024, 4), tl.tall_dense(6, 3, 63)]
    mixed, perm = eng.permanent_probs([f.block for f in frames], [f.nL for f in frames], [f.nM for f in frames])
    for b, f in enumerate(frames):
        (alone,), perm_alone = eng.permanent_probs([f.block], [f.nL], [f.nM])
        assert np.array_equal(bits(mixed[b]), bits(alone)) and bits(perm[b]) == bits(perm_alone[0]), b
    tl.check_probs(mixed[0], tl.true_dense(65, 3), "65x3 in the mixed batch")
    tl.check_probs(mixed[1], tl.true_dense(1024, 4), "1024x4 in the mixed batch")
    tl.check_probs(mixed[2], tl.true_dense(6, 3, 63), "6x3 in the mixed batch")


# ---- 2. clustered_probs and the hybrid entry on the same frames -------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tl.CLUSTERED))
def test_clustered_probs(eng, name):
    f = tl.tall_clusters(tl.CLUSTERED[name])
    (p,), logperm, info, maxc, lab = eng.clustered_probs([f.block], [f.nL], [f.nM], labels=True)
    err = tl.check_clustered(name, p, logperm[0], info[0], maxc[0], lab[0])
    print(f"{name}: vs long double {err:.3g}, logPerm {logperm[0]!r} vs {tl.true_clusters(name).logperm!r}")
    # nothing is open under the default caps: the hybrid entry answers with the same bits
    (hp,), method, nOpen, nBig, hmaxc, hlp, nFr = eng.hybrid_frontier_probs([f.block], [f.nL], [f.nM], 0)
    assert (method[0], nOpen[0], nBig[0], nFr[0], hmaxc[0]) == (0, 0, 0, 0, maxc[0])
    assert np.array_equal(bits(hp), bits(p)) and bits(hlp[0]) == bits(logperm[0])


def test_three_column_clusters_opened_to_the_frontier_tier(eng):
    """max_exact = 2 on edges_low: the clusters of 3 columns and 46 / 47 rows go to the frontier tier, the rest keep their bits."""
    name = "edges_low"
    f, t = tl.tall_clusters(tl.CLUSTERED[name]), tl.true_clusters(name)
    (p,), _, _, _ = eng.clustered_probs([f.block], [f.nL], [f.nM])
    (hp,), method, nOpen, nBig, maxc, hlp, nFr = eng.hybrid_frontier_probs([f.block], [f.nL], [f.nM], 0, max_exact=2)
    assert (method[0], nOpen[0], nBig[0], nFr[0], maxc[0]) == (0, 2, 0, 2, 3)
    err = tl.check_probs(hp, t, name)
    tl.close(hlp[0], t.logperm, name)
    opened = np.concatenate([cols for cols, _ in f.clusters if len(cols) == 3])
    kept = np.setdiff1d(np.arange(f.nM), opened)
    assert len(opened) == 6 and np.array_equal(bits(hp[kept]), bits(p[kept]))
    print(f"{name}, max_exact 2: vs long double {err:.3g} (opened columns {np.abs(hp[opened] - t.probs[opened]).max():.3g})")


# ---- 3. sample_assoc ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nR,nM", list(tl.SAMPLED))
def test_sample_assoc_dense(eng, nR, nM):
    n = tl.SAMPLED[(nR, nM)]
    f, t, want = tl.tall_dense(nR, nM), tl.true_dense(nR, nM), tl.dense_draws(nR, nM, n)
    print(f"{nR}x{nM}: margin {want.margin:.3g}")
    assert want.margin >= MIN_MARGIN
    (asg,), (lp,), perm = eng.sample_assoc([f.block], [f.nL], [f.nM], n, seed=tl.SEED, frame_key=[0])
    assert asg.dtype == np.int32 and np.array_equal(asg, want.assign)
    err = tl.check_draws(f, t.probs, np.log(t.Z), asg, lp, (nR, nM))
    _, perm_exact = eng.permanent_probs([f.block], [f.nL], [f.nM])
    assert bits(perm[0]) == bits(perm_exact[0])
    print(f"{nR}x{nM}: {n} draws equal, logProb vs long double {err:.3g}")


# ---- 4. clustered_sample_assoc -------------------------------------------------------------------------------------------------------------
def clustered_draws(eng, name, n):
    f, t, want = tl.tall_clusters(tl.CLUSTERED[name]), tl.true_clusters(name), tl.cluster_draws(name, n)
    print(f"{name}: margin {want.margin:.3g}")
    assert want.margin >= MIN_MARGIN
    (asg,), (lp,), logperm, info, maxc = eng.clustered_sample_assoc([f.block], [f.nL], [f.nM], n, seed=tl.SEED, frame_key=[0])
    assert asg.dtype == np.int32 and np.array_equal(asg, want.assign)
    err = tl.check_draws(f, t.probs, t.logperm, asg, lp, name)
    assert info[0] == len(f.clusters) and maxc[0] == max(len(c) for c, _ in f.clusters)
    tl.close(logperm[0], t.logperm, name)
    _, lp_exact, _, _ = eng.clustered_probs([f.block], [f.nL], [f.nM])
    assert bits(logperm[0]) == bits(lp_exact[0])
    print(f"{name}: {n} draws equal, logProb vs long double {err:.3g}")


@pytest.mark.parametrize("name", tl.CLUSTER_SAMPLED)
def test_clustered_sample_assoc(eng, name):
    clustered_draws(eng, name, 256)


def test_clustered_sample_assoc_marginals(eng):
    """4 096 draws on edges_low: the empirical marginals within 4 / sqrt(N) of the truth (tall_lib.check_draws)."""
    clustered_draws(eng, "edges_low", 4096)


# ---- 5. bounds -------------------------------------------------------------------------------------------------------------------------------
def test_a_frame_of_1025_rows_is_refused(eng):
    f = tl.tall_dense(1025, 2, 5)
    assert not tl.supported(1025, 2, 16)
    with pytest.raises(pk.KBestError, match="1024"):
        eng.permanent_probs([f.block], [f.nL], [f.nM])
    with pytest.raises(pk.KBestError, match="1024"):
        eng.sample_assoc([f.block], [f.nL], [f.nM], 4)
    with pytest.raises(pk.KBestError, match="1024"):
        eng.clustered_sample_assoc([f.block], [f.nL], [f.nM], 4)
    # the context still answers
    g, t = tl.tall_dense(64, 3), tl.true_dense(64, 3)
    (p,), _ = eng.permanent_probs([g.block], [g.nL], [g.nM])
    tl.check_probs(p, t, "64x3 after the refusals")
