"""Tall frames for the exact tiers -- up to the 1 024 rows include/kbest_c.h promises -- and their truth in long double, for
tests/test_tall_cpu.py and tests/test_gpu_tall.py.  Plain numpy.

Every case is a named, deterministic shape at a seam the kernels themselves define:

    kbest_perm.hip, kbest_sample.hip          more rows than perm_threads(maxCol) threads, more than one chunk of 64 rows in the two
                                              compactions by ballot, 1 024 rows, every mode of perm_plan with hundreds of rows
    kbest_cluster.hip, kbest_cluster_sample.hip   cl_small(m, R) on either side of its row boundary for every m it knows, the workgroup
                                              tier at m <= 3, the three placements of its layers (arena / a and G in the arena / slot)

The predicates of those files are restated below in a few lines each.  The tests use them ONLY to assert that a case sits where its
name says; no expected value comes from them.

The truth: range_lib.subset_sums_ld (the recurrences of permanent_check.subset_sums in np.longdouble) on permanent_check.to_probs of
the block.  For the clustered cases it runs per cluster of the GENERATOR's own list of clusters, not of cluster_check.clusters_of,
so that it checks the labelling too.  On x86 np.longdouble has 64 bits of mantissa: its rounding error is 2^-11 of float64's.
Cost blocks are column-major (nL+nM) x nM, as everywhere in this project."""
from __future__ import annotations

import collections
import functools

import numpy as np

import permanent_check as pc
import range_lib as rl

LD = np.longdouble
TOL = 1e-12
MAX_ROWS = 1024                        # KBEST_MAX_DIM_WIDE: rows (nL + nM) of a frame of the exact tiers
LDS_LIMITS = (64 << 10, 160 << 10)     # what hipDeviceAttributeMaxSharedMemoryPerBlock may report for the device
LDS_PER_CU = 160 << 10
ARENA = 64 << 10                       # cluster_plan: the arena of the workgroup tier where the LDS limit leaves it whole
SEED = 2024                            # the draws' seed (sample_check.SEED)


# ---- the predicates of the kernels, restated ---------------------------------------------------------------------------------------
def perm_threads(M):
    """kbest_perm_plan.h: threads of a launch whose widest frame has M columns."""
    t = (1 << M) // 4
    return 64 if t < 64 else 1024 if t > 1024 else t


def perm_lds(mode, max_raw_row, max_col):
    """kbest_perm_plan.h: bytes of dynamic LDS of mode 0 (all layers), 1 (a and the two G layers) or 2 (the tables alone)."""
    o = 2 * 16 * 16 * 8 + 16 * 8 + 16 * 8 + 16
    o += 3 * ((2 * max_raw_row + 7) & ~7)
    if mode < 2:
        o += max_raw_row * max_col * 8 + (2 << max_col) * 8
    if mode < 1:
        o += (max_raw_row << max_col) * 8
    return (o + 15) & ~15


def perm_mode(max_raw_row, max_col, lds_limit, lds_per_cu=LDS_PER_CU):
    """perm_plan (kbest_perm.hip): the mode of a launch."""
    lds0 = perm_lds(0, max_raw_row, max_col) if max_col <= 12 else 1 << 30
    lds1 = perm_lds(1, max_raw_row, max_col) if max_col <= 12 else 1 << 30
    if lds0 <= lds_limit and lds0 <= lds_per_cu // 4:
        return 0
    return 1 if lds1 <= lds_limit else 2


def perm_modes(max_raw_row, max_col):
    """The modes under either LDS limit, smaller limit first."""
    return tuple(perm_mode(max_raw_row, max_col, lim) for lim in LDS_LIMITS)


def cl_threads(m):
    """kbest_cluster.hip: threads that accumulate the marginals of a cluster of m columns in the workgroup tier."""
    t = (1 << m) // 4
    return 64 if t < 64 else 512 if t > 512 else t


def cl_small(m, R):
    """kbest_cluster.hip: the wave tier takes a cluster of m columns and R rows."""
    return m <= 6 and (R * (1 << m) + R * m) * 8 <= 4096


def cl_placement(m, R, arena=ARENA):
    """kbest_cluster.hip, the workgroup tier: 'arena' (a, G and F in LDS), 'ga' (a and G in LDS, F in the slot), 'slot'."""
    ga = (2 * (1 << m) + R * m) * 8
    if ga > arena:
        return "slot"
    return "arena" if ga + R * (1 << m) * 8 <= arena else "ga"


def cl_layer_bytes(m, R):
    """The layers (R + 2) 2^m 8 the slot cap of 64 MiB is compared with."""
    return ((R + 2) << m) * 8


def supported(nR, nM, max_cols):
    """check_frame_shape (kbest_capi.cpp): a launch whose tallest frame has nR rows and whose widest has nM columns is taken."""
    return 1 <= nM <= max_cols and nM <= nR <= MAX_ROWS


# ---- the named cases ---------------------------------------------------------------------------------------------------------------
DENSE = ((64, 3), (65, 3), (1024, 1), (512, 2), (1024, 4), (257, 10), (1023, 10), (1024, 12))
DENSE_MODES = {(65, 3): (0, 0), (1024, 1): (0, 0), (512, 2): (0, 0), (1024, 4): (1, 1), (257, 10): (1, 1), (1023, 10): (2, 1),
               (1024, 12): (2, 2)}                       # (under 64 KiB, under 160 KiB)
ROWS_WITHIN_THREADS = ((64, 3), (1024, 12))             # every other dense case has more rows than perm_threads
SAMPLED = {(1024, 1): 512, (1024, 4): 512, (257, 10): 512, (1024, 12): 64}  # the sampler's cases: draws on the GPU
EDGES_LOW = ((1, 170), (1, 171), (2, 85), (2, 86), (3, 46), (3, 47))       # 605 rows, 12 columns
EDGES_HIGH = ((6, 7), (6, 8), (5, 13), (5, 14), (4, 25), (4, 26))          # 93 rows, 30 columns
PLACEMENTS = {"ga": ((8, 600),), "slot": ((10, 1000),), "slot33": ((12, 1010),), "column": ((1, 1024),)}
CLUSTERED = dict(edges_low=EDGES_LOW, edges_high=EDGES_HIGH, **PLACEMENTS)
CLUSTER_SAMPLED = ("edges_low", "edges_high", "ga")     # the clustered sampler's cases, 256 draws on the GPU


def dense_seed(nR, nM):
    return 7000 + 16 * nR + nM


def flat(X):
    return np.ascontiguousarray(np.asarray(X, dtype=np.float64).T).reshape(-1)


def matrix(block, nL, nM):
    """(nL + nM, nM) view of a flat column-major block."""
    return np.asarray(block, dtype=np.float64).reshape(nM, nL + nM).T


Frame = collections.namedtuple("Frame", "block nL nM clusters")      # clusters: [(cols, rows)] of the generator, None: dense
Truth = collections.namedtuple("Truth", "probs Z logperm")            # Z: np.longdouble (dense), logperm: float of the LD sum


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def tall_dense(nR, nM, seed=None):
    """One dense block of costs in [0, 10), nL = nR - nM, not conditioned: every row is active."""
    from probabilisticsemslam_amd import workloads as wl
    seed = dense_seed(nR, nM) if seed is None else seed
    return Frame(_frozen(wl.dense_batch(1, nR, nM, seed)[0] * 10.0), nR - nM, nM, None)


@functools.lru_cache(maxsize=None)
def tall_clusters(spec, seed=11):
    """spec: ((m, R), ...).  Cluster k owns m consecutive columns and R - m consecutive landmark rows of its own; its landmark
    entries are 10 u, the miss row nL + c of each of its columns holds 5 + u, everything else is +inf."""
    rng = np.random.default_rng([seed, len(spec)] + [v for mr in spec for v in mr])
    nM = sum(m for m, _ in spec)
    nL = sum(R - m for m, R in spec)
    X = np.full((nL + nM, nM), np.inf)
    clusters, c0, l0 = [], 0, 0
    for m, R in spec:
        assert 1 <= m <= R
        cols, land = np.arange(c0, c0 + m), np.arange(l0, l0 + R - m)
        X[np.ix_(land, cols)] = 10.0 * rng.random((R - m, m))
        X[nL + cols, cols] = 5.0 + rng.random(m)
        clusters.append((cols, np.r_[land, nL + cols]))
        c0, l0 = c0 + m, l0 + R - m
    return Frame(_frozen(flat(X)), nL, nM, tuple(clusters))


@functools.lru_cache(maxsize=None)
def tall_conditioned():
    """One raw KITTI-like frame of 1 018 landmarks and 6 measurements for condition = True: raw rows up to 1 023 in the scatter."""
    from probabilisticsemslam_amd import workloads as wl
    return Frame(_frozen(wl.kitti_like_frames(1, nL=1018, nM=6)[0]), 1018, 6, None)


# ---- the truth ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def true_dense(nR, nM, seed=None):
    f = tall_dense(nR, nM, seed)
    w, Z = rl.subset_sums_ld(matrix(pc.to_probs(f.block), f.nL, f.nM))
    return Truth(_frozen(pc.fold(w, Z, f.nL)), Z, float(np.log(Z)))


def cluster_truth(frame, perturb=None):
    """Truth of a clustered frame from the generator's own clusters.  perturb: (column, slot, delta) added to one entry (the
    evidence that the checker bites, tests/test_tall_cpu.py)."""
    A = matrix(pc.to_probs(frame.block), frame.nL, frame.nM)
    probs = np.zeros((frame.nM, frame.nL + 1), dtype=LD)
    logperm = LD(0)
    for cols, rows in frame.clusters:
        w, Z = rl.subset_sums_ld(A[np.ix_(rows, cols)])
        assert Z > 0
        logperm = logperm + np.log(Z)
        for i, r in enumerate(rows):
            probs[cols, min(int(r), frame.nL)] += w[i] / Z
    probs = probs.astype(np.float64)
    if perturb is not None:
        probs[perturb[0], perturb[1]] += perturb[2]
    return Truth(_frozen(probs), None, float(logperm))


@functools.lru_cache(maxsize=None)
def true_clusters(name):
    return cluster_truth(tall_clusters(CLUSTERED[name]))


@functools.lru_cache(maxsize=None)
def true_conditioned():
    """(probs [6, 1019], Z) of tall_conditioned(): condition_costs, the long-double sums, scatter_back."""
    import oracle_lib as ol
    f = tall_conditioned()
    cond, idx = ol.condition_costs(f.block, f.nL + f.nM, f.nM)
    cL = len(idx) - f.nM
    w, Z = rl.subset_sums_ld(matrix(pc.to_probs(cond), cL, f.nM))
    return Truth(_frozen(pc.scatter_back(pc.fold(w, Z, cL), idx, f.nL, f.nM)), Z, float(np.log(Z))), np.asarray(idx)


def labels_of(frame):
    """label[c]: the lowest column of the generated cluster of column c."""
    lab = np.full(frame.nM, -1, np.int32)
    for cols, _ in frame.clusters:
        lab[cols] = cols.min()
    return lab


def true_log_prob(frame, assign, log_norm):
    """The long-double log-probability of every joint of assign [n, nM] (raw rows): sum_c log a[r_c][c] - log_norm.  Asserts that
    every joint is a complete assignment over non-zero entries."""
    A = matrix(pc.to_probs(frame.block), frame.nL, frame.nM)
    a = np.asarray(assign)
    assert a.shape[1] == frame.nM and (a >= 0).all() and (a < frame.nL + frame.nM).all()
    assert all(len(set(row)) == frame.nM for row in a.tolist()), "a row taken twice"
    v = A[a, np.arange(frame.nM)[None, :]]
    assert (v > 0.0).all(), "a zero entry taken"
    return (np.log(v.astype(LD)).sum(axis=1) - LD(log_norm)).astype(np.float64)


def draw_marginals(assign, nL, nM):
    """The empirical [nM, nL + 1] marginals of draws assign [n, nM]."""
    a = np.minimum(np.asarray(assign), nL)
    out = np.zeros((nM, nL + 1))
    for c in range(nM):
        out[c] = np.bincount(a[:, c], minlength=nL + 1) / len(a)
    return out


# ---- the restatements' draws: computed once, shared, read-only ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_draws(nR, nM, n):
    """sample_check.Draws of the restatement on tall_dense(nR, nM), frame key 0; draws 0 .. n-1 of one sequence."""
    import sample_check as sc
    f = tall_dense(nR, nM)
    d = sc.Draws(*sc.sample_assoc(f.block, f.nL, f.nM, n, seed=SEED, frame_key=0), n)
    for x in d[:2]:
        x.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def cluster_draws(name, n):
    """cluster_sample_check.ClusterDraws of the restatement on the clustered case `name`, frame key 0."""
    import cluster_sample_check as cs
    f = tall_clusters(CLUSTERED[name])
    d = cs.clustered_sample_assoc(f.block, f.nL, f.nM, n, seed=SEED, frame_key=0)
    for x in d[:2]:
        x.setflags(write=False)
    return d


# ---- the checker -------------------------------------------------------------------------------------------------------------------
def close(got, want, what):
    assert abs(got - want) <= TOL * max(1.0, abs(want)), (what, got, want)


def check_probs(probs, truth, what):
    """Probabilities within 1e-12 of the truth, every column summing to 1 within 1e-12.  Returns the worst error."""
    probs = np.asarray(probs)
    assert probs.shape == truth.probs.shape and not np.isnan(probs).any(), what
    err = float(np.abs(probs - truth.probs).max())
    assert err <= TOL, (what, err)
    assert np.abs(probs.sum(axis=1) - 1.0).max() <= TOL, what
    return err


def check_clustered(name, probs, logperm, info, maxc, lab, truth=None, want_info=None):
    """One answer to the clustered case `name` against the generator: the truth, the number of clusters, the largest cluster and
    the labels.  truth / want_info: replacements, for the evidence that this checker bites.  Returns the worst error."""
    f = tall_clusters(CLUSTERED[name])
    t = true_clusters(name) if truth is None else truth
    err = check_probs(probs, t, name)
    close(logperm, t.logperm, name)
    assert info == (len(f.clusters) if want_info is None else want_info), (name, info)
    assert maxc == max(len(cols) for cols, _ in f.clusters), (name, maxc)
    if lab is not None:
        assert np.array_equal(np.asarray(lab)[: f.nM], labels_of(f)), name
    return err


def check_draws(frame, truth_probs, log_norm, assign, logp, what, rel=False):
    """Draws against the truth: every joint complete, logProb the long-double log-probability within 1e-12 (rel: times
    max(1, |.|)), and from 1 024 draws on the empirical marginals within 4 / sqrt(N) of the true ones."""
    want = true_log_prob(frame, assign, log_norm)
    err = np.abs(np.asarray(logp) - want)
    assert (err <= (TOL * np.maximum(1.0, np.abs(want)) if rel else TOL)).all(), (what, float(err.max()))
    n = len(assign)
    if n >= 1024:
        dev = np.abs(draw_marginals(assign, frame.nL, frame.nM) - truth_probs).max()
        assert dev <= 4.0 / np.sqrt(n), (what, dev)
    return float(err.max())
