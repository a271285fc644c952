"""Clusters at and beyond the range of the column-scaled exact tiers (kbest_bigcluster.hip, kbest_frontier.hip,
kbest_frontier_sample.hip) and their truth in long double, for tests/test_range_cpu.py and tests/test_gpu_range.py.  Plain numpy.

Those tiers sum a'[r][c] = exp(colMin_c - x[r][c]) in float64 and answer while Z' >= 2^-970.  The generators
below make clusters whose every complete assignment is expensive, so that log Z' runs from about -600 to about -800, out of
ordinary costs: every finite entry of a cluster lies within the frame gate of 42 above the smallest one.

    hub          one landmark row that is cheap in every column, one miss row per column at colMin + miss: one column takes the hub,
                 m - 1 columns miss
    two_hubs     the same with two hubs over the halves of the columns and one link landmark between the halves: frontier width
                 <= 16 for m <= 20, and still few enough columns for the subset sums
    pair_chain   npair pairs of columns; a pair shares one cheap landmark, neighbouring pairs share one at + link, every column has
                 a miss row at + miss: a sparse chain of up to 64 columns
    no_matching  clusters without a complete assignment

A Case carries the cluster as the flat column-major (nLk + m) x m sub-block the _dev entries take (+inf for a zero) and the same
cluster inside a raw frame (cost, nL, nM) next to one ordinary cluster of two columns, with the columns of both.

The truth: the recurrences of permanent_check.subset_sums in np.longdouble (subset_sums_ld, by halves of the layers as
bigcluster_check._step) up to 20 columns, frontier_check.frontier_sums in np.longdouble beyond.  On x86 np.longdouble is the 80-bit
format: 64 bits of mantissa, smallest normal 3.4e-4932, so nothing here comes near its range and its rounding error is 2^-11 of
float64's."""
from __future__ import annotations

import collections
import functools
import itertools

import numpy as np

import frontier_check as fc

LD = np.longdouble
GATE = 42.0           # hybrid_check.GATE: the frame entries keep an entry below (smallest entry of the frame) + 42
SAFE, DEEP = -660.0, -700.0   # log Z' >= SAFE: a tier must answer; log Z' < DEEP: beyond the normal doubles (e^-708)
TOL = 1e-12

Case = collections.namedtuple("Case", "name block nLk m cost nL nM cols small_cols")


def flat(X):
    return np.ascontiguousarray(np.asarray(X, dtype=np.float64).T).reshape(-1)


def _case(name, land, miss_row):
    """land: (nLk, m) landmark rows, +inf for a zero; miss_row[c]: the entry of column c's own miss row (+inf: none).  The frame:
    the cluster's landmarks, then two landmarks of an ordinary cluster of two columns behind the cluster's columns."""
    land = np.asarray(land, dtype=np.float64)
    nLk, m = land.shape
    X = np.full((nLk + m, m), np.inf)
    X[:nLk] = land
    X[nLk + np.arange(m), np.arange(m)] = miss_row
    fin = X[np.isfinite(X)]
    assert fin.max() < fin.min() + GATE - 0.01 and fin.min() >= 0.0  # (every entry survives the gate of a frame)
    nL, nM = nLk + 2, m + 2
    F = np.full((nL + nM, nM), np.inf)
    F[:nLk, :m] = land
    F[nL + np.arange(m), np.arange(m)] = miss_row
    F[nLk:nL, m:] = fin.min() + np.array([[1.0, 2.5], [3.0, 0.5]])
    F[nL + m + np.arange(2), m + np.arange(2)] = fin.min() + np.array([2.0, 1.5])
    block, cost = flat(X), flat(F)
    block.setflags(write=False)
    cost.setflags(write=False)
    return Case(name, block, nLk, m, cost, nL, nM, np.arange(m), np.arange(m, m + 2))


def hub(m, miss, jitter=0.5, seed=0):
    """One hub landmark at [0, jitter / 4) in every column; column c's miss row at colMin_c + miss + [0, jitter / 2)."""
    rng = np.random.default_rng([seed, m, 1])
    h = rng.random(m) * jitter / 4
    return _case(f"hub({m}, {miss:g})", h[None, :], h + miss + rng.random(m) * jitter / 2)


def two_hubs(m, miss, jitter=0.5, seed=0):
    """Hub 0 over the columns < m // 2, hub 1 over the others, a link landmark at colMin + miss / 2 in the two columns where the
    halves meet, the miss rows as hub's."""
    assert 4 <= m <= 20
    rng = np.random.default_rng([seed, m, 2])
    h = rng.random(m) * jitter / 4
    half = m // 2
    land = np.full((3, m), np.inf)
    land[0, :half] = h[:half]
    land[1, half:] = h[half:]
    land[2, half - 1: half + 1] = h[half - 1: half + 1] + miss / 2
    return _case(f"two_hubs({m}, {miss:g})", land, h + miss + rng.random(m) * jitter / 2)


def pair_chain(npair, miss, link=None, jitter=0.5, seed=0):
    """Columns 2p and 2p + 1 share landmark p at [0, jitter / 4); columns 2p + 1 and 2p + 2 share landmark npair + p at colMin + link +
    [0, jitter / 2) (link: miss when None); the miss rows as hub's.  m = 2 npair, frontier width 2."""
    assert 2 <= npair <= 32
    link = miss if link is None else link
    rng = np.random.default_rng([seed, npair, 3])
    m = 2 * npair
    h = rng.random(m) * jitter / 4
    land = np.full((2 * npair - 1, m), np.inf)
    for p in range(npair):
        land[p, 2 * p: 2 * p + 2] = h[2 * p: 2 * p + 2]
    for p in range(npair - 1):
        land[npair + p, 2 * p + 1: 2 * p + 3] = h[2 * p + 1: 2 * p + 3] + link + rng.random(2) * jitter / 2  # (jitter: no two sums tie)
    name = f"pair_chain({npair}, {miss:g})" if link == miss else f"pair_chain({npair}, {miss:g}, {link:g})"
    return _case(name, land, h + miss + rng.random(m) * jitter / 2)


def no_matching():
    """Clusters of 17 columns without a complete assignment, by name.  The frame of 'empty_column' is left out of the frame tests:
    a column without an entry is a cluster by itself there."""
    rng = np.random.default_rng(5)
    m = 17
    h = rng.random(m) * 0.1
    missrow = h + 30.0 + rng.random(m) * 0.1
    out = {}
    land = np.full((1, m), np.inf)  # column 16 has no finite entry at all
    land[0, :16] = h[:16]
    out["empty_column"] = _case("no_matching: a column without a finite entry", land, np.where(np.arange(m) < 16, missrow, np.inf))
    land = np.full((3, m), np.inf)  # columns 14, 15, 16 live in landmarks 1 and 2 alone; landmark 1 ties them to the rest
    land[0, :14] = h[:14]
    land[1, [0, 14, 15, 16]] = h[[0, 14, 15, 16]] + [20.0, 0.0, 0.0, 0.0]
    land[2, 14:] = h[14:] + 1.0
    out["three_columns_two_rows"] = _case("no_matching: three columns on the same two landmarks", land,
                                          np.where(np.arange(m) < 14, missrow, np.inf))
    land = np.full((3, m), np.inf)  # two hubs, their link and thirteen miss rows: sixteen rows for seventeen columns
    land[0, :8] = h[:8]
    land[1, 8:] = h[8:]
    land[2, 7:9] = h[7:9] + 15.0
    out["fewer_rows_than_columns"] = _case("no_matching: fewer rows than columns", land, np.where(np.arange(m) < 13, missrow, np.inf))
    return out


# ---- the truth ---------------------------------------------------------------------------------------------------------------------
def _step_ld(layer, row):
    out = layer.copy()
    for c in np.flatnonzero(row):
        o, l = out.reshape(-1, 2, 1 << c), layer.reshape(-1, 2, 1 << c)
        o[:, 1, :] += row[c] * l[:, 0, :]
    return out


def subset_sums_ld(a):
    """a: (R, C) non-negative.  (w, Z) of permanent_check.subset_sums in np.longdouble, by halves of the layers."""
    a = np.asarray(a, dtype=LD)
    R, C = a.shape
    n = 1 << C
    F = np.zeros((R + 1, n), dtype=LD)
    F[0, 0] = 1
    for i in range(R):
        F[i + 1] = _step_ld(F[i], a[i])
    G = np.zeros(n, dtype=LD)
    G[0] = 1
    w = np.zeros((R, C), dtype=LD)
    for r in range(R - 1, -1, -1):
        T = np.ascontiguousarray(G[::-1])  # T[S] = G[all \ S]
        for c in np.flatnonzero(a[r]):
            w[r, c] = a[r, c] * np.sum(F[r].reshape(-1, 2, 1 << c)[:, 0, :] * T.reshape(-1, 2, 1 << c)[:, 1, :])
        G = _step_ld(G, a[r])
    return w, F[R, n - 1]


def permutation_sum_ld(a):
    """(w, Z) by the sum over all injections columns -> rows, in np.longdouble: for a handful of columns."""
    a = np.asarray(a, dtype=LD)
    R, C = a.shape
    w, Z = np.zeros((R, C), dtype=LD), LD(0)
    for rows in itertools.permutations(range(R), C):
        t = LD(1)
        for c, r in enumerate(rows):
            t = t * a[r, c]
        Z = Z + t
        for c, r in enumerate(rows):
            w[r, c] += t
    return w, Z


def scaled_ld(block, nLk, m):
    """(a' (R, m) in np.longdouble in the documented scaling exp(colMin_c - x), the counting rows, colMin in np.longdouble, X)."""
    X = np.asarray(block, dtype=np.float64).reshape(m, nLk + m).T
    fin = np.isfinite(X)
    colmin = np.where(fin, X, np.inf).min(axis=0).astype(LD)
    rows = np.flatnonzero(fin.any(axis=1))
    with np.errstate(invalid="ignore"):
        A = np.where(fin[rows], np.exp(colmin - X[rows].astype(LD)), LD(0))
    return A, rows, colmin, X


Truth = collections.namedtuple("Truth", "probs logZ logZprime")


def true_cluster(block, nLk, m, method=None):
    """(probs [m, nLk + 1] float64, log Z in the units a = exp(-x), log Z' in the scaling exp(colMin_c - x)) of one sub-block from
    long-double sums; no complete assignment: zeros, -inf, -inf.  method: 'subset' or 'frontier' (by m when None)."""
    A, rows, colmin, _ = scaled_ld(block, nLk, m)
    probs = np.zeros((m, nLk + 1))
    if not np.isfinite(colmin).all() or len(rows) < m:
        return Truth(probs, float("-inf"), float("-inf"))
    method = method or ("subset" if m <= 20 else "frontier")
    w, Z = subset_sums_ld(A) if method == "subset" else fc.frontier_sums(A, dtype=LD)
    if not Z > 0:
        return Truth(probs, float("-inf"), float("-inf"))
    acc = np.zeros((m, nLk + 1), dtype=LD)
    for i, r in enumerate(rows):
        acc[:, min(int(r), nLk)] += w[i] / Z
    lz = np.log(Z)
    return Truth(acc.astype(np.float64), float(lz - colmin.sum()), float(lz))


def true_log_term(block, nLk, m, assign_local, log_zprime):
    """log of the probability of every joint of assign_local [n, m] (the row of the sub-block each column takes), in long double:
    sum_c (colMin_c - x[r_c][c]) - log Z'.  Asserts that every joint is a complete assignment over finite entries."""
    _, _, colmin, X = scaled_ld(block, nLk, m)
    a = np.asarray(assign_local)
    assert a.shape[1] == m and (a >= 0).all() and (a < nLk + m).all()
    assert all(len(set(row)) == m for row in a.tolist()), "a row taken twice"
    x = X[a, np.arange(m)[None, :]]
    assert np.isfinite(x).all(), "a zero entry taken"
    return ((colmin[None, :] - x.astype(LD)).sum(axis=1) - LD(log_zprime)).astype(np.float64)


def draw_marginals(assign_local, nLk, m):
    """The empirical [m, nLk + 1] marginals of draws assign_local [n, m]."""
    a = np.minimum(np.asarray(assign_local), nLk)
    out = np.zeros((m, nLk + 1))
    for c in range(m):
        out[c] = np.bincount(a[:, c], minlength=nLk + 1) / len(a)
    return out


def true_frame(case, truth):
    """(probs [nM, nL + 1], logPerm) of the frame of `case` from the truth of its cluster and the long-double truth of the ordinary
    cluster beside it; logPerm in the frame's units a = exp(mn - x), mn the smallest entry: sum_k (log Z_k + m_k mn)."""
    nL, nM, nLk, m = case.nL, case.nM, case.nLk, case.m
    F = np.asarray(case.cost).reshape(nM, nL + nM).T
    mn = F.min()
    rows = np.r_[nLk: nL, nL + m: nL + nM]
    small = true_cluster(flat(F[np.ix_(rows, case.small_cols)]), 2, 2)
    probs = np.zeros((nM, nL + 1))
    probs[np.ix_(case.cols, np.arange(nLk))] = truth.probs[:, :nLk]
    probs[case.cols, nL] = truth.probs[:, nLk]
    probs[np.ix_(case.small_cols, np.arange(nLk, nL))] = small.probs[:, :2]
    probs[case.small_cols, nL] = small.probs[:, 2]
    return probs, (truth.logZ + m * mn) + (small.logZ + 2 * mn)


# ---- the families of the tests: generated once, shared, read-only --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def big_family():
    """The big-cluster tier's cases (m <= 20): log Z' from about -560 to about -780."""
    return (hub(17, 36), hub(17, 40), hub(17, 41), hub(18, 38), hub(19, 36), hub(20, 34), two_hubs(20, 36), two_hubs(18, 40),
            hub(18, 41), hub(18, 41.5), hub(19, 40), hub(19, 41), hub(20, 41), two_hubs(20, 41))


@functools.lru_cache(maxsize=None)
def frontier_family():
    """The frontier tier's and the frontier sampler's cases (width <= 16): two_hubs and pair chains of 9 .. 32 pairs."""
    return (two_hubs(20, 36), two_hubs(18, 40), two_hubs(16, 41), pair_chain(9, 41), pair_chain(16, 40), pair_chain(24, 27),
            pair_chain(31, 21), pair_chain(32, 20), pair_chain(32, 21),
            pair_chain(32, 22), pair_chain(32, 23.5), pair_chain(32, 25), pair_chain(31, 26), pair_chain(20, 41), two_hubs(20, 41))


@functools.lru_cache(maxsize=None)
def guard_family():
    """At most 16 columns, every non-zero entry above e^-42: the tiers of at most 16 measurements cannot leave the range."""
    return (hub(16, 41.9, jitter=0.1), two_hubs(16, 41.9, jitter=0.1))


_TRUTH = {}


def truth_of(case):
    """true_cluster of a case, computed once (the names of the cases are unique)."""
    if case.name not in _TRUTH:
        t = true_cluster(case.block, case.nLk, case.m)
        t.probs.setflags(write=False)
        _TRUTH[case.name] = t
    return _TRUTH[case.name]


def counts(family):
    """(cases with log Z' >= SAFE, cases with log Z' < DEEP)."""
    lz = [truth_of(c).logZprime for c in family]
    return sum(z >= SAFE for z in lz), sum(z < DEEP for z in lz)


# ---- the contract ("Range"): what every entry may say about a case ----------------------------------------------
OUT_OF_RANGE = -5     # KBEST_INFO_OUT_OF_RANGE
OPEN_TOL = 1e-9       # columns of an enumerated cluster against oracle_lib.assignment_prob (tests/test_gpu_hybrid.py)


def close(got, want, what):
    assert abs(got - want) <= TOL * max(1.0, abs(want)), (what, got, want)


def check_cluster(case, probs, logZ, info):
    """One answer of a per-cluster entry or restatement.  probs / logZ: None where the caller saw its sentinels untouched.
    A: answered means within tolerance of the truth.  B: infeasible only without a complete assignment.  C, D: declined only with
    one, and only below SAFE.  Returns info."""
    t = truth_of(case)
    feasible = t.logZprime > -np.inf
    if info == 1:
        assert feasible, case.name
        err = np.abs(probs - t.probs).max()
        assert err <= TOL, (case.name, err, t.logZprime)
        close(logZ, t.logZ, case.name)
    elif info == 0:
        assert not feasible, (case.name, "reported infeasible", t.logZprime)
        assert not probs.any() and logZ == -np.inf, case.name
    else:
        assert info == OUT_OF_RANGE and feasible and t.logZprime < SAFE, (case.name, info, t.logZprime)
        assert probs is None and logZ is None, (case.name, "a declined cluster's outputs were written")
    return info


def check_frame(case, probs, method, logperm, n_exact, k):
    """One frame of a probability entry or restatement; n_exact: the deep cluster's count in nBig / nFrontier.  Returns method."""
    import oracle_lib as ol
    t = truth_of(case)
    feasible = t.logZprime > -np.inf
    want, want_lp = true_frame(case, t)
    if method == 0:
        assert feasible and n_exact == 1, (case.name, n_exact)
        err = np.abs(probs - want).max()
        assert err <= TOL, (case.name, err, t.logZprime)
        close(logperm, want_lp, case.name)
    elif method in (1, 2):  # declined by every exact tier, enumerated
        assert k >= 1 and feasible and t.logZprime < SAFE and n_exact == 0, (case.name, method, t.logZprime, n_exact)
        p, nf = ol.assignment_prob(case.block, case.nLk, case.m, k)
        assert nf > 0 and np.abs(probs[np.ix_(case.cols, np.arange(case.nLk))] - p[:, :case.nLk]).max() <= OPEN_TOL, case.name
        assert np.abs(probs[case.cols, case.nL] - p[:, case.nLk]).max() <= OPEN_TOL, case.name
        assert np.abs(probs[case.small_cols] - want[case.small_cols]).max() <= TOL, case.name
    elif method == -1:
        assert k < 1 and feasible and t.logZprime < SAFE, (case.name, "refused", k, t.logZprime)
        assert not probs.any() and np.isnan(logperm), case.name
    else:
        assert method == -2 and not feasible, (case.name, method, t.logZprime)
        assert not probs.any() and logperm == -np.inf, case.name
    return method


def local_rows(case, assign):
    """The rows of the sub-blocks (the deep cluster's, the ordinary one's) the raw rows of frame draws assign [n, nM] are."""
    a = np.asarray(assign)
    deep, small = a[:, case.cols], a[:, case.small_cols]
    deep = np.where(deep >= case.nL, deep - case.nL + case.nLk, deep)
    small = np.where(small >= case.nL, small - case.nL - case.m + 2, small - case.nLk)
    return deep, small


def check_draws(case, assign_local, log_term, what=""):
    """Draws of the deep cluster with their terms: every joint a complete assignment, its term the long-double log-probability,
    the empirical marginals within 4 / sqrt(N) of the true ones."""
    t = truth_of(case)
    want = true_log_term(case.block, case.nLk, case.m, assign_local, t.logZprime)
    err = np.abs(log_term - want).max()
    assert err <= TOL * max(1.0, abs(t.logZprime)), (case.name, what, err)
    n = len(assign_local)
    if n >= 1024:
        dev = np.abs(draw_marginals(assign_local, case.nLk, case.m) - t.probs).max()
        assert dev <= 4.0 / np.sqrt(n), (case.name, what, dev)


def check_frame_draws(case, assign, logp, method, logperm, n_frontier, k):
    """One frame of a draw entry or restatement.  Returns method."""
    t = truth_of(case)
    feasible = t.logZprime > -np.inf
    n = len(assign)
    if method == 0:
        assert feasible and n_frontier == 1, (case.name, n_frontier)
        deep, small = local_rows(case, assign)
        F = np.asarray(case.cost).reshape(case.nM, case.nL + case.nM).T
        rows = np.r_[case.nLk: case.nL, case.nL + case.m: case.nL + case.nM]
        sblock = flat(F[np.ix_(rows, case.small_cols)])
        st = true_cluster(sblock, 2, 2)
        want = true_log_term(case.block, case.nLk, case.m, deep, t.logZprime) + true_log_term(sblock, 2, 2, small, st.logZprime)
        err = np.abs(logp - want).max()
        assert err <= TOL * max(1.0, abs(t.logZprime)), (case.name, err)
        close(logperm, true_frame(case, t)[1], case.name)
        if n >= 1024:
            dev = np.abs(draw_marginals(deep, case.nLk, case.m) - t.probs).max()
            assert dev <= 4.0 / np.sqrt(n), (case.name, dev)
    elif method in (1, 2):  # declined by the sampler, drawn from the enumeration: complete assignments over finite entries
        assert k >= 1 and feasible and t.logZprime < SAFE and n_frontier == 0, (case.name, method, t.logZprime)
        deep, _ = local_rows(case, assign)
        true_log_term(case.block, case.nLk, case.m, deep, t.logZprime)
        assert np.isfinite(logp).all(), case.name
    elif method == -1:
        assert k < 1 and feasible and t.logZprime < SAFE, (case.name, "refused", k, t.logZprime)
        assert (assign == -1).all() and np.isnan(logp).all() and np.isnan(logperm), case.name
    else:
        assert method == -2 and not feasible, (case.name, method, t.logZprime)
        assert (assign == -1).all() and np.isnan(logp).all() and logperm == -np.inf, case.name
    return method
