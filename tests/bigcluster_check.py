"""numpy restatement of the big-cluster tier (kbest_bigcluster.hip, kbest_hybrid_exact_probs_batch_f64) for
the tests.

    per cluster: its (nL_k + m_k) x m_k sub-block x (hybrid_check: the value toProbs is applied to, +inf for a zero)
    a'[r][c] = exp(colMin_c - x[r][c]), colMin_c the column's smallest finite entry inside the sub-block; all-+inf rows left out
    the recurrences of permanent_check on a' (vectorised over the subsets by halves, so that 20 columns take seconds)
    probs[c][min(r, nL_k)] += w[r][c] / Z';  log Z_k = log Z' - sum_c colMin_c  in the units a = exp(-x)
    answered (info 1) while Z' >= RANGE_MIN = 2^-970.  Below it, Z' = 0 included: the complete assignments of the pattern a' > 0 are
    counted by the same recurrence on ones; none, and no finite entry whose a' is 0: info 0 (zeros, log Z = -inf); else the cluster
    is declined, info OUT_OF_RANGE = -5, nothing written
    the frame: clusters as cluster_check.clusters_of; a cluster of at most max_exact columns whose layers fit the slot: exactly as
    cluster_check; an open one of at most max_big columns whose layers (nL_k + m_k + 3) 2^m_k 8 bytes fit work_cap: the sums
    above; whatever else is open, a cluster the tier declines included: hybrid_check's assignmentProb(k) on the sub-block, or,
    with k = 0, the frame is refused
    logPerm = sum of log Z_k over the exactly answered clusters in the frame's units a = exp(min - x): + m_k min for a big one

Cost blocks are column-major (nL+nM) x nM, as everywhere in this project."""
from __future__ import annotations

import numpy as np

import cluster_check as cc
import hybrid_check as hc
import oracle_lib as ol
import permanent_check as pc

MAX_BIG = 20          # KBEST_BIGCLUSTER_MAX_SIZE
WORK_CAP = 1 << 30    # KBEST_BIGCLUSTER_WORK_CAP
RANGE_MIN = 2.0 ** -970   # KB_RANGE_MIN_Z: the column-scaled tiers answer while Z' >= this
OUT_OF_RANGE = -5         # KBEST_INFO_OUT_OF_RANGE


def layers_bytes(m, nLk):
    """What a cluster needs of the work space: (rows + 3) 2^m 8 bytes, rows counted as the sub-block's nL_k + m."""
    return ((nLk + m + 3) << m) * 8


def _step(layer, row):
    out = layer.copy()
    for c in np.flatnonzero(row):
        o, l = out.reshape(-1, 2, 1 << c), layer.reshape(-1, 2, 1 << c)
        o[:, 1, :] += row[c] * l[:, 0, :]
    return out


def scaled_subset_sums(a):
    """a: (R, C) non-negative.  (w (R, C), Z) as permanent_check.subset_sums, by halves of the layers instead of index lists."""
    R, C = a.shape
    n = 1 << C
    F = np.zeros((R + 1, n))
    F[0, 0] = 1.0
    for i in range(R):
        F[i + 1] = _step(F[i], a[i])
    G = np.zeros(n)
    G[0] = 1.0
    w = np.zeros((R, C))
    for r in range(R - 1, -1, -1):
        T = np.ascontiguousarray(G[::-1])  # T[S] = G[all \ S]: G[all \ S \ c] = T[S | c]
        for c in np.flatnonzero(a[r]):
            w[r, c] = a[r, c] * np.sum(F[r].reshape(-1, 2, 1 << c)[:, 0, :] * T.reshape(-1, 2, 1 << c)[:, 1, :])
        G = _step(G, a[r])
    return w, F[R, n - 1]


def count_assignments(pattern):
    """pattern: (R, C) bool.  The number of ways to give every column a row of its own among its True entries, as a float."""
    layer = np.zeros(1 << pattern.shape[1])
    layer[0] = 1.0
    for row in pattern:
        layer = _step(layer, row.astype(np.float64))
    return layer[-1]


def big_cluster(block, nLk, m):
    """One sub-block (flat column-major (nLk + m) x m).  Returns (probs [m, nLk + 1], logZ in the units a = exp(-x), info); declined
    (info OUT_OF_RANGE): (None, None, info)."""
    X = np.asarray(block, dtype=np.float64).reshape(m, nLk + m).T
    fin = np.isfinite(X)
    colmin = np.where(fin, X, np.inf).min(axis=0)
    rows = np.flatnonzero(fin.any(axis=1))
    probs = np.zeros((m, nLk + 1))
    if not np.isfinite(colmin).all() or len(rows) < m:
        return probs, float("-inf"), 0
    with np.errstate(invalid="ignore"):
        A = np.where(fin[rows], np.exp(colmin - X[rows]), 0.0)
    w, Z = scaled_subset_sums(A)
    if not Z >= RANGE_MIN:
        if count_assignments(A > 0.0) > 0.0 or (fin[rows] & (A == 0.0)).any():
            return None, None, OUT_OF_RANGE
        return probs, float("-inf"), 0
    for i, r in enumerate(rows):
        probs[:, min(int(r), nLk)] += w[i] / Z
    return probs, float(np.log(Z) - colmin.sum()), 1


def hybrid_exact_probs(cost, nL, nM, k=0, condition=False, max_exact=cc.MAX_SIZE, max_big=MAX_BIG, slot_bytes=cc.SLOT_CAP,
                       work_cap=WORK_CAP):
    """One frame.  Returns (probs [nM, nL+1], method, opens, nBig, maxCluster, logPerm); opens: hybrid_check's dicts of the open
    clusters in label order, with big=True and logZ for the ones the tier answers."""
    X, A = hc.gated_block(cost, nL, nM, condition)
    mn = X.min()
    clusters, lab = cc.clusters_of(A)
    maxc = max(len(cols) for cols, _ in clusters)
    zeros = np.zeros((nM, nL + 1))
    probs = zeros.copy()
    nan = float("nan")
    opens, answered = [], []
    for cols, rows in clusters:
        m, R = len(cols), len(rows)
        if m > max_exact or ((R + 2) << m) * 8 > slot_bytes:
            cL = int((rows < nL).sum())
            if R - cL > m:  # (whatever else the frame holds)
                return zeros, -1, [], 0, maxc, nan
            blk = np.full((cL + m, m), np.inf)
            blk[:R] = np.where(A[np.ix_(rows, cols)] > 0.0, X[np.ix_(rows, cols)], np.inf)
            opens.append(dict(root=int(cols[0]), m=m, nL=cL, R=R, rows=rows[:cL].astype(np.int32), cols=cols,
                              block=np.ascontiguousarray(blk.T).reshape(-1),
                              big=bool(0 < m <= max_big and layers_bytes(m, cL) <= work_cap)))
        else:
            answered.append((cols, rows))
    logperm = 0.0
    for cols, rows in answered:
        w, Z = (np.zeros((0, len(cols))), 0.0) if len(rows) == 0 else pc.subset_sums(A[np.ix_(rows, cols)])
        if not Z > 0.0:
            return zeros, -2, [], 0, maxc, float("-inf")
        logperm = logperm + float(np.log(Z))
        for i, r in enumerate(rows):
            probs[cols, min(int(r), nL)] += w[i] / Z
    for o in opens:
        if o["big"]:
            o["probs"], o["logZ"], o["info"] = big_cluster(o["block"], o["nL"], o["m"])
            o["big"] = o["info"] >= 0  # (declined: on to the enumeration)
    if k < 1 and any(not o["big"] for o in opens):
        return zeros, -1, opens, 0, maxc, nan
    method, nbig = 0, 0
    for o in opens:
        if o["big"]:
            p, info = o["probs"], o["info"]
            if info <= 0:
                method = -2
            else:
                nbig += 1
                logperm = logperm + (o["logZ"] + o["m"] * mn)
        else:
            p, nf = ol.assignment_prob(o["block"], o["nL"], o["m"], k)
            o["nf"] = int(nf)
            if nf <= 0:
                method = -2
            elif method >= 0:
                method = 2 if (nf >= k or method == 2) else 1
        o["probs"] = p
        probs[np.ix_(o["cols"], o["rows"])] = p[:, : o["nL"]]
        probs[o["cols"], nL] = p[:, o["nL"]]
    if method == -2:
        return zeros, -2, opens, 0, maxc, float("-inf")
    return probs, method, opens, nbig, maxc, logperm
