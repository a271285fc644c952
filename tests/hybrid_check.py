"""numpy restatement of the hybrid association probabilities (kbest_hybrid_probs_batch_f64) for the tests.

    x = the frame's cost block, with condition: x - colMin[c] where x <= colMin[c] + 42, else +inf (conditionCosts; the rows it
        drops are all +inf and belong to no cluster)
    a = toProbs(x) (the minimum of the WHOLE block); clusters and labels as cluster_check.clusters_of
    a cluster of more than max_exact columns, or whose layers (R_k + 2) 2^m_k 8 bytes exceed slot_bytes, is OPEN
    every other cluster: permanent_check.subset_sums, exactly as cluster_check.clustered_probs; some Z_k == 0: zeros, method -2
    an open cluster, in label order: its rows in ascending order, nL_k of them < nL; more than m_k rows >= nL: the FRAME is refused
        (method -1, zeros).  Its sub-block is (nL_k + m_k) x m_k column-major: those rows (x where a > 0, else +inf), then rows of
        +inf; columns ascending.  oracle_lib.assignment_prob(sub-block, nL_k, m_k, k) -- the pinned CPU oracle -- gives
        [m_k][nL_k + 1] and nf; slot nL_k -> slot nL, landmark row i -> the cluster's i-th row.
    method: 0 nothing open; 1 every open cluster has nf < k; 2 some nf >= k; -2 infeasible (some nf == 0 too); -1 refused

Cost blocks are column-major (nL+nM) x nM, as everywhere in this project."""
from __future__ import annotations

import numpy as np

import cluster_check as cc
import oracle_lib as ol
import permanent_check as pc

GATE = 42.0


def gated_block(cost, nL, nM, condition=False):
    """(x, a): the (nR, nM) matrix toProbs is applied to and toProbs of it."""
    nR = nL + nM
    X = np.array(np.asarray(cost, dtype=np.float64).reshape(nM, nR).T)
    if condition:
        colmin = X.min(axis=0)
        with np.errstate(invalid="ignore"):
            X = np.where(X <= colmin + GATE, X - colmin, np.inf)
    A = pc.to_probs(X)
    return X, A


def hybrid_probs(cost, nL, nM, k, condition=False, max_exact=cc.MAX_SIZE, slot_bytes=cc.SLOT_CAP):
    """One frame.  Returns (probs [nM, nL+1], method, opens, info, maxCluster, label[nM]); opens: one dict per open cluster in label
    order with root, m, nL (= nL_k), R, nf, rows (its landmark rows, caller numbering), cols, block (flat column-major sub-block)
    and probs ([m, nL_k + 1])."""
    X, A = gated_block(cost, nL, nM, condition)
    clusters, lab = cc.clusters_of(A)
    maxc = max(len(cols) for cols, _ in clusters)
    zeros = np.zeros((nM, nL + 1))
    probs = zeros.copy()
    opens, answered = [], []
    for cols, rows in clusters:
        m, R = len(cols), len(rows)
        if m > max_exact or ((R + 2) << m) * 8 > slot_bytes:
            cL = int((rows < nL).sum())
            if R - cL > m:  # (whatever else the frame holds)
                return zeros, -1, [], -2, maxc, lab
            blk = np.full((cL + m, m), np.inf)
            blk[:R] = np.where(A[np.ix_(rows, cols)] > 0.0, X[np.ix_(rows, cols)], np.inf)
            opens.append(dict(root=int(cols[0]), m=m, nL=cL, R=R, rows=rows[:cL].astype(np.int32), cols=cols,
                              block=np.ascontiguousarray(blk.T).reshape(-1)))
        else:
            answered.append((cols, rows))
    for cols, rows in answered:
        w, Z = (np.zeros((0, len(cols))), 0.0) if len(rows) == 0 else pc.subset_sums(A[np.ix_(rows, cols)])
        if not Z > 0.0:
            return zeros, -2, [], 0, maxc, lab
        for i, r in enumerate(rows):
            probs[cols, min(int(r), nL)] += w[i] / Z
    method = 0
    for o in opens:
        p, nf = ol.assignment_prob(o["block"], o["nL"], o["m"], k)
        o["nf"], o["probs"] = int(nf), p
        if nf <= 0:
            method = -2
        elif method >= 0:
            method = 2 if (nf >= k or method == 2) else 1
        probs[np.ix_(o["cols"], o["rows"])] = p[:, : o["nL"]]
        probs[o["cols"], nL] = p[:, o["nL"]]
    if method == -2:
        probs = zeros
    return probs, method, opens, len(clusters), maxc, lab
