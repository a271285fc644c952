"""numpy restatement of the clustered exact association probabilities (kbest_cluster.hip) for the tests.

    a = toProbs(cost) (R x C; the minimum of the WHOLE block)
    columns c and c' are adjacent when some row r has a[r][c] > 0 and a[r][c'] > 0; a cluster is a connected component of columns
    with every row that has a non-zero entry in one of them; a column without a non-zero entry is a cluster by itself
    label[c] = the lowest column of the cluster of c; clusters are ordered by label
    per cluster k: permanent_check.subset_sums on the sub-matrix (rows and columns in ascending order) gives w and Z_k,
        probs[c][min(r, nL)] += w[r][c] / Z_k
    logPerm = sum_k log Z_k in cluster order; some Z_k == 0: all zeros, logPerm = -inf, info = 0
    a cluster of more than 16 columns: info = -2; layers (R_k + 2) 2^m_k 8 bytes beyond slot_bytes: info = -3; zeros, logPerm NaN

The labels come from a union-find over the rows.  Cost blocks are column-major (nL+nM) x nM, as everywhere in this project."""
from __future__ import annotations

import numpy as np

import permanent_check as pc

MAX_SIZE = 16               # KBEST_CLUSTER_MAX_SIZE
SLOT_CAP = 64 << 20         # KBEST_CLUSTER_SLOT_CAP
REFUSED_SIZE, REFUSED_SLOT = -2, -3


def labels_of(A):
    """A: (R, C) non-negative.  label[c] = the lowest column of the connected component of column c (union-find over the rows)."""
    R, C = A.shape
    parent = list(range(C))

    def find(c):
        while parent[c] != c:
            parent[c] = parent[parent[c]]
            c = parent[c]
        return c

    for r in range(R):
        cols = np.flatnonzero(A[r] > 0.0)
        for c in cols[1:]:
            x, y = find(int(cols[0])), find(int(c))
            if x != y:
                parent[max(x, y)] = min(x, y)  # the root is the lowest column
    return np.array([find(c) for c in range(C)], dtype=np.int32)


def clusters_of(A):
    """[(columns, rows)] of every cluster in label order, both ascending; and the labels."""
    lab = labels_of(A)
    out = []
    for root in np.flatnonzero(lab == np.arange(A.shape[1])):
        cols = np.flatnonzero(lab == root)
        rows = np.flatnonzero((A[:, cols] > 0.0).any(axis=1))
        out.append((cols, rows))
    return out, lab


def clustered_probs(cost, nL, nM, a=None, slot_bytes=SLOT_CAP):
    """(probs [nM, nL+1], logPerm, info, maxCluster, label[nM]) of one frame.  a: the frame's toProbs matrix, flat column-major,
    when the caller has it from elsewhere."""
    nR = nL + nM
    a = pc.to_probs(cost) if a is None else a
    A = np.asarray(a, dtype=np.float64).reshape(nM, nR).T
    clusters, lab = clusters_of(A)
    maxc = max(len(cols) for cols, _ in clusters)
    probs = np.zeros((nM, nL + 1))
    if maxc > MAX_SIZE:
        return probs, float("nan"), REFUSED_SIZE, maxc, lab
    if any(((len(rows) + 2) << len(cols)) * 8 > slot_bytes for cols, rows in clusters):
        return probs, float("nan"), REFUSED_SLOT, maxc, lab
    logperm = 0.0
    for cols, rows in clusters:
        w, Z = (np.zeros((0, len(cols))), 0.0) if len(rows) == 0 else pc.subset_sums(A[np.ix_(rows, cols)])
        if not Z > 0.0:
            return np.zeros((nM, nL + 1)), float("-inf"), 0, maxc, lab
        logperm = logperm + float(np.log(Z))
        for i, r in enumerate(rows):
            probs[cols, min(int(r), nL)] += w[i] / Z
    return probs, logperm, len(clusters), maxc, lab


def operation_counts(cost, nL, nM):
    """(sum_k R_k 2^m_k m_k, R 2^M M) of one frame: the clustered and the whole-frame formula (R: rows that are non-zero)."""
    A = np.asarray(pc.to_probs(cost), dtype=np.float64).reshape(nM, nL + nM).T
    clusters, _ = clusters_of(A)
    R = int((A > 0.0).any(axis=1).sum())
    return sum(len(rows) * float(2 ** len(cols)) * len(cols) for cols, rows in clusters), R * float(2 ** nM) * nM


def assembled_frame():
    """Three conditioned kitti_like_frames(3, 6, 6, seed=99) blocks interleaved into one 36 x 18 frame: landmark r of part p ->
    row 3 r + p, column c -> 3 c + p, miss rows likewise.  Returns (frame, nL, nM, parts [(block, cL, nM)])."""
    import oracle_lib as ol
    from probabilisticsemslam_amd import workloads as wl
    parts = []
    for f in wl.kitti_like_frames(3, nL=6, nM=6, seed=99):
        cond, idx = ol.condition_costs(f, 12, 6)
        parts.append((cond, len(idx) - 6, 6))
    assert all(cL == 6 for _, cL, _ in parts)  # (nothing dropped: the interleaving below needs equal parts)
    nL, nM = 18, 18
    big = np.full((nL + nM, nM), np.inf)
    for p, (blk, cL, m) in enumerate(parts):
        A = np.asarray(blk).reshape(m, cL + m).T  # (rows, columns)
        for r in range(cL):
            big[3 * r + p, p::3] = A[r]
        for r in range(m):
            big[nL + 3 * r + p, p::3] = A[cL + r]
    return np.ascontiguousarray(big.T).reshape(-1), nL, nM, parts
