"""numpy restatement of the exact association probabilities (permanentProb) for the tests: the column-subset recurrences of
DESIGN.md section 9, vectorised over the subsets, and the plain permutation sum they are pinned against.

    F[0][{}] = 1,  F[i+1][S] = F[i][S] + sum_{c in S} a[i][c] F[i][S \\ {c}]
    G[R][{}] = 1,  G[i][S]   = G[i+1][S] + sum_{c in S} a[i][c] G[i+1][S \\ {c}]
    Z = F[R][all],  w[r][c] = a[r][c] sum_{S in all \\ {c}} F[r][S] G[r+1][all \\ {c} \\ S],  probs[c][min(r, nL)] += w[r][c] / Z

Cost blocks are column-major (nL+nM) x nM, as everywhere in this project."""
from __future__ import annotations

import itertools

import numpy as np

GATE = 42.0  # assignment.cpp:9


def to_probs(block):
    """toProbs (assignment.cpp:527-542): exp(min - c) where min + 42 > c, else 0; min over the whole block."""
    x = np.asarray(block, dtype=np.float64)
    m = x.min()
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(m + GATE > x, np.exp(m - x), 0.0)


def _as_matrix(flat, nR, nM):
    return np.asarray(flat, dtype=np.float64).reshape(nM, nR).T  # (nR, nM)


def subset_sums(a):
    """a: (R, C) non-negative.  Returns (w (R, C) with w[r][c] = a[r][c] perm(a without row r and column c), Z = perm(a))."""
    R, C = a.shape
    n = 1 << C
    S = np.arange(n)
    full = n - 1
    has = [((S >> c) & 1).astype(bool) for c in range(C)]

    def step(layer, row):
        out = layer.copy()
        for c in range(C):
            if row[c] != 0.0:
                out[has[c]] += row[c] * layer[S[has[c]] ^ (1 << c)]
        return out

    F = np.zeros((R + 1, n))
    F[0, 0] = 1.0
    for i in range(R):
        F[i + 1] = step(F[i], a[i])
    G = np.zeros(n)
    G[0] = 1.0
    w = np.zeros((R, C))
    for r in range(R - 1, -1, -1):
        for c in range(C):
            if a[r, c] != 0.0:
                s = S[~has[c]]
                w[r, c] = a[r, c] * np.dot(F[r, s], G[(full ^ (1 << c)) ^ s])
        G = step(G, a[r])
    return w, F[R, full]


def fold(w, Z, nL):
    """probs[c][min(r, nL)] += w[r][c] / Z; all zeros when Z == 0."""
    R, C = w.shape
    probs = np.zeros((C, nL + 1))
    if Z > 0.0:
        for r in range(R):
            probs[:, min(r, nL)] += w[r] / Z
    return probs


def permanent_probs(cost, nL, nM, a=None):
    """Exact probs [nM, nL+1] and the permanent Z of the block's toProbs matrix (a: that matrix, flat column-major, when the
    caller has it from elsewhere)."""
    nR = nL + nM
    a = to_probs(cost) if a is None else a
    w, Z = subset_sums(_as_matrix(a, nR, nM))
    return fold(w, Z, nL), Z


def permutation_sum(cost, nL, nM):
    """The same by the sum over all injections columns -> rows of the product of the gated entries (O(R!/(R-C)!))."""
    nR = nL + nM
    A = _as_matrix(to_probs(cost), nR, nM)
    perms = np.array(list(itertools.permutations(range(nR), nM)), dtype=np.int64).reshape(-1, nM)
    wgt = np.ones(len(perms))
    for c in range(nM):
        wgt = wgt * A[perms[:, c], c]
    Z = wgt.sum()
    probs = np.zeros((nM, nL + 1))
    slot = np.minimum(perms, nL)
    for c in range(nM):
        np.add.at(probs[c], slot[:, c], wgt)
    return (probs / Z if Z > 0.0 else np.zeros_like(probs)), Z


def scatter_back(cprobs, idx, nL, nM):
    """getAssignmentProbs' scatter (assignment.cpp:68-74): conditioned probs [nM, condL+1] -> [nM, nL+1] by rowIdx."""
    condL = len(idx) - nM
    out = np.zeros((nM, nL + 1))
    for l in range(condL):
        out[:, idx[l]] = cprobs[:, l]
    out[:, nL] = cprobs[:, condL]
    return out
