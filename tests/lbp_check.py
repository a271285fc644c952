"""numpy restatement of the belief-propagation association probabilities (kbest_lbp.hip) for the tests.

    a = toProbs(cost) (R x C, all-zero rows left out),  nu = 1
    one sweep, every entry from the previous nu (Jacobi):
        x[r][c]   = a[r][c] nu[r][c]
        s[r][c]   = sum_{r' != r} x[r'][c]
        mu[r][c]  = a[r][c] / s[r][c]  where a[r][c] > 0 (s = 0: +inf, a forced entry), 0 elsewhere
        nu'[r][c] = 1 / (1 + sum_{c' != c} mu[r][c'])
        resid     = max over a[r][c] > 0 of |nu'[r][c] - nu[r][c]|
    stop after the sweep whose resid <= tol, or after max_iter sweeps (tol <= 0: exactly max_iter sweeps)
    w = a nu,  probs[c][min(r, nL)] += w[r][c] / sum_r w[r][c];  a column whose w sums to 0: the frame is infeasible, all zeros.

Both exclusive sums are an exclusive prefix plus an exclusive suffix: sums over the OTHER terms, never total minus own, so a
forced entry (mu = inf) gives no inf - inf.  Cost blocks are column-major (nL+nM) x nM, as everywhere in this project."""
from __future__ import annotations

import numpy as np

import permanent_check as pc

INFEASIBLE = -2


def exclusive_sums(x, axis):
    """out[i] = sum_{j != i} x[j] along `axis`: exclusive prefix + exclusive suffix."""
    x = np.moveaxis(np.asarray(x, dtype=np.float64), axis, 0)
    pre = np.zeros_like(x)
    suf = np.zeros_like(x)
    if x.shape[0] > 1:
        pre[1:] = np.cumsum(x[:-1], axis=0)
        suf[:-1] = np.cumsum(x[:0:-1], axis=0)[::-1]
    return np.moveaxis(pre + suf, 0, axis)


def sweep(a, nu):
    """One Jacobi sweep on the (R, C) matrices a >= 0 and nu.  Returns (nu', resid)."""
    pos = a > 0.0
    s = exclusive_sums(a * nu, 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        mu = np.where(pos, a / np.where(pos, s, 1.0), 0.0)
        new = 1.0 / (1.0 + exclusive_sums(mu, 1))
    resid = float(np.abs(new - nu)[pos].max()) if pos.any() else 0.0
    return new, resid


def iterate(a, tol=1e-12, max_iter=10000):
    """The iteration on a (R, C).  Returns (nu, sweeps run, last resid)."""
    nu = np.ones_like(a)
    iters, resid = 0, 0.0
    while iters < max_iter:
        nu, resid = sweep(a, nu)
        iters += 1
        if tol > 0.0 and resid <= tol:
            break
    return nu, iters, resid


def fold(a, nu, rows, nL):
    """probs [C, nL+1] from w = a nu; rows[i]: the frame's row of matrix row i.  None when a column's w sums to 0."""
    w = a * nu
    S = w.sum(axis=0)
    if not (S > 0.0).all():
        return None
    probs = np.zeros((a.shape[1], nL + 1))
    q = w / S
    for i, r in enumerate(rows):
        probs[:, min(int(r), nL)] += q[i]
    return probs


def belief_probs(cost, nL, nM, tol=1e-12, max_iter=10000, a=None):
    """(probs [nM, nL+1], iters, resid) of one frame; iters = -2 and all zeros for an infeasible frame.  a: the frame's toProbs
    matrix, flat column-major, when the caller has it from elsewhere."""
    nR = nL + nM
    a = pc.to_probs(cost) if a is None else a
    A = np.asarray(a, dtype=np.float64).reshape(nM, nR).T
    rows = np.flatnonzero((A > 0.0).any(axis=1))
    A = np.ascontiguousarray(A[rows])
    probs = None
    iters, resid = INFEASIBLE, 0.0
    if len(rows):
        nu, iters, resid = iterate(A, tol, max_iter)
        probs = fold(A, nu, rows, nL)
    if probs is None:
        return np.zeros((nM, nL + 1)), INFEASIBLE, resid
    return probs, iters, resid


def exact_probs(cost, nL, nM):
    """The exact marginals of the same frame (permanent_check.subset_sums)."""
    return pc.permanent_probs(cost, nL, nM)[0]


def crowded_frame(rng, n=8, miss=10.0):
    """The slowly converging family: n landmarks, n measurements, every landmark plausible for every measurement (costs
    12 u u', as the plausible entries of workloads.kitti_like_frames) and a dear miss (its gate of 10)."""
    nR = 2 * n
    C = np.full(nR * n, np.inf)
    for c in range(n):
        C[c * nR: c * nR + n] = 12.0 * rng.random(n) * rng.random(n)
        C[c * nR + n + c] = miss
    return C
