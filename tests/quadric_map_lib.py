"""Exact getAssignmentProbs from quadrics against a map of any size (kbest_quadric_map.hip): the scene generators and the numpy
restatement.  No GPU.

The restatement of a frame: the raw block from the oracle's cost builder (oracle_lib.quadric_costs), conditionCosts restated on it
(assignment.cpp:450-494: colMin over all nL + nM raw rows, a landmark row kept if some column has cost <= colMin + 42, an entry
x <= colMin + 42 ? x - colMin : +inf), the compact block -- kept landmark rows in order, then ALL nM dummy rows --, the exact tiers on
it by frontier_check.hybrid_frontier_probs(condition=False), and the expansion into the dense [nM, nL + 1] slice."""
from __future__ import annotations

import functools

import numpy as np

import frontier_check as fc
import oracle_lib as ol

CUT = 42.0  # assignment.cpp:9
TILE = 256  # KBEST_QUADRIC_MAP_TILE: landmark rows per workgroup of the passes over the map


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def draw_covs(rng, n):
    """n covariances Q diag(U(0.02, 0.06)^3) Q^T, symmetrised; Q from the QR of a normal 3 x 3 with the signs of R's diagonal fixed."""
    q, r = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    lam = rng.uniform(0.02, 0.06, size=(n, 3))
    cov = (q * lam[:, None, :]) @ np.transpose(q, (0, 2, 1))
    return (cov + np.transpose(cov, (0, 2, 1))) / 2


@functools.lru_cache(maxsize=None)
def make_map(seed, nMap, side, height):
    """(mean (nMap, 3), cov (nMap, 3, 3)).  Computed once; nobody changes it."""
    rng = np.random.default_rng(seed)
    mean = rng.random((nMap, 3)) * np.array([side, side, height], dtype=np.float64)
    cov = draw_covs(rng, nMap)
    mean.setflags(write=False)
    cov.setflags(write=False)
    return mean, cov


def make_frame(seed, mean, nM, hot, spread):
    """(measMean (nM, 3), measCov (nM, 3, 3)): measurements around `hot` centres, each near one of the `spread` landmarks nearest
    its centre."""
    rng = np.random.default_rng(seed)
    centres = mean[rng.integers(len(mean), size=hot)]
    mm = np.empty((nM, 3))
    for m in range(nM):
        c = centres[rng.integers(hot)]
        near = np.argsort(((mean - c) ** 2).sum(axis=1), kind="stable")[:spread]
        mm[m] = mean[near[rng.integers(spread)]] + 0.1 * rng.normal(size=3)
    return mm, draw_covs(rng, nM)


CHAIN = dict(map=(1, 5000, 45.0, 3.0), nM=40, hot=3, spread=25, gate=10.0)


@functools.lru_cache(maxsize=None)
def chain_frame(f):
    mean, _ = make_map(*CHAIN["map"])
    return make_frame(100 + f, mean, CHAIN["nM"], CHAIN["hot"], CHAIN["spread"])


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def raw_block(land_mean, land_cov, meas_mean, meas_cov, gate):
    """The (nL + nM, nM) raw cost matrix, bits of computeQuadricCostMatrix as the oracle restates it."""
    nL, nM = len(land_mean), len(meas_mean)
    flat = ol.quadric_costs(np.asarray(land_mean).reshape(-1, 3), np.asarray(land_cov).reshape(-1, 3, 3), meas_mean, meas_cov, gate)
    return np.array(flat.reshape(nM, nL + nM).T)


def compact(land_mean, land_cov, meas_mean, meas_cov, gate):
    """(rowIdx int32 [nKeep], the compact conditioned block flat column-major (nKeep + nM) x nM, the raw matrix)."""
    nL = len(land_mean)
    X = raw_block(land_mean, land_cov, meas_mean, meas_cov, gate)
    colmin = X.min(axis=0)
    with np.errstate(invalid="ignore"):
        good = X <= colmin + CUT
        C = np.where(good, X - colmin, np.inf)
    keep = np.flatnonzero(good[:nL].any(axis=1)).astype(np.int32)
    blk = np.vstack([C[keep], C[nL:]])
    return keep, np.ascontiguousarray(blk.T).reshape(-1), X


def expand(cprobs, rows, nL):
    """The dense [nM, nL + 1] slice of the compact [nM, nKeep + 1] one."""
    nM, nk = cprobs.shape[0], len(rows)
    out = np.zeros((nM, nL + 1))
    out[:, rows] = cprobs[:, :nk]
    out[:, nL] = cprobs[:, nk]
    return out


def restated(land_mean, land_cov, meas_mean, meas_cov, gate, k=0, max_exact=16, max_big=0, max_width=16):
    """One frame by the compact path.  Returns a dict: rows, ccost, cprobs [nM, nKeep + 1], probs [nM, nL + 1], method, opens,
    nFrontier, nBig, maxCluster, logPerm."""
    rows, cc, _ = compact(land_mean, land_cov, meas_mean, meas_cov, gate)
    nM = len(meas_mean)
    p, method, opens, nfr, nbig, maxc, lp = fc.hybrid_frontier_probs(cc, len(rows), nM, k, condition=False, max_exact=max_exact,
                                                                     max_big=max_big, max_width=max_width)
    return dict(rows=rows, ccost=cc, cprobs=p, probs=expand(p, rows, len(land_mean)), method=method, opens=opens, nFrontier=nfr,
                nBig=nbig, maxCluster=maxc, logPerm=lp)


def restated_raw(land_mean, land_cov, meas_mean, meas_cov, gate, k=0, max_exact=16, max_big=0, max_width=16):
    """The same frame by the parent's path: conditionCosts inside the tiers (condition=True) on the raw block."""
    X = raw_block(land_mean, land_cov, meas_mean, meas_cov, gate)
    flat = np.ascontiguousarray(X.T).reshape(-1)
    return fc.hybrid_frontier_probs(flat, len(land_mean), len(meas_mean), k, condition=True, max_exact=max_exact, max_big=max_big,
                                    max_width=max_width)


# ---- the smallest shapes at which the passes can go wrong ---------------------------------------------------------------------------------
def identity_frame(nL, kept, nM=1, far=1000.0):
    """nL landmarks and nM measurements with covariances 0.5 I each (S = I: the cost is |d|^2 exactly, in integers).  Measurement
    m sits at (100 m, 0, 0); the landmarks `kept` sit exactly on measurement (their position in the list) mod nM, every other one
    far away (cost >= far^2, dropped).  Returns (landMean, landCov, measMean, measCov)."""
    lm = np.zeros((nL, 3))
    lm[:, 1] = far + np.arange(nL)
    mm = np.zeros((nM, 3))
    mm[:, 0] = 100.0 * np.arange(nM)
    for i, r in enumerate(kept):
        lm[r] = mm[i % nM]
    half = np.broadcast_to(0.5 * np.eye(3), (nL, 3, 3)).copy()
    return lm, half, mm, np.broadcast_to(0.5 * np.eye(3), (nM, 3, 3)).copy()


def boundary_frame():
    """One column, identity covariances, gate 50: landmark 0 at d = 0 (cost 0 = colMin), landmark 1 at d = (4, 5, 1) (cost 42: kept,
    the comparison is <=), landmark 2 at d = (3, 3, 5) (43: dropped), landmark 3 far."""
    lm = np.array([[0.0, 0, 0], [4, 5, 1], [3, 3, 5], [500, 0, 0]])
    half = np.broadcast_to(0.5 * np.eye(3), (4, 3, 3)).copy()
    return lm, half, np.zeros((1, 3)), half[:1].copy()


def edge_kept(nL):
    """The rows to keep at nL: the first and the last landmark and the two either side of every tile boundary."""
    rows = {0, nL - 1}
    for t in range(TILE, nL, TILE):
        rows |= {t - 1, t}
    return sorted(r for r in rows if 0 <= r < nL)


@functools.lru_cache(maxsize=None)
def edge_batch():
    """(map_mean, map_cov, frames = [(landOff, nL, measMean, measCov)], gate): one map, every frame a window of it -- nL in
    {0, 1, T-1, T, T+1, 2T+3} x nM in {1, 128} with identity covariances, the kept rows exactly edge_kept(nL) (frames 0 .. 11);
    nothing kept (12); cost 0 / 42 / 43 in one column (13); two windows of a random map of 700 (14: landmarks 100 .. 699, 15:
    landmarks 0 .. 499).  Gate 50.  Computed once; nobody changes it."""
    parts, frames, at = [], [], 0

    def add(lm, lc, mm, mc, window=None):
        nonlocal at
        parts.append((lm, lc))
        lo, n = window or (0, len(lm))
        frames.append((at + lo, n, mm, mc))
        at += len(lm)

    for nL in (0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3):
        for nM in (1, 128):
            add(*identity_frame(nL, edge_kept(nL), nM))
    add(*identity_frame(300, [], 3))
    add(*boundary_frame())
    m3, c3 = make_map(3, 700, 12.0, 2.0)
    add(m3, c3, *make_frame(31, m3, 24, 3, 20), window=(100, 600))
    frames.append((at - 700, 500) + make_frame(32, m3[:500], 24, 3, 20))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), tuple(frames), 50.0


@functools.lru_cache(maxsize=None)
def limit_batch():
    """(map_mean, map_cov, frames, gate) for the bounds maxMap = 300, maxKeep = 8, maxCol = 4: a frame that keeps exactly 8 rows, one
    that keeps 9, one with nL = 301 > maxMap and one with nM = 5 > maxCol.  Gate 10."""
    a = identity_frame(300, [0, 5, 63, 64, 255, 256, 257, 299], 4)
    b = identity_frame(300, [0, 5, 63, 64, 128, 255, 256, 257, 299], 3)
    c = identity_frame(301, [0], 2)
    d = identity_frame(10, [0], 5)
    frames = ((0, 300, a[2], a[3]), (300, 300, b[2], b[3]), (600, 301, c[2], c[3]), (901, 10, d[2], d[3]))
    return np.concatenate([a[0], b[0], c[0], d[0]]), np.concatenate([a[1], b[1], c[1], d[1]]), frames, 10.0


@functools.lru_cache(maxsize=None)
def chain_restated(f, k):
    """The restatement of chain frame f (max_big = 0).  Computed once; nobody changes it."""
    mean, cov = make_map(*CHAIN["map"])
    mm, mc = chain_frame(f)
    return restated(mean, cov, mm, mc, CHAIN["gate"], k=k)


@functools.lru_cache(maxsize=None)
def window_restated(which, j, k=0, max_exact=16):
    """The restatement of frame j of edge_batch() / limit_batch() / a named batch.  Computed once; nobody changes it."""
    mean, cov, frames, gate = BATCHES[which]()
    off, nL, mm, mc = frames[j]
    return restated(mean[off:off + nL], cov[off:off + nL], mm, mc, gate, k=k, max_exact=max_exact)


@functools.lru_cache(maxsize=None)
def parity_batch():
    """Sixteen frames of map(1, 300, 12, 2), nM = 24, hot 3, spread 20, gate 10: small enough for the parent's path."""
    mean, cov = make_map(1, 300, 12.0, 2.0)
    return mean, cov, tuple((0, 300) + make_frame(200 + f, mean, 24, 3, 20) for f in range(16)), 10.0


@functools.lru_cache(maxsize=None)
def far_batch():
    """The six chain frames (landmarks 0 .. 4 999 of the map) and one frame of map(2, 100 000, 900, 3), nM = 24, hot 24, spread 1,
    behind them in the same map (landmarks 5 000 .. 104 999): kept rows beyond 65 535 catch 16-bit row numbers.  Gate 10."""
    m1, c1 = make_map(*CHAIN["map"])
    m2, c2 = make_map(2, 100000, 900.0, 3.0)
    frames = tuple((0, 5000) + chain_frame(f) for f in range(6)) + ((5000, 100000) + make_frame(7, m2, 24, 24, 1),)
    return np.concatenate([m1, m2]), np.concatenate([c1, c2]), frames, CHAIN["gate"]


BATCHES = dict(edge=edge_batch, limit=limit_batch, parity=parity_batch, far=far_batch)
