"""Joint associations from quadrics against a map of any size (kbest_quadric_map_sample_assoc_batch_f64[_dev]): the numpy
restatement and the shared cases of the tests.  No GPU.

The restatement of a frame: quadric_map_lib.compact (the kept rows and the compact conditioned block), the draws of
frontier_sample_check.hybrid_frontier_sample_assoc on it with condition = False, and the compact rows mapped back to the rows of
the notional raw (nL + nM) x nM block -- v < 0 stays -1, v < nKeep becomes rowIdx[v], otherwise nL + (v - nKeep)."""
from __future__ import annotations

import functools

import numpy as np

import frontier_check as fc
import frontier_sample_check as fsc
import quadric_map_lib as qm

SEED = fsc.SEED
N = 5                   # draws a frame unless a test says otherwise
STAT_DRAWS = 8192       # ... of the statistical check
STAT_SEED = 20240229    # ... and its one fixed seed
SPARSE = dict(map=(1, 5000, 200.0, 3.0), nM=24, hot=24, spread=1, gate=10.0)  # the sparse frames of tests/test_gpu_quadric_map.py


def map_rows(assign, rows, nL):
    """Compact rows to the rows of the raw block."""
    a = np.asarray(assign)
    nk = len(rows)
    out = a.copy()
    kept = (a >= 0) & (a < nk)
    out[kept] = np.asarray(rows)[a[kept]]
    miss = a >= nk
    out[miss] = nL + (a[miss] - nk)
    return out


def restated(land_mean, land_cov, meas_mean, meas_cov, gate, n_sample, seed=SEED, frame_key=0, sample_base=0, max_exact=16,
             max_width=fc.MAX_WIDTH):
    """One frame.  Returns a dict: rows, ccost, compact (the FrameDraws on the compact block), assign (raw rows), logp, method,
    nOpen, nFrontier, maxCluster, logPerm, margin."""
    rows, cc, _ = qm.compact(land_mean, land_cov, meas_mean, meas_cov, gate)
    d = fsc.hybrid_frontier_sample_assoc(cc, len(rows), len(meas_mean), n_sample, seed, False, frame_key, sample_base, max_exact,
                                         max_width)
    return dict(rows=rows, ccost=cc, compact=d, assign=map_rows(d.assign, rows, len(land_mean)), logp=d.logp, method=d.method,
                nOpen=d.nopen, nFrontier=d.nfrontier, maxCluster=d.maxc, logPerm=d.logperm, margin=d.margin)


@functools.lru_cache(maxsize=None)
def chain_draws(f, n_sample=N, frame_key=None, sample_base=0, max_width=fc.MAX_WIDTH):
    """The restated draws of chain frame f under key f (or frame_key).  Computed once; nobody changes it."""
    mean, cov = qm.make_map(*qm.CHAIN["map"])
    mm, mc = qm.chain_frame(f)
    return restated(mean, cov, mm, mc, qm.CHAIN["gate"], n_sample, frame_key=f if frame_key is None else frame_key,
                    sample_base=sample_base, max_width=max_width)


@functools.lru_cache(maxsize=None)
def sparse_batch():
    """(map_mean, map_cov, frames = [(landOff, nL, measMean, measCov)], gate): four frames against a sparse map of 5 000 -- a few
    dozen kept rows, small clusters only.  Computed once; nobody changes it."""
    mean, cov = qm.make_map(*SPARSE["map"])
    frames = tuple((0, 5000) + qm.make_frame(300 + f, mean, SPARSE["nM"], SPARSE["hot"], SPARSE["spread"]) for f in range(4))
    return mean, cov, frames, SPARSE["gate"]


@functools.lru_cache(maxsize=None)
def sparse_restated(f):
    """quadric_map_lib.restated of sparse frame f: the exact marginals.  Computed once; nobody changes it."""
    mean, cov, frames, gate = sparse_batch()
    return qm.restated(mean, cov, frames[f][2], frames[f][3], gate)


def frequencies(assign, nL):
    """[nM, nL + 1]: how often measurement c took landmark l, or (slot nL) its miss row, over the draws."""
    n, nM = assign.shape
    out = np.zeros((nM, nL + 1))
    for c in range(nM):
        a = assign[:, c]
        assert ((a >= 0) & ((a < nL) | (a == nL + c))).all(), c  # a landmark, or the column's own miss row
        np.add.at(out[c], np.minimum(a, nL), 1.0)
    return out / n


def worst_excess(freq, p, n):
    """max over all (measurement, landmark or miss) of |freq - p| - (5 sqrt(p (1 - p) / n) + 1 / n): the binomial five-sigma bound
    holds where this is <= 0."""
    return float((np.abs(freq - p) - (5.0 * np.sqrt(p * (1.0 - p) / n) + 1.0 / n)).max())


def worst_sigmas(freq, p, n):
    """max |freq - p| / sqrt(p (1 - p) / n) over the entries with 0 < p < 1: for the record, the assertion is worst_excess."""
    open_ = (p > 0.0) & (p < 1.0)
    return float((np.abs(freq - p)[open_] / np.sqrt(p[open_] * (1.0 - p[open_]) / n)).max()) if open_.any() else 0.0


def enumerated_rows(f, k=50):
    """The rows (nL_k + m_k) of every sub-block of chain frame f that kbest_hybrid_sample_assoc_batch_f64(k) would enumerate: the
    open clusters the frontier sampler does not take."""
    return [o["nL"] + o["m"] for o in qm.chain_restated(f, k)["opens"] if o["tier"] == "kbest"]
