"""numpy restatement of the draws from the exact posterior by gated clusters (kbest_cluster_sample.hip) for
the tests: the clusters of cluster_check.clusters_of on the frame's ACTIVE rows, per cluster the layers of
sample_check.forward_layers and the walk of sample_check.sample_assoc with the kernel's order of additions -- but the uniform of a
cluster's row is sample_check.uniforms(seed, draw, i, key) with i the row's index among the frame's active rows, not inside the
cluster.

    logProb[s] = sum_k (log prod_k a - log Z_k), one term per cluster, left to right in label order from 0.0
    logPerm = sum_k log Z_k likewise; info = the number of clusters
    a cluster of more than 16 columns: info = -2; layers (R_k + 2) 2^m_k 8 bytes beyond slot_bytes: -3; assign -1, logProb NaN,
    logPerm NaN;  some Z_k == 0: assign -1, logProb NaN, logPerm -inf, info 0

Returns the smallest RELATIVE MARGIN min |T - acc| / tot over every comparison made, as sample_check does.  Cost blocks are
column-major (nL+nM) x nM, as everywhere in this project."""
from __future__ import annotations

import collections
import functools

import numpy as np

import cluster_check as cc
import sample_check as sc

ClusterDraws = collections.namedtuple("ClusterDraws", "assign logp logperm info maxc margin n")
# one cluster as the walk sees it: a (R, m), F (R+1, 2^m), Z, cols (m) frame columns, gidx (R) active-row indices, raw (R) raw rows
ClusterPart = collections.namedtuple("ClusterPart", "a F Z cols gidx raw")


def walk_cluster(part, n_sample, seed, frame_key, sample_base, assign):
    """The walk of sample_check.sample_assoc on one cluster, vectorised over the draws; writes the cluster's columns of assign.
    Returns (prod [n_sample], margin)."""
    a, F, Z, cols, gidx, raw = part
    R, m = a.shape
    full = (1 << m) - 1
    draw = np.arange(sample_base, sample_base + n_sample, dtype=np.uint64)
    S = np.full(n_sample, full, np.int64)
    prod = np.ones(n_sample)
    margin = np.inf
    for i in range(R - 1, -1, -1):
        live = S != 0
        if not live.any():
            break
        tot = F[i + 1][S]
        T = sc.uniforms(seed, draw, int(gidx[i]), frame_key) * tot
        acc = F[i][S]
        margin = min(margin, (np.abs(T - acc) / tot)[live].min())
        walking = live & ~(T < acc)
        take = np.full(n_sample, -1)
        for c in range(m):
            if a[i, c] == 0.0:
                continue
            on = walking & (((S >> c) & 1) == 1)
            if not on.any():
                continue
            term = a[i, c] * F[i][S ^ (on.astype(np.int64) << c)]
            acc = np.where(on, acc + term, acc)
            take = np.where(on & (term > 0.0), c, take)
            margin = min(margin, (np.abs(T - acc) / tot)[on].min())
            walking = walking & ~(on & (T < acc))
        for c in range(m):
            got = take == c
            assign[got, cols[c]] = raw[i]
            S = np.where(got, S ^ (1 << c), S)
            prod = np.where(got, prod * a[i, c], prod)
    assert (S == 0).all()  # a state is only entered through a term > 0: every column of the cluster is taken by some row
    return prod, margin


def cluster_parts(cost, nL, nM, condition=False):
    """[ClusterPart] of a frame in label order (F, Z = None where the cluster is beyond 16 columns), and the largest cluster."""
    a, raw = sc.gated_rows(cost, nL, nM, condition)
    keep = (a > 0.0).any(axis=1)
    a, raw = a[keep], raw[keep]  # the ACTIVE rows: their index here is the i of u(s, i)
    clusters, _ = cc.clusters_of(a)
    parts = []
    for cols, rows in clusters:
        sub = a[np.ix_(rows, cols)]
        R, m = sub.shape
        if m > cc.MAX_SIZE:
            parts.append(ClusterPart(sub, None, None, cols, rows, raw[rows]))
            continue
        F = sc.forward_layers(sub) if R else np.zeros((1, 1 << m))
        Z = F[R, (1 << m) - 1] if R >= m else 0.0
        parts.append(ClusterPart(sub, F, Z, cols, rows, raw[rows]))
    return parts, max(len(p.cols) for p in parts)


def clustered_sample_assoc(cost, nL, nM, n_sample, seed=0, condition=False, frame_key=0, sample_base=0, slot_bytes=cc.SLOT_CAP):
    """Returns ClusterDraws: assign int32 [n_sample, nM] (the raw row every column takes), logProb [n_sample], logPerm, info,
    maxCluster, margin, n_sample."""
    parts, maxc = cluster_parts(cost, nL, nM, condition)
    assign = np.full((n_sample, nM), -1, np.int32)
    nan = np.full(n_sample, np.nan)
    if maxc > cc.MAX_SIZE:
        return ClusterDraws(assign, nan, float("nan"), cc.REFUSED_SIZE, maxc, np.inf, n_sample)
    if any(((len(p.gidx) + 2) << len(p.cols)) * 8 > slot_bytes for p in parts):
        return ClusterDraws(assign, nan, float("nan"), cc.REFUSED_SLOT, maxc, np.inf, n_sample)
    if any(not p.Z > 0.0 for p in parts):
        return ClusterDraws(assign, nan, float("-inf"), 0, maxc, np.inf, n_sample)
    logp = np.zeros(n_sample)
    logperm = 0.0
    margin = np.inf
    for p in parts:
        prod, mg = walk_cluster(p, n_sample, seed, frame_key, sample_base, assign)
        logp = logp + (np.log(prod) - np.log(p.Z))
        logperm = logperm + float(np.log(p.Z))
        margin = min(margin, mg)
    return ClusterDraws(assign, logp, logperm, len(parts), maxc, margin, n_sample)


@functools.lru_cache(maxsize=None)
def scene_draws(F, nL, nM, side, n_sample, condition=False, seed=sc.SEED):
    """The draws of every frame of scene_frames(F, nL, nM, side), frameKey = b.  Computed once, shared, read-only."""
    from probabilisticsemslam_amd import workloads as wl
    out = []
    for b, f in enumerate(wl.scene_frames(F, nL, nM, side)):
        d = clustered_sample_assoc(f, nL, nM, n_sample, seed=seed, condition=condition, frame_key=b)
        for x in d[:2]:
            x.setflags(write=False)
        out.append(d)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def assembled_draws(n_sample, seed=sc.SEED, frame_key=0):
    """(frame, nL, nM, parts, ClusterDraws) of cluster_check.assembled_frame()."""
    f, nL, nM, parts = cc.assembled_frame()
    d = clustered_sample_assoc(f, nL, nM, n_sample, seed=seed, frame_key=frame_key)
    for x in d[:2]:
        x.setflags(write=False)
    return f, nL, nM, parts, d
