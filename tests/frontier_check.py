"""Python restatement of the frontier tier (kbest_frontier.hip, kbest_hybrid_frontier_probs_batch_f64) for the
tests.

    per cluster: its (nL_k + m_k) x m_k sub-block x, +inf for a zero, all-+inf rows left out; a'[r][c] = exp(colMin_c - x[r][c])
    as bigcluster_check.big_cluster; N_r the non-zero columns of row r as a bit mask
    the row order (greedy_plan): a pure function of the masks.  left[c] = unprocessed rows with c in N_r, seen = the union of N_r
    over the processed rows; of the unprocessed rows the one with the smallest (f, pk, r),
        pk(r) = |(seen | N_r) & {left > 0}|,  f(r) = |(seen | N_r) & {left - [c in N_r] > 0}|
    Phi_i = seen & {left > 0} before step i, Psi_i = Phi_i | (N_r \\ seen), W = max |Psi_i|;
    layers: sum_{i = 0 .. R} 2^|Phi_i| + 2 2^W doubles
    the sweep (frontier_sums): dicts keyed by the FULL mask of the columns used so far -- no bit compaction, no index maps.  After a
    row, a state that lacks a column whose last row this was is dropped.  Z' = F_R[all columns];
    w[r][c] = a'[r][c] sum_{S in F_i, c not in S} F_i[S] G_{i+1}[S | c]
    probs[c][min(r, nL_k)] += w[r][c] / Z';  log Z_k = log Z' - sum_c colMin_c
    info: 1 answered (Z' >= bigcluster_check.RANGE_MIN), 0 no complete assignment, -5 Z' below the range although the pattern has
    one (the same sweep on ones counts them), -4 W > max_width, -3 layers beyond slot_bytes (refusals: nothing written)
    the frame (hybrid_frontier_probs): bigcluster_check.hybrid_exact_probs with this tier first among the open clusters

Cost blocks are column-major (nL+nM) x nM, as everywhere in this project."""
from __future__ import annotations

import functools

import numpy as np

import bigcluster_check as bc
import cluster_check as cc
import hybrid_check as hc
import oracle_lib as ol
import permanent_check as pc
from probabilisticsemslam_amd import workloads as wl

MAX_COLS = 64          # KBEST_FRONTIER_MAX_COLS
MAX_WIDTH = 16         # KBEST_FRONTIER_MAX_WIDTH
SLOT = 4 << 20         # KBEST_FRONTIER_SLOT
REFUSED_SLOT, REFUSED_WIDTH = -3, -4


def popcount(x):
    return bin(x).count("1")


def row_masks(A):
    """A: (R, C) non-negative.  The non-zero columns of every row as an int."""
    return [sum(1 << int(c) for c in np.flatnonzero(row > 0.0)) for row in np.asarray(A)]


def greedy_plan(masks, m):
    """masks: N_r of every counting row.  Returns (steps, W, layer_doubles); steps: one dict per row in processing order with row,
    phi (open columns before it), new (N_r \\ seen), psi, closing, nxt (open columns after it)."""
    left = [sum((n >> c) & 1 for n in masks) for c in range(m)]
    todo = list(range(len(masks)))
    seen, steps, W = 0, [], 0
    layers = 0
    while todo:
        open_ = sum(1 << c for c in range(m) if left[c] > 0)
        last = sum(1 << c for c in range(m) if left[c] == 1)
        best = None
        for r in todo:
            reach = seen | masks[r]
            key = (popcount(reach & open_ & ~(masks[r] & last)), popcount(reach & open_), r)
            if best is None or key < best:
                best = key
        r = best[2]
        todo.remove(r)
        n = masks[r]
        phi, new = seen & open_, n & ~seen
        closing = n & last
        for c in range(m):
            left[c] -= (n >> c) & 1
        seen |= n
        steps.append(dict(row=r, phi=phi, new=new, psi=phi | new, closing=closing, nxt=(phi | new) & ~closing))
        W = max(W, best[1])
        layers += 1 << popcount(phi)
    layers += 1  # F_R: Phi_R is empty
    return steps, W, layers + 2 * (1 << W)


def layers_bytes(masks, m):
    return greedy_plan(masks, m)[2] * 8


def frontier_sums(a, order=None, dtype=np.float64):
    """a: (R, C) non-negative.  Returns (w (R, C), Z) as permanent_check.subset_sums; the rows are taken in `order` (the greedy
    order when None).  dtype: the arithmetic (np.longdouble for the tests' truth; float64 is the kernels')."""
    a = np.asarray(a, dtype=dtype)
    one, zero = a.dtype.type(1), a.dtype.type(0)
    R, C = a.shape
    masks = row_masks(a)
    if order is None:
        order = [s["row"] for s in greedy_plan(masks, C)[0]]
    full = (1 << C) - 1
    last_row = {}
    for i, r in enumerate(order):
        for c in range(C):
            if (masks[r] >> c) & 1:
                last_row[c] = i
    F = [{0: one}]
    for i, r in enumerate(order):
        cols = [c for c in range(C) if (masks[r] >> c) & 1]
        must = sum(1 << c for c in cols if last_row[c] == i)
        nxt = {}
        for S, v in F[i].items():  # (a row may stay unassigned)
            nxt[S] = nxt.get(S, zero) + v
        for c in cols:
            for S, v in F[i].items():
                if not (S >> c) & 1:
                    T = S | (1 << c)
                    nxt[T] = nxt.get(T, zero) + a[r, c] * v
        F.append({S: v for S, v in nxt.items() if S & must == must})
    Z = F[len(order)].get(full, zero)
    w = np.zeros((R, C), dtype=a.dtype)
    G = {full: one}
    for i in range(len(order) - 1, -1, -1):
        r = order[i]
        cols = [c for c in range(C) if (masks[r] >> c) & 1]
        prev = {}
        for S, v in F[i].items():
            g = G.get(S, zero)
            for c in cols:
                if not (S >> c) & 1:
                    t = G.get(S | (1 << c), zero)
                    w[r, c] += v * t
                    g += a[r, c] * t
            prev[S] = g
        w[r] *= a[r]
        G = prev
    return w, Z


def scaled_block(block, nLk, m):
    """(a' (R, m), the counting rows, colMin) of a flat column-major (nLk + m) x m sub-block."""
    X = np.asarray(block, dtype=np.float64).reshape(m, nLk + m).T
    fin = np.isfinite(X)
    colmin = np.where(fin, X, np.inf).min(axis=0)
    rows = np.flatnonzero(fin.any(axis=1))
    with np.errstate(invalid="ignore"):
        A = np.where(fin[rows], np.exp(colmin - X[rows]), 0.0)
    return A, rows, colmin


def frontier_cluster(block, nLk, m, slot_bytes=SLOT, max_width=MAX_WIDTH):
    """One sub-block.  Returns (probs [m, nLk + 1] or None when refused, logZ in the units a = exp(-x), info, W)."""
    A, rows, colmin = scaled_block(block, nLk, m)
    masks = row_masks(A)
    steps, W, layers = greedy_plan(masks, m)
    if W > max_width:
        return None, None, REFUSED_WIDTH, W
    if layers * 8 > slot_bytes:
        return None, None, REFUSED_SLOT, W
    probs = np.zeros((m, nLk + 1))
    if not np.isfinite(colmin).all():
        return probs, float("-inf"), 0, W
    order = [s["row"] for s in steps]
    w, Z = frontier_sums(A, order)
    if not Z >= bc.RANGE_MIN:
        fin = np.isfinite(np.asarray(block, dtype=np.float64).reshape(m, nLk + m).T[rows])
        if frontier_sums((A > 0.0).astype(np.float64), order)[1] > 0.0 or (fin & (A == 0.0)).any():
            return None, None, bc.OUT_OF_RANGE, W
        return probs, float("-inf"), 0, W
    for i, r in enumerate(rows):
        probs[:, min(int(r), nLk)] += w[i] / Z
    return probs, float(np.log(Z) - colmin.sum()), 1, W


def hybrid_frontier_probs(cost, nL, nM, k=0, condition=False, max_exact=cc.MAX_SIZE, max_big=bc.MAX_BIG, max_width=MAX_WIDTH,
                          slot_bytes=cc.SLOT_CAP, work_cap=bc.WORK_CAP, frontier_slot=SLOT):
    """One frame.  Returns (probs [nM, nL+1], method, opens, nFrontier, nBig, maxCluster, logPerm); opens: hybrid_check's dicts of
    the open clusters in label order with tier ('frontier', 'big' or 'kbest'), W and, for the exactly answered ones, logZ."""
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
                return zeros, -1, [], 0, 0, maxc, nan
            blk = np.full((cL + m, m), np.inf)
            blk[:R] = np.where(A[np.ix_(rows, cols)] > 0.0, X[np.ix_(rows, cols)], np.inf)
            opens.append(dict(root=int(cols[0]), m=m, nL=cL, R=R, rows=rows[:cL].astype(np.int32), cols=cols,
                              block=np.ascontiguousarray(blk.T).reshape(-1)))
        else:
            answered.append((cols, rows))
    logperm = 0.0
    for cols, rows in answered:
        w, Z = (np.zeros((0, len(cols))), 0.0) if len(rows) == 0 else pc.subset_sums(A[np.ix_(rows, cols)])
        if not Z > 0.0:
            return zeros, -2, [], 0, 0, maxc, float("-inf")
        logperm = logperm + float(np.log(Z))
        for i, r in enumerate(rows):
            probs[cols, min(int(r), nL)] += w[i] / Z
    infeasible = False
    for o in opens:
        o["tier"], o["W"] = "kbest", None
        if max_width > 0 and o["m"] <= MAX_COLS:
            p, lz, info, o["W"] = frontier_cluster(o["block"], o["nL"], o["m"], frontier_slot, min(max_width, MAX_WIDTH))
            if info >= 0:
                o["tier"], o["probs"], o["logZ"], o["info"] = "frontier", p, lz, info
                continue
        if 0 < o["m"] <= max_big and bc.layers_bytes(o["m"], o["nL"]) <= work_cap:
            p, lz, info = bc.big_cluster(o["block"], o["nL"], o["m"])
            if info >= 0:  # (declined: on to the enumeration)
                o["tier"], o["probs"], o["logZ"], o["info"] = "big", p, lz, info
    if k < 1 and any(o["tier"] == "kbest" for o in opens):
        return zeros, -1, opens, 0, 0, maxc, nan
    method, nfr, nbig = 0, 0, 0
    for o in opens:
        if o["tier"] in ("frontier", "big"):
            if o["info"] <= 0:
                infeasible = True
            else:
                nfr += o["tier"] == "frontier"
                nbig += o["tier"] == "big"
                logperm = logperm + (o["logZ"] + o["m"] * mn)
        else:
            o["probs"], nf = ol.assignment_prob(o["block"], o["nL"], o["m"], k)
            o["nf"] = int(nf)
            if nf <= 0:
                infeasible = True
            else:
                method = 2 if (nf >= k or method == 2) else 1
        p = o["probs"]
        probs[np.ix_(o["cols"], o["rows"])] = p[:, : o["nL"]]
        probs[o["cols"], nL] = p[:, o["nL"]]
    if infeasible:
        return zeros, -2, opens, 0, 0, maxc, float("-inf")
    return probs, method, opens, nfr, nbig, maxc, logperm


# ---- the smallest shapes at which the kernel can go wrong (tests/test_gpu_frontier.py, tests/test_frontier_cpu.py) -------------------
def flat(blk):
    return np.ascontiguousarray(np.asarray(blk, dtype=np.float64).T).reshape(-1)


def with_miss_rows(land, rng=None, miss=None):
    """(block, nL_k, m): the landmark rows `land` (nL_k x m, +inf for a zero) and one miss row per column."""
    land = np.asarray(land, dtype=np.float64)
    nLk, m = land.shape
    diag = np.full(m, 0.5) if rng is None else 0.2 + rng.random(m)
    if miss is not None:
        diag = np.where(miss, diag, np.inf)
    return flat(np.vstack([land, np.where(np.eye(m, dtype=bool), diag, np.inf)])), nLk, m


def two_rows_over(m):
    return with_miss_rows(0.1 + np.random.default_rng(m).random((2, m)), np.random.default_rng(100 + m))


@functools.lru_cache(maxsize=None)
def edge_clusters():
    """The smallest shapes at which the kernel can go wrong, by name."""
    rng = np.random.default_rng(42)
    out = {"one_by_one": (flat([[1.5]]), 0, 1), "two_by_one": (flat([[0.7], [1.2]]), 1, 1)}
    land = np.where(rng.random((5, 4)) < 0.6, rng.random((5, 4)) * 3.0, np.inf)
    out["fewer_states_than_a_wave"] = with_miss_rows(land, rng)
    out["more_states_than_the_workgroup"] = two_rows_over(12)  # W = 12: 4 096 states
    # column 4 lives in landmark row 1 alone (its miss row is a zero): it opens and closes there, between columns 1 and 2
    chain = np.full((3, 5), np.inf)
    chain[0, [0, 1]] = [0.3, 1.1]
    chain[1, [1, 2, 4]] = [0.9, 0.2, 0.6]
    chain[2, [2, 3]] = [1.4, 0.8]
    out["opens_and_closes_in_one_row"] = with_miss_rows(chain, rng, miss=np.array([1, 1, 1, 1, 0], bool))
    band = np.full((23, 24), np.inf)
    for r in range(23):
        band[r, [r, r + 1]] = rng.random(2) * 2.0
    out["band_of_24"] = with_miss_rows(band, rng)
    rows = np.full((300, 4), np.inf)  # more rows than the workgroup has lanes
    for r in range(300):
        rows[r, r % 4] = 1.0 + rng.random() * 4.0
        if r % 3 == 0:
            rows[r, (r + 1) % 4] = 1.0 + rng.random() * 4.0
    out["more_rows_than_lanes"] = with_miss_rows(rows, rng)
    out["width_16"] = two_rows_over(16)
    out["width_17"] = two_rows_over(17)
    out["same_only_row"] = (flat([[1.0, 2.0], [np.inf, np.inf], [np.inf, np.inf], [np.inf, np.inf]]), 2, 2)
    return out


# ---- the oversized clusters of the three scene families (tests/test_frontier_cpu.py, tests/test_frontier_sample_cpu.py) ------------
FAMILIES = ((200, 40, 24, 24), (200, 60, 40, 30), (64, 200, 128, 60))  # README.md: F, nL, nM, side


@functools.lru_cache(maxsize=None)
def scene(F, nL, nM, side):
    return wl.scene_frames(F, nL, nM, side)


@functools.lru_cache(maxsize=None)
def oversized(shape, condition):
    """[(frame, a' of the cluster (R, m))] of every cluster of more than 16 columns of the family.  Computed once."""
    _, nL, nM, _ = shape
    out = []
    for b, f in enumerate(scene(*shape)):
        _, A = hc.gated_block(f, nL, nM, condition)
        for cols, rows in cc.clusters_of(A)[0]:
            if len(cols) > cc.MAX_SIZE:
                out.append((b, A[np.ix_(rows, cols)]))
    return out


def raw_cluster(shape, frame, size):
    """The one oversized cluster of that frame with a = permanent_check.to_probs(frame), column-scaled as the tier does."""
    (A,) = [A for b, A in oversized(shape, False) if b == frame]
    assert A.shape == size
    return A / A.max(axis=0)
