"""numpy restatement of the draws from a table of k best assignments (kbest_table_sample.hip, kbest_hybrid_sample_assoc_batch_f64,
DESIGN.md section 20) for the tests.

    per problem: gain[0 .. nf-1] ascending, row4col[j][0 .. m-1] (what kBest2DCutoff returns)
        w_j = exp(gain_0 - gain_j) where gain_0 + cutoff > gain_j (strictly), else 0
        P_j = P_{j-1} + w_j from 0.0, one addition per slot in table order; total = P_{nf-1}
        draw s: T = u total; the FIRST j with T < P_j, else the last j with w_j > 0
        logTerm[s] = (gain_0 - gain_j) - log(total); assign[s][c] = row4col[j][c]; pick[s] = j
    u: Philox4x32-10 of sample_check, key (seed low, seed high), counter (sampleBase + s, 0x40000000 | clusterKey, frameKey low,
    frameKey high), words 0 and 1
    the frame (hybrid_sample_assoc): frontier_sample_check.hybrid_frontier_sample_assoc where k = 0; else its small clusters and
    its frontier clusters as there, and every open cluster the frontier tier does not take by oracle_lib.orc_kbest(sub, cL + m, m,
    k, cutoff = 42) and the draws above with clusterKey = the cluster's label; ONE loop over the open clusters in label order joins
    them; method, nOpen, nFrontier, maxCluster, logPerm: frontier_check.hybrid_frontier_probs(k, max_big = 0)

Besides the draws everything returns the smallest RELATIVE MARGIN min |T - P_j| / total over every slot of the table (a superset of
the comparisons any search makes), as sample_check does.  Cost blocks are column-major (nL+nM) x nM, as everywhere in this project."""
from __future__ import annotations

import collections
import functools

import numpy as np

import cluster_check as cc
import cluster_sample_check as csc
import frontier_check as fc
import frontier_sample_check as fsc
import oracle_lib as ol
import sample_check as sc

M32 = sc.M32
DOMAIN = 0x40000000   # bit 30 of the counter's second word: the table sampler's uniforms
MAX_KEY = 1 << 30     # clusterKey < 2^30
MAX_K = 4096          # KBEST_TABLE_SAMPLE_MAX_K
CUTOFF = 42.0
FrameDraws = collections.namedtuple("FrameDraws", "assign logp logperm method nopen nfrontier nenum maxc margin opens small_cols")


def counter(cluster_key):
    """Word 1 of the counter of a cluster."""
    assert 0 <= cluster_key < MAX_KEY
    return DOMAIN | cluster_key


def uniform(seed, draw, cluster_key, frame_key):
    """u of the draws `draw` (uint64 array of sampleBase + s) on the cluster with key cluster_key of the frame with key frame_key."""
    w = sc.philox4x32_10((draw, np.uint64(counter(int(cluster_key))), frame_key & M32, (frame_key >> 32) & M32),
                         (seed & M32, (seed >> 32) & M32))
    return (((w[1] << np.uint64(32)) | w[0]) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def table_weights(gain, nf, cutoff=CUTOFF):
    """(w[nf], P[nf], last): the weights, their running sums (sequential, from 0.0) and the last slot with a weight > 0 (-1: none)."""
    g = np.asarray(gain, dtype=np.float64)[:nf]
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.where(g[0] + cutoff > g, np.exp(g[0] - g), 0.0)
    P = np.zeros(nf)
    acc = 0.0
    for j in range(nf):
        acc = acc + float(w[j])
        P[j] = acc
    pos = np.nonzero(w > 0.0)[0]
    return w, P, (int(pos[-1]) if len(pos) else -1)


def pick_slots(P, last, T):
    """The first j with T < P[j] for every T, else last: the linear scan, stated as a count (P does not decrease)."""
    j = (~(T[:, None] < P[None, :])).sum(axis=1)  # slots with NOT T < P_j: all of them in front of the first one with it
    return np.where(j < len(P), j, last).astype(np.int32)


def sample_tables(row4col, gain, nf, n_sample, seed=0, cluster_key=0, frame_key=0, sample_base=0, cutoff=CUTOFF, m=None):
    """kbest_table_sample_f64_dev on ONE problem: row4col [k, maxCol], gain [k], nf.  Returns (assign int32 [n_sample, m], pick
    int32 [n_sample], logterm [n_sample], margin); nf <= 0 or no weight > 0: -1s, -1s, NaNs, inf."""
    r4c = np.asarray(row4col, dtype=np.int32)
    m = r4c.shape[1] if m is None else m
    nf = min(int(nf), r4c.shape[0])
    nothing = (np.full((n_sample, m), -1, np.int32), np.full(n_sample, -1, np.int32), np.full(n_sample, np.nan), np.inf)
    if nf <= 0:
        return nothing
    g = np.asarray(gain, dtype=np.float64)
    w, P, last = table_weights(g, nf, cutoff)
    if last < 0:
        return nothing
    total = P[nf - 1]
    draw = np.arange(sample_base, sample_base + n_sample, dtype=np.uint64)
    T = uniform(seed, draw, cluster_key, frame_key) * total
    pick = pick_slots(P, last, T)
    margin = float((np.abs(T[:, None] - P[None, :]) / total).min())
    logterm = (g[0] - g[pick]) - np.log(total)
    return r4c[pick, :m].copy(), pick, logterm, margin


def enumerate_cluster(o, k):
    """(nf, row4col [nf, m], gain [nf]) of an open cluster: kBest2DCutoff(k, 42) on its sub-block, in the engine's one order of exact
    ties where there are any (oracle_lib.canonical_kbest)."""
    N, M = o["nL"] + o["m"], o["m"]
    nf, r4c, _, g = ol.orc_kbest(o["block"], N, M, k, cutoff=CUTOFF)
    if nf > 1 and (np.diff(g[:nf]) == 0.0).any():
        nf, r4c, g, _, _ = ol.canonical_kbest(o["block"], N, M, k, cutoff=CUTOFF)
    nf = max(int(nf), 0)
    return nf, np.asarray(r4c[:nf]), np.asarray(g[:nf])


def hybrid_sample_assoc(cost, nL, nM, n_sample, k, seed=0, condition=False, frame_key=0, sample_base=0, max_exact=cc.MAX_SIZE,
                        max_width=fc.MAX_WIDTH, frontier_slot=fc.SLOT):
    """One frame.  Returns FrameDraws; opens: frontier_check.hybrid_frontier_probs' dicts (tier 'frontier' or 'kbest') with all_rows
    (raw) and, on a drawn frame, assign_local, logterm, margin and (tier 'kbest') pick, nf, row4col, gain."""
    if k == 0:
        d = fsc.hybrid_frontier_sample_assoc(cost, nL, nM, n_sample, seed, condition, frame_key, sample_base, max_exact, max_width,
                                             frontier_slot)
        return FrameDraws(d.assign, d.logp, d.logperm, d.method, d.nopen, d.nfrontier, 0, d.maxc, d.margin, d.opens, d.small_cols)
    import hybrid_check as hc
    assert 1 <= k <= MAX_K
    _, method, opens, nfr, _, maxc, logperm = fc.hybrid_frontier_probs(cost, nL, nM, k, condition, max_exact, 0, max_width,
                                                                       frontier_slot=frontier_slot)
    parts, _ = csc.cluster_parts(cost, nL, nM, condition)
    _, A = hc.gated_block(cost, nL, nM, condition)
    clusters, _ = cc.clusters_of(A)
    open_roots = {}
    for cols, rows in clusters:
        if len(cols) > max_exact or ((len(rows) + 2) << len(cols)) * 8 > cc.SLOT_CAP:
            open_roots[int(cols[0])] = rows
    for o in opens:
        o["all_rows"] = open_roots[o["root"]]
    small = [p for p in parts if int(p.cols[0]) not in open_roots]
    assign = np.full((n_sample, nM), -1, np.int32)
    small_cols = np.concatenate([p.cols for p in small]) if small else np.zeros(0, np.int64)
    if method < 0:
        return FrameDraws(assign, np.full(n_sample, np.nan), logperm, method, len(opens), 0, 0, maxc, np.inf, opens, small_cols)
    logp = np.zeros(n_sample)
    margin = np.inf
    for p in small:
        prod, mg = csc.walk_cluster(p, n_sample, seed, frame_key, sample_base, assign)
        logp = logp + (np.log(prod) - np.log(p.Z))
        margin = min(margin, mg)
    nenum = 0
    for o in opens:  # ONE loop in label order, whichever tier answered
        keys = fsc.open_row_keys(o, nL)
        if o["tier"] == "frontier":
            L = fsc.cluster_layers(o["block"], o["nL"], o["m"], frontier_slot)
            a, lt, mg = fsc.walk(L, keys, n_sample, seed, frame_key, sample_base)
        else:
            assert o["tier"] == "kbest"
            o["nf"], o["row4col"], o["gain"] = enumerate_cluster(o, k)
            a, o["pick"], lt, mg = sample_tables(o["row4col"], o["gain"], o["nf"], n_sample, seed, o["root"], frame_key, sample_base)
            nenum += 1
        o["assign_local"], o["logterm"], o["margin"] = a, lt, mg
        assign[:, o["cols"]] = np.where((a >= 0) & (a < o["R"]), keys[np.clip(a, 0, len(keys) - 1)], -1)
        logp = logp + lt
        margin = min(margin, mg)
    if not opens:  # the bits of the clustered sampler's sum
        logperm = 0.0
        for p in small:
            logperm = logperm + float(np.log(p.Z))
    return FrameDraws(assign, logp, logperm, method, len(opens), nfr, nenum, maxc, float(margin), opens, small_cols)


# ---- the cases of the tests: computed once, shared, read-only ------------------------------------------------------------------------
SMALL = fsc.SMALL
SEED = fsc.SEED
SIXTEEN = tuple(range(16))
K_GPU, N_GPU = 50, 512    # the frame cases of tests/test_gpu_table_sample.py


@functools.lru_cache(maxsize=None)
def frame_draws(shape, index, n_sample, k, max_exact=4, condition=True, seed=SEED, frame_key=None, sample_base=0, max_width=fc.MAX_WIDTH):
    _, nL, nM, _ = shape
    d = hybrid_sample_assoc(fsc.scene(*shape)[index], nL, nM, n_sample, k, seed, condition, index if frame_key is None else frame_key,
                            sample_base, max_exact, max_width)
    d.assign.setflags(write=False)
    d.logp.setflags(write=False)
    return d


DENSE = (18, 18)  # (nL, nM) of dense_frame
DENSE_K, DENSE_N = 60, 32


@functools.lru_cache(maxsize=None)
def dense_frame():
    """One dense cluster of 18 measurements (every entry within the gate): W = 18, so no exact tier of the draw entries takes it."""
    nL, nM = DENSE
    f = np.random.default_rng(18).uniform(0.0, 6.0, (nL + nM) * nM)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def dense_draws(k=DENSE_K, n_sample=DENSE_N, seed=SEED):
    return hybrid_sample_assoc(dense_frame(), *DENSE, n_sample, k, seed, False, 0)


BLOCKS = (14, 17)  # (nL, nM) of block_frame
BLOCKS_ALL = 600   # a k beyond the 501 assignments a 5 x 4 cluster with its miss rows has: every enumeration is complete


@functools.lru_cache(maxsize=None)
def block_frame(feasible):
    """Three clusters of 5 measurements x 4 landmarks and one of 2 x 2, in label order; the miss rows of the SECOND are +inf unless
    `feasible`: five columns on four rows, no assignment."""
    nL, nM = BLOCKS
    rng = np.random.default_rng(14)
    X = np.full((nL + nM, nM), np.inf)
    for j, (r0, c0, nr, nc) in enumerate(((0, 0, 4, 5), (4, 5, 4, 5), (8, 10, 4, 5), (12, 15, 2, 2))):
        X[r0: r0 + nr, c0: c0 + nc] = rng.uniform(0.0, 5.0, (nr, nc))
        if j != 1 or feasible:
            for c in range(c0, c0 + nc):
                X[nL + c, c] = rng.uniform(2.0, 4.0)
    f = fc.flat(X)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def block_draws(feasible, k=K_GPU, n_sample=64, seed=SEED):
    return hybrid_sample_assoc(block_frame(feasible), *BLOCKS, n_sample, k, seed, False, 7, 0, 4, 0)


BATCH_FRAME, BATCH_KEY, BATCH_N = 8, 1234567890123, 96  # the frame of the batch-of-forty case, its explicit key, its draws


def gpu_frame_cases():
    """{name: FrameDraws} of every frame case tests/test_gpu_table_sample.py compares with: the CPU suite asserts their margins."""
    out = {}
    for b in SIXTEEN:
        out[f"all_enumerated_{b}"] = frame_draws(SMALL, b, N_GPU, K_GPU, max_width=0)
        out[f"width_5_{b}"] = frame_draws(SMALL, b, 128, K_GPU, max_width=5)
    out["batch_of_forty"] = frame_draws(SMALL, BATCH_FRAME, BATCH_N, K_GPU, frame_key=BATCH_KEY, max_width=5)
    out["dense"] = dense_draws()
    out["blocks"] = block_draws(True)
    out["blocks_complete"] = block_draws(True, BLOCKS_ALL)
    return out


def handcrafted():
    """{name: (row4col [k, maxCol] int32, gain [k], nf, m)}: the smallest tables at which the kernel can go wrong."""
    rng = np.random.default_rng(20)

    def table(k, max_col, gains, m, nf=None):
        nf = len(gains) if nf is None else nf
        r4c = np.full((k, max_col), -7, np.int32)
        for j in range(min(len(gains), k)):
            r4c[j, :m] = rng.permutation(m + 3)[:m] + 10 * j  # (any numbers: the sampler copies them)
        g = np.full(k, np.nan)
        g[: len(gains)] = gains
        return r4c, g, nf, m

    edge = 3.0 + CUTOFF  # gain_0 + 42 exactly: never picked; one ulp below: kept
    out = {
        "nf_1": table(8, 5, [2.5], 5),
        "nf_0": table(8, 5, [], 5, nf=0),
        "nf_below_k": table(16, 6, np.sort(rng.uniform(1.0, 4.0, 11)), 6),
        "nf_equals_k": table(12, 6, np.sort(rng.uniform(1.0, 4.0, 12)), 6),
        "nf_beyond_k": table(12, 6, np.sort(rng.uniform(1.0, 4.0, 12)), 6, nf=40),  # (an nf beyond k counts as k)
        "cutoff_edge": table(8, 4, [3.0, 3.5, 4.0, np.nextafter(edge, 0.0), edge, edge + 1.0], 4),
        "equal_gains": table(8, 4, [1.0, 1.5, 1.5, 2.0], 4),
        "m_1": table(8, 1, np.sort(rng.uniform(0.0, 3.0, 8)), 1),
        "m_128": table(6, 128, np.sort(rng.uniform(0.0, 3.0, 5)), 128),
        "m_narrow": table(6, 9, np.sort(rng.uniform(0.0, 3.0, 6)), 4),  # m < maxCol: the stride is maxCol
        "k_4096": table(4096, 3, np.sort(rng.uniform(0.0, 9.0, 4096)), 3),
        "many_draws": table(40, 7, np.sort(rng.uniform(0.0, 6.0, 33)), 7),  # more than one round of 256 draws
    }
    return out


PACK_K, PACK_COLS, PACK_N = 12, 6, 40


@functools.lru_cache(maxsize=None)
def pack_problems():
    """70 problems of ONE call (k = 12, maxCol = 6): more than one launch of 64; m 1 .. 6 and nf 0 .. 14 in turn, and two problems
    with m outside 1 .. maxCol (info -1, untouched).  Returns ((row4col, gain, nf, m), ...)."""
    rng = np.random.default_rng(70)
    out = []
    for i in range(70):
        m = 0 if i == 20 else PACK_COLS + 1 if i == 66 else 1 + i % PACK_COLS
        nf = i % 15
        r4c = rng.integers(0, 50, (PACK_K, PACK_COLS)).astype(np.int32)
        g = np.full(PACK_K, np.nan)
        g[: min(nf, PACK_K)] = np.sort(rng.uniform(0.0, 5.0, min(nf, PACK_K)))
        out.append((r4c, g, nf, m))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pack_draws(i):
    """(assign, pick, logterm, margin) of pack_problems()[i]: clusterKey i, frameKey 1000 + i; None where m is out of range."""
    r4c, g, nf, m = pack_problems()[i]
    if m < 1 or m > PACK_COLS:
        return None
    return sample_tables(r4c, g, nf, PACK_N, HAND_SEED, i, 1000 + i, 3, m=m)


HAND_DRAWS = {"many_draws": 700}  # draws of a handcrafted case (default 64)
HAND_SEED = 77


@functools.lru_cache(maxsize=None)
def handcrafted_draws(name):
    """(assign, pick, logterm, margin) of a handcrafted table: clusterKey = its place in the list, frameKey 5, sampleBase 3."""
    cases = handcrafted()
    r4c, g, nf, m = cases[name]
    key = list(cases).index(name)
    return sample_tables(r4c, g, nf, HAND_DRAWS.get(name, 64), HAND_SEED, key, 5, 3, m=m)
