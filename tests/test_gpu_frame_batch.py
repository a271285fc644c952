"""GPU: the slice contract of the six host-pointer probability entries of include/kbest_c.h -- a frame's cost block and its
probability slice may lie anywhere in the caller's buffers, in any order; the answer does not depend on where, bit for bit, and
what lies between the slices (and behind the last one) in the caller's probs buffer is the caller's.  Through ctypes, so that the
offsets are the test's own."""
import functools

import numpy as np
import pytest

import probabilisticsemslam_amd as pk
from probabilisticsemslam_amd import workloads as wl
from probabilisticsemslam_amd.engine import _ptr

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
GAP = 7  # doubles in front of every block and every slice of the second layout, and behind the last slice of both


@pytest.fixture(scope="module")
def eng():
    e = pk.KBestEngine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def frames():
    """[(raw block, nL, nM)]: shapes and slice sizes differ within the batch.  With max_exact = 4 frames 0 .. 4 hold one open
    cluster each (of 6, 5, 10, 5 and 5 measurements), the others none."""
    fr = [(f, 14, 10) for f in wl.scene_frames(6, 14, 10, 12.0)]
    fr.append((wl.scene_frames(6, 10, 8, 8.0)[5], 10, 8))
    fr.append((wl.kitti_like_frames(1, nL=3, nM=3)[0], 3, 3))
    return fr


def layout(reverse):
    """(cost buffer, costOff, probs buffer pre-filled with the sentinel, probOff, mask of the doubles of probs that belong to no frame)."""
    fr = frames()
    B = len(fr)
    gap = GAP if reverse else 0
    costOff, probOff = np.zeros(B, np.int64), np.zeros(B, np.int64)
    cAt = pAt = 0
    for b in (range(B - 1, -1, -1) if reverse else range(B)):
        blk, nL, nM = fr[b]
        costOff[b], probOff[b] = cAt + gap, pAt + gap
        cAt += gap + blk.size
        pAt += gap + nM * (nL + 1)
    cost = np.full(cAt + GAP, SENTINEL)
    probs = np.full(pAt + GAP, SENTINEL)
    free = np.ones(probs.size, bool)
    for b, (blk, nL, nM) in enumerate(fr):
        cost[costOff[b]: costOff[b] + blk.size] = blk
        free[probOff[b]: probOff[b] + nM * (nL + 1)] = False
    assert free.sum() == (B * gap + GAP)
    return cost, costOff, probs, probOff, free


# name -> (per-frame scalar outputs in the entry's order: (name, dtype), call(lib, ctx, head, probs, probOff, outs))
# head: (B, nL, nM, cost, costOff, condition = 1)
ENTRIES = {
    "kbest_permanent_probs_batch_f64": (
        [("perm", np.float64)],
        lambda lib, ctx, h, p, po, o: lib.kbest_permanent_probs_batch_f64(ctx, *h, p, po, *o)),
    "kbest_belief_probs_batch_f64": (  # tol = 0: exactly maxIter sweeps
        [("iters", np.int32), ("resid", np.float64)],
        lambda lib, ctx, h, p, po, o: lib.kbest_belief_probs_batch_f64(ctx, *h, 0.0, 25, p, po, *o)),
    "kbest_clustered_probs_batch_f64": (
        [("logPerm", np.float64), ("info", np.int32), ("maxCluster", np.int32)],
        lambda lib, ctx, h, p, po, o: lib.kbest_clustered_probs_batch_f64(ctx, *h, p, po, *o, None, 0)),
    "kbest_hybrid_probs_batch_f64": (  # k = 200, maxExact = 4
        [("method", np.int32), ("nOpen", np.int32), ("maxCluster", np.int32)],
        lambda lib, ctx, h, p, po, o: lib.kbest_hybrid_probs_batch_f64(ctx, *h, 200, 4, p, po, *o)),
    "kbest_hybrid_exact_probs_batch_f64": (  # k = 0, maxExact = 4, maxBig = 20
        [("logPerm", np.float64), ("method", np.int32), ("nOpen", np.int32), ("nBig", np.int32), ("maxCluster", np.int32)],
        lambda lib, ctx, h, p, po, o: lib.kbest_hybrid_exact_probs_batch_f64(ctx, *h, 0, 4, 20, p, po, *o)),
    "kbest_hybrid_frontier_probs_batch_f64": (  # k = 200, maxExact = 4, maxBig = 5, maxWidth = 4: all three tiers in one call
        [("logPerm", np.float64), ("method", np.int32), ("nOpen", np.int32), ("nBig", np.int32), ("maxCluster", np.int32),
         ("nFrontier", np.int32)],
        lambda lib, ctx, h, p, po, o: lib.kbest_hybrid_frontier_probs_batch_f64(ctx, *h, 200, 4, 5, 4, p, po, *o)),
}


def as_bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


def run(eng, name, reverse):
    """One call: (probs buffer, probOff, mask of nobody's doubles, {scalar name: [B]})."""
    fr = frames()
    B = len(fr)
    cost, costOff, probs, probOff, free = layout(reverse)
    nL = np.array([f[1] for f in fr], np.int32)
    nM = np.array([f[2] for f in fr], np.int32)
    scalars, call = ENTRIES[name]
    outs = [np.full(B, -77, dt) for _, dt in scalars]
    rc = call(eng.lib, eng.ctx, (B, _ptr(nL), _ptr(nM), _ptr(cost), _ptr(costOff), 1), _ptr(probs), _ptr(probOff), [_ptr(o) for o in outs])
    assert rc == 0, (name, rc, eng.lib.kbest_last_error(eng.ctx).decode())
    return probs, probOff, free, {s[0]: o for s, o in zip(scalars, outs)}


@pytest.mark.parametrize("name", list(ENTRIES))
def test_slices_do_not_depend_on_the_layout(eng, name):
    fr = frames()
    pa, oa, fa, sa = run(eng, name, False)
    pb, ob, fb, sb = run(eng, name, True)
    for b, (_, nL, nM) in enumerate(fr):  # every frame, no exception
        n = nM * (nL + 1)
        a, r = pa[oa[b]: oa[b] + n], pb[ob[b]: ob[b] + n]
        assert np.array_equal(as_bits(a), as_bits(r)), (name, b, np.abs(a - r).max())
        assert not (a == SENTINEL).any(), (name, b)  # (a probability is never negative: the slice was written)
    for key in sa:
        assert len(sa[key]) == len(fr) and np.array_equal(as_bits(sa[key]), as_bits(sb[key])), (name, key, sa[key], sb[key])
    # gaps and tail: the caller's
    assert (pa[fa] == SENTINEL).all() and fa.sum() == GAP, name
    assert (pb[fb] == SENTINEL).all() and fb.sum() == (len(fr) + 1) * GAP, name
    print(name, {k: v.tolist() for k, v in sa.items()})
    if name == "kbest_hybrid_probs_batch_f64":  # the open path really ran: the enumeration ...
        assert (sa["method"] >= 1).any(), sa["method"]
        assert sa["nOpen"][:6].tolist() == [1, 1, 1, 1, 1, 0] and sa["method"][4] == 2, sa
    if name == "kbest_hybrid_exact_probs_batch_f64":  # ... and the big-cluster tier
        assert (sa["nBig"] >= 1).any(), sa["nBig"]
        assert sa["method"][4] == 0 and sa["nBig"][4] == 1, sa
    if name == "kbest_hybrid_frontier_probs_batch_f64":  # ... and frontier, big-cluster and enumeration side by side
        # (tests/frontier_check.hybrid_frontier_probs on these frames)
        assert sa["method"].tolist() == [0, 0, 2, 0, 0, 0, 0, 0], sa
        assert sa["nFrontier"].tolist() == [1, 0, 0, 1, 1, 0, 0, 0], sa
        assert sa["nBig"].tolist() == [0, 1, 0, 0, 0, 0, 0, 0], sa
        assert sa["nOpen"].tolist() == [1, 1, 1, 1, 1, 0, 0, 0], sa


@pytest.mark.parametrize("name", list(ENTRIES))
def test_no_frames_is_ok(eng, name):
    scalars, call = ENTRIES[name]
    assert call(eng.lib, eng.ctx, (0, None, None, None, None, 1), None, None, [None] * len(scalars)) == 0
