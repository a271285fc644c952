"""GPU: the slice contract of the four host-pointer draw entries of include/kbest_c.h -- a frame's draws (assign [nSample][nM],
logProb [nSample]) may lie anywhere in the caller's buffers, in any order; the draws do not depend on where, bit for bit, and what
lies between them (and behind the last) is the caller's.  The last entry sends the open clusters of one call through all three
legs (frontier sampler, enumeration, table sampler).  Through ctypes, so that the offsets are the test's own."""
import numpy as np
import pytest

import probabilisticsemslam_amd as pk
from probabilisticsemslam_amd.engine import _ptr
from test_gpu_frame_batch import as_bits, frames

pytestmark = pytest.mark.gpu

N_SAMPLE = 5
SEED = 2024
GAP = 7            # elements in front of every frame's draws in the second layout, and behind the last
ASG_SENTINEL = -77777  # (a row is >= -1)
LP_SENTINEL = 7.25     # (a logProb is <= 0 or NaN)
BAD_ARG = -2  # KBEST_ERR_BAD_ARG


@pytest.fixture(scope="module")
def eng():
    e = pk.KBestEngine(0)
    yield e
    e.close()


def layout(reverse):
    """(assign and logProb pre-filled with their sentinels, asgOff, lpOff, masks of the elements that belong to no frame)."""
    fr = frames()
    B = len(fr)
    gap = GAP if reverse else 0
    asgOff, lpOff = np.zeros(B, np.int64), np.zeros(B, np.int64)
    aAt = lAt = 0
    for b in (range(B - 1, -1, -1) if reverse else range(B)):
        asgOff[b], lpOff[b] = aAt + gap, lAt + gap
        aAt += gap + N_SAMPLE * fr[b][2]
        lAt += gap + N_SAMPLE
    assign = np.full(aAt + gap, ASG_SENTINEL, np.int32)
    logp = np.full(lAt + gap, LP_SENTINEL, np.float64)
    freeA, freeL = np.ones(assign.size, bool), np.ones(logp.size, bool)
    for b, (_, _, nM) in enumerate(fr):
        freeA[asgOff[b]: asgOff[b] + N_SAMPLE * nM] = False
        freeL[lpOff[b]: lpOff[b] + N_SAMPLE] = False
    assert freeA.sum() == freeL.sum() == (B + 1) * gap
    return assign, logp, asgOff, lpOff, freeA, freeL


# name -> (per-frame scalar outputs in the entry's order: (name, dtype), call(lib, ctx, head, draws, outs))
# head: (B, nL, nM, cost, costOff, condition = 1); draws: (nSample, seed, sampleBase = 0, frameKey = NULL, assign, asgOff, logProb, lpOff)
ENTRIES = {
    "kbest_sample_assoc_batch_f64": (
        [("perm", np.float64)],
        lambda lib, ctx, h, d, o: lib.kbest_sample_assoc_batch_f64(ctx, *h, *d, *o)),
    "kbest_clustered_sample_assoc_batch_f64": (
        [("logPerm", np.float64), ("info", np.int32), ("maxCluster", np.int32)],
        lambda lib, ctx, h, d, o: lib.kbest_clustered_sample_assoc_batch_f64(ctx, *h, *d, *o)),
    "kbest_hybrid_frontier_sample_assoc_batch_f64": (  # maxExact = 4, maxWidth = 16
        [("logPerm", np.float64), ("method", np.int32), ("nOpen", np.int32), ("nFrontier", np.int32), ("maxCluster", np.int32)],
        lambda lib, ctx, h, d, o: lib.kbest_hybrid_frontier_sample_assoc_batch_f64(ctx, *h, 4, 16, *d, *o)),
    "kbest_hybrid_sample_assoc_batch_f64": (  # k = 200, maxExact = 4, maxWidth = 4
        [("logPerm", np.float64), ("method", np.int32), ("nOpen", np.int32), ("nFrontier", np.int32), ("nEnum", np.int32),
         ("maxCluster", np.int32)],
        lambda lib, ctx, h, d, o: lib.kbest_hybrid_sample_assoc_batch_f64(ctx, *h, 200, 4, 4, *d, *o)),
}


def run(eng, name, reverse, bad_offset=False):
    """One call: (rc, assign, logProb, asgOff, lpOff, the two masks of nobody's elements, {scalar name: [B]})."""
    fr = frames()
    B = len(fr)
    cost = np.concatenate([f[0].reshape(-1) for f in fr])
    costOff = np.concatenate(([0], np.cumsum([f[0].size for f in fr])[:-1])).astype(np.int64)
    nL = np.array([f[1] for f in fr], np.int32)
    nM = np.array([f[2] for f in fr], np.int32)
    assign, logp, asgOff, lpOff, freeA, freeL = layout(reverse)
    if bad_offset:
        asgOff = asgOff.copy()
        asgOff[3] = -1
    scalars, call = ENTRIES[name]
    outs = [np.full(B, -77, dt) for _, dt in scalars]
    rc = call(eng.lib, eng.ctx, (B, _ptr(nL), _ptr(nM), _ptr(cost), _ptr(costOff), 1),
              (N_SAMPLE, SEED, 0, None, _ptr(assign), _ptr(asgOff), _ptr(logp), _ptr(lpOff)), [_ptr(o) for o in outs])
    return rc, assign, logp, asgOff, lpOff, freeA, freeL, {s[0]: o for s, o in zip(scalars, outs)}


@pytest.mark.parametrize("name", list(ENTRIES))
def test_draws_do_not_depend_on_the_layout(eng, name):
    fr = frames()
    rc, aa, la, ao, lo, fa, fl, sa = run(eng, name, False)
    assert rc == 0, (name, rc, eng.lib.kbest_last_error(eng.ctx).decode())
    rc, ab, lb, bo, mo, fb, gl, sb = run(eng, name, True)
    assert rc == 0, (name, rc, eng.lib.kbest_last_error(eng.ctx).decode())
    print(name, {k: v.tolist() for k, v in sa.items()})
    for b, (_, nL, nM) in enumerate(fr):  # every frame, no exception
        n = N_SAMPLE * nM
        a, r = aa[ao[b]: ao[b] + n], ab[bo[b]: bo[b] + n]
        assert np.array_equal(a, r), (name, b)
        assert not (a == ASG_SENTINEL).any(), (name, b)  # the slice was written
        p, q = la[lo[b]: lo[b] + N_SAMPLE], lb[mo[b]: mo[b] + N_SAMPLE]
        assert np.array_equal(as_bits(p), as_bits(q)), (name, b, p, q)
        assert not (p == LP_SENTINEL).any(), (name, b)
    for key in sa:
        assert len(sa[key]) == len(fr) and np.array_equal(as_bits(sa[key]), as_bits(sb[key])), (name, key, sa[key], sb[key])
    # gaps and tail: the caller's
    assert fa.sum() == 0 and fl.sum() == 0
    assert (ab[fb] == ASG_SENTINEL).all() and fb.sum() == (len(fr) + 1) * GAP, name
    assert (lb[gl] == LP_SENTINEL).all() and gl.sum() == (len(fr) + 1) * GAP, name
    if name == "kbest_hybrid_frontier_sample_assoc_batch_f64":  # every open cluster through the frontier sampler
        assert sa["nFrontier"].tolist() == [1, 1, 1, 1, 1, 0, 0, 0] and (sa["method"] == 0).all(), sa
    if name == "kbest_hybrid_sample_assoc_batch_f64":
        # all three legs in one call (tests/table_sample_check.hybrid_sample_assoc on these frames; the frontier widths of the five
        # open clusters are 4, 5, 7, 4, 4)
        assert sa["nOpen"].tolist() == [1, 1, 1, 1, 1, 0, 0, 0], sa
        assert sa["nFrontier"].tolist() == [1, 0, 0, 1, 1, 0, 0, 0], sa
        assert sa["nEnum"].tolist() == [0, 1, 1, 0, 0, 0, 0, 0], sa
        assert sa["method"].tolist() == [0, 2, 2, 0, 0, 0, 0, 0], sa


@pytest.mark.parametrize("name", list(ENTRIES))
def test_negative_offset_is_refused(eng, name):
    rc, assign, logp = run(eng, name, True, bad_offset=True)[:3]
    err = eng.lib.kbest_last_error(eng.ctx).decode()
    assert rc == BAD_ARG, (name, rc, err)
    assert err.startswith(name) and err.endswith(": a negative offset"), err
    assert (assign == ASG_SENTINEL).all() and (logp == LP_SENTINEL).all(), name


@pytest.mark.parametrize("name", list(ENTRIES))
def test_no_frames_is_ok(eng, name):
    scalars, call = ENTRIES[name]
    assert call(eng.lib, eng.ctx, (0, None, None, None, None, 1), (N_SAMPLE, SEED, 0, None, None, None, None, None),
                [None] * len(scalars)) == 0
