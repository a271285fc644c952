"""GPU: the two one-stream hybrid entries (kbest_hybrid_frontier_probs_batch_f64_dev, kbest_hybrid_frontier_sample_assoc_batch_f64_dev)
on batches longer than their kernels' seams.  hybrid_gather_kernel's prefix over the workgroups before its own (`base`) is non-zero
from frame 256 on; the scatter, key and join kernels cap their grid at 4 096 workgroups and take the frames beyond in a second
pass of their frame loop, on the LDS the first pass left.  B = 260 crosses the first seam, B = 4 100 both.

The batches tile the sixteen scene frames the tests of those entries pin to the restatement and to the host entry (max_exact = 4,
max_width = 16, conditioned) with an index that is not periodic in 256, and hold -- at irregular places on either side of 256 and
of 4 096 -- a small frame with nothing open and an infeasible one.  A frame's answer must not depend on the batch: frame j carries
the bits of its frame in one short call, and the bits of the host entry.  Sentinels before, between and behind every output stay
untouched (Call.collect of the two test files the helpers come from).

The work space of the largest call, by hybrid_layout (kbest_capi.cpp): 4 100 frames x maxCol 24 x maxRawRow 64 doubles of packed
probabilities, 50 MB, and 7 MB of lists and tables; the sampler's part 19 MB more.  It is reserved once."""
import functools

import numpy as np
import pytest

import probabilisticsemslam_amd as pk
import test_gpu_hybrid_dev as hd
import test_gpu_hybrid_sample_dev as hs
from probabilisticsemslam_amd import workloads as wl

pytestmark = pytest.mark.gpu

NL, NM = hd.SMALL[1], hd.SMALL[2]
MAX_EXACT, MAX_WIDTH, N_DRAWS = 4, 16, 16
LONGEST = 4100
QUIET, DEAD = 16, 17  # places in the pool behind the sixteen: nothing open; infeasible
SPECIAL = {250: QUIET, 253: DEAD, 257: DEAD, 258: QUIET, 4091: QUIET, 4094: DEAD, 4097: DEAD, 4098: QUIET}
HOST_EDGE = 300       # frames at either end of the longest batch that are also compared with the host entry


@pytest.fixture(scope="module")
def eng():
    e = pk.KBestEngine(0)
    e.reserve_hybrid_dev(LONGEST, NL + NM, NM)
    e.reserve_hybrid_sample_dev(LONGEST, NL + NM, NM, N_DRAWS)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def pool():
    """(frames, nL, nM): the sixteen scene frames, a 6 + 3 frame whose clusters all stay within max_exact, and scene frame 0 with
    its last column +inf (no assignment)."""
    dead = np.array(hd.small16()[0])
    dead[(NM - 1) * (NL + NM):] = np.inf
    frames = list(hd.small16()) + [wl.kitti_like_frames(1, nL=6, nM=3)[0], dead]
    return frames, [NL] * 16 + [6, NL], [NM] * 16 + [3, NM]


def index(B):
    """The pool entry of every frame of the batch of B frames."""
    j = np.arange(B)
    idx = (5 * j + j // 16 + 3 * (j // 256) + 7 * (j // 4096)) % 16  # (5 j + j // 16 alone repeats every 256 frames)
    for at, which in SPECIAL.items():
        if at < B:
            idx[at] = which
    return idx


def batch(B):
    frames, nL, nM = pool()
    idx = index(B)
    return [frames[i] for i in idx], [nL[i] for i in idx], [nM[i] for i in idx], idx


def take(out, idx):
    """The outputs of a call on the pool, rearranged as the batch has its frames."""
    return tuple([x[i] for i in idx] for x in out)


def part(out, lo, hi):
    return tuple(x[lo:hi] for x in out)


@functools.lru_cache(maxsize=None)
def short_probs(eng):
    frames, nL, nM = pool()
    return hd.run_dev(eng, frames, nL, nM, True, MAX_EXACT, MAX_WIDTH, reserve=False, maxRawRow=NL + NM, maxCol=NM)


@functools.lru_cache(maxsize=None)
def short_draws(eng):
    frames, nL, nM = pool()
    return hs.run_dev(eng, frames, nL, nM, N_DRAWS, True, MAX_EXACT, MAX_WIDTH, reserve=False, maxRawRow=NL + NM, maxCol=NM,
                      frame_key=list(range(len(frames))))


def test_the_batches_cross_the_seams(eng):
    """What the other tests stand on: the sixteen frames open different numbers of clusters, so the gather's `first` differs from
    frame to frame and its `base` behind the first 256 frames is non-zero; the index is not periodic in 256; both special frames
    sit on either side of both seams; the short call itself has the host entry's bits."""
    frames, nL, nM = pool()
    got = short_probs(eng)
    hd.same_bits(got, hd.host(eng, frames, nL, nM, True, MAX_EXACT, MAX_WIDTH))
    method, nOpen = got[1], got[2]
    idx = index(LONGEST)
    assert len(set(nOpen[:16].tolist())) > 1 and int(nOpen[idx[:256]].sum()) > 0 and int(nOpen[idx[:4096]].sum()) > 0
    assert (method[:16] == 0).all() and (nOpen[:16] > 0).all()
    assert (method[QUIET], nOpen[QUIET]) == (0, 0) and method[DEAD] == -2 and not got[0][DEAD].any() and got[5][DEAD] == -np.inf
    plain = np.delete(idx, list(SPECIAL))
    assert not np.array_equal(idx[:240], idx[256:496]) and not np.array_equal(idx[:4], idx[4096:])
    assert np.bincount(plain, minlength=16).min() >= 200  # every one of the sixteen, many times
    for lo, hi in ((0, 256), (256, 260), (256, 4096), (4096, LONGEST)):
        assert {idx[at] for at in SPECIAL if lo <= at < hi} == {QUIET, DEAD}, (lo, hi)
    print(f"nOpen of the sixteen {nOpen[:16].tolist()}, clusters before frame 256: {int(nOpen[idx[:256]].sum())}, "
          f"before frame 4096: {int(nOpen[idx[:4096]].sum())}")


@pytest.mark.parametrize("B", [260, LONGEST])
def test_probs_do_not_depend_on_the_batch(eng, B):
    frames, nL, nM, idx = batch(B)
    got = hd.run_dev(eng, frames, nL, nM, True, MAX_EXACT, MAX_WIDTH, reserve=False, maxRawRow=NL + NM, maxCol=NM)
    hd.same_bits(got, take(short_probs(eng), idx), what=f"{B} frames against the short call")
    for lo, hi in ([(0, B)] if B <= 2 * HOST_EDGE else [(0, HOST_EDGE), (B - HOST_EDGE, B)]):
        want = hd.host(eng, frames[lo:hi], nL[lo:hi], nM[lo:hi], True, MAX_EXACT, MAX_WIDTH)
        hd.same_bits(part(got, lo, hi), want, what=f"{B} frames, {lo} .. {hi} against the host entry")


@pytest.mark.parametrize("B", [260, LONGEST])
def test_draws_do_not_depend_on_the_batch(eng, B):
    frames, nL, nM, idx = batch(B)
    keys = [int(i) for i in idx]
    got = hs.run_dev(eng, frames, nL, nM, N_DRAWS, True, MAX_EXACT, MAX_WIDTH, reserve=False, maxRawRow=NL + NM, maxCol=NM,
                     frame_key=keys)
    short = short_draws(eng)
    assert all((short[0][i] >= 0).all() and np.isfinite(short[1][i]).all() for i in range(17))
    assert (short[0][DEAD] == -1).all() and np.isnan(short[1][DEAD]).all() and short[3][DEAD] == -2
    hs.same_bits(got, take(short, idx), what=f"{B} frames against the short call")
    for lo, hi in ([(0, B)] if B <= 2 * HOST_EDGE else [(0, HOST_EDGE), (B - HOST_EDGE, B)]):
        want = hs.host(eng, frames[lo:hi], nL[lo:hi], nM[lo:hi], N_DRAWS, True, MAX_EXACT, MAX_WIDTH, frame_key=keys[lo:hi])
        hs.same_bits(part(got, lo, hi), want, what=f"{B} frames, {lo} .. {hi} against the host entry")
