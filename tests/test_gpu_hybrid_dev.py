"""GPU: the asynchronous exact hybrid entry (kbest_hybrid_frontier_probs_batch_f64_dev: the partial clustered kernel, the gather of
kbest_hybrid.hip, the frontier sweep on the gathered list, the scatter) on resident buffers.  The yardstick is the host entry
kbest_hybrid_frontier_probs_batch_f64(k = 0, maxBig = 0) -- parent-commit code whose own tests compare it with the restatement --
and the requirement is EQUAL BITS on everything: probabilities, logPerm (NaN as NaN), method, nOpen, nFrontier, maxCluster.  Every
buffer of a call lies between sentinels (-5.0 / -7.0 / -77); d_probs is handed over full of -5.0, so a slice that comes back with
the host's bits was written in every element by the entry itself."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import frontier_check as fc
import probabilisticsemslam_amd as pk
from probabilisticsemslam_amd import workloads as wl
from test_gpu_permanent import bits, dense_frame

pytestmark = pytest.mark.gpu

BAD_ARG, NOT_RESERVED = -2, -6  # KBEST_ERR_BAD_ARG, KBEST_ERR_NOT_RESERVED
SMALL = (200, 40, 24, 24)
MID = (200, 60, 40, 30)
WIDE = (64, 200, 128, 60)
PAD, UNTOUCHED, COST_PAD, INT_PAD = 64, -5.0, -7.0, -77
INF = np.inf


@pytest.fixture(scope="module")
def eng():
    e = pk.KBestEngine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def scene(F, nL, nM, side):
    return wl.scene_frames(F, nL, nM, side)


@functools.lru_cache(maxsize=None)
def small16():
    return tuple(scene(*SMALL)[:16])


class Call:
    """The buffers of one call, sentinels between and around everything; launch() enqueues, collect() reads back and checks."""

    def __init__(self, frames, nL, nM, maxRawRow=None, maxCol=None):
        dev = torch.device("cuda", 0)
        self.nL, self.nM, self.B = list(nL), list(nM), len(frames)
        self.maxRawRow = maxRawRow or max(l + m for l, m in zip(nL, nM))
        self.maxCol = maxCol or max(nM)
        cost, self.costOff, self.probOff, at, pat = [np.full(PAD, COST_PAD)], [], [], PAD, PAD
        for f, l, m in zip(frames, nL, nM):
            f = np.ascontiguousarray(f, dtype=np.float64).reshape(-1)
            assert f.size == (l + m) * m
            self.costOff.append(at)
            self.probOff.append(pat)
            cost += [f, np.full(PAD, COST_PAD)]
            at += f.size + PAD
            pat += m * (l + 1) + PAD
        self.cost = np.concatenate(cost)
        self.d_cost = torch.from_numpy(self.cost).to(dev)
        self.d_sub = torch.full((at,), UNTOUCHED, dtype=torch.float64, device=dev)
        self.d_probs = torch.full((pat,), UNTOUCHED, dtype=torch.float64, device=dev)
        self.d_nL = torch.tensor(self.nL, dtype=torch.int32, device=dev)
        self.d_nM = torch.tensor(self.nM, dtype=torch.int32, device=dev)
        self.d_costOff = torch.tensor(self.costOff, dtype=torch.int64, device=dev)
        self.d_probOff = torch.tensor(self.probOff, dtype=torch.int64, device=dev)
        self.d_lp = torch.full((self.B + 2,), UNTOUCHED, dtype=torch.float64, device=dev)
        self.d_int = torch.full((4, self.B + 2), INT_PAD, dtype=torch.int32, device=dev)  # method | nOpen | nFrontier | maxCluster

    def launch(self, eng, condition, max_exact, max_width, stream=None, reserve=True):
        eng.hybrid_frontier_probs_dev(self.B, self.maxRawRow, self.maxCol, self.d_nL, self.d_nM, self.d_cost, self.d_costOff, self.d_sub,
                                      self.d_probs, self.d_probOff, self.d_int[0, 1:], self.d_lp[1:], self.d_int[1, 1:],
                                      self.d_int[2, 1:], self.d_int[3, 1:], condition=condition, max_exact=max_exact,
                                      max_width=max_width, stream=stream, reserve=reserve)

    def collect(self):
        """(list of [nM, nL + 1] slices, method, nOpen, nFrontier, maxCluster, logPerm) after the sentinel checks."""
        torch.cuda.synchronize()
        hp, hs, hl, hi = self.d_probs.cpu().numpy(), self.d_sub.cpu().numpy(), self.d_lp.cpu().numpy(), self.d_int.cpu().numpy()
        assert np.array_equal(bits(self.d_cost.cpu().numpy()), bits(self.cost))
        assert hl[0] == hl[-1] == UNTOUCHED and (hi[:, 0] == INT_PAD).all() and (hi[:, -1] == INT_PAD).all()
        out, end, send = [], 0, 0
        for b in range(self.B):
            l, m = self.nL[b], self.nM[b]
            assert (hp[end:self.probOff[b]] == UNTOUCHED).all() and (hs[send:self.costOff[b]] == UNTOUCHED).all(), b
            end, send = self.probOff[b] + m * (l + 1), self.costOff[b] + (l + m) * m
            out.append(hp[self.probOff[b]:end].reshape(m, l + 1).copy())
        assert (hp[end:] == UNTOUCHED).all() and (hs[send:] == UNTOUCHED).all()
        return out, hi[0, 1:-1].copy(), hi[1, 1:-1].copy(), hi[2, 1:-1].copy(), hi[3, 1:-1].copy(), hl[1:-1].copy()


def run_dev(eng, frames, nL, nM, condition, max_exact, max_width, stream=None, reserve=True, maxRawRow=None, maxCol=None):
    c = Call(frames, nL, nM, maxRawRow, maxCol)
    torch.cuda.synchronize()
    c.launch(eng, condition, max_exact, max_width, stream, reserve)
    return c.collect()


_HOST = {}


def host_small16(eng, condition, max_exact, max_width):
    """The host entry on the sixteen frames.  Computed once per setting; nobody changes it."""
    key = (condition, max_exact, max_width)
    if key not in _HOST:
        _HOST[key] = host(eng, small16(), [SMALL[1]] * 16, [SMALL[2]] * 16, condition, max_exact, max_width)
    return _HOST[key]


def host(eng, frames, nL, nM, condition, max_exact, max_width):
    out, method, nOpen, nBig, maxc, lp, nFr = eng.hybrid_frontier_probs(list(frames), nL, nM, 0, condition=condition, max_exact=max_exact,
                                                                        max_big=0, max_width=max_width)
    assert not nBig.any()
    return out, method, nOpen, nFr, maxc, lp


def same_bits(got, want, frames=None, what=""):
    """got, want: (slices, method, nOpen, nFrontier, maxCluster, logPerm); frames: the indices compared (all)."""
    idx = range(len(want[0])) if frames is None else frames
    for j in idx:
        assert np.array_equal(bits(got[0][j]), bits(want[0][j])), (what, j)
        for a, b in zip(got[1:5], want[1:5]):
            assert a[j] == b[j], (what, j, [x[j] for x in got[1:5]], [x[j] for x in want[1:5]])
        assert bits(got[5][j:j + 1])[0] == bits(want[5][j:j + 1])[0] or (np.isnan(got[5][j]) and np.isnan(want[5][j])), (what, j, got[5][j], want[5][j])


# ---- 1. the same bits as the host entry ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_exact,max_width", [(16, 16), (8, 16), (4, 16), (1, 16), (4, 5)])
def test_same_bits_as_the_host_entry(eng, max_exact, max_width):
    """Nothing open (16); frames with and without open clusters in one batch (8); several open clusters a frame (4, 1); the
    refusal mix (4 / 5: frames 8, 10, 12 and 15 refused)."""
    want = host_small16(eng, True, max_exact, max_width)
    got = run_dev(eng, small16(), [SMALL[1]] * 16, [SMALL[2]] * 16, True, max_exact, max_width)
    print(f"max_exact {max_exact}, max_width {max_width}: nOpen {want[2].tolist()}, method {want[1].tolist()}")
    same_bits(got, want)
    if max_exact == 16:
        assert not want[2].any() and (want[1] == 0).all()
    if max_exact == 8:
        assert (want[2] == 0).any() and (want[2] > 0).any()
    if max_exact in (4, 1) and max_width == 16:
        assert want[2].max() >= 3 and (want[1] == 0).all() and np.array_equal(want[2], want[3])
    if max_width == 5:
        assert np.flatnonzero(want[1] == -1).tolist() == [8, 10, 12, 15] and (np.delete(want[1], [8, 10, 12, 15]) == 0).all()
        for j in (8, 10, 12, 15):
            assert not got[0][j].any() and got[3][j] == 0 and np.isnan(got[5][j])


# ---- 2. raw costs --------------------------------------------------------------------------------------------------------------------------
def test_raw_costs(eng):
    """condition = False: the m_k * mn term of logPerm, mn the frame's block minimum computed on the device.  Frame 0 also against
    the restatement, with the tolerances of tests/test_gpu_frontier.py (1e-12 absolute, 1e-12 relative on logPerm)."""
    want = host_small16(eng, False, 4, 16)
    got = run_dev(eng, small16(), [SMALL[1]] * 16, [SMALL[2]] * 16, False, 4, 16)
    same_bits(got, want)
    assert (want[2] > 0).all() and (want[1] == 0).all()
    re = fc.hybrid_frontier_probs(small16()[0], SMALL[1], SMALL[2], 0, condition=False, max_exact=4, max_big=0)
    err = np.abs(got[0][0] - re[0]).max()
    print(f"frame 0 raw: probabilities vs restatement {err:.3g}, logPerm {got[5][0]!r} vs {re[6]!r}")
    assert re[1] == 0 and abs(re[6] + 67.176) < 1e-3  # (the restatement itself: a condition of the test)
    assert got[1][0] == 0 and got[3][0] == re[3] and err <= 1e-12 and abs(got[5][0] - re[6]) <= 1e-12 * max(1.0, abs(re[6]))


# ---- 3. the oversized scene clusters -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,index", [(MID, (1, 38, 89)), (WIDE, (54,))])
def test_oversized_scene_clusters(eng, shape, index):
    _, nL, nM, _ = shape
    frames = [scene(*shape)[b] for b in index]
    n = len(frames)
    want = host(eng, frames, [nL] * n, [nM] * n, True, 16, 16)
    got = run_dev(eng, frames, [nL] * n, [nM] * n, True, 16, 16)
    print(f"{shape[1:]} frames {index}: maxCluster {want[4].tolist()}, logPerm {want[5].tolist()}")
    same_bits(got, want)
    assert got[3].tolist() == [1] * n and got[1].tolist() == [0] * n and (got[4] > 16).all()


# ---- 4. edges ------------------------------------------------------------------------------------------------------------------------------------
def zero_z_frame():
    """nL = nM = 12, one cluster of all twelve columns (open from max_exact = 10 down) without an assignment: columns 0 and 1 have
    one finite entry each, both in landmark row 0, and +inf miss entries."""
    nL = nM = 12
    X = np.full((nL + nM, nM), INF)
    X[0, 0], X[0, 1], X[0, 2], X[2, 2] = 1.0, 2.0, 1.5, 0.5
    for c in range(3, nM):
        X[c - 1, c], X[c, c] = 1.0 + 0.1 * c, 0.5
    for c in range(2, nM):
        X[nL + c, c] = 3.0
    return fc.flat(X), nL, nM


def test_edges_in_one_batch(eng):
    """A dense 30 x 10 frame (one cluster, nothing open), a dense cluster of 21 columns (nobody takes it: -1), an open cluster with
    Z = 0 (-2, zeros, -inf) -- these three with the host entry's bits -- and a frame beyond the launch bounds, which the host entry
    cannot be handed (it sizes the launch itself): method -1, nOpen and nFrontier 0, logPerm NaN, its slice and maxCluster untouched."""
    zf, zl, zm = zero_z_frame()
    frames = [dense_frame(30, 10, 6), dense_frame(24, 21, 5), zf]
    nL, nM = [20, 3, zl], [10, 21, zm]
    want = host(eng, frames, nL, nM, False, 10, 16)
    assert want[1].tolist() == [0, -1, -2] and want[2].tolist() == [0, 1, 1] and want[3].tolist() == [0, 0, 0]
    assert np.isnan(want[5][1]) and want[5][2] == -INF and not want[0][1].any() and not want[0][2].any()
    beyond = dense_frame(40, 12, 3)
    got = run_dev(eng, frames + [beyond], nL + [28], nM + [12], False, 10, 16, maxRawRow=30, maxCol=21)
    same_bits(got, want, frames=range(3))
    assert (got[1][3], got[2][3], got[3][3], got[4][3]) == (-1, 0, 0, INT_PAD) and np.isnan(got[5][3])
    assert (got[0][3] == UNTOUCHED).all()


# ---- 5. where it runs ------------------------------------------------------------------------------------------------------------------------------
def test_same_bits_on_a_stream_reversed_alone_and_under_a_cap(eng):
    nL, nM = [SMALL[1]] * 16, [SMALL[2]] * 16
    want = host_small16(eng, True, 4, 16)
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    mine = run_dev(eng, small16(), nL, nM, True, 4, 16, stream=s.cuda_stream)
    same_bits(mine, want, what="a stream of the caller's")
    back = run_dev(eng, small16()[::-1], nL, nM, True, 4, 16)
    same_bits(tuple(x[::-1] for x in back), want, what="reversed")
    for j in (0, 8, 15):
        alone = run_dev(eng, small16()[j:j + 1], nL[:1], nM[:1], True, 4, 16)
        same_bits(alone, tuple(x[j:j + 1] for x in want), what=f"frame {j} alone")
    try:
        eng.set_frontier_work_cap(fc.SLOT)  # one slot: one workgroup, one cluster at a time
        one = run_dev(eng, small16(), nL, nM, True, 4, 16, reserve=False)
    finally:
        eng.set_frontier_work_cap(0)
    same_bits(one, want, what="one slot")


# ---- 6. arguments and reservation ----------------------------------------------------------------------------------------------------------------
def raw_call(e, c, B, max_exact=16, max_width=16):
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    return e.lib.kbest_hybrid_frontier_probs_batch_f64_dev(e.ctx, B, c.maxRawRow, c.maxCol, p(c.d_nL), p(c.d_nM), p(c.d_cost), p(c.d_costOff),
                                                           1, max_exact, max_width, p(c.d_sub), p(c.d_probs), p(c.d_probOff), None,
                                                           p(c.d_int[0, 1:]), None, None, None, None)


def test_arguments_and_reservation(eng):
    nL, nM = [SMALL[1]] * 16, [SMALL[2]] * 16
    c = Call(small16(), nL, nM)
    eng.reserve_hybrid_dev(16, c.maxRawRow, c.maxCol)
    for max_exact, max_width in ((-1, 16), (17, 16), (16, 0), (16, -1), (16, 17)):
        assert raw_call(eng, c, 16, max_exact, max_width) == BAD_ARG, (max_exact, max_width)
    assert "maxWidth = 0" in eng.lib.kbest_last_error(eng.ctx).decode()
    assert raw_call(eng, c, 0) == 0
    assert eng.lib.kbest_hybrid_frontier_probs_batch_f64_dev(eng.ctx, 0, 1, 1, *([None] * 4), 0, 16, 16, *([None] * 9)) == 0
    fresh = pk.KBestEngine(0)
    try:  # the asynchronous entry allocates nothing
        assert raw_call(fresh, c, 16) == NOT_RESERVED
        fresh.reserve_hybrid_dev(2, c.maxRawRow, c.maxCol)
        assert raw_call(fresh, c, 16) == NOT_RESERVED  # a larger batch than reserved
        assert raw_call(fresh, Call(small16()[:2], nL[:2], nM[:2]), 2) == 0
        torch.cuda.synchronize()
    finally:
        fresh.close()
    out = c.collect()  # nothing of the refused calls was launched on eng: every output still untouched
    assert (out[1] == INT_PAD).all() and all((o == UNTOUCHED).all() for o in out[0])


# ---- 7. no allocation, no synchronise --------------------------------------------------------------------------------------------------------------
def test_two_calls_on_one_stream_without_a_synchronise_between(eng):
    """Stream order alone protects the context's work space: two different batches back to back, reserve=False (the context's
    buffers are not torch's, so torch.cuda.memory_allocated() would show nothing; the fresh-engine test above has NOT_RESERVED)."""
    nL, nM = [SMALL[1]] * 16, [SMALL[2]] * 16
    want = host_small16(eng, True, 4, 16)
    eng.reserve_hybrid_dev(16, SMALL[1] + SMALL[2], SMALL[2])
    a = Call(small16(), nL, nM)
    b = Call(small16()[::-1][:9], nL[:9], nM[:9])
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    a.launch(eng, True, 4, 16, stream=s.cuda_stream, reserve=False)
    b.launch(eng, True, 4, 16, stream=s.cuda_stream, reserve=False)
    ga, gb = a.collect(), b.collect()
    same_bits(ga, want, what="first call")
    same_bits(gb, tuple(x[::-1][:9] for x in want), what="second call")
