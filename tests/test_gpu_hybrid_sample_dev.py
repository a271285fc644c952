"""GPU: the asynchronous exact hybrid draws (kbest_hybrid_frontier_sample_assoc_batch_f64_dev: the partial clustered kernel, the
clustered sampler's second instantiation, the gather of kbest_hybrid.hip, the key kernel of kbest_hybrid_sample.hip, the list
sampler of kbest_frontier_sample.hip, the join) on resident buffers.  The yardstick is the host entry
kbest_hybrid_frontier_sample_assoc_batch_f64 -- parent-commit code whose own tests compare it with the restatement -- and the
requirement is EQUAL BITS on everything: assign, logProb and logPerm (NaN as NaN), method, nOpen, nFrontier, maxCluster.  Every
buffer of a call lies between sentinels (-5.0 / -7.0 / -77); d_assign and d_logProb are handed over full of them, so a slice that
comes back with the host's bits was written in every element by the entry itself."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import frontier_check as fc
import frontier_sample_check as fsc
import probabilisticsemslam_amd as pk
from test_gpu_hybrid_dev import dense_frame, zero_z_frame
from test_gpu_permanent import bits

pytestmark = pytest.mark.gpu

BAD_ARG, NOT_RESERVED = -2, -6  # KBEST_ERR_BAD_ARG, KBEST_ERR_NOT_RESERVED
SMALL, MID, SEED = fsc.SMALL, fsc.MID, fsc.SEED
PAD, UNTOUCHED, COST_PAD, INT_PAD = 64, -5.0, -7.0, -77
INF = np.inf
N = 7
KEYS = (0x9E3779B97F4A7C15, 0x0123456789ABCDEF)  # non-trivial 64-bit frame keys


@pytest.fixture(scope="module")
def eng():
    e = pk.KBestEngine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def small16():
    return tuple(fsc.scene(*SMALL)[:16])


class Call:
    """The buffers of one call, sentinels between and around everything; launch() enqueues, collect() reads back and checks."""

    def __init__(self, frames, nL, nM, n, maxRawRow=None, maxCol=None, frame_key=None):
        dev = torch.device("cuda", 0)
        self.nL, self.nM, self.B, self.n = list(nL), list(nM), len(frames), n
        self.maxRawRow = maxRawRow or max(l + m for l, m in zip(nL, nM))
        self.maxCol = maxCol or max(nM)
        cost, self.costOff, self.asgOff, self.lpOff, at, aat, lat = [np.full(PAD, COST_PAD)], [], [], [], PAD, PAD, PAD
        for f, l, m in zip(frames, nL, nM):
            f = np.ascontiguousarray(f, dtype=np.float64).reshape(-1)
            assert f.size == (l + m) * m
            self.costOff.append(at)
            self.asgOff.append(aat)
            self.lpOff.append(lat)
            cost += [f, np.full(PAD, COST_PAD)]
            at += f.size + PAD
            aat += n * m + PAD
            lat += n + PAD
        self.cost = np.concatenate(cost)
        self.d_cost = torch.from_numpy(self.cost).to(dev)
        self.d_sub = torch.full((at,), UNTOUCHED, dtype=torch.float64, device=dev)
        self.d_assign = torch.full((aat,), INT_PAD, dtype=torch.int32, device=dev)
        self.d_logp = torch.full((lat,), UNTOUCHED, dtype=torch.float64, device=dev)
        self.d_nL = torch.tensor(self.nL, dtype=torch.int32, device=dev)
        self.d_nM = torch.tensor(self.nM, dtype=torch.int32, device=dev)
        self.d_costOff = torch.tensor(self.costOff, dtype=torch.int64, device=dev)
        self.d_asgOff = torch.tensor(self.asgOff, dtype=torch.int64, device=dev)
        self.d_lpOff = torch.tensor(self.lpOff, dtype=torch.int64, device=dev)
        self.d_key = None if frame_key is None else torch.from_numpy(np.array(frame_key, dtype=np.uint64).view(np.int64)).to(dev)
        self.d_lp = torch.full((self.B + 2,), UNTOUCHED, dtype=torch.float64, device=dev)
        self.d_int = torch.full((4, self.B + 2), INT_PAD, dtype=torch.int32, device=dev)  # method | nOpen | nFrontier | maxCluster

    def launch(self, eng, condition, max_exact, max_width, stream=None, reserve=True, seed=SEED, base=0):
        eng.hybrid_frontier_sample_assoc_dev(self.B, self.maxRawRow, self.maxCol, self.d_nL, self.d_nM, self.d_cost, self.d_costOff,
                                             self.d_sub, self.n, self.d_assign, self.d_asgOff, self.d_logp, self.d_lpOff,
                                             self.d_int[0, 1:], self.d_lp[1:], self.d_int[1, 1:], self.d_int[2, 1:], self.d_int[3, 1:],
                                             seed=seed, sample_base=base, d_frameKey=self.d_key, condition=condition,
                                             max_exact=max_exact, max_width=max_width, stream=stream, reserve=reserve)

    def collect(self):
        """(list of [n, nM] draws, list of [n] logProb, logPerm, method, nOpen, nFrontier, maxCluster) after the sentinel checks."""
        torch.cuda.synchronize()
        ha, hp, hs = self.d_assign.cpu().numpy(), self.d_logp.cpu().numpy(), self.d_sub.cpu().numpy()
        hl, hi = self.d_lp.cpu().numpy(), self.d_int.cpu().numpy()
        assert np.array_equal(bits(self.d_cost.cpu().numpy()), bits(self.cost))
        assert hl[0] == hl[-1] == UNTOUCHED and (hi[:, 0] == INT_PAD).all() and (hi[:, -1] == INT_PAD).all()
        asg, lp, aend, lend, send = [], [], 0, 0, 0
        for b in range(self.B):
            l, m = self.nL[b], self.nM[b]
            assert (ha[aend:self.asgOff[b]] == INT_PAD).all() and (hp[lend:self.lpOff[b]] == UNTOUCHED).all(), b
            assert (hs[send:self.costOff[b]] == UNTOUCHED).all(), b
            aend, lend, send = self.asgOff[b] + self.n * m, self.lpOff[b] + self.n, self.costOff[b] + (l + m) * m
            asg.append(ha[self.asgOff[b]:aend].reshape(self.n, m).copy())
            lp.append(hp[self.lpOff[b]:lend].copy())
        assert (ha[aend:] == INT_PAD).all() and (hp[lend:] == UNTOUCHED).all() and (hs[send:] == UNTOUCHED).all()
        return asg, lp, hl[1:-1].copy(), hi[0, 1:-1].copy(), hi[1, 1:-1].copy(), hi[2, 1:-1].copy(), hi[3, 1:-1].copy()


def run_dev(eng, frames, nL, nM, n, condition, max_exact, max_width, stream=None, reserve=True, maxRawRow=None, maxCol=None,
            frame_key=None, base=0):
    c = Call(frames, nL, nM, n, maxRawRow, maxCol, frame_key)
    torch.cuda.synchronize()
    c.launch(eng, condition, max_exact, max_width, stream, reserve, base=base)
    return c.collect()


def host(eng, frames, nL, nM, n, condition, max_exact, max_width, frame_key=None, base=0):
    """(assign, logProb, logPerm, method, nOpen, nFrontier, maxCluster) of the host entry."""
    return eng.hybrid_frontier_sample_assoc(list(frames), nL, nM, n, seed=SEED, condition=condition, frame_key=frame_key,
                                            sample_base=base, max_exact=max_exact, max_width=max_width)


_HOST = {}


def host_small16(eng, condition, max_exact, max_width):
    """The host entry on the sixteen frames, N draws.  Computed once per setting; nobody changes it."""
    key = (condition, max_exact, max_width)
    if key not in _HOST:
        _HOST[key] = host(eng, small16(), [SMALL[1]] * 16, [SMALL[2]] * 16, N, condition, max_exact, max_width)
    return _HOST[key]


def same_double_bits(a, b):
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def same_bits(got, want, frames=None, what=""):
    """got, want: (assign, logProb, logPerm, method, nOpen, nFrontier, maxCluster); frames: the indices compared (all)."""
    idx = range(len(want[0])) if frames is None else frames
    for j in idx:
        assert np.array_equal(got[0][j], want[0][j]), (what, j)
        assert same_double_bits(got[1][j], want[1][j]), (what, j, got[1][j], want[1][j])
        assert same_double_bits(got[2][j], want[2][j]), (what, j, got[2][j], want[2][j])
        for a, b in zip(got[3:7], want[3:7]):
            assert a[j] == b[j], (what, j, [x[j] for x in got[3:7]], [x[j] for x in want[3:7]])


def pick(out, index):
    return tuple([x[j] for j in index] for x in out)


# ---- 1. the same bits as the host entry ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_exact,max_width", [(16, 16), (8, 16), (4, 16), (1, 16), (4, 5)])
def test_same_bits_as_the_host_entry(eng, max_exact, max_width):
    """Nothing open (16: the clustered sampler's draws); frames with and without open clusters in one batch (8); several open
    clusters a frame (4, 1); the refusal mix (4 / 5: frames 8, 10, 12 and 15 refused, -1s and NaNs)."""
    want = host_small16(eng, True, max_exact, max_width)
    got = run_dev(eng, small16(), [SMALL[1]] * 16, [SMALL[2]] * 16, N, True, max_exact, max_width)
    method, nOpen, nFr = want[3], want[4], want[5]
    print(f"max_exact {max_exact}, max_width {max_width}: nOpen {nOpen.tolist()}, method {method.tolist()}")
    same_bits(got, want)
    if max_exact == 16:
        assert not nOpen.any() and (method == 0).all()
    if max_exact == 8:
        assert (nOpen == 0).any() and (nOpen > 0).any()
    if max_exact in (4, 1) and max_width == 16:
        assert nOpen.max() >= 3 and (method == 0).all() and np.array_equal(nOpen, nFr)
    if max_width == 16:
        assert all((a >= 0).all() for a in got[0]) and all(np.isfinite(l).all() for l in got[1])
    if max_width == 5:
        assert np.flatnonzero(method == -1).tolist() == [8, 10, 12, 15] and (np.delete(method, [8, 10, 12, 15]) == 0).all()
        for j in (8, 10, 12, 15):
            assert (got[0][j] == -1).all() and np.isnan(got[1][j]).all() and got[5][j] == 0 and np.isnan(got[2][j])


def test_max_width_zero_refuses_every_frame_with_an_open_cluster(eng):
    """The host entry accepts maxWidth = 0; so does this one, with its bits: nothing goes through the list sampler."""
    index = [0, 8]
    frames = [small16()[j] for j in index]
    want = host(eng, frames, [SMALL[1]] * 2, [SMALL[2]] * 2, N, True, 4, 0)
    got = run_dev(eng, frames, [SMALL[1]] * 2, [SMALL[2]] * 2, N, True, 4, 0)
    same_bits(got, want)
    assert want[3].tolist() == [-1, -1] and (want[4] > 0).all() and all((a == -1).all() for a in got[0])


def test_one_frame_against_the_restatement(eng):
    """Frame 10 alone, 100 draws, against frontier_sample_check.frame_draws under the rules of tests/test_gpu_frontier_sample.py:
    the restatement's margin >= 1e-10 first, then assign exact and logProb within 1e-12."""
    want = fsc.frame_draws(SMALL, 10, 100)
    assert want.margin >= 1e-10 and want.method == 0 and want.nopen > 0
    got = run_dev(eng, [small16()[10]], [SMALL[1]], [SMALL[2]], 100, True, 4, 16, frame_key=[10])
    same_bits(got, host(eng, [small16()[10]], [SMALL[1]], [SMALL[2]], 100, True, 4, 16, frame_key=[10]))
    err = np.abs(got[1][0] - want.logp).max()
    print(f"frame 10: margin {want.margin:.3g}, logProb vs restatement {err:.3g}")
    assert np.array_equal(got[0][0], want.assign) and err <= 1e-12
    assert (got[3][0], got[4][0], got[5][0], got[6][0]) == (want.method, want.nopen, want.nfrontier, want.maxc)


# ---- 2. raw costs --------------------------------------------------------------------------------------------------------------------------
def test_raw_costs(eng):
    """condition = False: the gate of the miss-row keys on raw costs and the m_k * mn term of logPerm, both found on the device."""
    want = host_small16(eng, False, 4, 16)
    got = run_dev(eng, small16(), [SMALL[1]] * 16, [SMALL[2]] * 16, N, False, 4, 16)
    same_bits(got, want)
    assert (want[4] > 0).all() and (want[3] == 0).all() and all(f.min() != 0.0 for f in small16())


# ---- 3. more than one round of draws, continuation, frame keys ---------------------------------------------------------------------------------
@pytest.mark.parametrize("keys", [None, KEYS])
def test_many_draws_and_continuation(eng, keys):
    """1 030 draws: more than one round of 256 x 4 per workgroup of the list sampler; draws 1000 .. 1029 of that call are the call
    with sample_base = 1000 and 30 draws."""
    frames, nL, nM = [small16()[0], small16()[8]], [SMALL[1]] * 2, [SMALL[2]] * 2
    want = host(eng, frames, nL, nM, 1030, True, 4, 16, frame_key=keys)
    got = run_dev(eng, frames, nL, nM, 1030, True, 4, 16, frame_key=keys)
    same_bits(got, want)
    assert (want[3] == 0).all() and (want[4] > 0).all()
    tail = run_dev(eng, frames, nL, nM, 30, True, 4, 16, frame_key=keys, base=1000)
    for j in range(2):
        assert np.array_equal(tail[0][j], got[0][j][1000:]) and same_double_bits(tail[1][j], got[1][j][1000:]), j
    same_bits(tail, host(eng, frames, nL, nM, 30, True, 4, 16, frame_key=keys, base=1000))
    if keys is not None:  # (other keys, other draws)
        plain = host(eng, frames, nL, nM, 30, True, 4, 16, base=1000)
        assert not np.array_equal(plain[0][0], tail[0][0]) or not np.array_equal(plain[0][1], tail[0][1])


# ---- 4. the oversized scene clusters -----------------------------------------------------------------------------------------------------------
def test_oversized_scene_clusters(eng):
    _, nL, nM, _ = MID
    index = (1, 38, 89)
    frames = [fsc.scene(*MID)[b] for b in index]
    want = host(eng, frames, [nL] * 3, [nM] * 3, N, True, 16, 16)
    got = run_dev(eng, frames, [nL] * 3, [nM] * 3, N, True, 16, 16)
    print(f"{MID[1:]} frames {index}: maxCluster {want[6].tolist()}, logPerm {want[2].tolist()}")
    same_bits(got, want)
    assert got[5].tolist() == [1] * 3 and got[3].tolist() == [0] * 3 and (got[6] > 16).all()
    assert all((a >= 0).all() for a in got[0])


# ---- 5. edges ------------------------------------------------------------------------------------------------------------------------------------
def test_edges_in_one_batch(eng):
    """A dense 30 x 10 frame (one cluster, nothing open), a dense cluster of 21 columns (nobody takes it: -1), an open cluster with
    Z = 0 whose columns 0 and 1 have no miss row (padding keys; -2, -inf) -- these three with the host entry's bits -- and a frame
    beyond the launch bounds, which the host entry cannot be handed (it sizes the launch itself): method -1, nOpen and nFrontier 0,
    logPerm NaN, its assign, logProb and maxCluster untouched."""
    zf, zl, zm = zero_z_frame()
    frames = [dense_frame(30, 10, 6), dense_frame(24, 21, 5), zf]
    nL, nM = [20, 3, zl], [10, 21, zm]
    want = host(eng, frames, nL, nM, N, False, 10, 16)
    assert want[3].tolist() == [0, -1, -2] and want[4].tolist() == [0, 1, 1] and want[5].tolist() == [0, 0, 0]
    assert np.isnan(want[2][1]) and want[2][2] == -INF and (want[0][0] >= 0).all()
    for j in (1, 2):
        assert (want[0][j] == -1).all() and np.isnan(want[1][j]).all()
    beyond = dense_frame(40, 12, 3)
    got = run_dev(eng, frames + [beyond], nL + [28], nM + [12], N, False, 10, 16, maxRawRow=30, maxCol=21)
    same_bits(got, want, frames=range(3))
    assert (got[3][3], got[4][3], got[5][3], got[6][3]) == (-1, 0, 0, INT_PAD) and np.isnan(got[2][3])
    assert (got[0][3] == INT_PAD).all() and (got[1][3] == UNTOUCHED).all()


# ---- 6. where it runs ------------------------------------------------------------------------------------------------------------------------------
def test_same_bits_on_a_stream_reversed_alone_and_under_a_cap(eng):
    """A frame's outputs depend on (frame, seed, frame key, draw index) alone: frame b keeps the key b wherever it stands."""
    nL, nM = [SMALL[1]] * 16, [SMALL[2]] * 16
    want = host_small16(eng, True, 4, 16)
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    mine = run_dev(eng, small16(), nL, nM, N, True, 4, 16, stream=s.cuda_stream)
    same_bits(mine, want, what="a stream of the caller's")
    back = run_dev(eng, small16()[::-1], nL, nM, N, True, 4, 16, frame_key=list(range(15, -1, -1)))
    same_bits(tuple(x[::-1] for x in back), want, what="reversed")
    three = run_dev(eng, [small16()[j] for j in (0, 8, 15)], nL[:3], nM[:3], N, True, 4, 16, frame_key=[0, 8, 15])
    same_bits(three, pick(want, (0, 8, 15)), what="frames 0, 8 and 15 alone")
    try:
        eng.set_frontier_work_cap(fc.SLOT)  # one slot: one workgroup, one cluster at a time
        one = run_dev(eng, small16(), nL, nM, N, True, 4, 16, reserve=False)
    finally:
        eng.set_frontier_work_cap(0)
    same_bits(one, want, what="one slot")


# ---- 7. arguments and reservation ----------------------------------------------------------------------------------------------------------------
def raw_call(e, c, B, max_exact=16, max_width=16, n=None, base=0):
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    return e.lib.kbest_hybrid_frontier_sample_assoc_batch_f64_dev(
        e.ctx, B, c.maxRawRow, c.maxCol, p(c.d_nL), p(c.d_nM), p(c.d_cost), p(c.d_costOff), 1, max_exact, max_width,
        c.n if n is None else n, SEED, base, None, p(c.d_sub), p(c.d_assign), p(c.d_asgOff), p(c.d_logp), p(c.d_lpOff), None,
        p(c.d_int[0, 1:]), None, None, None, None)


def test_arguments_and_reservation(eng):
    nL, nM = [SMALL[1]] * 16, [SMALL[2]] * 16
    c = Call(small16(), nL, nM, N)
    eng.reserve_hybrid_sample_dev(16, c.maxRawRow, c.maxCol, N)
    for max_exact, max_width, n, base in ((-1, 16, N, 0), (17, 16, N, 0), (16, -1, N, 0), (16, 17, N, 0), (16, 16, 0, 0), (16, 16, -1, 0),
                                          (16, 16, 2, 2 ** 32 - 1), (16, 16, N, 2 ** 32 - N + 1)):
        assert raw_call(eng, c, 16, max_exact, max_width, n, base) == BAD_ARG, (max_exact, max_width, n, base)
        assert "sampleBase + nSample <= 2^32" in eng.lib.kbest_last_error(eng.ctx).decode()
    assert raw_call(eng, c, 0) == 0
    assert eng.lib.kbest_hybrid_frontier_sample_assoc_batch_f64_dev(eng.ctx, 0, 1, 1, *([None] * 4), 0, 16, 16, 1, 0, 0,
                                                                    *([None] * 12)) == 0
    assert eng.lib.kbest_reserve_hybrid_sample_dev(eng.ctx, 16, c.maxRawRow, c.maxCol, 0) == BAD_ARG
    for B, n in ((2, N), (16, N - 1)):  # (a reservation is sized for the largest of each number so far: an engine for each)
        fresh = pk.KBestEngine(0)
        try:  # the asynchronous entry allocates nothing
            assert raw_call(fresh, c, 16) == NOT_RESERVED
            fresh.reserve_hybrid_sample_dev(B, c.maxRawRow, c.maxCol, n)
            assert raw_call(fresh, c, 16) == NOT_RESERVED  # a larger batch, or more draws, than reserved
            assert raw_call(fresh, Call(small16()[:2], nL[:2], nM[:2], N - 1), 2) == 0
            torch.cuda.synchronize()
        finally:
            fresh.close()
    out = c.collect()  # nothing of the refused calls was launched on eng: every output still untouched
    assert (out[3] == INT_PAD).all() and all((a == INT_PAD).all() for a in out[0]) and all((l == UNTOUCHED).all() for l in out[1])


# ---- 8. no allocation, no synchronise --------------------------------------------------------------------------------------------------------------
def test_two_calls_on_one_stream_without_a_synchronise_between(eng):
    """Stream order alone protects the context's work space: two different batches back to back, reserve=False."""
    nL, nM = [SMALL[1]] * 16, [SMALL[2]] * 16
    want = host_small16(eng, True, 4, 16)
    eng.reserve_hybrid_sample_dev(16, SMALL[1] + SMALL[2], SMALL[2], N)
    a = Call(small16(), nL, nM, N)
    b = Call(small16()[::-1][:9], nL[:9], nM[:9], N, frame_key=list(range(15, 6, -1)))
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    a.launch(eng, True, 4, 16, stream=s.cuda_stream, reserve=False)
    b.launch(eng, True, 4, 16, stream=s.cuda_stream, reserve=False)
    ga, gb = a.collect(), b.collect()
    same_bits(ga, want, what="first call")
    same_bits(gb, tuple(x[::-1][:9] for x in want), what="second call")
