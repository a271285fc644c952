"""GPU: exact getAssignmentProbs from quadrics against a map of any size (kbest_quadric_map_probs_batch_f64_dev / _f64).  Where the
parent's path takes the frame (nL + nM <= 1 024) the yardstick is parent-commit code -- quadric_costs, then
hybrid_frontier_probs_dev(condition=1) on the raw block -- with EQUAL BITS; beyond it the numpy restatement (quadric_map_lib) for
everything that is counted or only moved (nKeep, rowIdx, the compact block, method, nOpen, nFrontier, maxCluster) and the parent's
hybrid_frontier_probs_dev(condition=0) on the restated compact block for the bits of the probabilities and of logPerm.  Every buffer
of a call lies between sentinels (-5.0 / -7.0 / -77); d_probs and d_cprobs are handed over full of -5.0."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import permanent_check as pc
import probabilisticsemslam_amd as pk
import quadric_map_lib as qm
from quadric_map_lib import bits
from test_gpu_hybrid_dev import run_dev

pytestmark = pytest.mark.gpu

BAD_ARG, NOT_RESERVED = -2, -6  # KBEST_ERR_BAD_ARG, KBEST_ERR_NOT_RESERVED
PAD, UNTOUCHED, COST_PAD, INT_PAD = 64, -5.0, -7.0, -77
T = qm.TILE


@pytest.fixture(scope="module")
def eng():
    e = pk.KBestEngine(0)
    yield e
    e.close()


class MapCall:
    """The buffers of one call, sentinels between and around everything; launch() enqueues, collect() reads back and checks."""

    def __init__(self, map_mean, map_cov, frames, gate, maxMap=None, maxKeep=None, maxCol=None, dense=True, d_map=None):
        dev = torch.device("cuda", 0)
        self.frames, self.gate, self.B = list(frames), gate, len(frames)
        self.nL, self.nM = [f[1] for f in frames], [len(f[2]) for f in frames]
        self.maxMap = maxMap or max(max(self.nL), 1)
        self.maxKeep, self.maxCol = maxKeep, maxCol or max(self.nM)
        up = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt, order="C")).to(dev)  # noqa: E731
        self.d_map = d_map or (up(map_mean, np.float64), up(np.asarray(map_cov).reshape(-1, 9), np.float64))
        self.d_meas = (up(np.concatenate([f[2] for f in frames]), np.float64),
                       up(np.concatenate([np.asarray(f[3]).reshape(-1, 9) for f in frames]), np.float64))
        self.d_landOff = up([f[0] for f in frames], np.int64)
        self.d_measOff = up(np.concatenate([[0], np.cumsum(self.nM)[:-1]]), np.int64)
        self.d_nL, self.d_nM = up(self.nL, np.int32), up(self.nM, np.int32)
        B, K, Cm = self.B, self.maxKeep, self.maxCol
        self.cstride, self.pstride = (K + Cm) * Cm, Cm * (K + 1)
        full = lambda n, v, dt: torch.full((n,), v, dtype=dt, device=dev)  # noqa: E731
        self.d_rows = full(B * K + 2 * PAD, INT_PAD, torch.int32)
        self.d_ccost = full(B * self.cstride + 2 * PAD, COST_PAD, torch.float64)
        self.d_cprobs = full(B * self.pstride + 2 * PAD, UNTOUCHED, torch.float64)
        self.probOff, at = [], PAD
        for l, m in zip(self.nL, self.nM):
            self.probOff.append(at)
            at += m * (max(l, 0) + 1) + PAD
        self.d_probs = full(at, UNTOUCHED, torch.float64) if dense else None
        self.d_probOff = up(self.probOff, np.int64)
        self.d_lp = full(B + 2, UNTOUCHED, torch.float64)
        self.d_int = torch.full((5, B + 2), INT_PAD, dtype=torch.int32, device=dev)  # nKeep | method | nOpen | nFrontier | maxCluster

    def launch(self, eng, max_exact=16, max_width=16, stream=None, reserve=True):
        eng.quadric_map_probs_dev(self.B, self.maxMap, self.maxKeep, self.maxCol, self.d_map[0], self.d_map[1], self.d_landOff, self.d_nL,
                                  self.d_meas[0], self.d_meas[1], self.d_measOff, self.d_nM, self.gate, self.d_int[0, 1:],
                                  self.d_rows[PAD:], self.d_cprobs[PAD:], self.d_int[1, 1:], d_ccost=self.d_ccost[PAD:],
                                  d_probs=self.d_probs, d_probOff=self.d_probOff if self.d_probs is not None else None,
                                  d_logPerm=self.d_lp[1:], d_nOpen=self.d_int[2, 1:], d_nFrontier=self.d_int[3, 1:],
                                  d_maxCluster=self.d_int[4, 1:], max_exact=max_exact, max_width=max_width, stream=stream, reserve=reserve)

    def collect(self):
        """Per frame a dict (nKeep, rows, ccost, cprobs, probs, method, nOpen, nFrontier, maxCluster, logPerm) after the sentinel
        checks: nothing outside the part of a slice that the frame's own numbers span was written."""
        torch.cuda.synchronize()
        rows, cc, cp = self.d_rows.cpu().numpy(), self.d_ccost.cpu().numpy(), self.d_cprobs.cpu().numpy()
        hl, hi = self.d_lp.cpu().numpy(), self.d_int.cpu().numpy()
        hp = self.d_probs.cpu().numpy() if self.d_probs is not None else None
        assert hl[0] == hl[-1] == UNTOUCHED and (hi[:, 0] == INT_PAD).all() and (hi[:, -1] == INT_PAD).all()
        for a, v in ((rows, INT_PAD), (cc, COST_PAD), (cp, UNTOUCHED)):
            assert (a[:PAD] == v).all() and (a[-PAD:] == v).all()
        out, end = [], 0
        K = self.maxKeep
        for b in range(self.B):
            l, m = self.nL[b], self.nM[b]
            nk = int(hi[0, 1 + b])
            took = 0 <= nk <= K and 1 <= m <= self.maxCol and 0 <= l <= self.maxMap  # in the bounds, and every kept row has a place
            r = rows[PAD + b * K:PAD + (b + 1) * K]
            c = cc[PAD + b * self.cstride:PAD + (b + 1) * self.cstride]
            p = cp[PAD + b * self.pstride:PAD + (b + 1) * self.pstride]
            d = dict(nKeep=nk, method=int(hi[1, 1 + b]), nOpen=int(hi[2, 1 + b]), nFrontier=int(hi[3, 1 + b]),
                     maxCluster=int(hi[4, 1 + b]), logPerm=hl[1 + b], took=bool(took))
            if took:
                assert (r[nk:] == INT_PAD).all() and (c[(nk + m) * m:] == COST_PAD).all() and (p[m * (nk + 1):] == UNTOUCHED).all(), b
                d.update(rows=r[:nk].copy(), ccost=c[:(nk + m) * m].copy(), cprobs=p[:m * (nk + 1)].reshape(m, nk + 1).copy())
            else:
                assert (r == INT_PAD).all() and (c == COST_PAD).all() and (p == UNTOUCHED).all(), b
            if hp is not None:
                assert (hp[end:self.probOff[b]] == UNTOUCHED).all(), b
                end = self.probOff[b] + m * (max(l, 0) + 1)
                d["probs"] = hp[self.probOff[b]:end].reshape(m, max(l, 0) + 1).copy()
            out.append(d)
        assert hp is None or (hp[end:] == UNTOUCHED).all()
        return out


def run_map(eng, which, index=None, **kw):
    mean, cov, frames, gate = qm.BATCHES[which]()
    launch = {k: kw.pop(k) for k in ("max_exact", "max_width", "stream", "reserve") if k in kw}
    c = MapCall(mean, cov, [frames[j] for j in (index if index is not None else range(len(frames)))], gate, **kw)
    torch.cuda.synchronize()
    c.launch(eng, **launch)
    return c.collect()


def same_float(a, b):
    return bits(a) == bits(b) or (np.isnan(a) and np.isnan(b))


def same_frame(got, want, what=""):
    """Two collected frames with equal bits everywhere."""
    for key in ("nKeep", "method", "nOpen", "nFrontier", "maxCluster"):
        assert got[key] == want[key], (what, key, got[key], want[key])
    assert same_float(got["logPerm"], want["logPerm"]), (what, got["logPerm"], want["logPerm"])
    for key in ("rows", "ccost", "cprobs", "probs"):
        assert (key in got) == (key in want) and (key not in got or np.array_equal(bits(got[key]), bits(want[key]))), (what, key)


_PARENT = {}


def parent_on_compact(eng, which, index, max_exact=16, max_width=16):
    """The parent's hybrid_frontier_probs_dev(condition=0) on the restated compact blocks of the frames.  Computed once per setting."""
    key = (which, tuple(index), max_exact, max_width)
    if key not in _PARENT:
        re = [qm.window_restated(which, j, 0, max_exact) if which != "far" or j == 6 else qm.chain_restated(j, 0) for j in index]
        nM = [len(qm.BATCHES[which]()[2][j][2]) for j in index]
        _PARENT[key] = run_dev(eng, [r["ccost"] for r in re], [len(r["rows"]) for r in re], nM, False, max_exact, max_width)
    return _PARENT[key]


def check_against_restatement(eng, which, got, index, max_exact=16, max_width=16):
    """nKeep, rowIdx and the compact block with the restatement's bits, the counted outputs equal to it; the compact probabilities
    and logPerm with the bits of the parent's one-stream entry on the restated compact block; the dense slice the expansion of them."""
    par = parent_on_compact(eng, which, index, max_exact, max_width)
    frames = qm.BATCHES[which]()[2]
    for i, j in enumerate(index):
        re = qm.window_restated(which, j, 0, max_exact) if which != "far" or j == 6 else qm.chain_restated(j, 0)
        g = got[i]
        assert g["took"] and g["nKeep"] == len(re["rows"]) and np.array_equal(g["rows"], re["rows"]), (which, j, g["nKeep"], len(re["rows"]))
        assert np.array_equal(bits(g["ccost"]), bits(re["ccost"])), (which, j)
        if max_width == 16:
            assert (g["method"], g["nOpen"], g["nFrontier"], g["maxCluster"]) == (re["method"], len(re["opens"]), re["nFrontier"], re["maxCluster"]), (which, j)
        assert (g["method"], g["nOpen"], g["nFrontier"], g["maxCluster"]) == (par[1][i], par[2][i], par[3][i], par[4][i]), (which, j)
        assert np.array_equal(bits(g["cprobs"]), bits(par[0][i])) and same_float(g["logPerm"], par[5][i]), (which, j)
        if "probs" in g:
            assert np.array_equal(bits(g["probs"]), bits(qm.expand(g["cprobs"], g["rows"], frames[j][1]))), (which, j)


# ---- 1. parity where the parent takes the frame -----------------------------------------------------------------------------------------------
def parity_raw(eng):
    mean, cov, frames, gate = qm.parity_batch()
    return eng.quadric_costs([(mean, cov, f[2], f[3]) for f in frames], gate)


def test_parity_with_the_parent_on_the_device(eng):
    """Sixteen frames of a map of 300: quadric_costs, upload, hybrid_frontier_probs_dev(condition=1) -- all parent-commit code --
    against the new entry: dense probabilities, logPerm, method, nOpen, nFrontier and maxCluster with equal bits."""
    want = run_dev(eng, parity_raw(eng), [300] * 16, [24] * 16, True, 16, 16)
    got = run_map(eng, "parity", maxKeep=300)
    print("kept", [g["nKeep"] for g in got], "method", want[1].tolist(), "nOpen", want[2].tolist())
    for j, g in enumerate(got):
        assert np.array_equal(bits(g["probs"]), bits(want[0][j])), j
        assert (g["method"], g["nOpen"], g["nFrontier"], g["maxCluster"]) == (want[1][j], want[2][j], want[3][j], want[4][j]), j
        assert same_float(g["logPerm"], want[5][j]), j
    assert (want[1] == 0).any()


def test_parity_with_the_parent_on_the_host_at_k_50(eng):
    mean, cov, frames, gate = qm.parity_batch()
    want = eng.hybrid_frontier_probs(parity_raw(eng), [300] * 16, [24] * 16, 50, condition=True)
    out, method, nKeep, nOpen, nBig, nFr, maxc, lp = eng.quadric_map_probs(mean, cov, frames, gate, k=50)
    for j in range(16):
        assert np.array_equal(bits(out[j]), bits(want[0][j])), j
        assert (method[j], nOpen[j], nBig[j], maxc[j], nFr[j]) == (want[1][j], want[2][j], want[3][j], want[4][j], want[6][j]), j
        assert same_float(lp[j], want[5][j]), j
    assert (method >= 0).all()


# ---- 2. beyond the parent's reach ----------------------------------------------------------------------------------------------------------------
def test_maps_beyond_the_parents_reach(eng):
    """Six frames against a map of 5 000 and one against 100 000 landmarks, windows of one map of 105 000."""
    got = run_map(eng, "far", maxKeep=256)
    print("kept", [g["nKeep"] for g in got], "method", [g["method"] for g in got], "nFrontier", [g["nFrontier"] for g in got])
    check_against_restatement(eng, "far", got, list(range(7)))
    assert got[6]["rows"].max() > 65535 and got[6]["method"] == 0
    assert any(g["method"] == 0 and g["nFrontier"] >= 1 for g in got) and any(g["method"] == -1 for g in got)


def test_host_entry_answers_every_chain_frame_at_k_50(eng):
    """The frames the one-stream path refuses go on through the parent's host entry: against the restatement at k = 50 (counted
    outputs equal, probabilities within 1e-12: the k-best leg's sums are the oracle's there) and against the parent's host entry on
    the restated compact block with equal bits."""
    mean, cov, frames, gate = qm.far_batch()
    out, method, nKeep, nOpen, nBig, nFr, maxc, lp = eng.quadric_map_probs(mean, cov, frames[:6], gate, k=50, max_big=0)
    re = [qm.chain_restated(f, 50) for f in range(6)]
    par = eng.hybrid_frontier_probs([r["ccost"] for r in re], [len(r["rows"]) for r in re], [40] * 6, 50, condition=False, max_big=0)
    print("method", method.tolist(), "nKeep", nKeep.tolist())
    for f in range(6):
        assert (method[f], nKeep[f], nOpen[f], nFr[f], maxc[f]) == (re[f]["method"], len(re[f]["rows"]), len(re[f]["opens"]), re[f]["nFrontier"], re[f]["maxCluster"]), f
        assert np.abs(out[f] - re[f]["probs"]).max() <= 1e-12, f
        assert np.array_equal(bits(out[f]), bits(qm.expand(par[0][f], re[f]["rows"], 5000))) and same_float(lp[f], par[5][f]), f
    assert (method >= 0).all() and (method > 0).any()


def test_host_entry_takes_every_frame_that_fits_and_refuses_the_rest(eng):
    """One call: 1 010 kept landmarks beside 24 measurements (more than 1 024 - nM: method -1, the true count, zeros, and the call
    succeeds); 950 kept beside ONE measurement and a frame of 128 measurements (together beyond 1 024: two rounds of the entry); a
    frame of the parity batch.  Every taken frame has the bits it has alone."""
    mean, cov, frames, _ = qm.parity_batch()
    parts = [qm.identity_frame(1100, list(range(1010)), 24), qm.identity_frame(1000, list(range(950)), 1),
             qm.identity_frame(10, [0, 9], 128), (mean, cov) + frames[0][2:]]
    map_mean, map_cov = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    offs = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])])
    batch = [(int(offs[i]), len(p[0]), p[2], p[3]) for i, p in enumerate(parts)]
    got = eng.quadric_map_probs(map_mean, map_cov, batch, 10.0)
    assert got[1].tolist() == [-1, 0, 0, got[1][3]] and got[2][:3].tolist() == [1010, 950, 2]
    assert not got[0][0].any() and np.isnan(got[7][0]) and (got[3][0], got[5][0]) == (0, 0)
    for j in (1, 2, 3):
        alone = eng.quadric_map_probs(map_mean, map_cov, [batch[j]], 10.0)
        assert np.array_equal(bits(got[0][j]), bits(alone[0][0])), j
        assert all(got[i][j] == alone[i][0] for i in range(1, 7)) and same_float(got[7][j], alone[7][0]), j
    assert np.abs(got[0][1].sum(axis=1) - 1.0).max() <= 1e-12 and got[0][1][0, :950].min() > 0.0


# ---- 3. edge shapes ------------------------------------------------------------------------------------------------------------------------------
def test_edge_shapes(eng):
    """quadric_map_lib.edge_batch(): nL in {0, 1, T-1, T, T+1, 2T+3} x nM in {1, 128}, kept rows at both ends and either side of the
    tile boundaries, nothing kept, cost 0 / 42 / 43, two windows of one random map -- in one batch with bounds larger than needed."""
    got = run_map(eng, "edge", maxMap=4 * T, maxKeep=300, maxCol=128)
    check_against_restatement(eng, "edge", got, list(range(16)))
    assert [g["nKeep"] for g in got[:14]] == [0, 0, 1, 1, 2, 2, 2, 2, 3, 3, 6, 6, 0, 2]
    assert got[10]["rows"].tolist() == [0, T - 1, T, 2 * T - 1, 2 * T, 2 * T + 2] and got[13]["rows"].tolist() == [0, 1]
    for j in (0, 1, 12):  # no landmark (nL = 0) or none kept: every measurement gets 1.0 in slot nL, and nothing else
        want = np.zeros_like(got[j]["probs"])
        want[:, -1] = 1.0
        assert np.array_equal(bits(got[j]["probs"]), bits(want)) and got[j]["method"] == 0, j


def test_full_refused_and_untaken_frames(eng):
    """quadric_map_lib.limit_batch() at maxMap 300, maxKeep 8, maxCol 4: nKeep = maxKeep is answered; nKeep = maxKeep + 1 gives
    method -1, the true nKeep, nothing in its slices but zeros in the dense one; frames beyond the bounds are not touched."""
    got = run_map(eng, "limit", maxMap=300, maxKeep=8, maxCol=4)
    check_against_restatement(eng, "limit", got[:1], [0])
    assert got[0]["nKeep"] == 8 and got[0]["method"] == 0
    g = got[1]
    assert (g["nKeep"], g["method"], g["nOpen"], g["nFrontier"], g["maxCluster"]) == (9, -1, 0, 0, INT_PAD) and np.isnan(g["logPerm"])
    assert not g["took"] and not g["probs"].any()
    for g in got[2:]:
        assert (g["nKeep"], g["method"], g["nOpen"], g["nFrontier"], g["maxCluster"]) == (INT_PAD, -1, 0, 0, INT_PAD), g
        assert np.isnan(g["logPerm"]) and (g["probs"] == UNTOUCHED).all()


# ---- 4. batch and layout independence ----------------------------------------------------------------------------------------------------------------
def test_same_bits_alone_in_a_batch_under_larger_bounds_and_reversed(eng):
    base = run_map(eng, "parity", maxKeep=300)
    wide = run_map(eng, "parity", maxMap=3 * T + 5, maxKeep=700, maxCol=60)
    back = run_map(eng, "parity", index=list(range(15, -1, -1)), maxKeep=300)
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    mine = run_map(eng, "parity", maxKeep=300, stream=s.cuda_stream)
    for j in range(16):
        same_frame(wide[j], base[j], f"larger bounds {j}")
        same_frame(back[15 - j], base[j], f"reversed {j}")
        same_frame(mine[j], base[j], f"a stream of the caller's {j}")
    for j in (0, 7, 15):
        same_frame(run_map(eng, "parity", index=[j], maxKeep=300)[0], base[j], f"alone {j}")
    far = run_map(eng, "far", index=[4, 6, 0], maxKeep=256, dense=False)
    check_against_restatement(eng, "far", far, [4, 6, 0])


# ---- 5. reservation and arguments -----------------------------------------------------------------------------------------------------------------------
def raw_call(e, c, B=None, maxMap=None, maxKeep=None, maxCol=None, max_exact=16, max_width=16, gate=None):
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    return e.lib.kbest_quadric_map_probs_batch_f64_dev(
        e.ctx, c.B if B is None else B, maxMap or c.maxMap, maxKeep or c.maxKeep, maxCol or c.maxCol, p(c.d_map[0]), p(c.d_map[1]),
        p(c.d_landOff), p(c.d_nL), p(c.d_meas[0]), p(c.d_meas[1]), p(c.d_measOff), p(c.d_nM), c.gate if gate is None else gate, max_exact,
        max_width, p(c.d_int[0, 1:]), p(c.d_rows[PAD:]), p(c.d_ccost[PAD:]), p(c.d_cprobs[PAD:]), None, None, None, p(c.d_int[1, 1:]),
        None, None, None, None)


def test_arguments_and_reservation(eng):
    mean, cov, frames, gate = qm.parity_batch()
    c = MapCall(mean, cov, frames, gate, maxKeep=300, dense=False)
    eng.reserve_quadric_map_dev(16, 300, 300, 24)
    for kw in (dict(max_exact=-1), dict(max_exact=17), dict(max_width=0), dict(max_width=17), dict(maxCol=129), dict(maxKeep=1001),
               dict(maxMap=(1 << 22) + 1), dict(B=-1), dict(gate=float("nan"))):
        assert raw_call(eng, c, **kw) == BAD_ARG, kw
    for bad in ((16, 0, 300, 24), (16, 300, 0, 24), (16, 300, 300, 0), (16, 300, 901, 124)):
        assert eng.lib.kbest_reserve_quadric_map_dev(eng.ctx, *bad) == BAD_ARG, bad
    assert raw_call(eng, c, B=0) == 0
    fresh = pk.KBestEngine(0)
    try:  # the asynchronous entry allocates nothing
        assert raw_call(fresh, c) == NOT_RESERVED
        for held in ((2, 299, 299, 23), (16, 299, 299, 23), (16, 300, 299, 23), (16, 300, 300, 23)):  # frames, map, kept rows, columns
            fresh.reserve_quadric_map_dev(*held)
            assert raw_call(fresh, c) == NOT_RESERVED, held
        fresh.reserve_quadric_map_dev(2, 300, 300, 24)  # (never shrinks: 16 frames stay reserved)
        two = MapCall(mean, cov, frames[:2], gate, maxKeep=300, dense=False)
        assert raw_call(fresh, two) == 0
        assert [g["method"] for g in two.collect()] == [g["method"] for g in run_map(eng, "parity", index=[0, 1], maxKeep=300)]
    finally:
        fresh.close()
    for g in c.collect():  # nothing of the refused calls was launched: every output still untouched
        assert g["nKeep"] == INT_PAD and g["method"] == INT_PAD and not g["took"]


def test_two_calls_on_one_stream_without_a_synchronise_between(eng):
    mean, cov, frames, gate = qm.parity_batch()
    base = run_map(eng, "parity", maxKeep=300)
    eng.reserve_quadric_map_dev(16, 300, 300, 24)
    a = MapCall(mean, cov, frames, gate, maxKeep=300)
    b = MapCall(mean, cov, frames[::-1][:9], gate, maxKeep=300)
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    a.launch(eng, stream=s.cuda_stream, reserve=False)
    b.launch(eng, stream=s.cuda_stream, reserve=False)
    ga, gb = a.collect(), b.collect()
    for j in range(16):
        same_frame(ga[j], base[j], f"first call {j}")
    for j in range(9):
        same_frame(gb[j], base[15 - j], f"second call {j}")


# ---- 6. graph capture ------------------------------------------------------------------------------------------------------------------------------------
def test_captured_and_replayed_on_other_data(eng):
    """Reserve, run eagerly, capture the entry on one stream, replay on two other data sets inside the same bounds (other frames of
    the same map: only the measurement and shape buffers change): the bits of the eager launches.  Afterwards a reservation that
    would grow the held work space is refused with KBEST_ERR_BAD_ARG."""
    mean, cov, frames, gate = qm.parity_batch()
    base = run_map(eng, "parity", maxKeep=300)
    own = pk.KBestEngine(0)  # a context of the test's own: a captured launch marks its work spaces for life
    try:
        sets = [list(range(0, 6)), list(range(10, 16)), [9, 3, 8, 2, 7, 1]]
        calls = [MapCall(mean, cov, [frames[j] for j in idx], gate, maxKeep=300) for idx in sets]  # (the data sets; only main is launched)
        main = MapCall(mean, cov, [frames[j] for j in sets[0]], gate, maxKeep=300)
        own.reserve_quadric_map_dev(6, 300, 300, 24)
        s = torch.cuda.Stream(device=torch.device("cuda", 0))
        torch.cuda.synchronize()
        main.launch(own, stream=s.cuda_stream, reserve=False)
        for i, g in enumerate(main.collect()):
            same_frame(g, base[sets[0][i]], f"eager {i}")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            main.launch(own, stream=s.cuda_stream, reserve=False)
        for k in (1, 2, 0):
            with torch.cuda.stream(s):
                main.d_meas[0].copy_(calls[k].d_meas[0])
                main.d_meas[1].copy_(calls[k].d_meas[1])
                for t in (main.d_rows, main.d_int):
                    t.fill_(INT_PAD)
                main.d_ccost.fill_(COST_PAD)
                main.d_cprobs.fill_(UNTOUCHED)
                main.d_probs.fill_(UNTOUCHED)
                main.d_lp.fill_(UNTOUCHED)
                graph.replay()
            s.synchronize()
            for i, g in enumerate(main.collect()):
                same_frame(g, base[sets[k][i]], f"replay of set {k}, frame {i}")
        assert own.lib.kbest_reserve_quadric_map_dev(own.ctx, 4096, 1 << 20, 300, 24) == BAD_ARG
        assert "captured" in own.lib.kbest_last_error(own.ctx).decode()
        with torch.cuda.stream(s):
            graph.replay()
        s.synchronize()
        for i, g in enumerate(main.collect()):
            same_frame(g, base[sets[0][i]], f"replay after the refused growth {i}")
    finally:
        own.close()


# ---- 7. absolute truth --------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_clusters(cc, nk, nM):
    """The clusters (columns, rows) of a compact block, where every one has at most 6 measurements and at most 2e6 assignments;
    else None."""
    import cluster_check as ck
    import hybrid_check as hc
    X, A = hc.gated_block(np.frombuffer(cc, dtype=np.float64), nk, nM, False)
    clusters, _ = ck.clusters_of(A)
    if max(len(cols) for cols, _ in clusters) > 6 or max(float(np.prod([len(rows) - i for i in range(len(cols))])) for cols, rows in clusters) > 2e6:
        return None  # (or more assignments in a cluster than the sum over all of them is for)
    return [(tuple(int(c) for c in cols), tuple(int(r) for r in rows)) for cols, rows in clusters]


def test_against_the_sum_over_all_assignments(eng):
    """Frames whose kept block has at most 6 measurements per cluster: each cluster's probabilities within 1e-12 of
    permanent_check.permutation_sum on its part of the compact block (the project's tolerance for that comparison)."""
    mean, cov, frames, gate = qm.far_batch()
    sparse = qm.make_map(1, 5000, 200.0, 3.0)
    cases = [(sparse[0], sparse[1], (0, 5000) + qm.make_frame(300 + f, sparse[0], 24, 24, 1), 10.0) for f in range(3)]
    cases.append((mean, cov, frames[6], gate))
    checked = 0
    for lm, lc, fr, g in cases:
        got = MapCall(lm, lc, [fr], g, maxKeep=256, dense=False)
        got.launch(eng)
        r = got.collect()[0]
        nk, nM = r["nKeep"], len(fr[2])
        cl = small_clusters(r["ccost"].tobytes(), nk, nM)
        if cl is None or r["method"] != 0:
            continue
        X = r["ccost"].reshape(nM, nk + nM).T
        worst = 0.0
        for cols, rows in cl:
            land = [x for x in rows if x < nk]
            miss = [x for x in rows if x >= nk]
            assert len(miss) <= len(cols)
            sub = np.full((len(land) + len(cols), len(cols)), np.inf)
            sub[:len(rows)] = X[np.ix_(land + miss, cols)]
            want, Z = pc.permutation_sum(np.ascontiguousarray(sub.T).reshape(-1), len(land), len(cols))
            assert Z > 0.0
            worst = max(worst, np.abs(r["cprobs"][np.ix_(cols, land)] - want[:, :len(land)]).max() if land else 0.0,
                        np.abs(r["cprobs"][list(cols), nk] - want[:, len(land)]).max())
        print(f"kept {nk}, clusters {len(cl)}: worst {worst:.3g}")
        assert worst <= 1e-12
        checked += 1
    assert checked >= 2
