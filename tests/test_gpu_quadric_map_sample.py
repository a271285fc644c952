"""GPU: joint associations from quadrics against a map of any size (kbest_quadric_map_sample_assoc_batch_f64_dev / _f64).  The
yardsticks are code that exists and is pinned by its own tests: kbest_quadric_map_probs_batch_f64_dev for everything the gate and
fill passes and the tiers count (nKeep, rowIdx, the compact block, logPerm, method, nOpen, nFrontier, maxCluster), and
kbest_hybrid_frontier_sample_assoc_batch_f64_dev(condition = 0) on the compact block that entry returned, mapped through its rowIdx,
for assign and logProb -- EQUAL BITS everywhere.  Where the older path can form the raw block (quadric_costs, then that sampler with
condition = 1) the draws have its bits on every frame without an open cluster; on a frame with a frontier cluster they differ by
design and are checked for validity.  Every buffer of a call lies between sentinels (-5.0 / -7.0 / -77).

No test here sends a k-best batch of at most 32 rows: the k >= 1 cases use the chain frames, whose enumerated sub-blocks have 125
and 150 rows (tests/test_quadric_map_sample_cpu.py asserts that from the restatement)."""
import ctypes as C

import numpy as np
import pytest
import torch

import probabilisticsemslam_amd as pk
import quadric_map_lib as qm
import quadric_map_sample_lib as qs
import test_gpu_hybrid_sample_dev as hs
from quadric_map_lib import bits
from test_gpu_quadric_map import MapCall, run_map, same_float

pytestmark = pytest.mark.gpu

BAD_ARG, NOT_RESERVED = -2, -6  # KBEST_ERR_BAD_ARG, KBEST_ERR_NOT_RESERVED
PAD, UNTOUCHED, INT_PAD = 64, -5.0, -77
SEED, N = qs.SEED, qs.N
COUNTED = ("nKeep", "method", "nOpen", "nFrontier", "maxCluster")


@pytest.fixture(scope="module")
def eng():
    e = pk.KBestEngine(0)
    yield e
    e.close()


class SampleCall:
    """The buffers of one call: test_gpu_quadric_map.MapCall's (sentinels between and around everything) and the draws, every
    frame's [n][nM] assign and [n] logProb between pads; launch() enqueues, collect() reads back and checks."""

    def __init__(self, map_mean, map_cov, frames, gate, n=N, frame_key=None, **kw):
        dev = torch.device("cuda", 0)
        self.m = MapCall(map_mean, map_cov, frames, gate, dense=False, **kw)
        self.n, self.B = n, self.m.B
        self.asgOff, self.lpOff, at, lat = [], [], PAD, PAD
        for m in self.m.nM:
            self.asgOff.append(at)
            self.lpOff.append(lat)
            at += n * m + PAD
            lat += n + PAD
        self.d_assign = torch.full((at,), INT_PAD, dtype=torch.int32, device=dev)
        self.d_logp = torch.full((lat,), UNTOUCHED, dtype=torch.float64, device=dev)
        self.d_asgOff = torch.tensor(self.asgOff, dtype=torch.int64, device=dev)
        self.d_lpOff = torch.tensor(self.lpOff, dtype=torch.int64, device=dev)
        self.d_key = None if frame_key is None else torch.from_numpy(np.array(frame_key, dtype=np.uint64).view(np.int64)).to(dev)

    def launch(self, eng, max_exact=16, max_width=16, stream=None, reserve=True, seed=SEED, base=0, n=None):
        m = self.m
        eng.quadric_map_sample_assoc_dev(m.B, m.maxMap, m.maxKeep, m.maxCol, m.d_map[0], m.d_map[1], m.d_landOff, m.d_nL, m.d_meas[0],
                                         m.d_meas[1], m.d_measOff, m.d_nM, m.gate, self.n if n is None else n, m.d_int[0, 1:],
                                         m.d_rows[PAD:], self.d_assign, self.d_asgOff, self.d_logp, self.d_lpOff, m.d_int[1, 1:],
                                         d_ccost=m.d_ccost[PAD:], d_logPerm=m.d_lp[1:], d_nOpen=m.d_int[2, 1:],
                                         d_nFrontier=m.d_int[3, 1:], d_maxCluster=m.d_int[4, 1:], seed=seed, sample_base=base,
                                         d_frameKey=self.d_key, max_exact=max_exact, max_width=max_width, stream=stream, reserve=reserve)

    def refill(self):
        """Every output as before a launch (on the current stream)."""
        m = self.m
        for t in (m.d_rows, m.d_int, self.d_assign):
            t.fill_(INT_PAD)
        m.d_ccost.fill_(-7.0)
        m.d_lp.fill_(UNTOUCHED)
        self.d_logp.fill_(UNTOUCHED)

    def collect(self):
        """MapCall.collect()'s dicts with assign [n, nM] and logp [n] added, after the sentinel checks."""
        out = self.m.collect()
        ha, hp = self.d_assign.cpu().numpy(), self.d_logp.cpu().numpy()
        aend = lend = 0
        for b, d in enumerate(out):
            m = self.m.nM[b]
            assert (ha[aend:self.asgOff[b]] == INT_PAD).all() and (hp[lend:self.lpOff[b]] == UNTOUCHED).all(), b
            aend, lend = self.asgOff[b] + self.n * m, self.lpOff[b] + self.n
            d["assign"] = ha[self.asgOff[b]:aend].reshape(self.n, m).copy()
            d["logp"] = hp[self.lpOff[b]:lend].copy()
            d.pop("cprobs", None)  # (this entry has none: MapCall's buffer stays as it was handed over)
        assert (ha[aend:] == INT_PAD).all() and (hp[lend:] == UNTOUCHED).all()
        return out


def run_sample(eng, which, index=None, n=N, frame_key=None, **kw):
    mean, cov, frames, gate = (qm.BATCHES[which] if which in qm.BATCHES else SCENES[which])()
    launch = {k: kw.pop(k) for k in ("max_exact", "max_width", "stream", "reserve", "seed", "base") if k in kw}
    c = SampleCall(mean, cov, [frames[j] for j in (index if index is not None else range(len(frames)))], gate, n, frame_key, **kw)
    torch.cuda.synchronize()
    c.launch(eng, **launch)
    return c.collect()


SCENES = dict(sparse=qs.sparse_batch)


def same_draws(got, want, what=""):
    """Two collected frames with equal bits everywhere."""
    for key in COUNTED:
        assert got[key] == want[key], (what, key, got[key], want[key])
    assert same_float(got["logPerm"], want["logPerm"]), (what, got["logPerm"], want["logPerm"])
    for key in ("rows", "ccost"):
        assert (key in got) == (key in want) and (key not in got or np.array_equal(bits(got[key]), bits(want[key]))), (what, key)
    assert np.array_equal(got["assign"], want["assign"]), (what, "assign")
    assert hs.same_double_bits(got["logp"], want["logp"]), (what, "logProb", got["logp"], want["logp"])


_BASE = {}


def base(eng, which, maxKeep):
    """run_sample(eng, which, maxKeep=maxKeep) with everything else at its default.  Computed once; nobody changes it."""
    if (which, maxKeep) not in _BASE:
        _BASE[which, maxKeep] = run_sample(eng, which, maxKeep=maxKeep)
    return _BASE[which, maxKeep]


def check_against_what_exists(eng, which, got, n=N, index=None, frame_key=None, **bounds):
    """The counted outputs, rowIdx, the compact block and logPerm with the bits of quadric_map_probs_dev on the same frames; assign
    and logProb with the bits of hybrid_frontier_sample_assoc_dev(condition = 0) on the compact blocks THAT entry returned, mapped
    through ITS rowIdx.  Every frame of the batch is within the bounds and keeps at most maxKeep rows."""
    frames = (qm.BATCHES[which] if which in qm.BATCHES else SCENES[which])()[2]
    index = list(range(len(frames))) if index is None else index
    ref = run_map(eng, which, index=index, dense=False, **bounds)
    assert all(r["took"] for r in ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        for key in COUNTED:
            assert g[key] == r[key], (which, i, key, g[key], r[key])
        assert same_float(g["logPerm"], r["logPerm"]) and np.array_equal(g["rows"], r["rows"]), (which, i)
        assert np.array_equal(bits(g["ccost"]), bits(r["ccost"])), (which, i)
    nM = [len(frames[j][2]) for j in index]
    keys = list(range(len(index))) if frame_key is None else frame_key
    want = hs.run_dev(eng, [r["ccost"] for r in ref], [r["nKeep"] for r in ref], nM, n, False, 16, 16, frame_key=keys)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert np.array_equal(g["assign"], qs.map_rows(want[0][i], r["rows"], frames[index[i]][1])), (which, i)
        assert hs.same_double_bits(g["logp"], want[1][i]), (which, i)
        assert (g["method"], g["nOpen"], g["nFrontier"], g["maxCluster"]) == (want[3][i], want[4][i], want[5][i], want[6][i]), (which, i)


def check_valid(g, nL, what=""):
    """A drawn frame: every measurement takes a kept landmark or its own miss row, no landmark twice, every chosen entry finite in
    the compact block, and logProb[s] = -sum_c ccost[row_c][c] - logPerm within 1e-9 (a few hundred terms of magnitude <= 42)."""
    nk, (n, nM) = g["nKeep"], g["assign"].shape
    X = g["ccost"].reshape(nM, nk + nM).T
    pos = {int(r): i for i, r in enumerate(g["rows"])}
    for s in range(n):
        a = g["assign"][s]
        land = a[a < nL]
        assert (a >= 0).all() and len(set(land.tolist())) == len(land), (what, s)
        assert (a[a >= nL] == nL + np.flatnonzero(a >= nL)).all(), (what, s)
        comp = np.array([pos[int(v)] if v < nL else nk + (int(v) - nL) for v in a])
        chosen = X[comp, np.arange(nM)]
        assert np.isfinite(chosen).all(), (what, s)
        assert abs(g["logp"][s] - (-chosen.sum() - g["logPerm"])) <= 1e-9, (what, s, g["logp"][s], -chosen.sum() - g["logPerm"])


# ---- 1. bits against what exists ------------------------------------------------------------------------------------------------------------
def test_parity_batch_against_the_existing_entries_and_the_older_path(eng):
    """Sixteen frames of a map of 300.  Against quadric_map_probs_dev and the sampler on its compact blocks: equal bits.  Against the
    older path -- quadric_costs, upload, hybrid_frontier_sample_assoc_dev(condition = 1) on the raw 324 x 24 block --: equal bits in
    assign and logProb on every frame with nOpen = 0, equal method, logPerm, nOpen, nFrontier and maxCluster on all sixteen; the
    frames with a frontier cluster, where the draws differ by design, are valid draws."""
    mean, cov, frames, gate = qm.parity_batch()
    got = base(eng, "parity", 300)
    check_against_what_exists(eng, "parity", got, maxKeep=300)
    raw = eng.quadric_costs([(mean, cov, f[2], f[3]) for f in frames], gate)
    old = hs.run_dev(eng, raw, [300] * 16, [24] * 16, N, True, 16, 16, frame_key=list(range(16)))
    closed = [j for j in range(16) if got[j]["nOpen"] == 0]
    frontier = [j for j in range(16) if got[j]["method"] == 0 and got[j]["nFrontier"] >= 1]
    print("nOpen = 0:", closed, "frontier:", frontier, "method", [g["method"] for g in got])
    assert closed and frontier
    for j, g in enumerate(got):
        assert (g["method"], g["nOpen"], g["nFrontier"], g["maxCluster"]) == (old[3][j], old[4][j], old[5][j], old[6][j]), j
        assert same_float(g["logPerm"], old[2][j]), j
    for j in closed:
        assert np.array_equal(got[j]["assign"], old[0][j]) and hs.same_double_bits(got[j]["logp"], old[1][j]), j
        check_valid(got[j], 300, f"parity {j}")
    for j in frontier:
        check_valid(got[j], 300, f"parity {j}")


def test_maps_beyond_the_older_paths_reach(eng):
    """The six chain frames against a map of 5 000 and one frame against 100 000 landmarks, windows of one map of 105 000: kept rows
    beyond 65 535; frames 4 and 5 are refused because of an open cluster (-1s and NaNs, as the sampler writes them)."""
    got = base(eng, "far", 256)
    print("kept", [g["nKeep"] for g in got], "method", [g["method"] for g in got], "nFrontier", [g["nFrontier"] for g in got])
    check_against_what_exists(eng, "far", got, maxKeep=256)
    assert [g["method"] for g in got] == [0, 0, 0, 0, -1, -1, 0] and got[0]["nFrontier"] >= 1
    assert got[6]["rows"].max() > 65535 and got[6]["assign"].max() > 65535 + 5
    for j in (0, 1, 2, 3, 6):
        check_valid(got[j], qm.far_batch()[2][j][1], f"far {j}")
    for j in (4, 5):
        assert (got[j]["assign"] == -1).all() and np.isnan(got[j]["logp"]).all() and got[j]["nOpen"] >= 1


def test_three_hundred_draws_of_a_chain_frame(eng):
    """More draws than one workgroup of the mapping kernel has threads: chain frame 0 (a frontier cluster), 300 draws."""
    got = run_sample(eng, "far", index=[0], n=300, maxKeep=256)
    check_against_what_exists(eng, "far", got, n=300, index=[0], maxKeep=256)
    check_valid(got[0], 5000, "chain 0")
    same = base(eng, "far", 256)[0]
    assert np.array_equal(got[0]["assign"][:N], same["assign"]) and hs.same_double_bits(got[0]["logp"][:N], same["logp"])


def test_one_chain_frame_against_the_restatement(eng):
    """Chain frame 0 alone under key 0, 100 draws, against quadric_map_sample_lib under the rules of
    tests/test_gpu_hybrid_sample_dev.py: the restatement's margin >= 1e-10 first, then assign exact and logProb within 1e-12."""
    want = qs.chain_draws(0, 100)
    assert want["margin"] >= 1e-10 and want["method"] == 0 and want["nFrontier"] >= 1
    g = run_sample(eng, "far", index=[0], n=100, maxKeep=256)[0]
    err = np.abs(g["logp"] - want["logp"]).max()
    print(f"chain frame 0: margin {want['margin']:.3g}, logProb vs restatement {err:.3g}")
    assert np.array_equal(g["assign"], want["assign"]) and err <= 1e-12
    assert np.array_equal(g["rows"], want["rows"]) and np.array_equal(bits(g["ccost"]), bits(want["ccost"]))
    assert (g["method"], g["nOpen"], g["nFrontier"], g["maxCluster"]) == (want["method"], want["nOpen"], want["nFrontier"], want["maxCluster"])


# ---- 2. the statistical check ------------------------------------------------------------------------------------------------------------------
def test_frequencies_meet_the_exact_marginals(eng):
    """tests/test_quadric_map_sample_cpu.py's check on the device entry's draws: four sparse frames, 8 192 draws each, one fixed
    seed; every frequency of (measurement -> landmark or miss) within 5 sqrt(p (1 - p) / n) + 1 / n of the dense marginal p that
    quadric_map_probs_dev returns for the frame."""
    n = qs.STAT_DRAWS
    mean, cov, frames, gate = qs.sparse_batch()
    own = pk.KBestEngine(0)  # (a context of the test's own: 8 192 draws a frame would size the shared one's work space for good)
    try:
        got = run_sample(own, "sparse", n=n, maxKeep=64, seed=qs.STAT_SEED)
        c = MapCall(mean, cov, frames, gate, maxKeep=64)
        c.launch(own)
        exact = c.collect()
    finally:
        own.close()
    for f in range(4):
        assert got[f]["method"] == 0 and exact[f]["method"] == 0
        freq = qs.frequencies(got[f]["assign"], 5000)
        worst = qs.worst_excess(freq, exact[f]["probs"], n)
        print(f"sparse frame {f}: kept {got[f]['nKeep']}, worst excess over the bound {worst:.3g}, "
              f"largest deviation {qs.worst_sigmas(freq, exact[f]['probs'], n):.2f} sigma")
        assert worst <= 0.0, f


# ---- 3. edges ------------------------------------------------------------------------------------------------------------------------------------
def test_edge_shapes(eng):
    """quadric_map_lib.edge_batch() in one batch with bounds larger than needed: tile edges, nothing kept, cost 0 / 42 / 43; with
    no landmark (nL = 0) or none kept every measurement takes its own miss row: assign[s][c] = nL + c."""
    got = run_sample(eng, "edge", maxMap=4 * qm.TILE, maxKeep=300, maxCol=128)
    check_against_what_exists(eng, "edge", got, maxMap=4 * qm.TILE, maxKeep=300, maxCol=128)
    frames = qm.edge_batch()[2]
    for j in (0, 1, 12):
        nM = len(frames[j][2])
        assert np.array_equal(got[j]["assign"], np.tile(frames[j][1] + np.arange(nM), (N, 1))) and got[j]["method"] == 0, j
    assert np.array_equal(got[0]["assign"], np.zeros((N, 1))) and np.array_equal(got[1]["assign"], np.tile(np.arange(128), (N, 1)))
    for j, g in enumerate(got):
        if g["method"] == 0:
            check_valid(g, frames[j][1], f"edge {j}")
    assert sum(g["method"] == 0 for g in got) >= 14


def test_full_refused_and_untaken_frames(eng):
    """quadric_map_lib.limit_batch() at maxMap 300, maxKeep 8, maxCol 4: nKeep = maxKeep is drawn; nKeep = maxKeep + 1 gives method
    -1, the true nKeep, every assign -1 and every logProb NaN, nothing in its rowIdx and compact block; frames beyond the bounds are
    not touched."""
    got = run_sample(eng, "limit", maxMap=300, maxKeep=8, maxCol=4)
    check_against_what_exists(eng, "limit", got[:1], index=[0], maxMap=300, maxKeep=8, maxCol=4)
    assert got[0]["nKeep"] == 8 and got[0]["method"] == 0
    check_valid(got[0], 300, "limit 0")
    g = got[1]
    assert (g["nKeep"], g["method"], g["nOpen"], g["nFrontier"], g["maxCluster"]) == (9, -1, 0, 0, INT_PAD) and np.isnan(g["logPerm"])
    assert not g["took"] and (g["assign"] == -1).all() and np.isnan(g["logp"]).all()
    for g in got[2:]:
        assert (g["nKeep"], g["method"], g["nOpen"], g["nFrontier"], g["maxCluster"]) == (INT_PAD, -1, 0, 0, INT_PAD), g
        assert np.isnan(g["logPerm"]) and (g["assign"] == INT_PAD).all() and (g["logp"] == UNTOUCHED).all()


def test_max_width_zero_refuses_exactly_the_frames_with_an_open_cluster(eng):
    ref = base(eng, "parity", 300)
    got = run_sample(eng, "parity", maxKeep=300, max_width=0)
    for j, (g, r) in enumerate(zip(got, ref)):
        assert g["nOpen"] == r["nOpen"] and (g["method"] == -1) == (r["nOpen"] > 0), j
        if r["nOpen"] == 0:
            same_draws(g, r, f"max_width 0, frame {j}")
        else:
            assert (g["assign"] == -1).all() and np.isnan(g["logp"]).all() and g["nFrontier"] == 0, j
    assert any(r["nOpen"] > 0 and r["method"] == 0 for r in ref) and any(r["nOpen"] == 0 for r in ref)


# ---- 4. batch and layout independence ----------------------------------------------------------------------------------------------------------------
def test_same_bits_alone_in_a_batch_reversed_on_a_stream_and_under_larger_reservations(eng):
    """A frame's draws are a function of (frame, seed, frame key, draw index) alone."""
    ref = base(eng, "parity", 300)
    wide = run_sample(eng, "parity", maxMap=3 * qm.TILE + 5, maxKeep=700, maxCol=60)
    back = run_sample(eng, "parity", index=list(range(15, -1, -1)), maxKeep=300, frame_key=list(range(15, -1, -1)))
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    mine = run_sample(eng, "parity", maxKeep=300, stream=s.cuda_stream)
    eng.reserve_quadric_map_sample_dev(40, 1000, 400, 30, 64)  # larger in every one of the five numbers
    again = run_sample(eng, "parity", maxKeep=300, reserve=False)
    for j in range(16):
        same_draws(wide[j], ref[j], f"larger bounds {j}")
        same_draws(back[15 - j], ref[j], f"reversed {j}")
        same_draws(mine[j], ref[j], f"a stream of the caller's {j}")
        same_draws(again[j], ref[j], f"a larger reservation {j}")
    for j in (0, 8, 15):
        same_draws(run_sample(eng, "parity", index=[j], maxKeep=300, frame_key=[j])[0], ref[j], f"alone {j}")


def test_sample_base_continues_a_call(eng):
    """Draws 3 .. 4 of a call of 5 are the call of 2 at base 3."""
    ref = base(eng, "parity", 300)
    tail = run_sample(eng, "parity", n=2, maxKeep=300, base=3)
    for j in range(16):
        assert np.array_equal(tail[j]["assign"], ref[j]["assign"][3:]) and hs.same_double_bits(tail[j]["logp"], ref[j]["logp"][3:]), j
        for key in COUNTED:
            assert tail[j][key] == ref[j][key], (j, key)


def test_two_calls_on_one_stream_without_a_synchronise_between(eng):
    mean, cov, frames, gate = qm.parity_batch()
    ref = base(eng, "parity", 300)
    eng.reserve_quadric_map_sample_dev(16, 300, 300, 24, N)
    a = SampleCall(mean, cov, frames, gate, maxKeep=300)
    b = SampleCall(mean, cov, frames[::-1][:9], gate, frame_key=list(range(15, 6, -1)), maxKeep=300)
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    a.launch(eng, stream=s.cuda_stream, reserve=False)
    b.launch(eng, stream=s.cuda_stream, reserve=False)
    ga, gb = a.collect(), b.collect()
    for j in range(16):
        same_draws(ga[j], ref[j], f"first call {j}")
    for j in range(9):
        same_draws(gb[j], ref[15 - j], f"second call {j}")


# ---- 5. reservation and arguments -----------------------------------------------------------------------------------------------------------------------
def raw_call(e, c, B=None, maxMap=None, maxKeep=None, maxCol=None, max_exact=16, max_width=16, gate=None, n=None, base=0, drop=()):
    m = c.m
    p = lambda name, t: None if name in drop else C.c_void_p(t.data_ptr())  # noqa: E731
    return e.lib.kbest_quadric_map_sample_assoc_batch_f64_dev(
        e.ctx, m.B if B is None else B, maxMap or m.maxMap, maxKeep or m.maxKeep, maxCol or m.maxCol, p("mapMean", m.d_map[0]),
        p("mapCov", m.d_map[1]), p("landOff", m.d_landOff), p("nL", m.d_nL), p("measMean", m.d_meas[0]), p("measCov", m.d_meas[1]),
        p("measOff", m.d_measOff), p("nM", m.d_nM), m.gate if gate is None else gate, max_exact, max_width, c.n if n is None else n,
        SEED, base, None, p("nKeep", m.d_int[0, 1:]), p("rowIdx", m.d_rows[PAD:]), p("ccost", m.d_ccost[PAD:]), p("assign", c.d_assign),
        p("asgOff", c.d_asgOff), p("logProb", c.d_logp), p("lpOff", c.d_lpOff), None, p("method", m.d_int[1, 1:]), None, None, None, None)


def test_arguments_and_reservation(eng):
    mean, cov, frames, gate = qm.parity_batch()
    c = SampleCall(mean, cov, frames, gate, maxKeep=300)
    eng.reserve_quadric_map_sample_dev(16, 300, 300, 24, N)
    for kw in (dict(max_exact=-1), dict(max_exact=17), dict(max_width=-1), dict(max_width=17), dict(maxCol=129), dict(maxKeep=1001),
               dict(maxMap=(1 << 22) + 1), dict(B=-1), dict(gate=float("nan")), dict(n=0), dict(n=-1), dict(n=2, base=2 ** 32 - 1),
               dict(base=2 ** 32 - N + 1)):
        assert raw_call(eng, c, **kw) == BAD_ARG, kw
    for name in ("mapMean", "mapCov", "landOff", "nL", "measMean", "measCov", "measOff", "nM", "nKeep", "rowIdx", "assign", "asgOff",
                 "logProb", "lpOff", "method"):
        assert raw_call(eng, c, drop=(name,)) == BAD_ARG, name
        assert "NULL" in eng.lib.kbest_last_error(eng.ctx).decode()
    for bad in ((16, 0, 300, 24, N), (16, 300, 0, 24, N), (16, 300, 300, 0, N), (16, 300, 901, 124, N), (16, 300, 300, 24, 0)):
        assert eng.lib.kbest_reserve_quadric_map_sample_dev(eng.ctx, *bad) == BAD_ARG, bad
    assert raw_call(eng, c, B=0) == 0 and raw_call(eng, c, drop=("ccost",)) == 0  # (d_ccost may be NULL: the context's)
    torch.cuda.synchronize()
    c.refill()
    torch.cuda.synchronize()
    fresh = pk.KBestEngine(0)
    try:  # the asynchronous entry allocates nothing
        assert raw_call(fresh, c) == NOT_RESERVED
        fresh.reserve_quadric_map_dev(16, 300, 300, 24)  # (the marginals' reservation alone does not do)
        assert raw_call(fresh, c) == NOT_RESERVED
    finally:
        fresh.close()
    fresh = pk.KBestEngine(0)
    try:
        for held in ((2, 299, 299, 23, N - 1), (16, 299, 299, 23, N - 1), (16, 300, 299, 23, N - 1), (16, 300, 300, 23, N - 1),
                     (16, 300, 300, 24, N - 1)):  # frames, map, kept rows, columns, draws: each one short in turn
            fresh.reserve_quadric_map_sample_dev(*held)
            assert raw_call(fresh, c) == NOT_RESERVED, held
        fresh.reserve_quadric_map_sample_dev(2, 300, 300, 24, N)  # (never shrinks: 16 frames stay reserved)
        for g in c.collect():  # nothing of the refused calls was launched: every output still untouched
            assert g["nKeep"] == INT_PAD and g["method"] == INT_PAD and not g["took"]
            assert (g["assign"] == INT_PAD).all() and (g["logp"] == UNTOUCHED).all()
        assert raw_call(fresh, c) == 0
        ref = base(eng, "parity", 300)
        for j, g in enumerate(c.collect()):  # (raw_call hands over NULL for every output that may be NULL: those stay untouched)
            assert (g["nKeep"], g["method"]) == (ref[j]["nKeep"], ref[j]["method"]) and g["logPerm"] == UNTOUCHED, j
            assert (g["nOpen"], g["nFrontier"], g["maxCluster"]) == (INT_PAD,) * 3, j
            assert np.array_equal(g["rows"], ref[j]["rows"]) and np.array_equal(bits(g["ccost"]), bits(ref[j]["ccost"])), j
            assert np.array_equal(g["assign"], ref[j]["assign"]) and hs.same_double_bits(g["logp"], ref[j]["logp"]), j
    finally:
        fresh.close()


# ---- 6. graph capture ------------------------------------------------------------------------------------------------------------------------------------
def test_captured_and_replayed_on_other_data(eng):
    """Reserve, run eagerly, capture the entry on one stream, replay on two other data sets inside the same bounds (other frames of
    the same map: only the measurement buffers change), then on the first again: the bits of the eager launches.  The data sets
    live in buffers of their own, which no replay writes.  Afterwards a reservation that would grow the held work space is
    refused."""
    mean, cov, frames, gate = qm.parity_batch()
    ref = base(eng, "parity", 300)
    own = pk.KBestEngine(0)  # a context of the test's own: a captured launch marks its work spaces for life
    try:
        sets = [list(range(0, 6)), list(range(10, 16)), [9, 3, 8, 2, 7, 1]]
        keys = [np.array(idx, dtype=np.uint64) for idx in sets]
        data = [SampleCall(mean, cov, [frames[j] for j in idx], gate, maxKeep=300) for idx in sets]  # (only main is launched)
        main = SampleCall(mean, cov, [frames[j] for j in sets[0]], gate, frame_key=sets[0], maxKeep=300)
        d_keys = [torch.from_numpy(k.view(np.int64)).to(main.d_key.device) for k in keys]
        own.reserve_quadric_map_sample_dev(6, 300, 300, 24, N)
        s = torch.cuda.Stream(device=torch.device("cuda", 0))
        torch.cuda.synchronize()
        main.launch(own, stream=s.cuda_stream, reserve=False)
        for i, g in enumerate(main.collect()):
            same_draws(g, ref[sets[0][i]], f"eager {i}")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            main.launch(own, stream=s.cuda_stream, reserve=False)
        for k in (1, 2, 0):
            with torch.cuda.stream(s):
                main.m.d_meas[0].copy_(data[k].m.d_meas[0])
                main.m.d_meas[1].copy_(data[k].m.d_meas[1])
                main.d_key.copy_(d_keys[k])
                main.refill()
                graph.replay()
            s.synchronize()
            for i, g in enumerate(main.collect()):
                same_draws(g, ref[sets[k][i]], f"replay of set {k}, frame {i}")
        assert own.lib.kbest_reserve_quadric_map_sample_dev(own.ctx, 4096, 1 << 20, 300, 24, N) == BAD_ARG
        assert "captured" in own.lib.kbest_last_error(own.ctx).decode()
        assert own.lib.kbest_reserve_quadric_map_sample_dev(own.ctx, 6, 300, 300, 24, 4096) == BAD_ARG
        assert "captured" in own.lib.kbest_last_error(own.ctx).decode()
        with torch.cuda.stream(s):
            main.refill()
            graph.replay()
        s.synchronize()
        for i, g in enumerate(main.collect()):
            same_draws(g, ref[sets[0][i]], f"replay after the refused growth {i}")
    finally:
        own.close()


# ---- 7. the host entry -----------------------------------------------------------------------------------------------------------------------------------------
HOST_KEYS = ("assign", "logp", "logPerm", "method", "nKeep", "nOpen", "nFrontier", "nEnum", "maxCluster")


def test_host_entry_at_k_0_has_the_device_entrys_bits(eng):
    mean, cov, frames, gate = qm.parity_batch()
    ref = base(eng, "parity", 300)
    out = dict(zip(HOST_KEYS, eng.quadric_map_sample_assoc(mean, cov, frames, gate, N, seed=SEED)))
    for j, r in enumerate(ref):
        assert np.array_equal(out["assign"][j], r["assign"]) and hs.same_double_bits(out["logp"][j], r["logp"]), j
        assert same_float(out["logPerm"][j], r["logPerm"]) and out["nEnum"][j] == 0, j
        for key in COUNTED:
            assert out[key][j] == r[key], (j, key)
    keyed = dict(zip(HOST_KEYS, eng.quadric_map_sample_assoc(mean, cov, frames[::-1], gate, N, seed=SEED, frame_key=list(range(15, -1, -1)))))
    for j, r in enumerate(ref):
        assert np.array_equal(keyed["assign"][15 - j], r["assign"]) and hs.same_double_bits(keyed["logp"][15 - j], r["logp"]), j


def test_host_entry_draws_every_chain_frame_at_k_50(eng):
    """The frames the one-stream path refuses go on through hybrid_sample_assoc(k = 50, condition = 0): methods 0, 0, 0, 0, 2, 2, and
    nEnum and every output with the bits of that entry on the restated compact blocks, mapped through the kept rows."""
    mean, cov, frames, gate = qm.far_batch()
    out = dict(zip(HOST_KEYS, eng.quadric_map_sample_assoc(mean, cov, frames[:6], gate, N, k=50, seed=SEED)))
    re = [qm.chain_restated(f, 0) for f in range(6)]
    want = eng.hybrid_sample_assoc([r["ccost"] for r in re], [len(r["rows"]) for r in re], [40] * 6, N, 50, seed=SEED, condition=False)
    print("method", out["method"].tolist(), "nEnum", out["nEnum"].tolist(), "nKeep", out["nKeep"].tolist())
    assert out["method"].tolist() == [0, 0, 0, 0, 2, 2] and out["nEnum"].tolist() == [0, 0, 0, 0, 1, 1]
    for f in range(6):
        assert np.array_equal(out["assign"][f], qs.map_rows(want[0][f], re[f]["rows"], 5000)), f
        assert hs.same_double_bits(out["logp"][f], want[1][f]) and same_float(out["logPerm"][f], want[2][f]), f
        assert (out["method"][f], out["nOpen"][f], out["nFrontier"][f], out["nEnum"][f], out["maxCluster"][f]) == tuple(w[f] for w in want[3:8]), f
        assert out["nKeep"][f] == len(re[f]["rows"]) and (out["assign"][f] >= 0).all() and np.isfinite(out["logp"][f]).all(), f
    ref = base(eng, "far", 256)
    for f in range(4):  # the frames the one-stream path took: its bits
        assert np.array_equal(out["assign"][f], ref[f]["assign"]) and hs.same_double_bits(out["logp"][f], ref[f]["logp"]), f


def test_host_entry_refuses_a_frame_that_keeps_too_many_rows(eng):
    """1 010 kept landmarks beside 24 measurements (more than 1 024 - nM): method -1, the true count, -1s and NaNs, and the call
    succeeds; the frame beside it has the bits it has alone."""
    mean, cov, frames, _ = qm.parity_batch()
    parts = [qm.identity_frame(1100, list(range(1010)), 24), (mean, cov) + frames[0][2:]]
    map_mean, map_cov = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    batch = [(0, 1100, parts[0][2], parts[0][3]), (1100, 300, parts[1][2], parts[1][3])]
    out = dict(zip(HOST_KEYS, eng.quadric_map_sample_assoc(map_mean, map_cov, batch, 10.0, N, seed=SEED)))
    assert out["method"][0] == -1 and out["nKeep"][0] == 1010 and (out["assign"][0] == -1).all() and np.isnan(out["logp"][0]).all()
    assert np.isnan(out["logPerm"][0]) and (out["nOpen"][0], out["nFrontier"][0], out["nEnum"][0]) == (0, 0, 0)
    alone = dict(zip(HOST_KEYS, eng.quadric_map_sample_assoc(map_mean, map_cov, batch[1:], 10.0, N, seed=SEED, frame_key=[1])))
    assert np.array_equal(out["assign"][1], alone["assign"][0]) and hs.same_double_bits(out["logp"][1], alone["logp"][0])
    assert all(out[key][1] == alone[key][0] for key in ("method", "nKeep", "nOpen", "nFrontier", "nEnum", "maxCluster"))
