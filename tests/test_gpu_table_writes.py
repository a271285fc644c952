"""GPU tests of the result-table writes of the 64-row kernel (kbest_engine.hip): the slots that have become final are widened into
row4col / col4row behind a wave's children when the tables are in device memory, at the start of the children phase when they are
in host memory, with the next slot's ticket and state entry fetched ahead of the current slot's stores.  What can go wrong there is a
slot written twice, not at all, with another slot's row, or handed over wrongly between the pieces of a relay -- so every output
buffer is pre-filled with a sentinel and compared WHOLE: the emitted slots with the checker (oracle_lib: nf, gain bits, row4col,
col4row), everything else with what the entry documents for it.

  device entry (kbest_batch_f64_dev): the kernels never write a slot past nf nor the padding of a ragged problem's emitted slots:
      the sentinel must still be there (gain: from slot nf + 1 on -- with a cutoff the reference, and the kernel, write the gain
      of the slot that ended the enumeration without counting it);
  host entry (kbest_batch_f64, tables in registered host memory, written by the kernel over the link): -1 in both tables and
      gain 0 past nf and in the padding.

col4row of a row on a zero-padded column (numCol < numRow) is compared as -1 on both sides, as test_gpu_round4.py does.
The knobs are read when a context is created: each combination makes a context of its own (test_gpu_round_chain.py)."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

import oracle_lib as ol
import probabilisticsemslam_amd as pk
from probabilisticsemslam_amd import engine as eng_mod

pytestmark = pytest.mark.gpu

ROUTE_FAST, ROUTE_RELAY = 4, 16
LDS_LIMIT = 160 * 1024
OPT_BYTES = 16 * 8 * 3 + 16 + 8 + 64 * 10 + 8
KNOBS = ("KBEST_NWAVES", "KBEST_RELAY", "KBEST_NO_SMALL", "KBEST_NO_LANE")
S32, S8, SG, SNF = 0x5A5A5A5A, 0x5A, -7.25, 99  # sentinels: int32 tables (four bytes of the int8 one), gain, nf


def lds_total(maxRow, k, spec, nw):
    """kb::lds_layout(...).total (kbest_engine.h), restated as in test_gpu_round_chain.py."""
    o = maxRow * (maxRow | 1) * 8
    o += spec * ((18 * maxRow + 24 + 7) & ~7)
    o += max(spec * 64, 16) * 8 + k * 8 + spec * 64 * 4 + k * 4 + k * 2 + spec * 64 * 2 + spec * 64 * 2 + maxRow
    o = (o + 3) & ~3
    o += 128
    o = (o + 7) & ~7
    o += 240
    o = (o + 7) & ~7
    o += OPT_BYTES
    o = (o + 15) & ~15
    o += nw * 512
    return (o + 15) & ~15


def fits(N, k, nw):
    return N <= 64 and k + 1 <= 4 * nw * 64 and lds_total(64, k + 1, nw, nw) <= LDS_LIMIT


@contextlib.contextmanager
def engine_with(nw, relay):
    old = {n: os.environ.get(n) for n in KNOBS}
    for n in KNOBS:
        os.environ.pop(n, None)
    os.environ.update(KBEST_NWAVES=str(nw), KBEST_RELAY=str(relay), KBEST_NO_SMALL="1", KBEST_NO_LANE="1")
    try:
        eng = pk.KBestEngine(0)
        try:
            yield eng
        finally:
            eng.close()
    finally:
        for n, v in old.items():
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v


class Batch:
    """One batch: uniform (costs [B, N * M]) or ragged (flat costs + nRow / nCol / off)."""

    def __init__(self, costs, N, M, k, maximize=False, cutoff=None, nRow=None, nCol=None, off=None):
        self.N, self.M, self.k, self.maximize, self.cutoff = N, M, k, maximize, cutoff
        self.nRow, self.nCol, self.off = nRow, nCol, off
        self.costs = np.ascontiguousarray(costs, dtype=np.float64)
        self.B = len(nRow) if nRow is not None else self.costs.reshape(-1, N * M).shape[0]
        self._want = None

    def shape(self, b):
        return (int(self.nRow[b]), int(self.nCol[b])) if self.nRow is not None else (self.N, self.M)

    def want(self):
        """The checker's answer, computed once per batch: nf[B] and per problem (row4col[nf, m], col4row[nf, n], gain[nf])."""
        if self._want is None:
            kw = dict(maximize=self.maximize, cutoff=self.cutoff)
            if self.nRow is None:
                nf, r4c, c4r, g, _ = ol.orc_kbest_batch(self.costs.reshape(-1, self.N * self.M), self.N, self.M, self.k, **kw)
                per = [(r4c[b, :nf[b]], c4r[b, :nf[b]], g[b, :nf[b]]) for b in range(self.B)]
            else:
                nf, per = np.zeros(self.B, np.int32), []
                for b in range(self.B):
                    n, m = self.shape(b)
                    if n == 0 or m == 0:  # an empty frame: nothing to assign, nothing found
                        per.append((np.zeros((0, 0), np.int32), np.zeros((0, 0), np.int32), np.zeros(0)))
                        continue
                    o = int(self.off[b])
                    onf, r4c, c4r, g = ol.orc_kbest(self.costs[o: o + n * m], n, m, self.k, **kw)
                    nf[b] = onf
                    per.append((r4c[:onf], c4r[:onf], g[:onf]))
            self._want = (nf, per)
        return self._want


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def check_tables(bt, got, past, what, i8=False, has_c4r=True):
    """got = (nf, row4col, col4row or None, gain) of one launch against the checker; `past`: what every entry outside the emitted
    slots' own rows / columns must hold: ("sentinel", first gain slot checked past nf) or ("fill",)."""
    nf, r4c, c4r, g = got
    wnf, per = bt.want()
    assert (nf == wnf).all(), (what, nf, wnf)
    tab_s = (S8 if i8 else S32) if past[0] == "sentinel" else -1
    if i8:
        tab_s = np.int8(tab_s)
    for b in range(bt.B):
        n, m = bt.shape(b)
        f = int(wnf[b])
        wr, wc, wg = per[b]
        assert (r4c[b, :f, :m] == wr).all(), (what, b, "row4col")
        assert (r4c[b, :f, m:] == tab_s).all() and (r4c[b, f:] == tab_s).all(), (what, b, "row4col outside the emitted slots")
        assert (bits(g[b, :f]) == bits(wg)).all(), (what, b, "gain")
        if past[0] == "sentinel":
            assert (g[b, f + past[1]:] == SG).all(), (what, b, "gain past nf")
        else:
            assert (g[b, f:] == 0.0).all(), (what, b, "gain past nf")
        if has_c4r:
            a, w = c4r[b, :f, :n].astype(np.int64), np.asarray(wc).astype(np.int64)
            a[a >= m] = -1
            w[w >= m] = -1
            assert (a == w).all(), (what, b, "col4row")
            assert (c4r[b, :f, n:] == tab_s).all() and (c4r[b, f:] == tab_s).all(), (what, b, "col4row outside the emitted slots")


def run_dev(eng, bt, i8=False, has_c4r=True):
    """kbest_batch_f64_dev on a stream of the caller's, every output pre-filled with its sentinel.  Returns (tables, route, relays)."""
    dev = torch.device("cuda", 0)
    tdt = torch.int8 if i8 else torch.int32
    d_r4c = torch.full((bt.B, bt.k, bt.M), S8 if i8 else S32, dtype=tdt, device=dev)
    d_c4r = torch.full((bt.B, bt.k, bt.N), S8 if i8 else S32, dtype=tdt, device=dev) if has_c4r else None
    d_g = torch.full((bt.B, bt.k), SG, dtype=torch.float64, device=dev)
    d_nf = torch.full((bt.B,), SNF, dtype=torch.int32, device=dev)
    d_cost = torch.from_numpy(bt.costs.reshape(-1)).to(dev)
    kw = {}
    if bt.nRow is not None:
        kw = dict(d_nRow=torch.from_numpy(bt.nRow).to(dev), d_nCol=torch.from_numpy(bt.nCol).to(dev), d_costOff=torch.from_numpy(bt.off).to(dev))
    s = torch.cuda.Stream()
    before = eng.relay_launches()
    torch.cuda.synchronize()
    eng.kbest_dev(d_cost, bt.B, bt.N, bt.M, bt.k, d_r4c, d_c4r, d_g, d_nf, maximize=bt.maximize, cutoff=bt.cutoff, stream=s.cuda_stream,
                  tables_i8=i8, **kw)
    s.synchronize()
    got = (d_nf.cpu().numpy(), d_r4c.cpu().numpy(), d_c4r.cpu().numpy() if has_c4r else None, d_g.cpu().numpy())
    return got, eng.last_route(), eng.relay_launches() - before


def run_host(eng, bt, i8=False, has_c4r=True):
    """kbest_batch_f64 with every buffer registered: the kernel writes the tables into host memory itself."""
    tdt = np.int8 if i8 else np.int32
    r4c = np.full((bt.B, bt.k, bt.M), S8 if i8 else S32, tdt)
    c4r = np.full((bt.B, bt.k, bt.N), S8 if i8 else S32, tdt) if has_c4r else None
    g = np.full((bt.B, bt.k), SG)
    nf = np.full(bt.B, SNF, np.int32)
    costs = bt.costs.reshape(-1).copy()
    regs = [a for a in (costs, r4c, c4r, g, nf) if a is not None]
    eng.register_host(*regs)
    try:
        o = eng._opts(bt.maximize, bt.cutoff, eng_mod.KBEST_FLAG_TABLES_I8 if i8 else 0)
        p = eng_mod._ptr
        eng._check(eng.lib.kbest_batch_f64(eng.ctx, C.byref(o), bt.B, bt.N, bt.M, p(bt.nRow), p(bt.nCol), p(costs), p(bt.off), bt.k,
                                           p(r4c), p(c4r), p(g), p(nf), None))
        route = eng.last_route()
    finally:
        eng.unregister_host(*regs)
    return (nf, r4c, c4r, g), route


def both_entries(eng, bt, what, want_relay=None, **fmt):
    """The device entry and the host entry against the checker and the entries' rules for everything not emitted."""
    got, route, relays = run_dev(eng, bt, **fmt)
    assert route & ROUTE_FAST, (what, route)
    if want_relay is not None:
        assert bool(route & ROUTE_RELAY) == want_relay and (relays > 0) == want_relay, (what, route, relays)
    check_tables(bt, got, ("sentinel", 1 if bt.cutoff is not None else 0), what + " (device entry)", **fmt)
    if not (bt.nRow is not None and ((bt.nRow == 0) | (bt.nCol == 0)).any()):  # (the host entry refuses an empty frame)
        hgot, hroute = run_host(eng, bt, **fmt)
        assert hroute & ROUTE_FAST and not hroute & ROUTE_RELAY, (what, hroute)  # (tables in host memory: never a relay)
        check_tables(bt, hgot, ("fill",), what + " (host entry)", **fmt)
    return got


def whole(a, b, what):
    """Two launches of one build, word for word, sentinels included."""
    for x, y, name in zip(a, b, ("nf", "row4col", "col4row", "gain")):
        if x is not None:
            assert (np.ascontiguousarray(x).view(np.uint8) == np.ascontiguousarray(y).view(np.uint8)).all(), (what, name)


def dense(seed, B, N, M=None, scale=10.0):
    return np.random.default_rng(seed).random((B, N * (M or N))) * scale


def planted_pairs(seed, B, N):
    """Column-major N x N costs with a planted block structure: row i on column i costs 0, swapping the neighbours (2j, 2j + 1) costs
    d_j (distinct, around 1e-3 ... 1e-2), everything else 10 ... 20.  The k best are then the optimum with a few cheap, mutually
    independent 2-cycles applied: hundreds of solutions within a narrow band of gains whose parents are split long before they are
    emitted -- what lets the kernel's emission go in long runs."""
    rng = np.random.default_rng(seed)
    out = np.empty((B, N * N))
    for b in range(B):
        c = 10.0 + 10.0 * rng.random((N, N))  # c[row, col]
        d = 1e-3 * (1.0 + 9.0 * rng.random(N // 2))
        for j in range(N // 2):
            c[2 * j, 2 * j] = c[2 * j + 1, 2 * j + 1] = 0.0
            c[2 * j, 2 * j + 1] = d[j] * 0.5
            c[2 * j + 1, 2 * j] = d[j] * 0.5
        if N & 1:
            c[N - 1, N - 1] = 0.0
        out[b] = c.T.reshape(-1)
    return out


def pair_run(r4c):
    """Longest stretch of consecutive solutions of one problem that are the optimum with planted 2-cycles only (CPU, on the checker's list)."""
    best = cur = 0
    ident = np.arange(r4c.shape[1])
    for row in r4c:
        moved = np.nonzero(row != ident)[0]
        ok = all(row[c] == (c ^ 1) for c in moved)
        cur = cur + 1 if ok else 0
        best = max(best, cur)
    return best


# (waves, k, rows, problems): one pool entry per thread, and k beyond it (four entries per thread) at every wave count
WAVE_CASES = [(4, 120, 52, 24), (4, 300, 22, 12), (8, 120, 56, 24), (8, 600, 22, 12), (12, 200, 64, 16), (12, 800, 22, 8),
              (16, 120, 64, 16), (16, 1100, 22, 8)]


@pytest.mark.parametrize("nw,k,N,B", WAVE_CASES)
def test_wave_counts_both_entries(nw, k, N, B):
    """Every wave count and pool depth that instantiates the kernel, plain launches, both entries; where the relay is compiled
    (4 / 8 / 12 waves) the three-piece relay of the same build must give the same buffers word for word."""
    assert fits(N, k, nw) and (k > nw * 64 or k + 1 <= nw * 64)
    bt = Batch(dense(8000 + nw + k, B, N), N, N, k)
    with engine_with(nw, 0) as eng:
        plain = both_entries(eng, bt, f"nw={nw} k={k}", want_relay=False)
    if nw != 16:
        with engine_with(nw, 3) as eng:
            got, route, relays = run_dev(eng, bt)
            assert route & ROUTE_RELAY and relays > 0, (route, relays)
            whole(plain, got, f"nw={nw} k={k}: relay against plain")


@pytest.mark.parametrize("nw", (4, 8, 12))
@pytest.mark.parametrize("pieces", (2, 3, 5))
def test_relay_hand_over_table_formats(nw, pieces):
    """Forced relays of 2, 3 and 5 pieces (a piece hands over behind phase D with the last round's slots emitted but not written: its
    successor writes them) in every table format: int32, int8, without col4row, maximise, and a cutoff that ends lists inside the
    tables on a slot that is written, not counted.  Each against the checker and, whole buffers, against the plain launch."""
    N, k, B = 64, 200, 12
    assert fits(N, k, nw)
    costs = dense(8100 + 16 * nw + pieces, B, N)
    plainb, mx = Batch(costs, N, N, k), Batch(costs, N, N, k, maximize=True)
    g0 = ol.orc_kbest(costs[0], N, N, k)[3]
    ct = Batch(costs, N, N, k, cutoff=0.999 * float(g0[k // 2] - g0[0]))
    assert (ct.want()[0] < k).any()
    cases = [("int32", plainb, {}), ("int8", plainb, dict(i8=True)), ("no col4row", plainb, dict(has_c4r=False)), ("maximize", mx, {}),
             ("cutoff", ct, {})]
    ref = {}
    with engine_with(nw, 0) as eng:
        for name, bt, fmt in cases:
            ref[name] = both_entries(eng, bt, f"plain {name}", want_relay=False, **fmt)
    with engine_with(nw, pieces) as eng:
        for name, bt, fmt in cases:
            got = both_entries(eng, bt, f"{pieces} pieces {name}", want_relay=True, **fmt)
            whole(ref[name], got, f"{pieces} pieces {name}: relay against plain")


@pytest.mark.parametrize("nw", (4, 12))
def test_short_lists_and_phase3(nw):
    """k = 1, 2, 3: everything the rounds emit is left to phase 3 or written by one round; 4x4 with k = 30: all 24 assignments, the
    enumeration ends with the pool empty; rectangular problems (rows without a column: -1)."""
    with engine_with(nw, 0) as eng:
        for k in (1, 2, 3):
            both_entries(eng, Batch(dense(8200 + k, 8, 64), 64, 64, k), f"k={k}", want_relay=False)
        bt = Batch(dense(8210, 40, 4), 4, 4, 30)
        both_entries(eng, bt, "4x4 k=30", want_relay=False)
        assert (bt.want()[0] == 24).all()
        both_entries(eng, Batch(dense(8220, 16, 40, 23), 40, 23, 60), "40x23", want_relay=False)
        both_entries(eng, Batch(dense(8221, 16, 64, 8), 64, 8, 60, maximize=True), "64x8 maximize", want_relay=False)
    with engine_with(nw, 3) as eng:  # (k < 16 and rectangular batches run without the relay: the library's rule; the route is not asserted)
        both_entries(eng, Batch(dense(8230, 16, 40, 23), 40, 23, 60), "40x23, relay forced")


@pytest.mark.parametrize("nw,relay", [(4, 0), (8, 3), (12, 0), (12, 5), (16, 0)])
def test_long_emission_runs(nw, relay):
    """Costs with planted cheap 2-cycles (planted_pairs): measured on the CPU with the checker, for the seeds used here (8300 + nw),
    12 problems of 64 rows, k = 200: in every problem ALL 200 solutions are the optimum with planted 2-cycles only -- one stretch of
    200 (asserted below: at least 65, more than any wave count and more than 64) --, their gains within 0.012 of the optimum, no two
    equal, while any other assignment costs 10 more.  (The kernel's own per-round emission is not visible through the C ABI: what the CPU check pins
    is that the inputs have the structure -- many candidates split before the ones in front of them go out -- that makes it long.)"""
    N, k, B = 64, 200, 12
    assert fits(N, k, nw)
    bt = Batch(planted_pairs(8300 + nw, B, N), N, N, k)
    wnf, per = bt.want()
    assert (wnf == k).all() and min(pair_run(p[0]) for p in per) >= 65
    with engine_with(nw, relay) as eng:
        got = both_entries(eng, bt, f"planted pairs nw={nw} relay={relay}", want_relay=(relay > 0) if nw != 16 else None)
    if relay:
        with engine_with(nw, 0) as eng:
            whole(run_dev(eng, bt)[0], got, "planted pairs: relay against plain")


@pytest.mark.parametrize("nw,relay", [(4, 0), (8, 0), (12, 0), (12, 3)])
def test_ragged_batch_with_infeasible_and_empty_frame(nw, relay):
    """A ragged batch (8 ... 64 rows, columns <= rows) with one infeasible frame (a column of +inf) through both entries, and the same
    batch with an empty frame (0 x 0) through the device entry: the padding of emitted slots and every slot past nf untouched
    (device entry) or -1 / gain 0 (host entry)."""
    rng = np.random.default_rng(8400 + nw)
    B, N, M, k = 20, 64, 48, 40
    nRow = rng.integers(8, N + 1, B).astype(np.int32)
    nCol = np.minimum(rng.integers(2, M + 1, B), nRow).astype(np.int32)
    nRow[0], nCol[0] = N, M
    off = np.zeros(B, np.int64)
    off[1:] = np.cumsum(nRow[:-1].astype(np.int64) * nCol[:-1])
    flat = rng.random(int((nRow.astype(np.int64) * nCol).sum())) * 10.0
    flat[off[3]: off[3] + nRow[3]] = np.inf  # frame 3: its first column takes no row
    with engine_with(nw, relay) as eng:
        bt = Batch(flat, N, M, k, nRow=nRow, nCol=nCol, off=off)
        both_entries(eng, bt, "ragged")
        assert bt.want()[0][3] == 0
        nR2, nC2 = nRow.copy(), nCol.copy()
        nR2[5] = nC2[5] = 0
        bt2 = Batch(flat, N, M, k, nRow=nR2, nCol=nC2, off=off)
        both_entries(eng, bt2, "ragged with an empty frame")
        assert bt2.want()[0][5] == 0


def test_shapes_fit_on_cpu():
    """Every (rows, k, waves) used above passes the launcher's own fit rule (no case depends on a silent fallback)."""
    for nw, k, N, _ in WAVE_CASES:
        assert fits(N, k, nw)
    for nw in (4, 8, 12, 16):
        assert fits(64, 200, nw) and fits(64, 60, nw) and fits(4, 30, nw)
