"""GPU tests of the loads outside the round loop of the 64-row kernel (kbest_engine.hip): phase 0 reads a wave's columns of the cost
block in chunks of 8 with all loads of a chunk in flight (one pass where a wave has at most 8 columns), phase 1b loads the tile's
columns again in the enumeration's own order, and a later piece of a relay copies the image in chunks of 8 x 16 bytes per thread.  What can go wrong
there is a column or a row at a chunk's edge taken from the wrong place, a padded column that is not zero, a lane without a row
that takes part in the minimum, a short last chunk of the image -- so the cases are the smallest shapes at those edges, every
output is pre-filled with a sentinel, and the tables are compared bit for bit with the checker (the helpers of
test_gpu_table_writes.py, through kbest_batch_f64_dev).  The knobs are read when a context is created: one context per
(waves, relay pieces)."""
import numpy as np
import pytest

import oracle_lib as ol
from test_gpu_table_writes import ROUTE_FAST, ROUTE_RELAY, Batch, check_tables, dense, engine_with, planted_pairs, run_dev, whole

LDS_LIMIT = 160 * 1024
OPT_BYTES = 16 * 8 * 3 + 16 + 8 + 64 * 10 + 8
SETUP_CHUNK = 8  # columns of a wave whose loads are in flight together (phase 0)
IMG_CHUNK = 8    # 16-byte words of a thread in flight together (the relay image)
K_SMALL = 20     # (>= 3: the column order is chosen; small: the checker's lists stay short)

# columns against (waves x chunk): one column per wave, the first chunk's edge (8 per wave), two chunks
COLS = {4: (3, 4, 5, 31, 32, 33, 64), 8: (7, 8, 9, 64), 12: (11, 12, 13, 60, 61, 64)}
RELAY_K = (16, 17, 200, 600)
# rows of the relay cases: 8 waves with 64 rows and k = 200 copy exactly 8 words per thread -- 56 rows end every image inside a chunk
RELAY_ROWS = {4: 64, 8: 56, 12: 64}


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


def spec_of(nw):
    """Hypotheses per round of a batch that does not fill the chip (choose_shape, kbest_capi.cpp): as many as waves, 8 below 12."""
    return nw if nw >= 12 else min(nw, 8)


def image_trips(k, nw, rows=64):
    """16-byte words per thread of the relay image of a launch that enumerates k + 1 solutions."""
    total = lds_total(rows, k + 1, spec_of(nw), nw)
    assert total <= LDS_LIMIT and k + 1 <= 4 * nw * 64
    return -(-(total // 16) // (nw * 64))


def dev_case(eng, bt, what, want_relay=None):
    got, route, relays = run_dev(eng, bt)
    assert route & ROUTE_FAST, (what, route)
    if want_relay is not None:
        assert bool(route & ROUTE_RELAY) == want_relay and (relays > 0) == want_relay, (what, route, relays)
    check_tables(bt, got, ("sentinel", 0), what)
    return got


def test_image_trip_counts_on_cpu():
    """The relay cases below really end their image copy inside a chunk: no trip count is a multiple of the chunk, 12 and 8 waves
    copy one short chunk (fewer than 8 words per thread), 4 waves two chunks, the second one short."""
    trips = {(nw, k): image_trips(k, nw, RELAY_ROWS[nw]) for nw in (4, 8, 12) for k in RELAY_K}
    assert all(t % IMG_CHUNK for t in trips.values()), trips
    assert all(trips[nw, k] < IMG_CHUNK for nw in (8, 12) for k in RELAY_K), trips
    assert all(IMG_CHUNK < trips[4, k] < 2 * IMG_CHUNK for k in RELAY_K), trips
    assert image_trips(200, 8, 64) == IMG_CHUNK  # (why 8 waves run 56 rows)
    # the words of the image are no multiple of the workgroup's threads either: the last trip is ragged inside the workgroup
    assert all((lds_total(RELAY_ROWS[nw], k + 1, spec_of(nw), nw) // 16) % (nw * 64) for nw in (4, 8, 12) for k in RELAY_K)
    # phase 0: the column counts straddle one column per wave and the chunk's edge
    for nw, cols in COLS.items():
        assert nw - 1 in cols and nw in cols and nw + 1 in cols and 64 in cols
    assert SETUP_CHUNK * 4 - 1 in COLS[4] and SETUP_CHUNK * 4 in COLS[4] and SETUP_CHUNK * 4 + 1 in COLS[4]


@pytest.mark.gpu
@pytest.mark.parametrize("nw", (4, 8, 12))
def test_columns_per_wave_against_the_chunk(nw):
    """M columns on nw waves, square (N = M) and with N = 64 > M (zero-padded columns): the optimum needs every entry of the tile."""
    with engine_with(nw, 0) as eng:
        for M in COLS[nw]:
            dev_case(eng, Batch(dense(9000 + 100 * nw + M, 4, M), M, M, K_SMALL), f"nw={nw} {M}x{M}", want_relay=False)
            if M < 64:
                dev_case(eng, Batch(dense(9050 + 100 * nw + M, 4, 64, M), 64, M, K_SMALL), f"nw={nw} 64x{M}", want_relay=False)


@pytest.mark.gpu
@pytest.mark.parametrize("nw", (4, 12))
def test_lanes_without_a_row_and_value_paths(nw):
    """Rows fewer than lanes, maximise, NaN / +inf entries, an all-inf matrix, and the assign2D / shortestPathCPP route (no shift,
    rectangular root) with its duals."""
    with engine_with(nw, 0) as eng:
        for N in (1, 2, 5, 33, 63):
            dev_case(eng, Batch(dense(9300 + N, 4, N), N, N, K_SMALL), f"nw={nw} {N}x{N}")
        dev_case(eng, Batch(dense(9310, 8, 28, 10), 28, 10, K_SMALL), f"nw={nw} 28x10")
        dev_case(eng, Batch(dense(9311, 4, 33) - 5.0, 33, 33, K_SMALL, maximize=True), f"nw={nw} 33x33 maximize")
        dev_case(eng, Batch(dense(9312, 4, 28, 10), 28, 10, K_SMALL, maximize=True), f"nw={nw} 28x10 maximize")
        c = dense(9313, 4, 13)
        c[0, 5 * 13 + 7] = np.nan       # one NaN entry: that arc behaves like +inf
        c[1, 3 * 13: 4 * 13] = np.inf   # a +inf column: infeasible
        c[2, :] = np.inf                # an all-inf matrix: inf - inf in the shift
        bt = Batch(c, 13, 13, K_SMALL)
        dev_case(eng, bt, f"nw={nw} NaN / inf")
        assert bt.want()[0][0] > 0 and bt.want()[0][1] == 0 and bt.want()[0][2] == 0
        for N, M, shift, mx in ((24, 9, True, False), (24, 9, False, False), (33, 33, True, True), (64, 61, False, False)):
            costs = dense(9320 + N + M, 4, N, M) + (0.0 if shift else 0.5)
            ok, r4c, c4r, g, u, v = eng.assign(costs, N, M, maximize=mx, shift=shift)
            for b in range(4):
                o = ol.orc_assign2d_ex(costs[b], N, M, mx, shift, 0)
                assert ok[b] == o[0] and r4c[b].tolist() == o[1].tolist() and c4r[b].tolist() == o[2].tolist(), (N, M, shift, b)
                assert g[b] == o[3] and u[b].tolist() == o[4].tolist() and v[b].tolist() == o[5].tolist(), (N, M, shift, b)


@pytest.mark.gpu
@pytest.mark.parametrize("nw", (4, 8, 12))
def test_ragged_batch(nw):
    """nRow / nCol / costOff with an empty frame and an infeasible one in the middle."""
    rng = np.random.default_rng(9400 + nw)
    nRow = np.array([64, 9, 33, 0, 40, 13, 64, 5], np.int32)
    nCol = np.array([61, 9, 32, 0, 13, 12, 8, 5], np.int32)
    off = np.zeros(8, np.int64)
    off[1:] = np.cumsum(nRow[:-1].astype(np.int64) * nCol[:-1])
    flat = rng.random(int((nRow.astype(np.int64) * nCol).sum())) * 10.0
    flat[off[4] + 2 * 40: off[4] + 3 * 40] = np.inf  # frame 4: its third column takes no row
    with engine_with(nw, 0) as eng:
        bt = Batch(flat, 64, 61, K_SMALL, nRow=nRow, nCol=nCol, off=off)
        dev_case(eng, bt, f"nw={nw} ragged")
        assert bt.want()[0][3] == 0 and bt.want()[0][4] == 0 and bt.want()[0][0] == K_SMALL


@pytest.mark.gpu
@pytest.mark.parametrize("nw", (4, 12))
def test_column_reorder(nw):
    """M = 2 (no reorder), M = 3 (the first size with it), and planted equal keys: the columns (2j, 2j + 1) of planted_pairs share
    their cheapest cycle, so their keys are equal and the order must still be a permutation -- the tables decide."""
    with engine_with(nw, 0) as eng:
        dev_case(eng, Batch(dense(9500, 8, 2), 2, 2, K_SMALL), f"nw={nw} 2x2")
        dev_case(eng, Batch(dense(9501, 8, 3), 3, 3, K_SMALL), f"nw={nw} 3x3")
        dev_case(eng, Batch(dense(9502, 8, 17, 3), 17, 3, K_SMALL), f"nw={nw} 17x3")
        for N in (12, 33):
            bt = Batch(planted_pairs(9510 + N, 4, N), N, N, K_SMALL)
            g = [p[2] for p in bt.want()[1]]
            assert all(len(x) == K_SMALL and (np.diff(x) > 0).all() for x in g)  # (no two gains equal: one answer)
            dev_case(eng, bt, f"nw={nw} planted pairs {N}")


RELAY_BATCHES = {}


def relay_batch(k, rows):
    """One batch, and one run of the checker, per (k, rows)."""
    if (k, rows) not in RELAY_BATCHES:
        RELAY_BATCHES[k, rows] = Batch(dense(9600 + k + rows, 6, rows), rows, rows, k)
    return RELAY_BATCHES[k, rows]


@pytest.mark.gpu
@pytest.mark.parametrize("nw", (4, 8, 12))
def test_relay_image(nw):
    """Forced relays of 2 and 3 pieces, k = 16, 17, 200, 600 (four pool entries per thread at 4 and 8 waves): against the checker
    and, whole buffers, against the plain launch of the same build; the relay launch counter must have moved."""
    plain, rows = {}, RELAY_ROWS[nw]
    with engine_with(nw, 0) as eng:
        for k in RELAY_K:
            plain[k] = dev_case(eng, relay_batch(k, rows), f"nw={nw} k={k} plain", want_relay=False)
    for pieces in (2, 3):
        with engine_with(nw, pieces) as eng:
            for k in RELAY_K:
                got = dev_case(eng, relay_batch(k, rows), f"nw={nw} k={k} {pieces} pieces", want_relay=True)
                whole(plain[k], got, f"nw={nw} k={k} {pieces} pieces: relay against plain")
