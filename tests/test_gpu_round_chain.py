"""GPU tests of the round chain of the 64-row kernel (kbest_engine.hip) as rewritten in round 7: the a-priori threshold (combination
lists, doubling bracket + one histogram pass, ranks counted by all waves), the selection written to the control block by the walk
itself.  Every combination of wave count x relay off / forced x launch flavour, each problem against the checker (nf, gain bits,
row4col, col4row), and the default launch against the KBEST_FLAG_NO_PRUNE launch of the same batch: a threshold that is not a bound
shows up there and nowhere else.

The knobs (KBEST_NWAVES, KBEST_RELAY, KBEST_NO_SMALL, KBEST_NO_LANE, KBEST_EAGER) are read when a context is created: each
combination makes a context of its own with the environment set, one at a time, and puts the environment back."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as ol
import probabilisticsemslam_amd as pk
from probabilisticsemslam_amd import engine as eng_mod

pytestmark = pytest.mark.gpu

FLAG_NO_PRUNE, FLAG_NO_T0, FLAG_NO_OPT, FLAG_NO_TIE_CHECK = 1, 32, 256, 512
ROUTE_FAST, ROUTE_RELAY = 4, 16
LDS_LIMIT = 160 * 1024
OPT_BYTES = 16 * 8 * 3 + 16 + 8 + 64 * 10 + 8
KNOBS = ("KBEST_NWAVES", "KBEST_RELAY", "KBEST_NO_SMALL", "KBEST_NO_LANE", "KBEST_EAGER")


def lds_total(maxRow, k, spec, nw):
    """kb::lds_layout(...).total (kbest_engine.h), restated: the shapes below are checked against it on the CPU."""
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
    """<= 64 rows, k + 1 (the tie check's extra solution) within 4 * NW * 64 pool entries, the layout within the LDS at the widest spec."""
    return N <= 64 and k + 1 <= 4 * nw * 64 and lds_total(64, k + 1, nw, nw) <= LDS_LIMIT


@contextlib.contextmanager
def engine_with(**knobs):
    old = {n: os.environ.get(n) for n in KNOBS}
    for n in KNOBS:
        os.environ.pop(n, None)
    for n, v in knobs.items():
        if v is not None:
            os.environ[n] = str(v)
    try:
        yield pk.KBestEngine(0)
    finally:
        for n, v in old.items():
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v


def relay_knobs(nw, relay):
    # (the forced-relay legs of tools/soak.sh; the same routing switches without the relay, so that both run the 64-row kernel)
    return dict(KBEST_NWAVES=nw, KBEST_RELAY=3 if relay else 0, KBEST_NO_SMALL=1, KBEST_NO_LANE=1)


def launch(eng, costs, N, M, k, flags=0, maximize=False, cutoff=None):
    """kbest_batch_f64 with any KBEST_FLAG_* (the wrapper names only some of them)."""
    costs = np.ascontiguousarray(costs, dtype=np.float64).reshape(-1, N * M)
    B = costs.shape[0]
    r4c = np.empty((B, k, M), np.int32)
    c4r = np.empty((B, k, N), np.int32)
    gain = np.empty((B, k), np.float64)
    nf = np.empty(B, np.int32)
    o = eng._opts(maximize, cutoff, flags)
    p = eng_mod._ptr
    eng._check(eng.lib.kbest_batch_f64(eng.ctx, C.byref(o), B, N, M, None, None, p(costs), None, k, p(r4c), p(c4r), p(gain), p(nf), None))
    return nf, r4c, c4r, gain


def same(a, b, what):
    nfa, ra, ca, ga = a
    nfb, rb, cb, gb = b
    assert (nfa == nfb).all(), (what, nfa, nfb)
    for i, n in enumerate(nfa):
        n = max(int(n), 0)
        assert (ga[i, :n].view(np.int64) == gb[i, :n].view(np.int64)).all(), (what, i, "gain")
        assert (ra[i, :n] == rb[i, :n]).all(), (what, i, "row4col")
        assert (ca[i, :n] == cb[i, :n]).all(), (what, i, "col4row")


def check(eng, costs, N, M, k, what, flags=0, maximize=False, cutoff=None, want_relay=None):
    got = launch(eng, costs, N, M, k, flags, maximize, cutoff)
    route = eng.last_route()
    assert route & ROUTE_FAST, (what, route)
    if want_relay is not None:
        assert bool(route & ROUTE_RELAY) == want_relay, (what, route)
    onf, or4c, oc4r, og, _ = ol.orc_kbest_batch(np.ascontiguousarray(costs).reshape(-1, N * M), N, M, k, maximize=maximize, cutoff=cutoff)
    same(got, (onf, or4c, oc4r, og), what)
    return got


def dense(seed, B, N, scale=10.0):
    return np.random.default_rng(seed).random((B, N * N)) * scale


def few_free_columns(seed, B, N, free, maximize=False):
    """Square problems with `free` columns that have a choice: every other column has ONE finite entry (the forbidden ones are +inf,
    or -inf when maximising), the free columns share a dense free x free block.  The root then has at most `free` children with
    a solution: fewer known combinations than most k need, and with free <= 1 none."""
    rng = np.random.default_rng(seed)
    bad = -np.inf if maximize else np.inf
    out = np.empty((B, N * N))
    for b in range(B):
        c = np.full((N, N), bad)   # c[row, col]
        perm = rng.permutation(N)  # column j's own row
        for j in range(N):
            c[perm[j], j] = rng.random() * 10
        fc = rng.choice(N, size=free, replace=False)
        for j in fc:
            for j2 in fc:
                c[perm[j2], j] = rng.random() * 10
        out[b] = c.T.reshape(-1)  # column-major, as the library reads it: element (r, col) at r + col * N
    return out


COMBOS = [(nw, relay) for nw in (4, 8, 12, 16) for relay in (False, True)]


@pytest.mark.parametrize("nw,relay", COMBOS)
def test_launch_flavours_against_checker(nw, relay):
    """plain, cutoff, maximize, KBEST_FLAG_NO_T0, KBEST_FLAG_NO_OPT (no tickets) against the default (tickets), KBEST_FLAG_NO_TIE_CHECK
    (k) against the default (k + 1), and each pruned launch against the KBEST_FLAG_NO_PRUNE launch of the same batch."""
    N, k, B = 48 + nw, 120, 24
    assert fits(N, k, nw)
    want_relay = relay if nw != 16 else None  # (the relay is compiled for 4 / 8 / 12 waves; what 16 falls back to is the library's choice)
    costs = dense(7000 + nw, B, N)
    with engine_with(**relay_knobs(nw, relay)) as eng:
        plain = check(eng, costs, N, N, k, "plain", want_relay=want_relay)
        same(plain, launch(eng, costs, N, N, k, FLAG_NO_PRUNE), "plain vs no-prune")
        same(plain, check(eng, costs, N, N, k, "no-t0", FLAG_NO_T0), "t0 vs no-t0")
        same(plain, check(eng, costs, N, N, k, "no-opt", FLAG_NO_OPT), "tickets vs none")
        same(plain, check(eng, costs, N, N, k, "no-tie-check", FLAG_NO_TIE_CHECK), "k + 1 vs k")
        mx = check(eng, costs, N, N, k, "maximize", maximize=True)
        same(mx, launch(eng, costs, N, N, k, FLAG_NO_PRUNE, maximize=True), "maximize vs no-prune")
        # a cutoff that ends the list inside it: half-way up the gains of the first problem
        cut = 0.999 * float(plain[3][0, k // 2] - plain[3][0, 0])
        ct = check(eng, costs, N, N, k, "cutoff", cutoff=cut)
        assert (ct[0] < k).any()
        same(ct, launch(eng, costs, N, N, k, FLAG_NO_PRUNE, cutoff=cut), "cutoff vs no-prune")


@pytest.mark.parametrize("nw,relay", COMBOS)
def test_lazy_resolves_small_eager_region(nw, relay):
    """KBEST_EAGER: state slots for children kept in full when they are found.  With few of them most selected candidates have no saved
    state and phase A re-solves them from their parents' (the path behind the selection walk); the default keeps them all."""
    N, k, B = 64, 200, 12
    assert fits(N, k, nw)
    costs = dense(7100 + nw, B, N)
    res = []
    for eager in (4, None):
        with engine_with(KBEST_EAGER=eager, **relay_knobs(nw, relay)) as eng:
            res.append(check(eng, costs, N, N, k, f"eager={eager}"))
            same(res[-1], launch(eng, costs, N, N, k, FLAG_NO_PRUNE), f"eager={eager} vs no-prune")
    same(res[0], res[1], "small vs default eager region")


@pytest.mark.parametrize("nw", (8, 12, 16))
@pytest.mark.parametrize("k", (2, 3, 50, 200, 768))
def test_threshold_over_k(nw, k):
    """The a-priori threshold at the k the search's exits depend on (it runs with 8 waves or more): k = 2 (off), k = 3 (two known
    assignments are enough), 50 and 200 (the bracket's first steps), 768 (more doublings; 16 waves' pool).  Dense problems, and
    problems whose root has 0, 2, 3, 4 children with a solution -- fewer than k - 1 known combinations: the search must leave
    without a threshold, not with a wrong one."""
    N, B = 64, 6
    assert fits(N, k, nw)
    with engine_with(**relay_knobs(nw, False)) as eng:
        costs = dense(7200 + nw + k, 2 * B, N)
        got = check(eng, costs, N, N, k, "dense")
        same(got, launch(eng, costs, N, N, k, FLAG_NO_PRUNE), "dense vs no-prune")
        same(got, launch(eng, costs, N, N, k, FLAG_NO_T0), "dense vs no-t0")
        for free in (0, 2, 3, 4):
            for mx in (False, True):
                c = few_free_columns(7300 + nw + k + free, B, N, free, maximize=mx)
                got = check(eng, c, N, N, k, f"free={free} maximize={mx}", maximize=mx)
                same(got, launch(eng, c, N, N, k, FLAG_NO_PRUNE, maximize=mx), f"free={free} maximize={mx} vs no-prune")
        # a wide spread of the atoms (the doubling runs on) and a narrow one (the bracket holds nearly everything)
        rng = np.random.default_rng(7400 + nw + k)
        wide = np.exp(rng.random((B, N * N)) * 12.0)
        got = check(eng, wide, N, N, k, "wide spread")
        same(got, launch(eng, wide, N, N, k, FLAG_NO_PRUNE), "wide spread vs no-prune")
        narrow = 10.0 + rng.random((B, N * N)) * 1e-2  # (gains 640 +- 1e-2: far from exact ties in fp64)
        got = check(eng, narrow, N, N, k, "narrow spread")
        same(got, launch(eng, narrow, N, N, k, FLAG_NO_PRUNE), "narrow spread vs no-prune")


def test_shapes_fit_on_cpu():
    """Every (rows, k, waves) used above passes the launcher's own fit rule (no case is skipped for size)."""
    for nw in (4, 8, 12, 16):
        assert fits(48 + nw, 120, nw) and fits(64, 200, nw)
    for nw in (8, 12, 16):
        for k in (2, 3, 50, 200, 768):
            assert fits(64, k, nw)
