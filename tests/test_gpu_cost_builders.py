"""GPU: the cost builders of kbest_costs.hip and the box matching behind them against the reference's own answers
(tests/golden/boxes_golden.npz, toprobs_golden.npz: see test_boxes_golden.py), against the checker bit for bit, and against
exact rational arithmetic (quadric_lib.py) within the bound measured and derived in test_boxes_golden.py."""
import numpy as np
import pytest

import boxes_lib as bl
import oracle_lib as ol
import quadric_lib as ql
from test_boxes_golden import BOXES, QUADRIC_K, QUADRIC_SEED, bits, quadric_bound_miss, toprobs_cases
from test_cost_builders import synth_quadric_frame

pytestmark = pytest.mark.gpu


def idx(name):
    return BOXES.names.index(name)


def same_bits(got, want, what):
    """Bit for bit; NaNs (any payload) only where the other side has one."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    assert np.isnan(got).tolist() == np.isnan(want).tolist(), what
    ok = ~np.isnan(want)
    bad = np.flatnonzero(got[ok].view(np.int64) != want[ok].view(np.int64))
    assert bad.size == 0, f"{what}: {bad.size} entries differ, first {got[ok][bad[0]]!r} against {want[ok][bad[0]]!r}"


# ------------------------------------------------------------------------------------------------ box profits
def test_bb_costs_equal_reference_golden_bits(engine):
    g = BOXES
    whole = engine.bb_costs(g.L, g.R, 0.2)            # one gate per call: the frames recorded with it are compared below
    for gate in sorted(set(g.gate.tolist())):
        sel = [f for f in range(len(g)) if g.gate[f] == gate]
        got = engine.bb_costs([g.L[f] for f in sel], [g.R[f] for f in sel], gate)
        for f, c in zip(sel, got):
            same_bits(c, g.cost[f], g.names[f])
        if gate == 0.2:
            for f in sel:
                same_bits(whole[f], g.cost[f], g.names[f] + " (in the whole golden as one batch)")
    # the IoU part does not depend on the gate: every frame of the one whole batch, with its dummies' profit set aside
    for f in range(len(g)):
        nL, nRows = g.nL[f], g.nL[f] + g.nR[f]
        if nL:
            same_bits(whole[f].reshape(nL, nRows)[:, : g.nR[f]], g.cost[f].reshape(nL, nRows)[:, : g.nR[f]], g.names[f])


def test_bb_costs_alone_and_reversed(engine):
    g = BOXES
    alone = [idx("e_beyond_64_rows"), idx("e_three_strides"), idx("e_many_right"), idx("e_1x1"), idx("d_overlap_only_after_offset"),
             idx("d_inverted_x"), idx("a0"), idx("a1")]
    for f in alone:
        same_bits(engine.bb_costs([g.L[f]], [g.R[f]], g.gate[f])[0], g.cost[f], g.names[f] + " alone")
    sel = [f for f in range(len(g)) if g.gate[f] == 0.2][::-1]
    assert idx("e_beyond_64_rows") in sel and idx("e_nL0") in sel and idx("e_nR0") in sel
    got = engine.bb_costs([g.L[f] for f in sel], [g.R[f] for f in sel], 0.2)
    for f, c in zip(sel, got):
        same_bits(c, g.cost[f], g.names[f] + " reversed")


# ------------------------------------------------------------------------------------------------ box matching
def match_by_gate(engine, frames, reverse=False):
    """bb_match on the given golden frames, one call per gate (the gate is a launch parameter): {frame: assignment}."""
    g = BOXES
    out = {}
    for gate in sorted({float(g.gate[f]) for f in frames}):
        sel = [f for f in frames if g.gate[f] == gate]
        if reverse:
            sel = sel[::-1]
        for f, a in zip(sel, engine.bb_match([g.L[f] for f in sel], [g.R[f] for f in sel], gate)):
            out[f] = a
    return out


@pytest.fixture(scope="module")
def matched(engine):
    return match_by_gate(engine, list(range(len(BOXES))))


def test_bb_match_equals_reference_golden(matched):
    g = BOXES
    miss = {}
    for f, a in matched.items():
        if a.tolist() != g.assign[f].tolist():
            miss.setdefault(g.family[f], []).append(g.names[f])
    tied = [f for f in matched if g.tied[f] == 1]
    tied_miss = [g.names[f] for f in tied if matched[f].tolist() != g.assign[f].tolist()]
    notfirst = [f for f in matched if g.ref_not_first[f] == 1]
    notfirst_miss = [g.names[f] for f in notfirst if matched[f].tolist() != g.assign[f].tolist()]
    print("mismatches per family:", {k: len(v) for k, v in miss.items()}, "| tied optimum:", len(tied_miss), "of", len(tied),
          "| reference not the lexicographically first optimum:", len(notfirst_miss), "of", len(notfirst))
    assert not miss, miss


def test_bb_match_is_valid_and_as_profitable_as_the_reference(matched):
    """Independently of which optimum the reference took: a matching, and of the reference's total on the golden profits."""
    g = BOXES
    for f, a in matched.items():
        nL, nR = g.nL[f], g.nR[f]
        assert len(a) == nL and all(-1 <= x < nR for x in a), g.names[f]
        used = [x for x in a if x >= 0]
        assert len(set(used)) == len(used), g.names[f]
        mine = bl.total_profit(g.cost[f], nL, nR, bl.row4col_of(a, nR))
        assert mine is not None and mine == bl.total_profit(g.cost[f], nL, nR, bl.row4col_of(g.assign[f], nR)), g.names[f]


def test_bb_match_on_a_tied_frame_does_not_depend_on_its_batch(engine, matched):
    g = BOXES
    gate = 0.2
    tied = [f for f in range(len(g)) if g.ref_not_first[f] == 1 and g.gate[f] == gate][:6]
    assert len(tied) >= 3
    others = [f for f in range(len(g)) if g.gate[f] == gate and f not in tied]
    for t in tied:
        alone = engine.bb_match([g.L[t]], [g.R[t]], gate)[0]
        sel = [t] + others
        first = engine.bb_match([g.L[f] for f in sel], [g.R[f] for f in sel], gate)[0]
        sel = others[::-1] + [t]
        last = engine.bb_match([g.L[f] for f in sel], [g.R[f] for f in sel], gate)[-1]
        assert alone.tolist() == first.tolist() == last.tolist() == matched[t].tolist() == g.assign[t].tolist(), g.names[t]
    rev = match_by_gate(engine, list(range(len(g))), reverse=True)
    assert all(rev[f].tolist() == matched[f].tolist() for f in matched)


# ------------------------------------------------------------------------------------------------ quadric costs
def orc_costs(frames, gate):
    return [ol.quadric_costs(*f, gate) for f in frames]


def test_quadric_costs_bit_equal_to_checker_and_within_bound_of_exact(engine):
    P = ql.pairs(np.random.default_rng(QUADRIC_SEED), 1000)
    frames = [(p[1][None], p[2][None], p[3][None], p[4][None]) for p in P]
    got = engine.quadric_costs(frames, 10.0)
    want = orc_costs(frames, 10.0)
    worst = 0.0
    for p, c, o in zip(P, got, want):
        same_bits(c, o, p[0])
        worst = max(worst, ql.ratio(c[0], *ql.formed(p)))
        assert quadric_bound_miss(c[0], p) is None, quadric_bound_miss(c[0], p)
    print(f"device worst |error| / (eps cond_2(S) d^T|S|^-1 d) = {worst:.3g} over {len(P)} pairs (bound {QUADRIC_K:g})")
    # the same pairs as frames of several landmarks and measurements: every (landmark, measurement) combination
    rng = np.random.default_rng(5)
    frames = []
    for _ in range(30):
        a, b = rng.choice(len(P), size=int(rng.integers(1, 9))), rng.choice(len(P), size=int(rng.integers(1, 6)))
        frames.append((np.array([P[i][1] for i in a]), np.array([P[i][2] for i in a]), np.array([P[i][3] for i in b]), np.array([P[i][4] for i in b])))
    for f, c, o in zip(frames, engine.quadric_costs(frames, 55.0), orc_costs(frames, 55.0)):
        same_bits(c, o, "combined")


def test_quadric_costs_singular_and_mixed_shapes(engine):
    rng = np.random.default_rng(6)
    v = rng.normal(size=3)
    singular = [np.zeros((3, 3)), np.outer(v, v), np.diag([1.0, 2.0, 0.0]), np.diag([0.0, 0.0, 3.0]), np.ones((3, 3))]
    # S = the singular matrix + 0: the pivot is 0 somewhere, the checker's (and the kernel's) divisions give inf and NaN
    f_sing = (rng.normal(size=(len(singular), 3)), np.array(singular), rng.normal(size=(2, 3)), np.zeros((2, 3, 3)))
    empty = (np.zeros((0, 3)), np.zeros((0, 3, 3)))
    frames = [f_sing,
              empty + synth_quadric_frame(rng, 0, 4)[2:],                 # nL = 0: gates and +inf only
              synth_quadric_frame(rng, 7, 1),                              # nM = 1
              synth_quadric_frame(rng, 60, 9),                             # (60 + 9) 9 = 621 entries: three strides of 256
              synth_quadric_frame(rng, 1, 1)]
    got = engine.quadric_costs(frames, 10.0)
    want = orc_costs(frames, 10.0)
    for i, (c, o) in enumerate(zip(got, want)):
        assert np.isinf(c).tolist() == np.isinf(o).tolist(), i
        same_bits(c, o, f"frame {i}")
    assert not np.isfinite(want[0].reshape(2, 7)[:, :5]).all()            # (the singular frame does produce NaN / inf costs)
    for i in (1, 2, 3, 4):                                                 # the same frames alone
        same_bits(engine.quadric_costs([frames[i]], 10.0)[0], want[i], f"frame {i} alone")


# ------------------------------------------------------------------------------------------------ toProbs
def test_to_probs_matches_reference_golden(engine):
    for name, x, want in toprobs_cases():
        got = engine.to_probs(x)
        assert not np.isnan(got).any(), name
        assert ((got == 0) == (want == 0)).all(), (name, np.flatnonzero((got == 0) != (want == 0))[:8].tolist())
        np.testing.assert_allclose(got, want, rtol=1e-14, atol=0, err_msg=name)
