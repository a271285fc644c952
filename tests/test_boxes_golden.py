"""CPU: the checker's cost builders and toProbs pinned to the reference and to exact arithmetic.

Boxes: tests/golden/boxes_golden.npz holds what the reference's OWN computeBBCostMatrix and asgnBB return (verbatim slices of
boundBox.h:62-75 and assignment.cpp:724-797, oracle/ref_boxes_shim.cpp; gen_boxes_golden.py) on random stereo pairs with
non-zero offsets on both sides, duplicated boxes, integer-grid boxes whose optima tie exactly, geometric edge cases and edge
shapes.  orc_bb_costs / orc_asgn_bb must reproduce the profits and the matchings bit for bit.

Quadric costs: Eigen's LDLT is no part of the reference's tree, so d^T S^-1 d is held to exact rational arithmetic instead
(quadric_lib.py), relative to eps cond_2(S) d^T|S|^-1 d with eps = 2^-53 -- for a positive definite S that is eps cond_2(S) times
the value itself; for an indefinite S the value may cancel to nothing while its terms do not, and d^T|S|^-1 d is the sum without the
cancellation.  Measured on the checker over the 4 000 + 800 pairs of quadric_lib.pairs(default_rng(0xF2), 4000), cond_2 from 1 to
1e12: worst ratio 5.34 (an indefinite S of cond_2 1.09); positive definite alone 2.53 (S a multiple of the identity), structured
cases 1.57 (equal diagonal) and 0.55 (diagonal); above cond_2 = 100 every ratio is below 1.  QUADRIC_K = 32 is four times the
worst, rounded up to a power of two: the margin is for pairs the generator did not draw, not for the device, which must agree
with the checker bit for bit (test_gpu_cost_builders.py).

toProbs: tests/golden/toprobs_golden.npz (gen_toprobs_golden.py) -- sizes around the device kernel's 256-wide reduction, the
minimum last / repeated, entries at and next to min + 42, infinities, and NaN first (std::min_element keeps it: all zeros) and
inside (skipped)."""
import os

import numpy as np
import pytest

import boxes_lib as bl
import oracle_lib as ol
import quadric_lib as ql

GOLD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
QUADRIC_K = 32.0
QUADRIC_SEED, QUADRIC_N = 0xF2, 4000


class Boxes:
    """tests/golden/boxes_golden.npz, frame by frame."""

    def __init__(self):
        z = np.load(os.path.join(GOLD_DIR, "boxes_golden.npz"))
        self.names = [str(n) for n in z["names"]]
        self.family = [str(f) for f in z["family"]]
        self.nL, self.nR, self.gate = z["nL"].astype(int), z["nR"].astype(int), z["gate"]
        self.tied, self.ref_not_first = z["tied"].astype(int), z["ref_not_first"].astype(int)
        oL = np.concatenate([[0], np.cumsum(self.nL)]); oR = np.concatenate([[0], np.cumsum(self.nR)])
        oC = np.concatenate([[0], np.cumsum((self.nL + self.nR) * self.nL)])
        self.L = [z["L"][oL[f]: oL[f + 1]] for f in range(len(self.names))]
        self.R = [z["R"][oR[f]: oR[f + 1]] for f in range(len(self.names))]
        self.cost = [z["cost"][oC[f]: oC[f + 1]] for f in range(len(self.names))]
        self.assign = [z["assign"][oL[f]: oL[f + 1]].astype(np.int32) for f in range(len(self.names))]

    def __len__(self):
        return len(self.names)


BOXES = Boxes()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64).tolist()


def test_golden_holds_the_families_and_only_finite_profits():
    g = BOXES
    assert {f: g.family.count(f) for f in "abcde"} == {"a": 40, "b": 36, "c": 320, "d": 12, "e": 9}
    assert int((g.tied == 1).sum()) >= 80 and int((g.ref_not_first == 1).sum()) >= 20
    assert any((r[:, 4] != 0).any() for r in g.R) and any((l[:, 4] != 0).any() for l in g.L)
    for f in range(len(g)):
        c = g.cost[f]
        assert not np.isnan(c).any() and not (c == np.inf).any(), g.names[f]     # only the -inf fill is non-finite
        assert np.abs(g.L[f]).max(initial=0) <= 1e6 and np.abs(g.R[f]).max(initial=0) <= 1e6


def test_oracle_bb_costs_match_reference_golden():
    g = BOXES
    for f in range(len(g)):
        assert bits(ol.bb_costs(g.L[f], g.R[f], g.gate[f])) == bits(g.cost[f]), g.names[f]


def test_oracle_asgn_bb_matches_reference_golden():
    g = BOXES
    for f in range(len(g)):
        assert ol.asgn_bb(g.L[f], g.R[f], g.gate[f]).tolist() == g.assign[f].tolist(), g.names[f]


@pytest.mark.skipif(not ol.have_ref_boxes(), reason="oracle/_ref/libref_boxes.so not built (needs the reference's sources)")
def test_golden_is_what_the_compiled_reference_returns():
    g = BOXES
    for f in range(len(g)):
        assert bits(ol.ref_bb_costs(g.L[f], g.R[f], g.gate[f])) == bits(g.cost[f]), g.names[f]
        assert ol.ref_asgn_bb(g.L[f], g.R[f], g.gate[f]).tolist() == g.assign[f].tolist(), g.names[f]


@pytest.mark.skipif(not ol.have_ref_boxes(), reason="oracle/_ref/libref_boxes.so not built (needs the reference's sources)")
def test_oracle_boxes_vs_compiled_reference_live():
    """Fresh random frames of families a to c through the compiled slices of the reference and through the checker."""
    rng = np.random.default_rng(0x11FE)
    frames = [bl.random_stereo(rng, int(rng.integers(1, 20)), int(rng.integers(0, 20))) + (0.2,) for _ in range(120)]
    for kind in ("R", "L", "LR"):
        frames += [bl.duplicates(rng, kind, int(rng.integers(2, 8)), int(rng.integers(2, 8))) + (bl.GATES[i % 4],) for i in range(120)]
    frames += [bl.grid(rng, int(rng.integers(1, 8)), int(rng.integers(1, 8))) + (bl.GRID_GATES[i % 4],) for i in range(600)]
    for L, R, gate in frames:
        assert bits(ol.bb_costs(L, R, gate)) == bits(ol.ref_bb_costs(L, R, gate))
        assert ol.asgn_bb(L, R, gate).tolist() == ol.ref_asgn_bb(L, R, gate).tolist()


# ------------------------------------------------------------------------------------------------ quadric costs, exactly
def quadric_pairs(n=QUADRIC_N):
    return ql.pairs(np.random.default_rng(QUADRIC_SEED), n)


def quadric_bound_miss(got, p):
    """None where `got` is within QUADRIC_K eps cond_2(S) of the exact d^T S^-1 d (relative to d^T|S|^-1 d); else a description."""
    d, S = ql.formed(p)
    r = ql.ratio(got, d, S)
    return None if r <= QUADRIC_K else f"{p[0]}: {got!r} against {float(ql.exact_quadric(d, S))!r}, ratio {r:.3g} (cond {ql.scale_and_cond(d, S)[1]:.3g})"


def test_oracle_quadric_costs_vs_exact_rationals():
    P = quadric_pairs()
    conds = np.array([ql.scale_and_cond(*ql.formed(p))[1] for p in P])
    assert conds.min() < 2 and conds.max() > 1e11 and {p[0] for p in P} == {"spd", "indef", "equal_diag", "diagonal", "identity", "d_zero"}
    worst = 0.0
    for p in P:
        got = ol.quadric_costs(p[1][None], p[2][None], p[3][None], p[4][None], 10.0)
        assert got[1] == 10.0                                   # the column's own dummy row
        if p[0] == "d_zero":
            assert got[0] == 0.0
        d, S = ql.formed(p)
        assert np.array_equal(S, S.T)
        worst = max(worst, ql.ratio(got[0], d, S))
        assert quadric_bound_miss(got[0], p) is None, quadric_bound_miss(got[0], p)
    print(f"worst |error| / (eps cond_2(S) d^T|S|^-1 d) = {worst:.3g} over {len(P)} pairs (bound {QUADRIC_K:g})")
    assert worst > 0.5                                          # (the bound is not vacuous: the checker does round)


# ------------------------------------------------------------------------------------------------ toProbs
def toprobs_cases():
    z = np.load(os.path.join(GOLD_DIR, "toprobs_golden.npz"))
    off = z["off"]
    return [(str(n), z["x"][off[i]: off[i + 1]], z["want"][off[i]: off[i + 1]]) for i, n in enumerate(z["names"])]


def test_oracle_to_probs_matches_reference_golden():
    cases = toprobs_cases()
    assert {len(x) for _, x, _ in cases} >= {1, 255, 256, 257, 1000}
    for name, x, want in cases:
        got = x.copy()
        ol.oracle().orc_to_probs(got, got.size)
        assert np.isnan(got).tolist() == np.isnan(want).tolist(), name
        ok = ~np.isnan(want)
        assert bits(got[ok]) == bits(want[ok]), name
    by = {n: (x, w) for n, x, w in cases}
    assert np.isnan(by["nan_first"][0][0]) and (by["nan_first"][1] == 0).all()          # std::min_element keeps a NaN first element
    assert (by["nan_interior"][1] > 0).any() and (by["nan_interior"][1][[130, 257]] == 0).all()
    x, w = by["exactly_at_gate"]
    assert w[3] == 0.0 and w[290] > 0.0 and w[291] == 0.0 and w[77] == 1.0               # min + 42 > x is strict


@pytest.mark.skipif(not ol.have_ref_assign(), reason="oracle/_ref/libref_assign.so not built (needs the reference's sources)")
def test_to_probs_golden_is_what_the_compiled_reference_returns():
    for name, x, want in toprobs_cases():
        got = x.copy()
        ol.ref_assign().ref_to_probs(got, got.size)
        assert bits(got) == bits(want), name
