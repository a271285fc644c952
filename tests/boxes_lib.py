"""Stereo box frames for the tests of computeBBCostMatrix / asgnBB: the families recorded in
tests/golden/boxes_golden.npz (gen_boxes_golden.py) and drawn afresh by the live comparison of the checker with the
compiled reference slice.  A frame is (L (nL, 5), R (nR, 5), gate); a box is (xmin, ymin, xmax, ymax, xOffset).
Every coordinate is finite and far below 1e6; no family produces a NaN or +inf profit."""
from __future__ import annotations

import itertools
from fractions import Fraction

import numpy as np

from test_cost_builders import synth_boxes

GATES = (0.0, 0.2, 0.6, 1.0)
GRID_GATES = (0.0, 0.2, 0.5, 1.0)


def random_stereo(rng, nL, nR):
    """Family a: synth_boxes with a non-zero xOffset on the right boxes too (boundBox::IoU applies the offset of *this in
    BOTH directions, boundBox.h:63-64: a kernel that took the wrong box's offset passes on right offsets of 0)."""
    L, R = synth_boxes(rng, nL, nR)
    R[:, 4] = rng.uniform(3.0, 40.0, size=nR) * rng.choice([-1.0, 1.0], size=nR)
    return L, R


def duplicates(rng, kind, nL, nR):
    """Family b: identical right boxes ("R"), identical left boxes ("L"), or both ("LR"): exactly equal IoUs."""
    L, R = random_stereo(rng, nL, nR)
    if "R" in kind:
        for j in range(1, nR):
            if rng.random() < 0.6:
                R[j] = R[rng.integers(j)]
    if "L" in kind:
        for i in range(1, nL):
            if rng.random() < 0.6:
                L[i] = L[rng.integers(i)]
    return L, R


def grid(rng, nL, nR):
    """Family c: corners on multiples of 10 in a small window, left offsets 0 or -10, right offsets 0 or 10: few distinct
    IoU values, so optima tie exactly."""
    def box(off):
        x0, y0 = 10.0 * rng.integers(0, 3), 10.0 * rng.integers(0, 2)
        return [x0, y0, x0 + 10.0 * rng.integers(1, 3), y0 + 10.0 * rng.integers(1, 3), off]
    L = np.array([box(-10.0 * rng.integers(0, 2)) for _ in range(nL)], dtype=np.float64).reshape(nL, 5)
    R = np.array([box(10.0 * rng.integers(0, 2)) for _ in range(nR)], dtype=np.float64).reshape(nR, 5)
    return L, R


def geometry():
    """Family d: (name, L, R, gate)."""
    b = lambda *v: np.array(v, dtype=np.float64).reshape(-1, 5)  # noqa: E731
    yield "touch_lr", b([0, 0, 10, 10, 0]), b([10, 0, 20, 10, 0], [5, 0, 15, 10, 0]), 0.2           # l == r on the first
    yield "touch_tb", b([0, 0, 10, 10, 0]), b([0, 10, 10, 20, 0], [0, 5, 10, 15, 0]), 0.2           # t == b on the first
    yield "touch_after_offset", b([0, 0, 10, 10, -5]), b([5, 0, 15, 10, 0], [-15, 0, -5, 10, 0]), 0.0
    yield "containment", b([0, 0, 100, 100, 0], [40, 40, 60, 60, 0]), b([40, 40, 60, 60, 0], [10, 10, 90, 90, 0], [0, 0, 100, 100, 0]), 0.2
    yield "identical_gate1", b([3, 4, 50, 60, 0], [100, 4, 150, 60, 0]), b([3, 4, 50, 60, 0], [100, 4, 150, 60, 0]), 1.0  # IoU 1 ties with the dummy
    yield "identical_gate1_offset", b([13, 4, 60, 60, -10]), b([3, 4, 50, 60, 0], [3, 4, 50, 60, 0]), 1.0
    yield "zero_area", b([10, 10, 10, 30, 0], [0, 0, 40, 40, 0]), b([10, 10, 10, 30, 0], [5, 5, 35, 35, 0], [0, 0, 0, 0, 0]), 0.2
    yield "zero_height", b([0, 20, 40, 20, 0], [0, 0, 40, 40, 0]), b([0, 0, 40, 40, 0], [0, 20, 40, 20, 0]), 0.0
    yield "inverted_x", b([30, 0, 10, 20, 0], [0, 0, 40, 20, 0]), b([0, 0, 40, 20, 0], [35, 0, 5, 20, 0], [12, 2, 28, 18, 0]), 0.2  # xmax < xmin
    yield "overlap_only_after_offset", b([100, 0, 140, 40, -80], [300, 0, 340, 40, 0]), b([20, 0, 60, 40, 0], [220, 0, 260, 40, 80]), 0.2
    yield "offset_separates", b([0, 0, 40, 40, -100]), b([0, 0, 40, 40, 0]), 0.1
    yield "negative_coordinates", b([-50, -50, -10, -10, 5], [-30, -30, 10, 10, -5]), b([-45, -50, -5, -10, 0], [-35, -30, 5, 10, 2.5]), 0.2


def shapes(rng):
    """Family e: (name, L, R, gate).  19 + 19: (nR + nL) nL = 722 entries, three strides of the cost kernel's 256 threads;
    50 + 30: 80 rows, the general-size kernel under maximise with the -inf fill."""
    for name, nL, nR, gate in (("nL0", 0, 3, 0.2), ("nR0", 3, 0, 0.2), ("nL0_nR0", 0, 0, 0.2), ("1x1", 1, 1, 0.2), ("1x1_gated", 1, 1, 0.99),
                               ("tall_cols", 8, 3, 0.2), ("many_right", 2, 30, 0.2), ("three_strides", 19, 19, 0.2),
                               ("beyond_64_rows", 30, 50, 0.2)):
        L, R = random_stereo(rng, nL, nR)
        yield name, L, R, gate


def row4col_of(asg, nR):
    """asgnBB's answer back as the solver's row4col: column c unmatched sits on its own dummy row nR + c (the only finite one)."""
    return tuple(int(a) if a >= 0 else nR + c for c, a in enumerate(asg))


def total_profit(cost, nL, nR, row4col):
    """Exact (rational) sum of the float64 profits of a matching, or None where it uses a -inf entry."""
    nRows = nR + nL
    s = Fraction(0)
    for c, r in enumerate(row4col):
        x = float(cost[c * nRows + r])
        if x == -np.inf:
            return None
        s += Fraction(x)
    return s


def all_optima(cost, nL, nR):
    """Every optimal row4col of the (nR + nL) x nL maximisation, by enumeration (small frames only), sorted
    lexicographically; the sums are compared exactly."""
    nRows = nR + nL
    C = np.asarray(cost, dtype=np.float64).reshape(nL, nRows)
    rows = [[r for r in range(nRows) if C[c, r] != -np.inf] for c in range(nL)]
    best, opt = None, []
    for pick in itertools.product(*rows):
        if len(set(pick)) != nL:
            continue
        s = float(sum(C[c, r] for c, r in enumerate(pick)))
        if best is None or s > best + 1e-9:
            best, opt = s, [pick]
        elif s >= best - 1e-9:
            opt.append(pick)
            best = max(best, s)
    exact = [(total_profit(cost, nL, nR, p), p) for p in opt]
    top = max(e[0] for e in exact)
    return sorted(p for s, p in exact if s == top)
