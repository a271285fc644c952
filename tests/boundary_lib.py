"""Problems that sit exactly on the cutoff and gate comparisons of the reference (shortestPathCPP.cpp's cutHyp and break,
assignment.cpp's conditionCosts and assignmentProb).  Random costs almost never land on them; these generators put values on
them on purpose and count how many problems they did put there, so that a test can assert a floor on that count.

k-best families (each returns (cases, on), a case as soak_lib.draw_case makes it, `on` = problems on a boundary):
  B1  tie-free, a gain exactly on g0 +- cutoff, one ulp inside or one ulp outside; the batch = row permutations of one matrix
  B2  an integer grid with an integer cutoff: whole tie levels on the boundary
  B3  a 0.1 grid (not exact in binary), with and without negative entries: CDelta != 0, the internal and external sums round
      apart
Association families (each returns (frames, on), a frame a dict nL, nM, cost):
  A1  raw blocks on an integer or 1/16 grid: entries colMin + {0 .. 43}, some one ulp beyond colMin + 42
  A2  nM == 1 frames with a conditioned entry of exactly 42

Own random streams: soak_lib's stream is untouched."""
import numpy as np

import oracle_lib as ol

GATE = 42.0  # assignment.cpp's `cutoff` (constsUtils.h)


def _edge(g0, c, maximize):
    return g0 - c if maximize else g0 + c


def cutoff_onto(g0, target, maximize):
    """A cutoff c > 0 with g0 + c == target in float64 (g0 - c when maximising), found by nextafter steps; None if none."""
    c = (g0 - target) if maximize else (target - g0)
    if not c > 0:
        return None
    for _ in range(64):
        v = _edge(g0, c, maximize)
        if v == target:
            return float(c)
        c = np.nextafter(c, np.inf if (v < target) != maximize else -np.inf)
        if not c > 0:
            return None
    return None


def on_edge(cost, N, M, k, maximize, cutoff, ulps=0):
    """Does some gain among the k best (no cutoff) lie on g0 +- cutoff (within `ulps` ulps; 0: exactly)?"""
    nf, _, _, g = ol.orc_kbest(cost, N, M, k, maximize)
    if nf < 2:
        return False
    e = _edge(g[0], cutoff, maximize)
    tol = ulps * np.spacing(abs(e))
    return bool((np.abs(g[1:nf] - e) <= tol).any())


def _tie_free(g, n):
    return n < 2 or bool((np.diff(g[:n]) != 0).all())


def b1_target(gj, which, maximize):
    """Where B1 puts g0 +- cutoff: on gain j (which = 0: kept, the comparisons are strict), one ulp short of it (1: gain j is
    beyond the cutoff) or one ulp past it (2: kept)."""
    if which == 0:
        return gj
    return np.nextafter(gj, (-np.inf if which == 1 else np.inf) * (-1 if maximize else 1))


def b1_cases(seed, n, rows=(2, 32), k=(3, 10, 40), B=4, square=False, max_frac=0.3, min_nf=4, max_cols=None):
    """B1: fine dyadic grid (exact sums: internal and external comparisons agree) or continuous costs.  The cutoff puts g0 +- c
    on gain j or one ulp to either side of it (b1_target); every problem of a case is a row permutation of the same matrix (calcGain
    sums over columns in column order: the same gains bit for bit).  max_cols caps the columns of the larger problems."""
    rng = np.random.default_rng(seed)
    cases, on = [], 0
    while len(cases) < n:
        N = int(rng.integers(rows[0], rows[1] + 1))
        M = N if square or rng.random() < 0.5 else int(rng.integers(1, N + 1))
        M = M if max_cols is None else min(M, max_cols)
        kk = int(rng.choice(k))
        maximize = bool(rng.random() < max_frac)
        dyadic = len(cases) % 2 == 0
        base = rng.integers(0, 1 << 24, N * M) * 2.0 ** -20 if dyadic else rng.random(N * M) * 10.0
        nf, _, _, g = ol.orc_kbest(base, N, M, kk + 1, maximize)
        if nf < min_nf or not _tie_free(g, nf):
            continue
        j = int(rng.integers(1, min(nf, kk)))
        which = len(cases) % 3
        target = b1_target(g[j], which, maximize)
        c = cutoff_onto(g[0], target, maximize)
        if c is None:
            continue
        assert _edge(g[0], c, maximize) == target
        C = np.empty((B, N * M))
        for b in range(B):
            perm = np.arange(N) if b == 0 else rng.permutation(N)
            C[b] = base.reshape(M, N)[:, perm].reshape(-1)
        cases.append(dict(N=N, M=M, k=kk, B=B, maximize=maximize, cutoff=c, kind="b1-" + ("dyadic" if dyadic else "cont"), C=C,
                          slot=j, which=which))
        on += B
    return cases, on


def b2_cases(seed, n, rows=(2, 8), k=(3, 10, 40, 200), B=3, max_frac=0.3):
    """B2: integers 0 - 4, an integer cutoff 1 - 3: tie levels on the boundary and straddling it."""
    rng = np.random.default_rng(seed)
    cases, on = [], 0
    for i in range(n):
        N = int(rng.integers(rows[0], rows[1] + 1))
        M = int(rng.integers(1, N + 1)) if i % 2 else N
        kk = int(rng.choice(k))
        maximize = bool(rng.random() < max_frac)
        cut = float(rng.integers(1, 4))
        C = rng.integers(0, 5, (B, N * M)).astype(np.float64)
        on += sum(on_edge(C[b], N, M, kk, maximize, cut) for b in range(B))
        cases.append(dict(N=N, M=M, k=kk, B=B, maximize=maximize, cutoff=cut, kind="b2-int", C=C))
    return cases, on


def b3_cases(seed, n, rows=(2, 8), k=(3, 10, 40, 200), B=3, max_frac=0.3):
    """B3: grids of 0.1 (not exact in binary): [-2, 1] with a cutoff of 0.1 - 1.1, [0, 1] (no negative entry), -0.6 .. 0.2 with
    0.3, and 1e15 + a 0.1 grid with 0.2.  CDelta = min * numCol is nonzero whenever the smallest entry is, so cutHyp (on C - min)
    and the break (CDelta added back) may round apart.  `on` counts gains within 2 ulps of the edge."""
    rng = np.random.default_rng(seed)
    cases, on = [], 0
    for i in range(n):
        N = int(rng.integers(rows[0], rows[1] + 1))
        M = int(rng.integers(1, N + 1)) if i % 2 else N
        kk = int(rng.choice(k))
        maximize = bool(rng.random() < max_frac)
        sub = i % 4
        if sub == 0:
            C = rng.integers(-20, 11, (B, N * M)) * 0.1
            cut = float(rng.integers(1, 12)) * 0.1
        elif sub == 1:
            C = rng.integers(0, 11, (B, N * M)) * 0.1
            cut = float(rng.integers(1, 12)) * 0.1
        elif sub == 2:
            C = rng.integers(-6, 3, (B, N * M)) * 0.1
            cut = 0.3
        else:
            C = 1e15 + rng.integers(0, 11, (B, N * M)) * 0.1
            cut = 0.2
        on += sum(on_edge(C[b], N, M, kk, maximize, cut, ulps=2) for b in range(B))
        cases.append(dict(N=N, M=M, k=kk, B=B, maximize=maximize, cutoff=cut, kind="b3-tenths", C=C))
    return cases, on


A1_STEPS = (0.0, 1.0, 2.0, 14.0, 21.0, 28.0, 40.0, 41.0, 42.0, 43.0)
A1_DUMMY = (0.0, 21.0, 42.0)


def a1_frames(seed, n, shapes, sixteenths_every=2, inf_frac=0.25, fine_frac=0.5):
    """A1: raw (nL + nM) x nM blocks.  Column c has its minimum colMin (one entry) on an integer (or 1/16) grid; the other
    landmark entries are colMin + one of A1_STEPS[1:], colMin + a value of the grid in [1, 40) (a share fine_frac: keeps the
    levels of equal gains small enough to be completed), +inf (a share inf_frac) or nextafter(colMin + 42, +inf) (must be
    dropped by conditionCosts); the dummy entry of column c (row nL + c) is colMin + {0, 21, 42}, the other dummies +inf.  `on`
    counts frames with a conditioned entry of exactly 42 or a k-best solution at exactly best + 42."""
    rng = np.random.default_rng(seed)
    frames, on = [], 0
    steps = np.asarray(A1_STEPS[1:])
    for i in range(n):
        nL, nM = shapes[i % len(shapes)]
        nR = nL + nM
        step = 1.0 / 16 if i % sixteenths_every == 1 else 1.0
        C = np.full((nM, nR), np.inf)
        for c in range(nM):
            cm = float(rng.integers(0, 200)) * step
            u = rng.random(nL)
            off = np.where(rng.random(nL) < fine_frac, rng.integers(int(1 / step), int(40 / step), nL) * step,
                           steps[rng.integers(0, len(steps), nL)])
            C[c, :nL] = cm + off
            C[c, :nL][u < inf_frac] = np.inf
            C[c, :nL][(u >= inf_frac) & (u < inf_frac + 0.07)] = np.nextafter(cm + GATE, np.inf)
            C[c, nL + c] = cm + A1_DUMMY[int(rng.integers(0, len(A1_DUMMY)))]
            if C[c, nL + c] != cm:  # the minimum is reached in every column: the dummy, or one landmark entry
                C[c, int(rng.integers(0, nL))] = cm
        frames.append(dict(nL=nL, nM=nM, cost=C.reshape(-1)))
    for f in frames:
        on += a_frame_on_edge(f)
    return frames, on


def a2_frames(seed, n, nLs=(1, 3, 8, 30, 63)):
    """A2: nM == 1: one column of colMin + {0 .. 43}, one ulp beyond colMin + 42 or +inf; a conditioned entry of exactly 42 in
    every frame (strictly below 42 weighs, 42 itself does not)."""
    rng = np.random.default_rng(seed)
    frames, on = [], 0
    for i in range(n):
        nL = int(nLs[i % len(nLs)])
        cm = float(rng.integers(0, 200)) * (1.0 / 16 if i % 2 else 1.0)
        col = cm + np.asarray(A1_STEPS)[rng.integers(0, len(A1_STEPS), nL + 1)]
        u = rng.random(nL + 1)
        col[u < 0.15] = np.inf
        col[(u >= 0.15) & (u < 0.25)] = np.nextafter(cm + GATE, np.inf)
        col[int(rng.integers(0, nL + 1))] = cm
        where42 = [r for r in range(nL + 1) if col[r] != cm]
        col[where42[int(rng.integers(0, len(where42)))] if where42 else 0] = cm + GATE
        frames.append(dict(nL=nL, nM=1, cost=col))
    for f in frames:
        on += a_frame_on_edge(f)
    return frames, on


def a_frame_on_edge(f):
    """A conditioned entry of exactly 42, or (nM > 1) a solution at exactly best + 42 among the k = 200 best."""
    nL, nM = f["nL"], f["nM"]
    cond, idx = ol.condition_costs(f["cost"], nL + nM, nM)
    if (cond == GATE).any():
        return 1
    if nM == 1:
        return 0
    nf, _, _, g = ol.orc_kbest(cond, len(idx), nM, 200)
    return int(nf > 0 and (g[:nf] == g[0] + GATE).any())
