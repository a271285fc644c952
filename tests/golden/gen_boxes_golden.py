"""Generate tests/golden/boxes_golden.npz from the reference's OWN stereo box matching.

Run in the build container only (needs the reference's sources for oracle/_ref):

    make -C oracle && python tests/golden/gen_boxes_golden.py

It loads oracle/_ref/libref_boxes.so -- verbatim line ranges of the reference's boundBox.h (IoU, :62-75) and
assignment.cpp (asgnBB and computeBBCostMatrix, :724-797), cut and compiled -O2 strict IEEE as oracle/Makefile and
oracle/ref_boxes_shim.cpp describe, linked against the unmodified solver -- and records, for the seeded frames of
tests/boxes_lib.py, exactly what computeBBCostMatrix and asgnBB return.  The fixture holds data only.

Layout (frames packed back to back; frame f owns L[offL[f]:offL[f+1]], R[offR[f]:offR[f+1]], cost[offC[f]:offC[f+1]] --
(nR + nL) x nL column-major -- and assign[offL[f]:offL[f+1]]):
    names, family ("a" .. "e"), nL, nR, gate, L, R, cost, assign,
    tied         1: the optimum is attained by more than one matching, 0: by one, -1: not enumerated (nL > 4 or nR > 5, or not family c)
    ref_not_first 1: ... and the reference's matching is not the lexicographically first optimal row4col, 0: it is, -1: as above
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import boxes_lib as bl  # noqa: E402
import oracle_lib as ol  # noqa: E402
from npz_fixed import savez_compressed_fixed  # noqa: E402


def frames():
    """Yields (name, family, L, R, gate)."""
    rng = np.random.default_rng(0xB0C5A)
    for i in range(40):
        nL, nR = int(rng.integers(1, 20)), int(rng.integers(0, 20))
        yield (f"a{i}", "a") + bl.random_stereo(rng, nL, nR) + (0.2,)
    rng = np.random.default_rng(0xB0C5B)
    for kind in ("R", "L", "LR"):
        for gate in bl.GATES:
            for i in range(3):
                nL, nR = int(rng.integers(2, 7)), int(rng.integers(2, 7))
                yield (f"b_{kind}_g{gate}_{i}", "b") + bl.duplicates(rng, kind, nL, nR) + (gate,)
    rng = np.random.default_rng(0xB0C5D)
    for i in range(320):
        # three frames in four small enough to enumerate every optimum
        small = i % 4 != 3
        nL, nR = int(rng.integers(1, 5 if small else 8)), int(rng.integers(1, 6 if small else 8))
        yield (f"c{i}", "c") + bl.grid(rng, nL, nR) + (bl.GRID_GATES[(i // 4 + i) % 4],)
    for name, L, R, gate in bl.geometry():
        yield "d_" + name, "d", L, R, gate
    rng = np.random.default_rng(0xB0C5E)
    for name, L, R, gate in bl.shapes(rng):
        yield "e_" + name, "e", L, R, gate


def main():
    names, fam, nLs, nRs, gates, Ls, Rs, costs, asgs, tied, notfirst = [], [], [], [], [], [], [], [], [], [], []
    for name, family, L, R, gate in frames():
        nL, nR = len(L), len(R)
        assert np.isfinite(L).all() and np.isfinite(R).all() and max(np.abs(L).max(initial=0), np.abs(R).max(initial=0)) <= 1e6, name
        cost = ol.ref_bb_costs(L, R, gate)
        # nothing non-finite other than the -inf fill may reach a solver entry
        assert not np.isnan(cost).any() and not (cost == np.inf).any(), name
        asg = ol.ref_asgn_bb(L, R, gate)
        t = nf = -1
        if family == "c" and nL <= 4 and nR <= 5:
            opt = bl.all_optima(cost, nL, nR)
            mine = bl.row4col_of(asg, nR)
            assert mine in opt, (name, mine, opt)          # the reference's matching is optimal
            t, nf = int(len(opt) > 1), int(mine != opt[0])
        names.append(name); fam.append(family); nLs.append(nL); nRs.append(nR); gates.append(gate)
        Ls.append(L.reshape(-1, 5)); Rs.append(R.reshape(-1, 5)); costs.append(cost); asgs.append(asg)
        tied.append(t); notfirst.append(nf)
    tied, notfirst = np.array(tied, np.int8), np.array(notfirst, np.int8)
    n_enum, n_tied, n_notfirst = int((tied >= 0).sum()), int((tied == 1).sum()), int((notfirst == 1).sum())
    print(f"{len(names)} frames; family c: {fam.count('c')}, enumerated {n_enum}, tied optimum {n_tied}, "
          f"reference not the lexicographically first optimum {n_notfirst}")
    assert n_tied >= 80 and n_notfirst >= 20, (n_tied, n_notfirst)
    out = dict(names=np.array(names), family=np.array(fam), nL=np.array(nLs, np.int32), nR=np.array(nRs, np.int32),
               gate=np.array(gates, np.float64), L=np.concatenate(Ls), R=np.concatenate(Rs), cost=np.concatenate(costs),
               assign=np.concatenate(asgs).astype(np.int8), tied=tied, ref_not_first=notfirst)
    path = os.path.join(HERE, "boxes_golden.npz")
    savez_compressed_fixed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.endswith(".npz") and f != "boxes_golden.npz")
    assert os.path.getsize(path) <= largest, (os.path.getsize(path), largest)


if __name__ == "__main__":
    main()
