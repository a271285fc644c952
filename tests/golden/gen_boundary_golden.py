"""Generate tests/golden/boundary_golden.npz: problems on the cutoff and gate boundaries (tests/boundary_lib.py) answered by the
compiled reference.

Run in the build container only (needs the reference sources for oracle/_ref):

    make -C oracle && python tests/golden/gen_boundary_golden.py

k-best cases: the first problem of B1 / B2 / B3 cases (kBest2DCutoff of the unmodified solver, oracle/_ref/libref_kbest.so).
Association frames: A1 / A2 raw blocks through the reference's own conditionCosts -> assignmentProb (and bruteForceProb on the
smaller ones) of oracle/_ref/libref_assign.so.  The fixture holds data only: inputs and what the reference returned.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import boundary_lib as bl  # noqa: E402
import oracle_lib as ol  # noqa: E402

SEED = 0xB0DA


def kbest_cases():
    for fam, (cases, _) in (("b1", bl.b1_cases(SEED, 14, rows=(2, 20), B=1)), ("b1wide", bl.b1_cases(SEED + 1, 2, rows=(65, 66), k=(3, 20), B=1)),
                            ("b2", bl.b2_cases(SEED + 2, 14, B=1)), ("b3", bl.b3_cases(SEED + 3, 16, B=1))):
        for i, c in enumerate(cases):
            yield f"{fam}_{i}", c
    # 0.1 grids where the fast kernels keep another number of solutions than the reference (a tree split in another order of
    # exact ties rounds apart at the cutoff): the default entry re-runs them on the reference-order kernel and must report the
    # re-run's nf (it reported the first pass' 45 / 20 where the reference finds 44 / 18)
    seen = bl.b3_cases(0xB1 + 20, 30)[0]
    for name, i, b in (("b3nf_0", 0, 1), ("b3nf_1", 14, 1)):
        c = dict(seen[i])
        c["C"] = c["C"][b:b + 1]
        yield name, c


def frames():
    a1, _ = bl.a1_frames(SEED + 4, 21, [(6, 3), (12, 5), (40, 2), (20, 10), (30, 16), (50, 8), (4, 4)])
    a2, _ = bl.a2_frames(SEED + 5, 10)
    for i, f in enumerate(a1):
        yield f"a1_{i}", f, 200
    for i, f in enumerate(a2):
        yield f"a2_{i}", f, 200


def main():
    out, knames, fnames = {}, [], []
    for name, c in kbest_cases():
        N, M, k, mx, cut = c["N"], c["M"], c["k"], c["maximize"], c["cutoff"]
        cost = np.ascontiguousarray(c["C"][0])
        nf, r4c, c4r, g = ol.ref_kbest(cost, N, M, k, mx, cut)
        knames.append(name)
        out[name + "/cost"] = cost
        out[name + "/meta"] = np.array([N, M, k, int(mx), nf], dtype=np.int64)
        out[name + "/cutoff"] = np.array([cut])
        out[name + "/row4col"] = r4c[:nf].astype(np.int16)
        out[name + "/col4row"] = c4r[:nf].astype(np.int16)
        out[name + "/gain"] = g[:nf]
        print(f"{name:10s} {N:3d}x{M:<3d} k={k:3d} max={int(mx)} cutoff={cut!r} nf={nf}")
    for name, f, k in frames():
        nL, nM, raw = f["nL"], f["nM"], np.ascontiguousarray(f["cost"])
        cond, ridx = ol.ref_condition_costs(raw, nL + nM, nM)
        cl = len(ridx) - nM
        brute = nM <= 5 and nL + nM <= 12
        fnames.append(name)
        out[name + "/raw"] = raw
        out[name + "/meta"] = np.array([nL, nM, k, len(ridx), int(brute)], dtype=np.int64)
        out[name + "/cond"] = cond
        out[name + "/rowIdx"] = ridx.astype(np.int16)
        out[name + "/probs"] = ol.ref_assignment_prob(cond, cl, nM, k)
        if brute:
            out[name + "/brute"] = ol.ref_brute_force_prob(cond, cl, nM)
        print(f"{name:10s} nL={nL:3d} nM={nM:3d} kept rows={len(ridx):3d} brute={int(brute)} entries of 42: {int((cond == 42.0).sum())}")
    out["kbest_names"] = np.array(knames)
    out["frame_names"] = np.array(fnames)
    path = os.path.join(HERE, "boundary_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
