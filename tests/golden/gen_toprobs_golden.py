"""Generate tests/golden/toprobs_golden.npz from the reference's OWN toProbs.

Run in the build container only (needs the reference's sources for oracle/_ref):

    make -C oracle && python tests/golden/gen_toprobs_golden.py

A sibling of gen_weights_golden.py: that one records toProbs on the conditioned frames only; these are synthetic vectors
at the sizes and values where a 256-wide reduction with a stride loop can go wrong (assignment.cpp:527-542 through
oracle/_ref/libref_assign.so: verbatim slices, see oracle/ref_assign_shim.cpp).  Data only:
    names, off (case i owns x[off[i]:off[i+1]] and want[off[i]:off[i+1]]), x (inputs), want (what toProbs left in place)
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import oracle_lib as ol  # noqa: E402
from npz_fixed import savez_compressed_fixed  # noqa: E402

INF, NAN = float("inf"), float("nan")


def vectors():
    rng = np.random.default_rng(0x70B0B5)
    draw = lambda n: rng.uniform(3.0, 70.0, size=n)  # noqa: E731  (a spread wider than the gate of 42: some entries go to 0)
    for n in (1, 255, 256, 257, 1000):
        yield f"n{n}", draw(n)
    x = draw(300); x[-1] = 1.25
    yield "min_last", x
    x = draw(700); x[[5, 261, 699]] = 2.0
    yield "min_repeated", x
    x = draw(300); x[:] += 10.0; x[77] = 1.5; x[3] = 43.5; x[290] = np.nextafter(43.5, 0.0); x[291] = np.nextafter(43.5, 100.0)
    yield "exactly_at_gate", x                      # 1.5 + 42 is exact: x[3] is not below the gate, x[290] just is
    yield "all_inf", np.full(10, INF)
    x = draw(20); x[7] = -INF
    yield "one_neg_inf", x
    x = draw(40); x[[0, 9]] = INF
    yield "some_inf", x
    x = draw(300); x[0] = NAN
    yield "nan_first", x                            # std::min_element keeps a NaN first element: every output 0
    x = draw(2); x[0] = NAN
    yield "nan_first_n2", x
    x = draw(300); x[[130, 257]] = NAN
    yield "nan_interior", x
    x = draw(300); x[299] = NAN
    yield "nan_last", x


def main():
    lib = ol.ref_assign()
    names, xs, wants = [], [], []
    for name, x in vectors():
        x = np.ascontiguousarray(x, dtype=np.float64)
        w = x.copy()
        lib.ref_to_probs(w, w.size)
        names.append(name); xs.append(x); wants.append(w)
        print(f"{name:18s} n={x.size:5d} zeros={int((w == 0).sum()):5d} nan={int(np.isnan(w).sum())}")
    off = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    path = os.path.join(HERE, "toprobs_golden.npz")
    savez_compressed_fixed(path, names=np.array(names), off=off, x=np.concatenate(xs), want=np.concatenate(wants))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
