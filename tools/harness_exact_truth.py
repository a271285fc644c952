"""compMethods (comparison.cpp:62-341) with the EXACT column: how far assignmentProb(k) is from the truth at production size.

Frames from the synthetic KITTI-like generator (workloads.kitti_like_frames) in three shapes -- 6 landmarks x 3 measurements,
12 x 5, and benchmark configuration 5 (20 x 10: 30x10 cost blocks).  Truth = the exact association probabilities
(KBestEngine.permanent_probs: conditionCosts -> permanentProb -> scatter back), which no enumeration can give beyond a few
million assignments.  assignmentProb for k in {1, 20, 100, 200, 1000}, all frames of one k in ONE batched call; per k the order
statistics of the maximum absolute probability error per frame (comparison.cpp:261-275) and the reference's acceptance counts
(frames above 1e-8, frames above 0.1 where compMethods aborts, comparison.cpp:319-331).

    python tools/harness_exact_truth.py [n_frames] [out.json]        (default: 200, profiles/exact_truth_c5.json)
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import probabilisticsemslam_amd as pk  # noqa: E402
from probabilisticsemslam_amd import workloads as wl  # noqa: E402

KS = (1, 20, 100, 200, 1000)
SHAPES = (("6x3", 6, 3), ("12x5", 12, 5), ("30x10", 20, 10))  # (name, landmarks, measurements); 30x10 is the cost block of C5


def run(n_frames: int = 200, verbose: bool = True):
    eng = pk.KBestEngine(0)
    result = {"frames": n_frames, "ks": list(KS), "generator": "workloads.kitti_like_frames (seed 0xC0FFEE)",
              "truth": "kbest_permanent_probs_batch_f64, condition = 1", "shapes": {}}
    for name, nL, nM in SHAPES:
        frames = wl.kitti_like_frames(n_frames, nL=nL, nM=nM)
        nLs, nMs = [nL] * n_frames, [nM] * n_frames
        truth, perm = eng.permanent_probs(frames, nLs, nMs, condition=True)
        rows = max(float(np.abs(t.sum(axis=1) - 1.0).max()) for t in truth)
        table = {}
        for k in KS:
            probs, nf = eng.weights(frames, nLs, nMs, k, condition=True)
            err = np.array([np.abs(p - t).max() for p, t in zip(probs, truth)])
            q = np.quantile(err, [0.0, 0.5, 0.95, 1.0])
            table[str(k)] = dict(min=float(q[0]), median=float(q[1]), p95=float(q[2]), max=float(q[3]),
                                 frames_above_1e_8=int((err > 1e-8).sum()), frames_above_0_1=int((err > 0.1).sum()),
                                 solutions_found_median=float(np.median(nf)))
            if verbose:
                print(f"{name:6s} k={k:5d}  max-abs-error vs exact: median {q[1]:.2e} p95 {q[2]:.2e} worst {q[3]:.2e}  "
                      f"frames > 1e-8: {(err > 1e-8).sum():4d}  > 0.1: {(err > 0.1).sum():4d}")
        result["shapes"][name] = dict(nL=nL, nM=nM, truth_rows_sum_to_one_within=rows, min_permanent=float(np.min(perm)), k=table)
    eng.close()
    return result


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "exact_truth_c5.json")
    res = run(n)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)
