"""How far the belief-propagation association probabilities (KBestEngine.belief_probs, kbest_lbp.hip) are from the truth at
production size, beside assignmentProb(k = 200) and assignmentProb(k = 1000).

The frames and the truth of tools/harness_exact_truth.py: workloads.kitti_like_frames in three shapes (6 landmarks x 3
measurements, 12 x 5, 20 x 10: the 30x10 cost blocks of benchmark configuration 5), truth = KBestEngine.permanent_probs with
condition = 1.  Per method the order statistics of the maximum absolute probability error per frame (comparison.cpp:261-275)
and the reference's acceptance counts (frames above 1e-8, frames above 0.1 where compMethods aborts, comparison.cpp:319-331);
for belief propagation also the sweeps it took (tol 1e-12).

    python tools/harness_belief_truth.py [n_frames] [out.json]        (default: 200, profiles/belief_truth_c5.json)
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

KS = (200, 1000)
SHAPES = (("6x3", 6, 3), ("12x5", 12, 5), ("30x10", 20, 10))
TOL, MAX_ITER = 1e-12, 10000


def row(err):
    q = np.quantile(err, [0.0, 0.5, 0.95, 1.0])
    return dict(min=float(q[0]), median=float(q[1]), p95=float(q[2]), max=float(q[3]),
                frames_above_1e_8=int((err > 1e-8).sum()), frames_above_0_1=int((err > 0.1).sum()))


def run(n_frames: int = 200, verbose: bool = True):
    eng = pk.KBestEngine(0)
    result = {"frames": n_frames, "generator": "workloads.kitti_like_frames (seed 0xC0FFEE)",
              "truth": "kbest_permanent_probs_batch_f64, condition = 1",
              "belief": f"kbest_belief_probs_batch_f64, condition = 1, tol {TOL:g}, at most {MAX_ITER} sweeps", "shapes": {}}
    for name, nL, nM in SHAPES:
        frames = wl.kitti_like_frames(n_frames, nL=nL, nM=nM)
        nLs, nMs = [nL] * n_frames, [nM] * n_frames
        truth, _ = eng.permanent_probs(frames, nLs, nMs, condition=True)
        probs, iters, resid = eng.belief_probs(frames, nLs, nMs, condition=True, tol=TOL, max_iter=MAX_ITER)
        err = np.array([np.abs(p - t).max() for p, t in zip(probs, truth)])
        table = {"belief": dict(row(err), sweeps_median=float(np.median(iters)), sweeps_max=int(iters.max()),
                                infeasible=int((iters < 0).sum()), worst_resid=float(resid.max()),
                                rows_sum_to_one_within=max(float(np.abs(p.sum(axis=1) - 1.0).max()) for p in probs))}
        for k in KS:
            pk_, nf = eng.weights(frames, nLs, nMs, k, condition=True)
            table[f"k{k}"] = row(np.array([np.abs(p - t).max() for p, t in zip(pk_, truth)]))
        if verbose:
            for m, t in table.items():
                print(f"{name:6s} {m:7s} max-abs-error vs exact: median {t['median']:.2e} p95 {t['p95']:.2e} worst {t['max']:.2e}  "
                      f"frames > 1e-8: {t['frames_above_1e_8']:4d}  > 0.1: {t['frames_above_0_1']:4d}")
        result["shapes"][name] = dict(nL=nL, nM=nM, methods=table)
    eng.close()
    return result


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "belief_truth_c5.json")
    res = run(n)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)
