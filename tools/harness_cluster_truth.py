"""How far the belief-propagation association probabilities (KBestEngine.belief_probs, tol 1e-12) and assignmentProb(k = 200),
assignmentProb(k = 1000) are from the truth on frames with geometry, beyond the 16 measurements the whole-frame exact entry takes.

Frames: workloads.scene_frames at (20 landmarks, 10 measurements, side 12), (40, 24, 24) and (60, 40, 30), raw blocks with
condition = 1.  Truth: KBestEngine.clustered_probs (kbest_cluster.hip), exact wherever the gate leaves clusters of at most 16
measurements; refused frames are counted and left out.  assignmentProb only where it takes the frame (at most 32 measurements).
Per method the order statistics of the maximum absolute probability error per frame and the frames above 1e-8 and above 0.1.

    python tools/harness_cluster_truth.py [n_frames] [out.json]        (default: 200, profiles/cluster_truth.json)
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
SHAPES = (("20+10_side12", 20, 10, 12), ("40+24_side24", 40, 24, 24), ("60+40_side30", 60, 40, 30))
TOL, MAX_ITER = 1e-12, 10000


def row(err):
    q = np.quantile(err, [0.0, 0.5, 0.95, 1.0])
    return dict(min=float(q[0]), median=float(q[1]), p95=float(q[2]), max=float(q[3]),
                frames_above_1e_8=int((err > 1e-8).sum()), frames_above_0_1=int((err > 0.1).sum()))


def run(n_frames: int = 200, verbose: bool = True):
    eng = pk.KBestEngine(0)
    result = {"frames": n_frames, "generator": "workloads.scene_frames (seed 0x5CE7E)",
              "truth": "kbest_clustered_probs_batch_f64, condition = 1; refused frames left out",
              "belief": f"kbest_belief_probs_batch_f64, condition = 1, tol {TOL:g}, at most {MAX_ITER} sweeps", "shapes": {}}
    for name, nL, nM, side in SHAPES:
        frames = wl.scene_frames(n_frames, nL, nM, side)
        nLs, nMs = [nL] * n_frames, [nM] * n_frames
        truth, _, info, maxc = eng.clustered_probs(frames, nLs, nMs, condition=True)
        ok = np.flatnonzero(info > 0)
        probs, iters, resid = eng.belief_probs(frames, nLs, nMs, condition=True, tol=TOL, max_iter=MAX_ITER)
        err = np.array([np.abs(probs[b] - truth[b]).max() for b in ok])
        table = {"belief": dict(row(err), sweeps_median=float(np.median(iters[ok])), sweeps_max=int(iters[ok].max()),
                                not_converged=int((resid[ok] > TOL).sum()))}
        for k in KS:
            try:
                pk_, nf = eng.weights(frames, nLs, nMs, k, condition=True)
                table[f"k{k}"] = row(np.array([np.abs(pk_[b] - truth[b]).max() for b in ok]))
            except pk.KBestError as e:
                table[f"k{k}"] = {"not_taken": str(e)[:120]}
        if verbose:
            for m, t in table.items():
                if "median" in t:
                    print(f"{name:14s} {m:7s} max-abs-error vs clustered exact: median {t['median']:.2e} p95 {t['p95']:.2e} "
                          f"worst {t['max']:.2e}  frames > 0.1: {t['frames_above_0_1']:4d} of {len(ok)}")
                else:
                    print(f"{name:14s} {m:7s} does not take the frames")
        result["shapes"][name] = dict(nL=nL, nM=nM, side=side, answered=int(len(ok)), refused=int((info < 0).sum()),
                                      infeasible=int((info == 0).sum()), clusters_median=float(np.median(info[ok])),
                                      largest_cluster_median=float(np.median(maxc)), largest_cluster_max=int(maxc.max()),
                                      rows_sum_to_one_within=max(float(np.abs(truth[b].sum(axis=1) - 1.0).max()) for b in ok),
                                      methods=table)
    eng.close()
    return result


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "cluster_truth.json")
    res = run(n)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)
