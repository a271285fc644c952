"""How far the approximate association probabilities are from the truth on the frames whose largest gated cluster has MORE than 20
measurements -- the frames that had no truth before the frontier tier (KBestEngine.hybrid_frontier_probs, kbest_frontier.hip).

Frames: workloads.scene_frames at (40 landmarks, 24 measurements, side 24), (60, 40, 30) -- n_frames each -- and (200, 128, 60) --
min(n_frames, 64) --, raw blocks with condition = 1.  Truth: hybrid_frontier_probs(k = 0), method 0.  Against it, per frame the
maximum absolute probability error of hybrid_probs and of hybrid_exact_probs (k = 200 and 1 000: the oversized cluster enumerated)
and of belief_probs; the widths of the clusters the tier answered; and how many frames of each family every entry answers exactly.

    python tools/harness_frontier_truth.py [n_frames] [out.json]        (default: 200, profiles/frontier_truth.json)
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
SHAPES = (("40+24_side24", 40, 24, 24, 1 << 30), ("60+40_side30", 60, 40, 30, 1 << 30), ("200+128_side60", 200, 128, 60, 64))
TOL, MAX_ITER = 1e-12, 10000


def row(err):
    q = np.quantile(err, [0.0, 0.5, 0.95, 1.0])
    return dict(min=float(q[0]), median=float(q[1]), p95=float(q[2]), max=float(q[3]), frames=int(len(err)),
                per_frame=[float(e) for e in err])


def run(n_frames: int = 200, verbose: bool = True):
    eng = pk.KBestEngine(0)
    result = {"frames": n_frames, "generator": "workloads.scene_frames (seed 0x5CE7E)",
              "truth": "kbest_hybrid_frontier_probs_batch_f64, k = 0, condition = 1, max_exact 16, max_big 20, max_width 16: method 0",
              "counted": "frames whose largest cluster has more than 20 measurements", "shapes": {}}
    for name, nL, nM, side, most in SHAPES:
        F = min(n_frames, most)
        frames = wl.scene_frames(F, nL, nM, side)
        nLs, nMs = [nL] * F, [nM] * F
        truth, method, nOpen, nBig, maxc, _, nFr = eng.hybrid_frontier_probs(frames, nLs, nMs, 0, condition=True)
        _, emethod, _, _, _, _ = eng.hybrid_exact_probs(frames, nLs, nMs, 0, condition=True)
        _, _, info, _ = eng.clustered_probs(frames, nLs, nMs, condition=True)
        sel = np.flatnonzero((maxc > 20) & (method == 0))
        table = {}
        if len(sel):
            sub = [frames[b] for b in sel]
            sL, sM = [nL] * len(sel), [nM] * len(sel)
            for k in KS:
                probs, hm, _, _ = eng.hybrid_probs(sub, sL, sM, k, condition=True)
                table[f"hybrid_k{k}"] = dict(row(np.array([np.abs(probs[j] - truth[b]).max() for j, b in enumerate(sel)])),
                                             complete=int((hm == 1).sum()), truncated=int((hm == 2).sum()))
                probs, hm, _, _, _, _ = eng.hybrid_exact_probs(sub, sL, sM, k, condition=True)
                table[f"hybrid_exact_k{k}"] = dict(row(np.array([np.abs(probs[j] - truth[b]).max() for j, b in enumerate(sel)])),
                                                   complete=int((hm == 1).sum()), truncated=int((hm == 2).sum()))
            bp, _, _ = eng.belief_probs(sub, sL, sM, condition=True, tol=TOL, max_iter=MAX_ITER)
            table["belief"] = row(np.array([np.abs(bp[j] - truth[b]).max() for j, b in enumerate(sel)]))
        if verbose:
            for m, t in table.items():
                print(f"{name:15s} {m:16s} max-abs-error vs the exact answer: median {t['median']:.2e} p95 {t['p95']:.2e} "
                      f"worst {t['max']:.2e}  ({len(sel)} frames)")
            print(f"{name:15s} exact: clustered_probs {int((info > 0).sum())}, hybrid_exact_probs {int((emethod == 0).sum())}, "
                  f"hybrid_frontier_probs {int((method == 0).sum())} of {F}")
        result["shapes"][name] = dict(nL=nL, nM=nM, side=side, frames=F, counted=[int(b) for b in sel],
                                      largest_cluster=[int(maxc[b]) for b in sel],
                                      answered_exactly=dict(clustered_probs=int((info > 0).sum()),
                                                            hybrid_exact_probs=int((emethod == 0).sum()),
                                                            hybrid_frontier_probs=int((method == 0).sum())),
                                      refused_by_hybrid_frontier_k0=int((method == -1).sum()),
                                      clusters_by_the_frontier_tier=int(nFr.sum()), clusters_by_the_big_tier=int(nBig.sum()),
                                      largest_cluster_max=int(maxc.max()), methods=table)
    eng.close()
    return result


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "frontier_truth.json")
    res = run(n)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)
