"""How far the hybrid association probabilities (KBestEngine.hybrid_probs) are from the truth where the truth is known, beside
whole-frame assignmentProb(k) and belief propagation on the same frames.

Frames: workloads.scene_frames at (20 landmarks, 10 measurements, side 12), (40, 24, 24) and (60, 40, 30), raw blocks with
condition = 1.  Truth: KBestEngine.clustered_probs (kbest_cluster.hip), exact wherever the gate leaves clusters of at most 16
measurements; the frames it refuses are left out.  hybrid_probs runs with max_exact = 8, so that clusters of 9 .. 16 measurements
are enumerated although their truth is known; only the frames that have such an open cluster are counted.  Per method the order
statistics of the maximum absolute probability error per frame.  Also, per shape, the frames hybrid_probs(max_exact = 16) answers
and clustered_probs refuses, with their methods.

    python tools/harness_hybrid_truth.py [n_frames] [out.json]        (default: 200, profiles/hybrid_truth.json)
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
MAX_EXACT = 8
SHAPES = (("20+10_side12", 20, 10, 12), ("40+24_side24", 40, 24, 24), ("60+40_side30", 60, 40, 30))
TOL, MAX_ITER = 1e-12, 10000


def row(err):
    q = np.quantile(err, [0.0, 0.5, 0.95, 1.0])
    return dict(min=float(q[0]), median=float(q[1]), p95=float(q[2]), max=float(q[3]),
                frames_above_1e_8=int((err > 1e-8).sum()), frames_above_0_1=int((err > 0.1).sum()))


def run(n_frames: int = 200, verbose: bool = True):
    eng = pk.KBestEngine(0)
    result = {"frames": n_frames, "generator": "workloads.scene_frames (seed 0x5CE7E)", "max_exact": MAX_EXACT,
              "truth": "kbest_clustered_probs_batch_f64, condition = 1; refused frames left out",
              "counted": f"answered frames with a cluster of more than {MAX_EXACT} measurements", "shapes": {}}
    for name, nL, nM, side in SHAPES:
        frames = wl.scene_frames(n_frames, nL, nM, side)
        nLs, nMs = [nL] * n_frames, [nM] * n_frames
        truth, _, info, maxc = eng.clustered_probs(frames, nLs, nMs, condition=True)
        table = {}
        sel = np.zeros(0, np.int64)
        for k in KS:
            probs, method, nOpen, _ = eng.hybrid_probs(frames, nLs, nMs, k, condition=True, max_exact=MAX_EXACT)
            sel = np.flatnonzero((info > 0) & (nOpen > 0))
            if len(sel):
                table[f"hybrid_k{k}"] = dict(row(np.array([np.abs(probs[b] - truth[b]).max() for b in sel])),
                                             complete=int((method[sel] == 1).sum()), truncated=int((method[sel] == 2).sum()))
            closed = np.flatnonzero((info > 0) & (nOpen == 0))
            assert all(np.array_equal(probs[b], truth[b]) for b in closed)  # nothing open: the bits of clustered_probs
        if len(sel):
            for k in KS:
                try:
                    pw, _ = eng.weights(frames, nLs, nMs, k, condition=True)
                    table[f"whole_k{k}"] = row(np.array([np.abs(pw[b] - truth[b]).max() for b in sel]))
                except pk.KBestError as e:
                    table[f"whole_k{k}"] = {"not_taken": str(e)[:120]}
            bp, _, _ = eng.belief_probs(frames, nLs, nMs, condition=True, tol=TOL, max_iter=MAX_ITER)
            table["belief"] = row(np.array([np.abs(bp[b] - truth[b]).max() for b in sel]))
        _, m16, open16, _ = eng.hybrid_probs(frames, nLs, nMs, KS[0], condition=True, max_exact=16)
        refused = np.flatnonzero(info < 0)
        if verbose:
            for m, t in table.items():
                if "median" in t:
                    print(f"{name:14s} {m:12s} max-abs-error vs clustered exact: median {t['median']:.2e} p95 {t['p95']:.2e} "
                          f"worst {t['max']:.2e}  ({len(sel)} frames)")
                else:
                    print(f"{name:14s} {m:12s} does not take the frames")
            print(f"{name:14s} refused by clustered_probs: {len(refused)}; answered by hybrid_probs(max_exact 16): "
                  f"{int((m16[refused] > 0).sum())}")
        result["shapes"][name] = dict(nL=nL, nM=nM, side=side, answered_exactly=int((info > 0).sum()), counted=int(len(sel)),
                                      refused_by_clustered=int(len(refused)),
                                      of_those_answered_by_hybrid_16=int((m16[refused] > 0).sum()),
                                      of_those_open_clusters_max=int(open16[refused].max()) if len(refused) else 0,
                                      of_those_methods={str(v): int((m16[refused] == v).sum()) for v in (-2, -1, 1, 2)},
                                      largest_cluster_max=int(maxc.max()), methods=table)
    eng.close()
    return result


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "hybrid_truth.json")
    res = run(n)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)
