"""Host-clock times of the hybrid association probabilities (KBestEngine.hybrid_probs, k = 200: synchronous, host buffers) beside
the entry it replaces, both sides in ONE process, alternating, warmed up; raw blocks with condition = 1.

    (d) 256 scene frames (60, 40, 30)      against exact_or_belief_probs (tol 1e-12): clustered, then belief on the refused frames
    (e) 64 scene frames (200, 128, 60)     against exact_or_belief_probs
    (b) 1 000 scene frames (20, 10, 12)    against clustered_probs: nothing is open, the difference is the price of the mode

Both sides stage the same host buffers through the same kind of synchronous call, so a wall clock around the call compares them.

    python tools/bench_hybrid.py [--steps 30] [--warmup 5] [--k 200] [--out profiles/hybrid_bench.json]

Prints one JSON line and writes it to --out.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--k", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hybrid_bench.json"))
    args = ap.parse_args()
    import torch  # torch first: its copy of the HIP runtime is the one the process loads (tests/conftest.py)
    torch.zeros(1, device=torch.device("cuda", 0))
    import probabilisticsemslam_amd as pk
    from probabilisticsemslam_amd import workloads as wl
    eng = pk.KBestEngine(0)
    TOL = 1e-12

    def timed_pair(one, two):
        for _ in range(args.warmup):
            one()
            two()
        ms = [[], []]
        for _ in range(args.steps):
            for j, call in enumerate((one, two)):
                t0 = time.perf_counter()
                call()
                ms[j].append((time.perf_counter() - t0) * 1e3)
        return [dict(median_ms=float(np.median(m)), min_ms=float(min(m)), max_ms=float(max(m)), calls=len(m)) for m in ms]

    res = {"tool": "tools/bench_hybrid.py", "device": torch.cuda.get_device_name(0), "clock": "time.perf_counter around the call",
           "k": args.k, "tol": TOL, "steps": args.steps, "warmup": args.warmup, "cases": {}}
    cases = (("d_256_scene_60+40", wl.scene_frames(256, 60, 40, 30), 60, 40, "exact_or_belief_probs"),
             ("e_64_scene_200+128", wl.scene_frames(64, 200, 128, 60), 200, 128, "exact_or_belief_probs"),
             ("b_1000_scene_20+10", wl.scene_frames(1000, 20, 10, 12), 20, 10, "clustered_probs"))
    for name, frames, nL, nM, other in cases:
        F = len(frames)
        nLs, nMs = [nL] * F, [nM] * F
        hybrid = lambda: eng.hybrid_probs(frames, nLs, nMs, args.k, condition=True)  # noqa: E731
        if other == "clustered_probs":
            base = lambda: eng.clustered_probs(frames, nLs, nMs, condition=True)  # noqa: E731
        else:
            base = lambda: eng.exact_or_belief_probs(frames, nLs, nMs, condition=True, tol=TOL)  # noqa: E731
        th, tb = timed_pair(hybrid, base)
        _, method, nOpen, _ = hybrid()
        res["cases"][name] = {"frames": F, "hybrid_probs": th, other: tb, "ratio_hybrid_to_" + other: th["median_ms"] / tb["median_ms"],
                              "frames_with_open_clusters": int((nOpen > 0).sum()), "open_clusters": int(nOpen.sum()),
                              "methods": {str(v): int((method == v).sum()) for v in (-2, -1, 0, 1, 2)}}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
