"""Times of the frontier tier (kbest_frontier.hip) beside the tiers it stands next to, both sides in ONE process, alternating,
warmed up, the median of --steps runs; raw blocks with condition = 1.

    tier       by HIP events around the device entries, on the same sub-blocks (the clusters of 17 .. 20 measurements of 256 scene
               frames (60, 40, 30) and of 64 scene frames (200, 128, 60), handed out by the partial clustered kernel):
               kbest_frontier_probs_f64_dev beside kbest_bigcluster_probs_f64_dev, one cluster a call and all of them as a pack;
               and the frontier tier alone on the clusters of more than 20 measurements, which no other tier answers
    frames     by the host clock around the synchronous host entries: hybrid_frontier_probs beside hybrid_exact_probs, k = 200, on
               the same two batches

No time is promised.  The expectation is the state counts (sum_i 2^|Psi_i| beside R 2^m, written beside every time) and that the tier
is latency-bound: about 4 R workgroup barriers a cluster.

    python tools/bench_frontier.py [--steps 30] [--warmup 5] [--k 200] [--out profiles/frontier_bench.json]

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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_bigcluster import open_clusters  # noqa: E402


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)), calls=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--k", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontier_bench.json"))
    args = ap.parse_args()
    import torch  # torch first: its copy of the HIP runtime is the one the process loads (tests/conftest.py)
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    import probabilisticsemslam_amd as pk
    from probabilisticsemslam_amd import workloads as wl
    eng = pk.KBestEngine(0)
    stream = torch.cuda.Stream(device=dev)

    def event_pair(calls):
        """calls: functions that enqueue on `stream`.  Alternating; one list of event times (ms) per function."""
        for _ in range(args.warmup):
            for call in calls:
                call()
        stream.synchronize()
        ms = [[] for _ in calls]
        for _ in range(args.steps):
            for j, call in enumerate(calls):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                call()
                t1.record(stream)
                stream.synchronize()
                ms[j].append(t0.elapsed_time(t1))
        return [stats(m) for m in ms]

    res = {"tool": "tools/bench_frontier.py", "device": torch.cuda.get_device_name(0), "k": args.k, "steps": args.steps,
           "warmup": args.warmup, "clock_tier": "HIP events on the caller's stream around the device entry",
           "clock_frames": "time.perf_counter around the synchronous host entry", "tier": {}, "frames": {}}
    cases = (("d_256_scene_60+40", wl.scene_frames(256, 60, 40, 30), 60, 40), ("e_64_scene_200+128", wl.scene_frames(64, 200, 128, 60), 200, 128))
    for name, frames, nL, nM in cases:
        d_sub, opens = open_clusters(eng, torch, frames, nL, nM)
        n = len(opens)
        at = np.array([o[0] for o in opens], np.int64)
        m = np.array([o[1] for o in opens], np.int32)
        cL = np.array([o[2] for o in opens], np.int32)
        poff = np.concatenate([[0], np.cumsum(m.astype(np.int64) * (cL + 1))])
        d_probs = torch.zeros(int(poff[-1]), dtype=torch.float64, device=dev)
        d_big = torch.zeros(int(poff[-1]), dtype=torch.float64, device=dev)
        d_logZ = torch.zeros(n, dtype=torch.float64, device=dev)
        d_info = torch.zeros(n, dtype=torch.int32, device=dev)
        d_width = torch.zeros(n, dtype=torch.int32, device=dev)
        eng.reserve_frontier(n, int(m.max()), int((m + cL).max()))
        both = np.flatnonzero(m <= 20)
        eng.reserve_bigcluster(int(m[both].max()), int((m + cL)[both].max()))

        def frontier(sel):
            return lambda: eng.frontier_probs_dev(m[sel], cL[sel], at[sel], poff[:-1][sel], d_sub, d_probs, d_logZ, d_info, d_width,
                                                  stream=stream.cuda_stream, reserve=False)

        def big(sel):
            return lambda: eng.bigcluster_probs_dev(m[sel], cL[sel], at[sel], poff[:-1][sel], d_sub, d_big, d_logZ, d_info,
                                                    stream=stream.cuda_stream, reserve=False)

        frontier(np.arange(n))()
        stream.synchronize()
        width, info = d_width.cpu().numpy(), d_info.cpu().numpy()
        per = []
        for j in range(n):
            sel = np.array([j])
            row = {"m": int(m[j]), "R": int(opens[j][3]), "W": int(width[j]), "info": int(info[j]), "full_sweep_states": int(opens[j][3]) << int(m[j])}
            if m[j] <= 20:
                tf, tb = event_pair([frontier(sel), big(sel)])
                row.update(frontier=tf, bigcluster=tb, ratio_big_to_frontier=tb["median_ms"] / tf["median_ms"])
            else:
                (tf,) = event_pair([frontier(sel)])
                row.update(frontier=tf)
            per.append(row)
        tf, tb = event_pair([frontier(both), big(both)])
        (ta,) = event_pair([frontier(np.arange(n))])
        big(both)()
        frontier(both)()
        stream.synchronize()
        worst = max(float((d_probs[int(poff[j]):int(poff[j + 1])] - d_big[int(poff[j]):int(poff[j + 1])]).abs().max()) for j in both)
        res["tier"][name] = {"open_clusters": n, "of_at_most_20": int(len(both)), "per_cluster": per,
                             "pack_of_at_most_20": {"frontier": tf, "bigcluster": tb, "ratio_big_to_frontier": tb["median_ms"] / tf["median_ms"],
                                                    "max_abs_difference": worst},
                             "pack_of_all_frontier": ta}
    for name, frames, nL, nM in cases:
        F = len(frames)
        nLs, nMs = [nL] * F, [nM] * F
        calls = (lambda: eng.hybrid_frontier_probs(frames, nLs, nMs, args.k, condition=True),
                 lambda: eng.hybrid_exact_probs(frames, nLs, nMs, args.k, condition=True))
        for _ in range(args.warmup):
            for call in calls:
                call()
        ms = [[], []]
        for _ in range(args.steps):
            for j, call in enumerate(calls):
                t0 = time.perf_counter()
                call()
                ms[j].append((time.perf_counter() - t0) * 1e3)
        _, method, nOpen, nBig, _, _, nFr = calls[0]()
        _, emethod, _, eBig, _, _ = calls[1]()
        tf, te = stats(ms[0]), stats(ms[1])
        res["frames"][name] = {"frames": F, "hybrid_frontier_probs": tf, "hybrid_exact_probs": te,
                               "ratio_exact_to_frontier": te["median_ms"] / tf["median_ms"], "open_clusters": int(nOpen.sum()),
                               "answered_by_the_frontier_tier": int(nFr.sum()), "answered_by_the_big_tier": int(nBig.sum()),
                               "big_tier_in_hybrid_exact_probs": int(eBig.sum()),
                               "methods_frontier": {str(v): int((method == v).sum()) for v in (-2, -1, 0, 1, 2)},
                               "methods_exact": {str(v): int((emethod == v).sum()) for v in (-2, -1, 0, 1, 2)}}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
