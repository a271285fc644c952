"""Times of the draws from the exact posterior of sparse clusters (kbest_frontier_sample.hip) beside the entries they share their
sums with, in ONE process and run, the two sides ALTERNATING launch by launch, the work space reserved beforehand: warm-up, then
the median of the timed launches of each side (min and max beside it).

    (a) the open clusters (more than 16 measurements) of 256 scene_frames(., 60, 40, 30.0), one call: kbest_frontier_sample_f64_dev at
        nSample = 1, 64, 1 024 beside kbest_frontier_probs_f64_dev on the same sub-blocks -- HIP events on the caller's stream
    (b) those 256 frames through hybrid_frontier_sample_assoc(nSample = 64) beside hybrid_frontier_probs(k = 0, max_big = 0) --
        synchronous host entries: time.perf_counter around the call
    (c) 1 000 scene_frames(., 20, 10, 12.0), nothing open: hybrid_frontier_sample_assoc(nSample = 64) beside clustered_sample_assoc --
        likewise

Raw frames, condition = 1.  The row keys of (a) are the rows' own indices in their sub-blocks.  No target: the numbers are a record.

    python tools/bench_frontier_sample.py [--steps 30] [--warmup 5] [--out profiles/frontier_sample_bench.json]

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontier_sample_bench.json"))
    args = ap.parse_args()
    import torch  # torch first: its copy of the HIP runtime is the one the process loads (tests/conftest.py)
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    import probabilisticsemslam_amd as pk
    from probabilisticsemslam_amd import workloads as wl
    eng = pk.KBestEngine(0)
    stream = torch.cuda.Stream(device=dev)

    def alternate(calls, clock):
        """One list of times (ms) per call, the calls alternating.  clock 'events': the calls enqueue on `stream`."""
        for _ in range(args.warmup):
            for call in calls:
                call()
        stream.synchronize()
        ms = [[] for _ in calls]
        for _ in range(args.steps):
            for j, call in enumerate(calls):
                if clock == "events":
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record(stream)
                    call()
                    t1.record(stream)
                    stream.synchronize()
                    ms[j].append(t0.elapsed_time(t1))
                else:
                    t0 = time.perf_counter()
                    call()
                    ms[j].append((time.perf_counter() - t0) * 1e3)
        return [stats(m) for m in ms]

    res = {"tool": "tools/bench_frontier_sample.py", "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
           "clock_a": "HIP events on the caller's stream around the device entry",
           "clock_b_c": "time.perf_counter around the synchronous host entry", "cases": {}}
    mid = wl.scene_frames(256, 60, 40, 30.0)
    d_sub, opens = open_clusters(eng, torch, mid, 60, 40)
    n = len(opens)
    at = np.array([o[0] for o in opens], np.int64)
    m = np.array([o[1] for o in opens], np.int32)
    cL = np.array([o[2] for o in opens], np.int32)
    poff = np.concatenate([[0], np.cumsum(m.astype(np.int64) * (cL + 1))])
    koff = np.concatenate([[0], np.cumsum((m + cL).astype(np.int64))])
    d_keys = torch.from_numpy(np.concatenate([np.arange(r, dtype=np.int32) for r in (m + cL)])).to(dev)
    d_probs = torch.zeros(int(poff[-1]), dtype=torch.float64, device=dev)
    d_out = [torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros((2, n), dtype=torch.int32, device=dev)]
    d_out2 = [torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros((2, n), dtype=torch.int32, device=dev)]
    eng.reserve_frontier_sample(n, int(m.max()), int((m + cL).max()))
    res["a_open_clusters"] = {"clusters": n, "m": m.tolist()}
    probs = lambda: eng.frontier_probs_dev(m, cL, at, poff[:-1], d_sub, d_probs, d_out2[0], d_out2[1][0], d_out2[1][1],  # noqa: E731
                                           stream=stream.cuda_stream, reserve=False)
    for ns in (1, 64, 1024):
        aoff = np.concatenate([[0], np.cumsum(m.astype(np.int64) * ns)])
        d_asg = torch.zeros(int(aoff[-1]), dtype=torch.int32, device=dev)
        d_lt = torch.zeros(n * ns, dtype=torch.float64, device=dev)
        draw = lambda: eng.frontier_sample_dev(m, cL, at, d_sub, d_keys, koff[:-1], ns, d_asg, aoff[:-1], d_lt,  # noqa: E731
                                               np.arange(n, dtype=np.int64) * ns, d_out[0], d_out[1][0], d_out[1][1], seed=2024,
                                               stream=stream.cuda_stream, reserve=False)
        ts, tp = alternate([draw, probs], "events")
        assert np.array_equal(d_out[0].cpu().numpy().view(np.int64), d_out2[0].cpu().numpy().view(np.int64)), "log Z differs"
        assert np.array_equal(d_out[1].cpu().numpy(), d_out2[1].cpu().numpy()), "info / width differ"
        res["cases"][f"a_{n}_clusters_n{ns}"] = {"frontier_sample": ts, "frontier_probs": tp,
                                                 "ratio_sample_to_probs": ts["median_ms"] / tp["median_ms"]}
    F = len(mid)
    ts, tp = alternate([lambda: eng.hybrid_frontier_sample_assoc(mid, [60] * F, [40] * F, 64, seed=2024, condition=True),
                        lambda: eng.hybrid_frontier_probs(mid, [60] * F, [40] * F, 0, condition=True, max_big=0)], "host")
    method = eng.hybrid_frontier_sample_assoc(mid, [60] * F, [40] * F, 64, seed=2024, condition=True)[3]
    res["cases"]["b_256x60+40_n64"] = {"hybrid_frontier_sample_assoc": ts, "hybrid_frontier_probs": tp,
                                       "ratio_sample_to_probs": ts["median_ms"] / tp["median_ms"],
                                       "methods": {str(v): int((method == v).sum()) for v in (-2, -1, 0)}}
    small = wl.scene_frames(1000, 20, 10, 12.0)
    F = len(small)
    ts, tc = alternate([lambda: eng.hybrid_frontier_sample_assoc(small, [20] * F, [10] * F, 64, seed=2024, condition=True),
                        lambda: eng.clustered_sample_assoc(small, [20] * F, [10] * F, 64, seed=2024, condition=True)], "host")
    res["cases"]["c_1000x20+10_n64"] = {"hybrid_frontier_sample_assoc": ts, "clustered_sample_assoc": tc,
                                        "ratio_hybrid_to_clustered": ts["median_ms"] / tc["median_ms"]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
