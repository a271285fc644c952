"""Times of the draws for every gated frame (kbest_hybrid_sample_assoc_batch_f64: the k-best leg and kbest_table_sample.hip) in ONE
process and run, the sides of a comparison ALTERNATING call by call: warm-up, then the median of the timed calls of each side (min
and max beside it).  Synchronous host entries: time.perf_counter around the call.

    (a) 1 000 scene_frames(., 20, 10, 12.0), nothing enumerated: hybrid_sample_assoc(k = 200, nSample = 64) beside
        hybrid_frontier_sample_assoc(nSample = 64) -- what the mode costs where it has nothing to do
    (b) 256 scene_frames(., 60, 40, 30.0) at max_width = 5 (the frontier tier leaves clusters to the enumeration), k = 200:
        hybrid_sample_assoc at nSample = 16 and 1 024, alternating with each other -- absolute times and the enumerated clusters;
        there is no counterpart

Raw frames, condition = 1.  No target: the numbers are a record.

    python tools/bench_hybrid_sample.py [--steps 30] [--warmup 5] [--out profiles/hybrid_sample_bench.json]

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


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)), calls=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hybrid_sample_bench.json"))
    args = ap.parse_args()
    import torch  # torch first: its copy of the HIP runtime is the one the process loads (tests/conftest.py)
    torch.zeros(1, device=torch.device("cuda", 0))
    import probabilisticsemslam_amd as pk
    from probabilisticsemslam_amd import workloads as wl
    eng = pk.KBestEngine(0)

    def alternate(calls):
        for _ in range(args.warmup):
            for call in calls:
                call()
        ms = [[] for _ in calls]
        for _ in range(args.steps):
            for j, call in enumerate(calls):
                t0 = time.perf_counter()
                call()
                ms[j].append((time.perf_counter() - t0) * 1e3)
        return [stats(m) for m in ms]

    K = 200
    res = {"tool": "tools/bench_hybrid_sample.py", "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
           "clock": "time.perf_counter around the synchronous host entry", "k": K, "cases": {}}
    small = wl.scene_frames(1000, 20, 10, 12.0)
    F = len(small)
    new = lambda: eng.hybrid_sample_assoc(small, [20] * F, [10] * F, 64, K, seed=2024, condition=True)  # noqa: E731
    old = lambda: eng.hybrid_frontier_sample_assoc(small, [20] * F, [10] * F, 64, seed=2024, condition=True)  # noqa: E731
    a, b = new(), old()
    assert not a[6].any() and np.array_equal(a[3], b[3]) and all(np.array_equal(x, y) for x, y in zip(a[0], b[0])), "the draws differ"
    tn, to = alternate([new, old])
    res["cases"]["a_1000x20+10_n64"] = {"hybrid_sample_assoc_k200": tn, "hybrid_frontier_sample_assoc": to,
                                        "ratio_new_to_existing": tn["median_ms"] / to["median_ms"], "enumerated": 0}
    mid = wl.scene_frames(256, 60, 40, 30.0)
    F = len(mid)
    draw = lambda ns: eng.hybrid_sample_assoc(mid, [60] * F, [40] * F, ns, K, seed=2024, condition=True, max_width=5)  # noqa: E731
    out = draw(16)
    t16, t1024 = alternate([lambda: draw(16), lambda: draw(1024)])
    res["cases"]["b_256x60+40_width5"] = {"n16": t16, "n1024": t1024, "enumerated_clusters": int(out[6].sum()),
                                          "frames_with_enumeration": int((out[6] > 0).sum()),
                                          "methods": {str(v): int((out[3] == v).sum()) for v in (-2, -1, 0, 1, 2)}}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
