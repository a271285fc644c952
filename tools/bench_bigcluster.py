"""Host-clock times of KBestEngine.hybrid_exact_probs (k = 200: exact up to clusters of 20 measurements, k-best beyond) beside
hybrid_probs (k = 200: exact up to 16), both sides in ONE process, alternating, warmed up; raw blocks with condition = 1.

    (d) 256 scene frames (60, 40, 30)
    (e) 64 scene frames (200, 128, 60)
    (f) frame 5 of (e) alone: one cluster of 20 measurements and 46 rows

and the big-cluster tier's own time per cluster by HIP events around kbest_bigcluster_probs_f64_dev, one cluster a call, against
(m_k, R_k): the clusters of 17 .. 20 measurements of (d) and (e), handed out by the partial clustered kernel.  No time is promised:
exactness costs what it costs; the ratios are written down.

    python tools/bench_bigcluster.py [--steps 30] [--warmup 5] [--k 200] [--out profiles/bigcluster_bench.json]

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


def open_clusters(eng, torch, frames, nL, nM):
    """The open clusters (more than 16 measurements) of the frames, by the partial kernel: (d_sub, [(subOff, m, nLk, R)])."""
    dev = torch.device("cuda", 0)
    B, size = len(frames), (nL + nM) * nM
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_cost = t(np.concatenate(frames))
    d_coff, d_poff = t(np.arange(B, dtype=np.int64) * size), t(np.arange(B, dtype=np.int64) * (nM * (nL + 1)))
    d_nL, d_nM = t(np.full(B, nL, np.int32)), t(np.full(B, nM, np.int32))
    d_probs = torch.zeros(B * nM * (nL + 1), dtype=torch.float64, device=dev)
    d_sub = torch.zeros(B * size, dtype=torch.float64, device=dev)
    d_nopen = torch.zeros(B, dtype=torch.int32, device=dev)
    d_desc = torch.zeros((B, nM, 4), dtype=torch.int32, device=dev)
    d_rows = torch.zeros((B, nL + nM), dtype=torch.int32, device=dev)
    eng.clustered_partial_dev(B, nL + nM, nM, d_nL, d_nM, d_cost, d_coff, d_probs, d_poff, d_nopen, d_desc, nM, d_rows, nL + nM, d_sub,
                              condition=True)
    torch.cuda.synchronize()
    nopen, desc = d_nopen.cpu().numpy(), d_desc.cpu().numpy()
    out = []
    for b in range(B):
        at = b * size
        for j in range(nopen[b]):
            _, m, cL, R = desc[b, j].tolist()
            out.append((at, m, cL, R))
            at += (cL + m) * m
    return d_sub, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--k", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bigcluster_bench.json"))
    args = ap.parse_args()
    import torch  # torch first: its copy of the HIP runtime is the one the process loads (tests/conftest.py)
    torch.zeros(1, device=torch.device("cuda", 0))
    import probabilisticsemslam_amd as pk
    from probabilisticsemslam_amd import workloads as wl
    eng = pk.KBestEngine(0)

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

    res = {"tool": "tools/bench_bigcluster.py", "device": torch.cuda.get_device_name(0), "clock": "time.perf_counter around the call",
           "k": args.k, "steps": args.steps, "warmup": args.warmup, "cases": {}, "tier_per_cluster": []}
    mid, wide = wl.scene_frames(256, 60, 40, 30), wl.scene_frames(64, 200, 128, 60)
    cases = (("d_256_scene_60+40", mid, 60, 40), ("e_64_scene_200+128", wide, 200, 128), ("f_one_cluster_of_20", [wide[5]], 200, 128))
    for name, frames, nL, nM in cases:
        F = len(frames)
        nLs, nMs = [nL] * F, [nM] * F
        exact = lambda: eng.hybrid_exact_probs(frames, nLs, nMs, args.k, condition=True)  # noqa: E731
        base = lambda: eng.hybrid_probs(frames, nLs, nMs, args.k, condition=True)  # noqa: E731
        te, tb = timed_pair(exact, base)
        _, method, nOpen, nBig, maxc, _ = exact()
        _, hmethod, _, _ = base()
        res["cases"][name] = {"frames": F, "hybrid_exact_probs": te, "hybrid_probs": tb,
                              "ratio_exact_to_hybrid": te["median_ms"] / tb["median_ms"], "open_clusters": int(nOpen.sum()),
                              "answered_by_the_tier": int(nBig.sum()),
                              "methods_exact": {str(v): int((method == v).sum()) for v in (-2, -1, 0, 1, 2)},
                              "methods_hybrid": {str(v): int((hmethod == v).sum()) for v in (-2, -1, 0, 1, 2)}}
    # the tier alone, one cluster a call, by HIP events
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    for name, frames, nL, nM in cases[:2]:
        d_sub, opens = open_clusters(eng, torch, frames, nL, nM)
        for at, m, cL, R in opens:
            if m > 20:
                continue
            d_probs = torch.zeros(m * (cL + 1), dtype=torch.float64, device=dev)
            d_out = torch.zeros(1, dtype=torch.float64, device=dev)
            d_info = torch.zeros(1, dtype=torch.int32, device=dev)
            ms = []
            for i in range(2 + 5):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                eng.bigcluster_probs_dev([m], [cL], [at], [0], d_sub, d_probs, d_out, d_info, stream=stream.cuda_stream)
                t1.record(stream)
                stream.synchronize()
                if i >= 2:
                    ms.append(t0.elapsed_time(t1))
            launches = 2 * (cL + m) + 4
            res["tier_per_cluster"].append({"case": name, "m": m, "R": R, "rows_launched": cL + m, "launches": launches,
                                            "median_ms": float(np.median(ms)), "min_ms": float(min(ms)),
                                            "layer_traffic_bytes": 2 * R * (1 << m) * 8, "info": int(d_info.cpu()[0])})
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
