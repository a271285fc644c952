"""Times of the asynchronous exact hybrid entry (kbest_hybrid_frontier_probs_batch_f64_dev) beside the host entry it restates
(hybrid_frontier_probs, k = 0, max_big = 0), both sides in ONE process, alternating, warmed up, the median of --steps runs; raw
blocks with condition = 1.  Three batches: 1 000 scene frames (20, 10, 12) -- nothing open --, 256 frames (60, 40, 30), 64 frames
(200, 128, 60).  Per batch:

    a  device_events    the device entry between HIP events on the caller's stream, buffers resident, work space reserved
    b  host_wall        the host entry, time.perf_counter around the synchronous call
    c  device_wall      the device entry plus the same upload (costs, offsets, counts) and read-back (probabilities, logPerm,
                        method, nOpen, nFrontier, maxCluster), time.perf_counter: the like-for-like number against b
    d  partial_events   the first batch only: clustered_partial_dev alone between events -- what the gather, sweep and scatter
                        launches cost when nothing is open is a - d

No time is promised: nothing of this had been measured when the entry was written.

    python tools/bench_hybrid_dev.py [--steps 30] [--warmup 5] [--out profiles/hybrid_dev_bench.json]

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hybrid_dev_bench.json"))
    args = ap.parse_args()
    import torch  # torch first: its copy of the HIP runtime is the one the process loads (tests/conftest.py)
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    import probabilisticsemslam_amd as pk
    from probabilisticsemslam_amd import workloads as wl
    from probabilisticsemslam_amd.engine import _pack_frames
    eng = pk.KBestEngine(0)
    stream = torch.cuda.Stream(device=dev)
    res = {"tool": "tools/bench_hybrid_dev.py", "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
           "clock_events": "HIP events on the caller's stream around the device entry",
           "clock_wall": "time.perf_counter around the synchronous call (device side: upload, entry, read-back, one synchronise)",
           "batches": {}}
    cases = (("a_1000_scene_20+10", wl.scene_frames(1000, 20, 10, 12), 20, 10), ("d_256_scene_60+40", wl.scene_frames(256, 60, 40, 30), 60, 40),
             ("e_64_scene_200+128", wl.scene_frames(64, 200, 128, 60), 200, 128))
    for ci, (name, frames, nL, nM) in enumerate(cases):
        B = len(frames)
        nLs, nMs = [nL] * B, [nM] * B
        hnL, hnM, _, flat, costOff, probOff, psizes, probs = _pack_frames(frames, nLs, nMs, "bench_hybrid_dev")
        maxRawRow, maxCol = nL + nM, nM
        eng.reserve_hybrid_dev(B, maxRawRow, maxCol)
        pin = lambda a: torch.from_numpy(a).pin_memory()  # noqa: E731
        h_cost, h_nL, h_nM, h_costOff, h_probOff = pin(flat), pin(hnL), pin(hnM), pin(costOff), pin(probOff)
        d_sub = torch.empty(flat.size, dtype=torch.float64, device=dev)
        d_probs = torch.zeros(probs.size, dtype=torch.float64, device=dev)
        d_lp = torch.zeros(B, dtype=torch.float64, device=dev)
        d_int = torch.zeros((4, B), dtype=torch.int32, device=dev)
        d_in = [t.to(dev) for t in (h_cost, h_nL, h_nM, h_costOff, h_probOff)]
        d_desc = torch.zeros((B, maxCol, 4), dtype=torch.int32, device=dev)
        d_rows = torch.zeros((B, maxRawRow), dtype=torch.int32, device=dev)

        def entry(bufs):
            d_cost, d_nL, d_nM, d_costOff, d_probOff = bufs
            eng.hybrid_frontier_probs_dev(B, maxRawRow, maxCol, d_nL, d_nM, d_cost, d_costOff, d_sub, d_probs, d_probOff, d_int[0], d_lp,
                                          d_int[1], d_int[2], d_int[3], condition=True, stream=stream.cuda_stream, reserve=False)

        def partial():
            d_cost, d_nL, d_nM, d_costOff, d_probOff = d_in
            eng.clustered_partial_dev(B, maxRawRow, maxCol, d_nL, d_nM, d_cost, d_costOff, d_probs, d_probOff, d_int[1], d_desc, maxCol,
                                      d_rows, maxRawRow, d_sub, d_logPerm=d_lp, d_info=d_int[0], d_maxCluster=d_int[3],
                                      stream=stream.cuda_stream, reserve=False)

        def events(call):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            call()
            t1.record(stream)
            stream.synchronize()
            return t0.elapsed_time(t1)

        def device_wall():
            t0 = time.perf_counter()
            with torch.cuda.stream(stream):
                bufs = [h.to(dev, non_blocking=True) for h in (h_cost, h_nL, h_nM, h_costOff, h_probOff)]
                entry(bufs)
                back = [t.to("cpu", non_blocking=True) for t in (d_probs, d_lp, d_int)]
            stream.synchronize()
            return (time.perf_counter() - t0) * 1e3, back

        def host_wall():
            t0 = time.perf_counter()
            out = eng.hybrid_frontier_probs(frames, nLs, nMs, 0, condition=True, max_big=0)
            return (time.perf_counter() - t0) * 1e3, out

        sides = {"device_events": lambda: events(lambda: entry(d_in)), "host_wall": lambda: host_wall()[0],
                 "device_wall": lambda: device_wall()[0]}
        if ci == 0:
            sides["partial_events"] = lambda: events(partial)
        for _ in range(args.warmup):
            for call in sides.values():
                call()
        ms = {k: [] for k in sides}
        for _ in range(args.steps):
            for k, call in sides.items():
                ms[k].append(call())
        _, (hp, hlp, hint) = device_wall()
        _, (out, method, nOpen, _, maxc, lp, nFr) = host_wall()
        hp, hlp, hint = hp.numpy(), hlp.numpy(), hint.numpy()
        same = (all(np.array_equal(hp[probOff[b]:probOff[b] + psizes[b]].view(np.int64), out[b].reshape(-1).view(np.int64)) for b in range(B))
                and np.array_equal(hint[0], method) and np.array_equal(hint[1], nOpen) and np.array_equal(hint[2], nFr)
                and np.array_equal(hint[3], maxc) and np.array_equal(hlp.view(np.int64)[~np.isnan(lp)], lp.view(np.int64)[~np.isnan(lp)]))
        row = {k: stats(v) for k, v in ms.items()}
        row.update(frames=B, open_clusters=int(nOpen.sum()), answered_by_the_frontier_tier=int(nFr.sum()),
                   methods={str(v): int((method == v).sum()) for v in (-2, -1, 0)}, same_bits_as_the_host_entry=bool(same),
                   ratio_host_to_device_wall=row["host_wall"]["median_ms"] / row["device_wall"]["median_ms"])
        res["batches"][name] = row
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
