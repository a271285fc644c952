"""Times of the asynchronous exact hybrid draws (kbest_hybrid_frontier_sample_assoc_batch_f64_dev) beside the host entry they restate
(hybrid_frontier_sample_assoc), both sides in ONE process, alternating, warmed up, the median of --steps runs; raw blocks with
condition = 1, max_exact = 16, max_width = 16.  Two batches -- 256 scene frames (60, 40, 30), 1 000 frames (20, 10, 12) -- with 16
and with 1 024 draws a frame.  Per case:

    a  device_events    the device entry between HIP events on the caller's stream, buffers resident, work space reserved
    b  host_wall        the host entry, time.perf_counter around the synchronous call (upload, kernels, read-back, host loops)

The yardstick of the ratio is b in the same run.  No time is asserted or promised anywhere.

    python tools/bench_hybrid_sample_dev.py [--steps 30] [--warmup 3] [--out profiles/hybrid_sample_dev_bench.json]

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
SEED = 0x5EED5EED


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)), calls=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hybrid_sample_dev_bench.json"))
    args = ap.parse_args()
    import torch  # torch first: its copy of the HIP runtime is the one the process loads (tests/conftest.py)
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    import probabilisticsemslam_amd as pk
    from probabilisticsemslam_amd import workloads as wl
    from probabilisticsemslam_amd.engine import _pack_frames
    eng = pk.KBestEngine(0)
    stream = torch.cuda.Stream(device=dev)
    res = {"tool": "tools/bench_hybrid_sample_dev.py", "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
           "clock_events": "HIP events on the caller's stream around the device entry",
           "clock_wall": "time.perf_counter around the synchronous host entry", "cases": {}}
    batches = (("256_scene_60+40", wl.scene_frames(256, 60, 40, 30), 60, 40), ("1000_scene_20+10", wl.scene_frames(1000, 20, 10, 12), 20, 10))
    for name, frames, nL, nM in batches:
        B = len(frames)
        nLs, nMs = [nL] * B, [nM] * B
        hnL, hnM, _, flat, costOff, _, _, _ = _pack_frames(frames, nLs, nMs, "bench_hybrid_sample_dev")
        maxRawRow, maxCol = nL + nM, nM
        d_cost, d_nL, d_nM, d_costOff = (torch.from_numpy(a).to(dev) for a in (flat, hnL, hnM, costOff))
        d_sub = torch.empty(flat.size, dtype=torch.float64, device=dev)
        d_lp = torch.zeros(B, dtype=torch.float64, device=dev)
        d_int = torch.zeros((4, B), dtype=torch.int32, device=dev)
        for n in (16, 1024):
            eng.reserve_hybrid_sample_dev(B, maxRawRow, maxCol, n)
            asgOff = np.arange(B, dtype=np.int64) * n * nM
            lpOff = np.arange(B, dtype=np.int64) * n
            d_asgOff, d_lpOff = torch.from_numpy(asgOff).to(dev), torch.from_numpy(lpOff).to(dev)
            d_assign = torch.zeros(B * n * nM, dtype=torch.int32, device=dev)
            d_logp = torch.zeros(B * n, dtype=torch.float64, device=dev)

            def entry():
                eng.hybrid_frontier_sample_assoc_dev(B, maxRawRow, maxCol, d_nL, d_nM, d_cost, d_costOff, d_sub, n, d_assign, d_asgOff,
                                                     d_logp, d_lpOff, d_int[0], d_lp, d_int[1], d_int[2], d_int[3], seed=SEED,
                                                     condition=True, stream=stream.cuda_stream, reserve=False)

            def device_events():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                entry()
                t1.record(stream)
                stream.synchronize()
                return t0.elapsed_time(t1)

            def host_wall():
                t0 = time.perf_counter()
                out = eng.hybrid_frontier_sample_assoc(frames, nLs, nMs, n, seed=SEED, condition=True)
                return (time.perf_counter() - t0) * 1e3, out

            sides = {"device_events": device_events, "host_wall": lambda: host_wall()[0]}
            for _ in range(args.warmup):
                for call in sides.values():
                    call()
            ms = {k: [] for k in sides}
            for _ in range(args.steps):
                for k, call in sides.items():
                    ms[k].append(call())
            device_events()
            _, (asg, lp, logPerm, method, nOpen, nFr, maxc) = host_wall()
            ha, hp, hl, hi = d_assign.cpu().numpy(), d_logp.cpu().numpy(), d_lp.cpu().numpy(), d_int.cpu().numpy()

            def same_doubles(a, b):
                return bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())

            same = (all(np.array_equal(ha[asgOff[b]:asgOff[b] + n * nM].reshape(n, nM), asg[b]) for b in range(B))
                    and all(same_doubles(hp[lpOff[b]:lpOff[b] + n], lp[b]) for b in range(B)) and same_doubles(hl, logPerm)
                    and np.array_equal(hi[0], method) and np.array_equal(hi[1], nOpen) and np.array_equal(hi[2], nFr)
                    and np.array_equal(hi[3], maxc))
            row = {k: stats(v) for k, v in ms.items()}
            row.update(frames=B, draws=n, open_clusters=int(nOpen.sum()), frames_with_open_clusters=int((nOpen > 0).sum()),
                       methods={str(v): int((method == v).sum()) for v in (-2, -1, 0)}, same_bits_as_the_host_entry=bool(same),
                       ratio_host_wall_to_device_events=row["host_wall"]["median_ms"] / row["device_events"]["median_ms"])
            res["cases"][f"{name}_x{n}"] = row
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
