"""Times of the factor lists (kbest_quadric_map_factors_batch_f64_dev: from quadrics against one resident map to the thresholded,
ordered factor and new-landmark lists and the support counts, on one stream, the dense slice never formed) beside the way to the
same lists before it -- quadric_map_probs_dev with the dense [nM][nL + 1] slice, a device-to-host copy of that slice, and the
reference's two loops (system.cpp:279-346) in numpy -- both in ONE process, alternating, warmed up, the median of --steps runs.  The
three scenes of tools/bench_quadric_map.py (gate 10):

    256_map900       256 frames of map(1, 900, 19, 3), nM = 40
    64_map5000       64 frames of map(1, 5 000, 45, 3), nM = 40
    16_map100000     16 frames of map(2, 100 000, 900, 3), nM = 24, hot 24, spread 1
        fused_events      the fused entry with d_probs = NULL between HIP events on the caller's stream, everything resident and reserved
        fused_wall        the same with the read-back of the lists, counts and support and one synchronise, perf_counter
        parent_wall       quadric_map_probs_dev with the dense slice, its copy to the host, the two loops in numpy, perf_counter
        probs_events      quadric_map_probs_dev without the dense slice between HIP events: what the fused entry adds to it
        factors_compact_events / factors_dense_events   the factor passes alone (assoc_factors_dev) on d_cprobs / on the dense slice

and the registers, scratch bytes and static LDS bytes of the four factor passes.  No time is promised.

    python tools/bench_factors.py [--steps 30] [--warmup 5] [--out profiles/factors_bench.json]

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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)), calls=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "factors_bench.json"))
    args = ap.parse_args()
    import torch  # torch first: its copy of the HIP runtime is the one the process loads (tests/conftest.py)
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    import factors_lib as fl
    import probabilisticsemslam_amd as pk
    import quadric_map_lib as qm
    eng = pk.KBestEngine(0)
    stream = torch.cuda.Stream(device=dev)
    ft, nt, sd = fl.FACTOR_THRESH, fl.NEW_THRESH, fl.BOX_SD
    res = {"tool": "tools/bench_factors.py", "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
           "thresholds": dict(factor=ft, new=nt, box_sd=sd), "clock_events": "HIP events on the caller's stream around the device entry",
           "clock_wall": "time.perf_counter around entry, read-back (and the host loops), one synchronise", "batches": {}, "kernels": {}}
    for which, name in enumerate(("factors_count_kernel", "factors_frame_scan_kernel", "factors_batch_scan_kernel", "factors_emit_kernel")):
        v = eng.factors_kernel_usage(which)
        res["kernels"][name] = dict(vgprs=v[0], scratch_bytes=v[1], lds_bytes=v[2])
    up = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt, order="C")).to(dev)  # noqa: E731
    cases = (("256_map900", (1, 900, 19.0, 3.0), 256, 40, 3, 25), ("64_map5000", (1, 5000, 45.0, 3.0), 64, 40, 3, 25),
             ("16_map100000", (2, 100000, 900.0, 3.0), 16, 24, 24, 1))
    for name, mp, B, nM, hot, spread in cases:
        mean, cov = qm.make_map(*mp)
        nMap, gate = len(mean), 10.0
        frames = [qm.make_frame(1000 + f, mean, nM, hot, spread) for f in range(B)]
        d_map = (up(mean, np.float64), up(cov.reshape(-1, 9), np.float64))
        d_meas = [up(np.concatenate([f[i] for f in frames]).reshape(-1, w), np.float64) for i, w in ((0, 3), (1, 9))]
        d_landOff = torch.zeros(B, dtype=torch.int64, device=dev)
        d_measOff = up(np.arange(B) * nM, np.int64)
        d_nL, d_nM = up([nMap] * B, np.int32), up([nM] * B, np.int32)
        probOff = np.arange(B, dtype=np.int64) * nM * (nMap + 1)
        d_probOff = up(probOff, np.int64)
        d_probs = torch.zeros(B * nM * (nMap + 1), dtype=torch.float64, device=dev)
        d_int = torch.zeros((2, B), dtype=torch.int32, device=dev)  # nKeep | method
        counts = (torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int64, device=dev),
                  torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int64, device=dev))
        total, support = torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(nMap, dtype=torch.int32, device=dev)

        def lists(cf, cn):
            i32, i64, f64 = (lambda n: torch.zeros(n, dtype=torch.int32, device=dev)), (lambda n: torch.zeros(n, dtype=torch.int64, device=dev)), \
                (lambda n: torch.zeros(n, dtype=torch.float64, device=dev))
            return (i32(cf), i32(cf), i32(cf), i64(cf), f64(cf), f64(cf)) if cf else None, (i32(cn), i32(cn), f64(cn), f64(cn)) if cn else None

        def probs(maxKeep, rows, cprobs, dense):
            eng.quadric_map_probs_dev(B, nMap, maxKeep, nM, d_map[0], d_map[1], d_landOff, d_nL, d_meas[0], d_meas[1], d_measOff, d_nM, gate,
                                      d_int[0], rows, cprobs, d_int[1], d_probs=d_probs if dense else None, d_probOff=d_probOff if dense else None,
                                      stream=stream.cuda_stream, reserve=False)

        def fused(maxKeep, rows, cprobs, cf, f, cn, n):
            eng.quadric_map_factors_dev(B, nMap, maxKeep, nM, d_map[0], d_map[1], d_landOff, d_nL, d_meas[0], d_meas[1], d_measOff, d_nM, gate,
                                        d_int[0], rows, cprobs, d_int[1], cf, f, cn, n, counts, total, d_support=support, n_support=nMap,
                                        factor_thresh=ft, new_thresh=nt, box_sd=sd, stream=stream.cuda_stream, reserve=False)

        # the kept rows and the totals of these frames, from a first call under the widest bound with capacity 0: the caller reserves
        # again from the true counts
        wide = 1024 - nM
        eng.reserve_quadric_map_factors_dev(B, nMap, wide, nM)
        rows, cprobs = torch.zeros(B * wide, dtype=torch.int32, device=dev), torch.zeros(B * nM * (wide + 1), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        fused(wide, rows, cprobs, 0, None, 0, None)
        stream.synchronize()
        kept = d_int[0].cpu().numpy().copy()
        maxKeep = int(kept.max())
        cf, cn = (int(x) for x in total.cpu().numpy())
        rows, cprobs = rows[:B * maxKeep], cprobs[:B * nM * (maxKeep + 1)]
        f, n = lists(cf, cn)
        d_cprobOff = up(np.arange(B, dtype=np.int64) * nM * (maxKeep + 1), np.int64)
        torch.cuda.synchronize()

        def events(call):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            call()
            t1.record(stream)
            stream.synchronize()
            return t0.elapsed_time(t1)

        def fused_wall():
            t0 = time.perf_counter()
            with torch.cuda.stream(stream):
                fused(maxKeep, rows, cprobs, cf, f, cn, n)
                back = [t.to("cpu", non_blocking=True) for t in (f or ()) + (n or ()) + counts + (total, support)]
            stream.synchronize()
            return (time.perf_counter() - t0) * 1e3, back

        def parent_wall():
            t0 = time.perf_counter()
            with torch.cuda.stream(stream):
                probs(maxKeep, rows, cprobs, True)
                hp, hm = d_probs.to("cpu", non_blocking=True), d_int[1].to("cpu", non_blocking=True)
            stream.synchronize()
            hp, hm = hp.numpy(), hm.numpy()
            out, sup = [], np.zeros(nMap, np.int32)
            for b in range(B):  # the two loops of system.cpp:279-346 over the dense slice, the support of the window update
                if hm[b] < 0:
                    continue
                r = fl.frame_lists(hp[probOff[b]:probOff[b] + nM * (nMap + 1)].reshape(nM, nMap + 1), None, ft, nt, sd)
                np.add.at(sup, r[1], 1)
                out.append((b,) + r)
            return (time.perf_counter() - t0) * 1e3, (out, sup)

        def compact_alone():
            eng.assoc_factors_dev(B, maxKeep, nM, cprobs, d_cprobOff, d_int[0], d_nM, cf, f, cn, n, counts, total, d_rowIdx=rows,
                                  row_stride=maxKeep, d_landOff=d_landOff, d_method=d_int[1], d_support=support, n_support=nMap,
                                  factor_thresh=ft, new_thresh=nt, box_sd=sd, stream=stream.cuda_stream, reserve=False)

        def dense_alone():
            eng.assoc_factors_dev(B, nMap, nM, d_probs, d_probOff, d_nL, d_nM, cf, f, cn, n, counts, total, d_landOff=d_landOff,
                                  d_method=d_int[1], d_support=support, n_support=nMap, factor_thresh=ft, new_thresh=nt, box_sd=sd,
                                  stream=stream.cuda_stream, reserve=False)

        sides = {"fused_events": lambda: events(lambda: fused(maxKeep, rows, cprobs, cf, f, cn, n)), "fused_wall": lambda: fused_wall()[0],
                 "parent_wall": lambda: parent_wall()[0], "probs_events": lambda: events(lambda: probs(maxKeep, rows, cprobs, False)),
                 "factors_compact_events": lambda: events(compact_alone), "factors_dense_events": lambda: events(dense_alone)}
        for _ in range(args.warmup):
            for call in sides.values():
                call()
        ms = {k: [] for k in sides}
        for _ in range(args.steps):
            for k, call in sides.items():
                ms[k].append(call())
        row = {k: stats(v) for k, v in ms.items()}
        _, back = fused_wall()
        _, (out, sup) = parent_wall()
        back = [t.numpy() for t in back]
        cat = lambda i, dt: np.concatenate([np.zeros(0, dt)] + [np.asarray(o[i]).astype(dt) for o in out])  # noqa: E731
        same = (np.array_equal(back[1], cat(1, np.int32)) and np.array_equal(back[2], cat(2, np.int32)) and
                np.array_equal(back[4].view(np.int64), cat(3, np.float64).view(np.int64)) and
                np.array_equal(back[5].view(np.int64), cat(4, np.float64).view(np.int64)) and np.array_equal(back[7], cat(5, np.int32)) and
                np.array_equal(back[9].view(np.int64), cat(7, np.float64).view(np.int64)) and np.array_equal(back[-1], sup)) if cf and cn else None
        method = d_int[1].cpu().numpy()
        row.update(frames=B, map=nMap, nM=nM, kept_rows=dict(min=int(kept.min()), max=maxKeep), factors=cf, new_landmarks=cn,
                   dense_slice_bytes=int(B * nM * (nMap + 1) * 8), methods={str(v): int((method == v).sum()) for v in (-2, -1, 0)},
                   same_lists_as_the_parent_way=same, ratio_parent_to_fused_wall=row["parent_wall"]["median_ms"] / row["fused_wall"]["median_ms"])
        res["batches"][name] = row
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
