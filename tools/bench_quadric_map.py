"""Times of the quadric-map entry (kbest_quadric_map_probs_batch_f64_dev: from quadrics against one resident map to the exact
association probabilities on one stream) beside the only path from quadrics to an exact answer before it -- quadric_costs (host in,
host out), upload of the raw blocks, hybrid_frontier_probs_dev(condition = 1) -- both in ONE process, alternating, warmed up, the
median of --steps runs.  Scenes of tests/quadric_map_lib.py (gate 10, hot 3, spread 25 unless said):

    both_256_map900     256 frames of map(1, 900, 19, 3), nM = 40: sizes both paths take (nL + nM = 940)
        new_events      the new entry between HIP events on the caller's stream, map and measurements resident, work space reserved
        new_wall        the same with the upload of the measurements and the read-back of the dense probabilities, perf_counter
        parent_wall     quadric_costs, upload, hybrid_frontier_probs_dev(condition = 1), read-back, perf_counter: like new_wall
    new_64_map5000      64 frames of map(1, 5 000, 45, 3), nM = 40: new_events alone (the parent's path stops at 1 024 rows)
    new_16_map100000    16 frames of map(2, 100 000, 900, 3), nM = 24, hot 24, spread 1: new_events alone

and the registers, scratch bytes and static LDS bytes of the three kernels that compute costs.  No time is promised.

    python tools/bench_quadric_map.py [--steps 30] [--warmup 5] [--out profiles/quadric_map_bench.json]

Prints one JSON line and writes it to --out.
"""
from __future__ import annotations

import argparse
import ctypes as C
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quadric_map_bench.json"))
    args = ap.parse_args()
    import torch  # torch first: its copy of the HIP runtime is the one the process loads (tests/conftest.py)
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    import probabilisticsemslam_amd as pk
    import quadric_map_lib as qm
    from probabilisticsemslam_amd.engine import _pack_frames
    eng = pk.KBestEngine(0)
    stream = torch.cuda.Stream(device=dev)
    res = {"tool": "tools/bench_quadric_map.py", "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
           "clock_events": "HIP events on the caller's stream around the device entry",
           "clock_wall": "time.perf_counter around upload, entry / entries, read-back, one synchronise", "batches": {}, "kernels": {}}
    for which, name in enumerate(("qmap_min_kernel", "qmap_flag_kernel", "qmap_fill_kernel")):
        v = (C.c_int32 * 3)()
        eng._check(eng.lib.kbest_quadric_map_kernel_usage(which, C.byref(v, 0), C.byref(v, 4), C.byref(v, 8)))
        res["kernels"][name] = dict(vgprs=int(v[0]), scratch_bytes=int(v[1]), lds_bytes=int(v[2]))
    up = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt, order="C")).to(dev)  # noqa: E731
    cases = (("both_256_map900", (1, 900, 19.0, 3.0), 256, 40, 3, 25, True), ("new_64_map5000", (1, 5000, 45.0, 3.0), 64, 40, 3, 25, False),
             ("new_16_map100000", (2, 100000, 900.0, 3.0), 16, 24, 24, 1, False))
    for name, mp, B, nM, hot, spread, both in cases:
        mean, cov = qm.make_map(*mp)
        nMap, gate = len(mean), 10.0
        frames = [qm.make_frame(1000 + f, mean, nM, hot, spread) for f in range(B)]
        d_map = (up(mean, np.float64), up(cov.reshape(-1, 9), np.float64))
        h_meas = [torch.from_numpy(np.ascontiguousarray(np.concatenate([f[i] for f in frames]).reshape(-1, w))).pin_memory() for i, w in ((0, 3), (1, 9))]
        d_meas = [h.to(dev) for h in h_meas]
        d_landOff = torch.zeros(B, dtype=torch.int64, device=dev)
        d_measOff = up(np.arange(B) * nM, np.int64)
        d_nL, d_nM = up([nMap] * B, np.int32), up([nM] * B, np.int32)
        d_probOff = up(np.arange(B) * nM * (nMap + 1), np.int64)
        d_probs = torch.zeros(B * nM * (nMap + 1), dtype=torch.float64, device=dev)
        d_lp = torch.zeros(B, dtype=torch.float64, device=dev)
        d_int = torch.zeros((5, B), dtype=torch.int32, device=dev)

        def new(meas, maxKeep, rows, cprobs):
            eng.quadric_map_probs_dev(B, nMap, maxKeep, nM, d_map[0], d_map[1], d_landOff, d_nL, meas[0], meas[1], d_measOff, d_nM, gate,
                                      d_int[0], rows, cprobs, d_int[1], d_probs=d_probs, d_probOff=d_probOff, d_logPerm=d_lp,
                                      d_nOpen=d_int[2], d_nFrontier=d_int[3], d_maxCluster=d_int[4], stream=stream.cuda_stream, reserve=False)

        # the kept rows of these frames, from a first call under the widest bound: the caller reserves again from the true counts
        wide = 1024 - nM
        eng.reserve_quadric_map_dev(B, nMap, wide, nM)
        rows, cprobs = torch.zeros(B * wide, dtype=torch.int32, device=dev), torch.zeros(B * nM * (wide + 1), dtype=torch.float64, device=dev)
        new(d_meas, wide, rows, cprobs)
        stream.synchronize()
        kept = d_int[0].cpu().numpy().copy()
        maxKeep = int(kept.max())
        rows, cprobs = rows[:B * maxKeep], cprobs[:B * nM * (maxKeep + 1)]

        def events(call):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            call()
            t1.record(stream)
            stream.synchronize()
            return t0.elapsed_time(t1)

        def new_wall():
            t0 = time.perf_counter()
            with torch.cuda.stream(stream):
                meas = [h.to(dev, non_blocking=True) for h in h_meas]
                new(meas, maxKeep, rows, cprobs)
                back = [t.to("cpu", non_blocking=True) for t in (d_probs, d_lp, d_int)]
            stream.synchronize()
            return (time.perf_counter() - t0) * 1e3, back

        sides = {"new_events": lambda: events(lambda: new(d_meas, maxKeep, rows, cprobs))}
        if both:
            sides["new_wall"] = lambda: new_wall()[0]
            quads = [(mean, cov, f[0], f[1]) for f in frames]
            eng.reserve_hybrid_dev(B, nMap + nM, nM)
            d_sub = torch.empty(B * (nMap + nM) * nM, dtype=torch.float64, device=dev)
            p_probs = torch.zeros(B * nM * (nMap + 1), dtype=torch.float64, device=dev)
            p_lp, p_int = torch.zeros(B, dtype=torch.float64, device=dev), torch.zeros((4, B), dtype=torch.int32, device=dev)

            def parent_wall():
                t0 = time.perf_counter()
                raw = eng.quadric_costs(quads, gate)
                _, _, _, flat, costOff, _, _, _ = _pack_frames(raw, [nMap] * B, [nM] * B, "bench_quadric_map")
                with torch.cuda.stream(stream):
                    d_cost, d_costOff = torch.from_numpy(flat).to(dev, non_blocking=True), torch.from_numpy(costOff).to(dev, non_blocking=True)
                    eng.hybrid_frontier_probs_dev(B, nMap + nM, nM, d_nL, d_nM, d_cost, d_costOff, d_sub, p_probs, d_probOff, p_int[0], p_lp,
                                                  p_int[1], p_int[2], p_int[3], condition=True, stream=stream.cuda_stream, reserve=False)
                    back = [t.to("cpu", non_blocking=True) for t in (p_probs, p_lp, p_int)]
                stream.synchronize()
                return (time.perf_counter() - t0) * 1e3, back

            sides["parent_wall"] = lambda: parent_wall()[0]
        for _ in range(args.warmup):
            for call in sides.values():
                call()
        ms = {k: [] for k in sides}
        for _ in range(args.steps):
            for k, call in sides.items():
                ms[k].append(call())
        row = {k: stats(v) for k, v in ms.items()}
        method = d_int[1].cpu().numpy()
        row.update(frames=B, map=nMap, nM=nM, kept_rows=dict(min=int(kept.min()), max=maxKeep),
                   methods={str(v): int((method == v).sum()) for v in (-2, -1, 0)})
        if both:
            _, (hp, hlp, hint) = new_wall()
            _, (pp, plp, pint) = parent_wall()
            hlp, plp = hlp.numpy(), plp.numpy()
            same = (np.array_equal(hp.numpy().view(np.int64), pp.numpy().view(np.int64)) and np.array_equal(hint.numpy()[1:], pint.numpy())
                    and np.array_equal(hlp.view(np.int64)[~np.isnan(plp)], plp.view(np.int64)[~np.isnan(plp)]))
            row.update(same_bits_as_the_parent_path=bool(same),
                       ratio_parent_to_new_wall=row["parent_wall"]["median_ms"] / row["new_wall"]["median_ms"])
        res["batches"][name] = row
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
