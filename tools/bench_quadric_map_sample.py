"""Times of the drawing quadric-map entry (kbest_quadric_map_sample_assoc_batch_f64_dev: from quadrics against one resident map to
joint associations on one stream, k = 0) beside the marginals' entry on the same frames and, where it can take them, the only path
from quadrics to joint associations before it -- quadric_costs (host in, host out), upload of the raw blocks,
hybrid_frontier_sample_assoc_dev(condition = 1) -- all in ONE process, alternating, warmed up, the median of --steps runs, at 16
and at 1 024 draws a frame.  Scenes of tests/quadric_map_lib.py and batches of tools/bench_quadric_map.py (gate 10, hot 3, spread 25
unless said):

    256_map900      256 frames of map(1, 900, 19, 3), nM = 40: sizes both paths take (nL + nM = 940)
        sample_events   the new entry between HIP events on the caller's stream, map and measurements resident, work space reserved
        probs_events    quadric_map_probs_dev (compact probabilities, no dense expansion) likewise: what drawing costs over the marginals
        sample_wall     the new entry with the upload of the measurements and the read-back of the draws, perf_counter
        older_wall      quadric_costs, upload, hybrid_frontier_sample_assoc_dev(condition = 1), read-back, perf_counter: like sample_wall
    64_map5000      64 frames of map(1, 5 000, 45, 3), nM = 40: sample_events and probs_events (the older path stops at 1 024 rows)
    16_map100000    16 frames of map(2, 100 000, 900, 3), nM = 24, hot 24, spread 1: likewise

and the registers, scratch bytes and static LDS bytes of the kernel that maps compact rows to raw rows.  No time is promised.

    python tools/bench_quadric_map_sample.py [--steps 30] [--warmup 5] [--out profiles/quadric_map_sample_bench.json]

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quadric_map_sample_bench.json"))
    args = ap.parse_args()
    import torch  # torch first: its copy of the HIP runtime is the one the process loads (tests/conftest.py)
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    import probabilisticsemslam_amd as pk
    import quadric_map_lib as qm
    from probabilisticsemslam_amd.engine import _pack_frames
    eng = pk.KBestEngine(0)
    stream = torch.cuda.Stream(device=dev)
    res = {"tool": "tools/bench_quadric_map_sample.py", "device": torch.cuda.get_device_name(0), "steps": args.steps,
           "warmup": args.warmup, "k": 0, "clock_events": "HIP events on the caller's stream around the device entry",
           "clock_wall": "time.perf_counter around upload, entry / entries, read-back, one synchronise", "batches": {}, "kernels": {}}
    v = eng.quadric_map_sample_kernel_usage()
    res["kernels"]["qmap_sample_rows_kernel"] = dict(vgprs=v[0], scratch_bytes=v[1], lds_bytes=v[2])
    up = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt, order="C")).to(dev)  # noqa: E731
    cases = (("256_map900", (1, 900, 19.0, 3.0), 256, 40, 3, 25, True), ("64_map5000", (1, 5000, 45.0, 3.0), 64, 40, 3, 25, False),
             ("16_map100000", (2, 100000, 900.0, 3.0), 16, 24, 24, 1, False))
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
        d_lp = torch.zeros(B, dtype=torch.float64, device=dev)
        d_int = torch.zeros((5, B), dtype=torch.int32, device=dev)

        def probs(maxKeep, rows, cprobs):
            eng.quadric_map_probs_dev(B, nMap, maxKeep, nM, d_map[0], d_map[1], d_landOff, d_nL, d_meas[0], d_meas[1], d_measOff, d_nM,
                                      gate, d_int[0], rows, cprobs, d_int[1], d_logPerm=d_lp, d_nOpen=d_int[2], d_nFrontier=d_int[3],
                                      d_maxCluster=d_int[4], stream=stream.cuda_stream, reserve=False)

        # the kept rows of these frames, from a first call under the widest bound: the caller reserves again from the true counts
        wide = 1024 - nM
        eng.reserve_quadric_map_dev(B, nMap, wide, nM)
        rows, cprobs = torch.zeros(B * wide, dtype=torch.int32, device=dev), torch.zeros(B * nM * (wide + 1), dtype=torch.float64, device=dev)
        probs(wide, rows, cprobs)
        stream.synchronize()
        kept = d_int[0].cpu().numpy().copy()
        maxKeep = int(kept.max())
        rows, cprobs = rows[:B * maxKeep], cprobs[:B * nM * (maxKeep + 1)]
        row = dict(frames=B, map=nMap, nM=nM, kept_rows=dict(min=int(kept.min()), max=maxKeep))

        def events(call):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            call()
            t1.record(stream)
            stream.synchronize()
            return t0.elapsed_time(t1)

        for n in (16, 1024):
            d_asgOff, d_lpOff = up(np.arange(B) * n * nM, np.int64), up(np.arange(B) * n, np.int64)
            d_assign = torch.zeros(B * n * nM, dtype=torch.int32, device=dev)
            d_logp = torch.zeros(B * n, dtype=torch.float64, device=dev)
            s_lp, s_int = torch.zeros(B, dtype=torch.float64, device=dev), torch.zeros((5, B), dtype=torch.int32, device=dev)
            eng.reserve_quadric_map_sample_dev(B, nMap, maxKeep, nM, n)

            def sample(meas):
                eng.quadric_map_sample_assoc_dev(B, nMap, maxKeep, nM, d_map[0], d_map[1], d_landOff, d_nL, meas[0], meas[1], d_measOff,
                                                 d_nM, gate, n, s_int[0], rows, d_assign, d_asgOff, d_logp, d_lpOff, s_int[1],
                                                 d_logPerm=s_lp, d_nOpen=s_int[2], d_nFrontier=s_int[3], d_maxCluster=s_int[4], seed=1,
                                                 stream=stream.cuda_stream, reserve=False)

            def sample_wall():
                t0 = time.perf_counter()
                with torch.cuda.stream(stream):
                    meas = [h.to(dev, non_blocking=True) for h in h_meas]
                    sample(meas)
                    back = [t.to("cpu", non_blocking=True) for t in (d_assign, d_logp, s_lp, s_int)]
                stream.synchronize()
                return (time.perf_counter() - t0) * 1e3, back

            sides = {"sample_events": lambda: events(lambda: sample(d_meas)),
                     "probs_events": lambda: events(lambda: probs(maxKeep, rows, cprobs))}
            if both:
                sides["sample_wall"] = lambda: sample_wall()[0]
                quads = [(mean, cov, f[0], f[1]) for f in frames]
                eng.reserve_hybrid_sample_dev(B, nMap + nM, nM, n)
                d_sub = torch.empty(B * (nMap + nM) * nM, dtype=torch.float64, device=dev)
                o_assign, o_logp = torch.zeros_like(d_assign), torch.zeros_like(d_logp)
                o_lp, o_int = torch.zeros(B, dtype=torch.float64, device=dev), torch.zeros((4, B), dtype=torch.int32, device=dev)

                def older_wall():
                    t0 = time.perf_counter()
                    raw = eng.quadric_costs(quads, gate)
                    _, _, _, flat, costOff, _, _, _ = _pack_frames(raw, [nMap] * B, [nM] * B, "bench_quadric_map_sample")
                    with torch.cuda.stream(stream):
                        d_cost, d_costOff = torch.from_numpy(flat).to(dev, non_blocking=True), torch.from_numpy(costOff).to(dev, non_blocking=True)
                        eng.hybrid_frontier_sample_assoc_dev(B, nMap + nM, nM, d_nL, d_nM, d_cost, d_costOff, d_sub, n, o_assign, d_asgOff,
                                                             o_logp, d_lpOff, o_int[0], o_lp, o_int[1], o_int[2], o_int[3], seed=1,
                                                             condition=True, stream=stream.cuda_stream, reserve=False)
                        back = [t.to("cpu", non_blocking=True) for t in (o_assign, o_logp, o_lp, o_int)]
                    stream.synchronize()
                    return (time.perf_counter() - t0) * 1e3, back

                sides["older_wall"] = lambda: older_wall()[0]
            for _ in range(args.warmup):
                for call in sides.values():
                    call()
            ms = {k: [] for k in sides}
            for _ in range(args.steps):
                for k, call in sides.items():
                    ms[k].append(call())
            part = {k: stats(t) for k, t in ms.items()}
            method = s_int[1].cpu().numpy()
            part.update(methods={str(m): int((method == m).sum()) for m in (-2, -1, 0)},
                        ratio_sample_to_probs_events=part["sample_events"]["median_ms"] / part["probs_events"]["median_ms"])
            if both:
                _, (na, nlp, _, nint) = sample_wall()
                _, (oa, olp, _, oint) = older_wall()
                na, oa, nint, oint = na.numpy().reshape(B, n * nM), oa.numpy().reshape(B, n * nM), nint.numpy(), oint.numpy()
                closed = np.flatnonzero(nint[2] == 0)  # the frames without an open cluster: the same draws by contract
                same = (np.array_equal(na[closed], oa[closed]) and np.array_equal(nint[1:], oint)
                        and np.array_equal(nlp.numpy().reshape(B, n)[closed].view(np.int64), olp.numpy().reshape(B, n)[closed].view(np.int64)))
                part.update(frames_without_an_open_cluster=int(len(closed)), same_bits_as_the_older_path_there=bool(same),
                            ratio_older_to_sample_wall=part["older_wall"]["median_ms"] / part["sample_wall"]["median_ms"])
            row[f"draws_{n}"] = part
        res["batches"][name] = row
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
