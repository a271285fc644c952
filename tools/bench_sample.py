"""HIP-event times of the draws from the exact posterior (kbest_sample_assoc_batch_f64_dev) beside the exact marginals
(kbest_permanent_probs_batch_f64_dev) on the same frames, in ONE process and run, the two sides ALTERNATING launch by launch:
warm-up, then the median of the timed launches of each side, buffers resident in HBM, KITTI-like frames
(workloads.kitti_like_frames).  The permanent entry is the yardstick because the load and the forward sweep are the same lines:
the ratio shows what replacing the backward sweep by the walk costs or saves.

    (a) 1 000 raw 30x10 frames, condition = 1, one launch       nSample = 1, 64, 1 024
    (b) one 30x10 frame per launch                               nSample = 1 024

    python tools/bench_sample.py [--steps 30] [--warmup 5] [--out profiles/sample_bench.json]

Prints one JSON line and writes it to --out.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_bench.json"))
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps must be at least 20 (median of >= 20 launches)")
    import torch  # torch first: its copy of the HIP runtime is the one the process loads (tests/conftest.py)
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    import probabilisticsemslam_amd as pk
    from probabilisticsemslam_amd import workloads as wl
    eng = pk.KBestEngine(0)
    tstream = torch.cuda.Stream(device=dev)
    stream = tstream.cuda_stream
    nL, nM = 20, 10
    nR = nL + nM

    def setup(frames, n):
        F = len(frames)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        return dict(F=F, n=n, d_cost=t(np.concatenate(frames)), d_nL=t(np.full(F, nL, np.int32)), d_nM=t(np.full(F, nM, np.int32)),
                    d_coff=t(np.arange(F, dtype=np.int64) * nR * nM), d_poff=t(np.arange(F, dtype=np.int64) * nM * (nL + 1)),
                    d_aoff=t(np.arange(F, dtype=np.int64) * nM * n), d_loff=t(np.arange(F, dtype=np.int64) * n),
                    d_probs=torch.zeros(F * nM * (nL + 1), dtype=torch.float64, device=dev),
                    d_asg=torch.zeros(F * nM * n, dtype=torch.int32, device=dev), d_lp=torch.zeros(F * n, dtype=torch.float64, device=dev),
                    d_perm=torch.zeros(F, dtype=torch.float64, device=dev), d_perm2=torch.zeros(F, dtype=torch.float64, device=dev))

    def both(s):
        """The two entries on the same frames, alternating: (sample, permanent) per step."""
        eng.reserve_sample(s["F"], nR, nM)  # (the permanent entry's work space: reserved once for both)
        torch.cuda.synchronize()
        sample = lambda: eng.sample_assoc_dev(s["F"], nR, nM, s["d_nL"], s["d_nM"], s["d_cost"], s["d_coff"], s["n"], s["d_asg"],  # noqa: E731
                                              s["d_aoff"], s["d_lp"], s["d_loff"], s["d_perm"], seed=2024, condition=True,
                                              stream=stream, reserve=False)
        permanent = lambda: eng.permanent_probs_dev(s["F"], nR, nM, s["d_nL"], s["d_nM"], s["d_cost"], s["d_coff"], s["d_probs"],  # noqa: E731
                                                    s["d_poff"], s["d_perm2"], condition=True, stream=stream, reserve=False)
        for _ in range(args.warmup):
            sample()
            permanent()
        torch.cuda.synchronize()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.steps)]
        for a, b, c in ev:
            a.record(tstream)
            sample()
            b.record(tstream)
            permanent()
            c.record(tstream)
        torch.cuda.synchronize()
        assert np.array_equal(s["d_perm"].cpu().numpy().view(np.int64), s["d_perm2"].cpu().numpy().view(np.int64)), "perm differs"
        out = {}
        for name, ms in (("sample", sorted(a.elapsed_time(b) for a, b, c in ev)), ("permanent", sorted(b.elapsed_time(c) for a, b, c in ev))):
            out[name] = dict(median_ms=float(np.median(ms)), min_ms=float(ms[0]), max_ms=float(ms[-1]), launches=len(ms))
        out["ratio_sample_to_permanent"] = out["sample"]["median_ms"] / out["permanent"]["median_ms"]
        return out

    c5 = wl.kitti_like_frames(1000, nL=nL, nM=nM)
    res = {"tool": "tools/bench_sample.py", "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
           "library": os.environ.get("KBEST_LIB", "libkbest_amd.so"), "cases": {}}
    for n in (1, 64, 1024):
        res["cases"][f"a_1000x30x10_n{n}"] = both(setup(c5, n))
    res["cases"]["b_1x30x10_n1024"] = both(setup(c5[:1], 1024))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
