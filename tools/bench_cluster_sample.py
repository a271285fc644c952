"""HIP-event times of the draws from the exact posterior by gated clusters (kbest_clustered_sample_assoc_batch_f64_dev) beside
the entry it shares its prologue and forward sweeps with (kbest_clustered_probs_batch_f64_dev) and beside the whole-frame sampler
(kbest_sample_assoc_batch_f64_dev), in ONE process and run, the two sides ALTERNATING launch by launch on the same device
buffers, the work space reserved beforehand: warm-up, then the median of the timed launches of each side (min and max beside it).

    (a) 1 000 scene_frames(., 20, 10, 12.0), one launch                              nSample = 1, 64, 1 024    vs clustered_probs
    (b) 256 scene_frames(., 60, 40, 30.0) without the frames clustered_probs refuses  nSample = 1, 64, 1 024    vs clustered_probs
    (c) one 40 + 24 frame per launch                                                  nSample = 1, 64, 1 024    vs clustered_probs
    (d) 1 000 KITTI-like 30x10 frames, one launch                                     nSample = 1, 64, 1 024    vs sample_assoc

Raw frames, condition = 1.  No target: the numbers are a record.

    python tools/bench_cluster_sample.py [--steps 30] [--warmup 5] [--out profiles/cluster_sample_bench.json]

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_sample_bench.json"))
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

    def setup(frames, nL, nM, n):
        F, nR = len(frames), nL + nM
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        z = lambda k, dt: torch.zeros(k, dtype=dt, device=dev)  # noqa: E731
        return dict(F=F, n=n, nR=nR, nM=nM, d_cost=t(np.concatenate(frames)), d_nL=t(np.full(F, nL, np.int32)),
                    d_nM=t(np.full(F, nM, np.int32)), d_coff=t(np.arange(F, dtype=np.int64) * nR * nM),
                    d_poff=t(np.arange(F, dtype=np.int64) * nM * (nL + 1)), d_aoff=t(np.arange(F, dtype=np.int64) * nM * n),
                    d_loff=t(np.arange(F, dtype=np.int64) * n), d_probs=z(F * nM * (nL + 1), torch.float64),
                    d_asg=z(F * nM * n, torch.int32), d_lp=z(F * n, torch.float64), d_asg2=z(F * nM * n, torch.int32),
                    d_lp2=z(F * n, torch.float64), d_logperm=z(F, torch.float64), d_logperm2=z(F, torch.float64),
                    d_info=z(F, torch.int32), d_info2=z(F, torch.int32), d_perm=z(F, torch.float64))

    def alternate(first, second, names):
        for _ in range(args.warmup):
            first()
            second()
        torch.cuda.synchronize()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.steps)]
        for a, b, c in ev:
            a.record(tstream)
            first()
            b.record(tstream)
            second()
            c.record(tstream)
        torch.cuda.synchronize()
        out = {}
        for name, ms in ((names[0], sorted(a.elapsed_time(b) for a, b, c in ev)), (names[1], sorted(b.elapsed_time(c) for a, b, c in ev))):
            out[name] = dict(median_ms=float(np.median(ms)), min_ms=float(ms[0]), max_ms=float(ms[-1]), launches=len(ms))
        out[f"ratio_{names[0]}_to_{names[1]}"] = out[names[0]]["median_ms"] / out[names[1]]["median_ms"]
        return out

    def cluster_sample(s, asg="d_asg", lp="d_lp"):
        return lambda: eng.clustered_sample_assoc_dev(s["F"], s["nR"], s["nM"], s["d_nL"], s["d_nM"], s["d_cost"], s["d_coff"], s["n"],
                                                      s[asg], s["d_aoff"], s[lp], s["d_loff"], s["d_logperm"], s["d_info"], None,
                                                      seed=2024, condition=True, stream=stream, reserve=False)

    def vs_clustered(s):
        eng.reserve_clustered_sample(s["F"], s["nR"], s["nM"])  # (the clustered entry's work space: reserved once for both)
        torch.cuda.synchronize()
        probs = lambda: eng.clustered_probs_dev(s["F"], s["nR"], s["nM"], s["d_nL"], s["d_nM"], s["d_cost"], s["d_coff"], s["d_probs"],  # noqa: E731
                                                s["d_poff"], s["d_logperm2"], s["d_info2"], condition=True, stream=stream, reserve=False)
        out = alternate(cluster_sample(s), probs, ("cluster_sample", "clustered_probs"))
        info = s["d_info"].cpu().numpy()
        assert (info > 0).all() and np.array_equal(info, s["d_info2"].cpu().numpy()), "info differs"
        assert np.array_equal(s["d_logperm"].cpu().numpy().view(np.int64), s["d_logperm2"].cpu().numpy().view(np.int64)), "logPerm differs"
        out["clusters_per_frame_mean"] = float(info.mean())
        return out

    def vs_sample(s):
        eng.reserve_clustered_sample(s["F"], s["nR"], s["nM"])
        eng.reserve_sample(s["F"], s["nR"], s["nM"])
        torch.cuda.synchronize()
        whole = lambda: eng.sample_assoc_dev(s["F"], s["nR"], s["nM"], s["d_nL"], s["d_nM"], s["d_cost"], s["d_coff"], s["n"], s["d_asg2"],  # noqa: E731
                                             s["d_aoff"], s["d_lp2"], s["d_loff"], s["d_perm"], seed=2024, condition=True, stream=stream,
                                             reserve=False)
        out = alternate(cluster_sample(s), whole, ("cluster_sample", "sample"))
        a, b = s["d_asg"].cpu().numpy().reshape(-1, s["nM"]), s["d_asg2"].cpu().numpy().reshape(-1, s["nM"])
        out["draws"] = int(len(a))
        out["draws_differing"] = int((a != b).any(axis=1).sum())  # (a uniform within the last bits of a boundary; expected: 0)
        out["logprob_max_abs_diff"] = float(np.nanmax(np.abs(s["d_lp"].cpu().numpy() - s["d_lp2"].cpu().numpy())))
        return out

    res = {"tool": "tools/bench_cluster_sample.py", "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
           "library": os.environ.get("KBEST_LIB", "libkbest_amd.so"), "cases": {}}
    small = wl.scene_frames(1000, 20, 10, 12.0)
    big = wl.scene_frames(256, 60, 40, 30.0)
    _, _, info, _ = eng.clustered_probs(big, [60] * 256, [40] * 256, condition=True)
    big = [f for f, i in zip(big, info) if i > 0]
    res["b_frames_kept"] = len(big)
    one = wl.scene_frames(1, 40, 24, 24.0)
    kitti = wl.kitti_like_frames(1000, nL=20, nM=10)
    for n in (1, 64, 1024):
        res["cases"][f"a_1000x20+10_n{n}"] = vs_clustered(setup(small, 20, 10, n))
        res["cases"][f"b_{len(big)}x60+40_n{n}"] = vs_clustered(setup(big, 60, 40, n))
        res["cases"][f"c_1x40+24_n{n}"] = vs_clustered(setup(one, 40, 24, n))
        res["cases"][f"d_1000x30x10_kitti_n{n}"] = vs_sample(setup(kitti, 20, 10, n))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
