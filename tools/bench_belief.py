"""HIP-event times of the belief-propagation association probabilities (kbest_belief_probs_batch_f64_dev) beside the k = 200 path
(kbest_assoc_probs_batch_f64_dev) and the exact path (kbest_permanent_probs_batch_f64_dev), in ONE process and run: warm-up, then
the median of the timed launches, buffers resident in HBM, KITTI-like frames (workloads.kitti_like_frames), tol 1e-12 and at most
10 000 sweeps.

    (a) 1 000 raw 30x10 frames, condition = 1, one launch       all three paths
    (b) one 30x10 frame per launch                               all three paths
    (c) one 6x3 frame per launch                                 all three paths
    (d) 64 raw frames of 24 measurements and 84 rows             belief propagation only (no other path takes them)
    (e) 64 raw frames of 48 measurements and 248 rows            belief propagation only

    python tools/bench_belief.py [--steps 30] [--warmup 5] [--out profiles/belief_bench.json]

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "belief_bench.json"))
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
    K, TOL, MAX_ITER = 200, 1e-12, 10000

    def setup(frames, nL, nM):
        F, nR = len(frames), nL + nM
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        return dict(F=F, nR=nR, nM=nM, d_cost=t(np.concatenate(frames)), d_nL=t(np.full(F, nL, np.int32)),
                    d_nM=t(np.full(F, nM, np.int32)), d_nRow=t(np.full(F, nR, np.int32)),
                    d_coff=t(np.arange(F, dtype=np.int64) * nR * nM), d_poff=t(np.arange(F, dtype=np.int64) * nM * (nL + 1)),
                    d_probs=torch.zeros(F * nM * (nL + 1), dtype=torch.float64, device=dev),
                    d_perm=torch.zeros(F, dtype=torch.float64, device=dev), d_nf=torch.zeros(F, dtype=torch.int32, device=dev),
                    d_iters=torch.zeros(F, dtype=torch.int32, device=dev), d_resid=torch.zeros(F, dtype=torch.float64, device=dev))

    def timed(launch):
        for _ in range(args.warmup):
            launch()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
        for a, b in ev:
            a.record(tstream)
            launch()
            b.record(tstream)
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in ev)
        return dict(median_ms=float(np.median(ms)), min_ms=float(ms[0]), max_ms=float(ms[-1]), launches=len(ms))

    def belief(s):
        eng.reserve_belief(s["F"], s["nR"], s["nM"])
        torch.cuda.synchronize()
        r = timed(lambda: eng.belief_probs_dev(s["F"], s["nR"], s["nM"], s["d_nL"], s["d_nM"], s["d_cost"], s["d_coff"], s["d_probs"],
                                               s["d_poff"], s["d_iters"], s["d_resid"], condition=True, tol=TOL, max_iter=MAX_ITER,
                                               stream=stream, reserve=False))  # (reserved above: only the C entry between the events)
        it = s["d_iters"].cpu().numpy()
        assert (it > 0).all(), "a frame did not come back with a sweep count"
        r.update(sweeps_median=float(np.median(it)), sweeps_max=int(it.max()))
        return r

    def permanent(s):
        eng.reserve_permanent(s["F"], s["nR"], s["nM"])
        torch.cuda.synchronize()
        return timed(lambda: eng.permanent_probs_dev(s["F"], s["nR"], s["nM"], s["d_nL"], s["d_nM"], s["d_cost"], s["d_coff"],
                                                     s["d_probs"], s["d_poff"], s["d_perm"], condition=True, stream=stream,
                                                     reserve=False))

    def kbest(s):
        eng.reserve_assoc(s["F"], s["nR"], s["nM"], K)
        torch.cuda.synchronize()
        r = timed(lambda: eng.assoc_probs_dev(s["F"], s["nR"], s["nM"], s["d_nL"], s["d_nM"], s["d_nRow"], s["d_cost"], s["d_coff"],
                                              K, s["d_probs"], s["d_poff"], s["d_nf"], condition=True, stream=stream))
        assert (s["d_nf"].cpu().numpy() >= 0).all(), "a frame did not fit the fused association kernel"
        return r

    c5 = wl.kitti_like_frames(1000, nL=20, nM=10)
    res = {"tool": "tools/bench_belief.py", "device": torch.cuda.get_device_name(0), "k": K, "tol": TOL, "max_iter": MAX_ITER,
           "steps": args.steps, "library": os.environ.get("KBEST_LIB", "libkbest_amd.so"), "warmup": args.warmup, "cases": {}}
    cases = (("a_1000x30x10", setup(c5, 20, 10)), ("b_1x30x10", setup(c5[:1], 20, 10)),
             ("c_1x6x3", setup(wl.kitti_like_frames(1, nL=6, nM=3), 6, 3)))
    for name, s in cases:
        bp, p, kb = belief(s), permanent(s), kbest(s)
        res["cases"][name] = dict(belief=bp, permanent=p, kbest200=kb, ratio_belief_to_kbest200=bp["median_ms"] / kb["median_ms"],
                                  ratio_belief_to_permanent=bp["median_ms"] / p["median_ms"])
    for name, nL, nM in (("d_64x84x24", 60, 24), ("e_64x248x48", 200, 48)):
        res["cases"][name] = dict(belief=belief(setup(wl.kitti_like_frames(64, nL=nL, nM=nM), nL, nM)))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
