"""HIP-event times of the clustered exact association probabilities (kbest_clustered_probs_batch_f64_dev) beside the whole-frame
exact entry (kbest_permanent_probs_batch_f64_dev) and the belief entry (kbest_belief_probs_batch_f64_dev, tol 1e-12), both sides
in ONE process and run, alternating, warmed up; buffers resident in HBM, raw blocks with condition = 1.

    (a) 1 000 kitti_like_frames 30x10 (one cluster each: the price of labelling)    against the exact entry
    (b) 1 000 scene frames (20 landmarks, 10 measurements, side 12)                  against the exact entry
    (c) one such frame per call                                                      against the exact entry
    (d) 256 scene frames (60, 40, 30)                                                against the belief entry
    (e) 64 scene frames (200, 128, 60)                                               against the belief entry

Per case also the operation counts sum_k R_k 2^m_k m_k (clustered) and R 2^M M (whole frame), computed from the frames' shapes
after the gate, and the number of refused frames.

    python tools/bench_clustered.py [--steps 30] [--warmup 5] [--only a,b,...] [--out profiles/clustered_bench.json]

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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def operation_counts(frames, nL, nM):
    """(sum over the frames of sum_k R_k 2^m_k m_k, of R 2^M M): the conditioned block's toProbs matrix, its clusters."""
    import cluster_check as cc
    import oracle_lib as ol
    clustered = whole = 0.0
    for f in frames:
        cond, idx = ol.condition_costs(f, nL + nM, nM)
        a, b = cc.operation_counts(cond, len(idx) - nM, nM)
        clustered += a
        whole += b
    return clustered, whole


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="a,b,c,d,e")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clustered_bench.json"))
    args = ap.parse_args()
    import torch  # torch first: its copy of the HIP runtime is the one the process loads (tests/conftest.py)
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    import probabilisticsemslam_amd as pk
    from probabilisticsemslam_amd import workloads as wl
    eng = pk.KBestEngine(0)
    tstream = torch.cuda.Stream(device=dev)
    stream = tstream.cuda_stream
    TOL, MAX_ITER = 1e-12, 10000

    def setup(frames, nL, nM):
        F, nR = len(frames), nL + nM
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        return dict(F=F, nR=nR, nM=nM, d_cost=t(np.concatenate(frames)), d_nL=t(np.full(F, nL, np.int32)),
                    d_nM=t(np.full(F, nM, np.int32)), d_coff=t(np.arange(F, dtype=np.int64) * nR * nM),
                    d_poff=t(np.arange(F, dtype=np.int64) * nM * (nL + 1)),
                    d_probs=torch.zeros(F * nM * (nL + 1), dtype=torch.float64, device=dev),
                    d_perm=torch.zeros(F, dtype=torch.float64, device=dev), d_info=torch.zeros(F, dtype=torch.int32, device=dev),
                    d_maxc=torch.zeros(F, dtype=torch.int32, device=dev), d_iters=torch.zeros(F, dtype=torch.int32, device=dev),
                    d_resid=torch.zeros(F, dtype=torch.float64, device=dev))

    def clustered(s):
        return lambda: eng.clustered_probs_dev(s["F"], s["nR"], s["nM"], s["d_nL"], s["d_nM"], s["d_cost"], s["d_coff"], s["d_probs"],
                                               s["d_poff"], s["d_perm"], s["d_info"], s["d_maxc"], condition=True, stream=stream,
                                               reserve=False)

    def permanent(s):
        return lambda: eng.permanent_probs_dev(s["F"], s["nR"], s["nM"], s["d_nL"], s["d_nM"], s["d_cost"], s["d_coff"], s["d_probs"],
                                               s["d_poff"], s["d_perm"], condition=True, stream=stream, reserve=False)

    def belief(s):
        return lambda: eng.belief_probs_dev(s["F"], s["nR"], s["nM"], s["d_nL"], s["d_nM"], s["d_cost"], s["d_coff"], s["d_probs"],
                                            s["d_poff"], s["d_iters"], s["d_resid"], condition=True, tol=TOL, max_iter=MAX_ITER,
                                            stream=stream, reserve=False)

    def timed_pair(one, two):
        """Both launches alternating in the same loop: warm-up, then `steps` event pairs each."""
        for _ in range(args.warmup):
            one()
            two()
        torch.cuda.synchronize()
        ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
              for _ in range(2)]
        for i in range(args.steps):
            for j, launch in enumerate((one, two)):
                a, b = ev[j][i]
                a.record(tstream)
                launch()
                b.record(tstream)
        torch.cuda.synchronize()
        out = []
        for j in range(2):
            ms = sorted(a.elapsed_time(b) for a, b in ev[j])
            out.append(dict(median_ms=float(np.median(ms)), min_ms=float(ms[0]), max_ms=float(ms[-1]), launches=len(ms)))
        return out

    res = {"tool": "tools/bench_clustered.py", "device": torch.cuda.get_device_name(0), "tol": TOL, "max_iter": MAX_ITER,
           "steps": args.steps, "warmup": args.warmup, "cases": {}}
    c5 = wl.kitti_like_frames(1000, nL=20, nM=10)
    sc = wl.scene_frames(1000, 20, 10, 12)
    cases = {"a": ("a_1000_c5_30x10", c5, 20, 10, "permanent"), "b": ("b_1000_scene_20+10", sc, 20, 10, "permanent"),
             "c": ("c_1_scene_20+10", sc[:1], 20, 10, "permanent"),
             "d": ("d_256_scene_60+40", None, 60, 40, "belief"), "e": ("e_64_scene_200+128", None, 200, 128, "belief")}
    for key in args.only.split(","):
        name, frames, nL, nM, other = cases[key]
        if frames is None:
            frames = wl.scene_frames(256, 60, 40, 30) if key == "d" else wl.scene_frames(64, 200, 128, 60)
        s = setup(frames, nL, nM)
        eng.reserve_clustered(s["F"], s["nR"], s["nM"])
        if other == "permanent":
            eng.reserve_permanent(s["F"], s["nR"], s["nM"])
        else:
            eng.reserve_belief(s["F"], s["nR"], s["nM"])
        torch.cuda.synchronize()
        tc, to = timed_pair(clustered(s), (permanent if other == "permanent" else belief)(s))
        clustered(s)()
        torch.cuda.synchronize()
        info = s["d_info"].cpu().numpy()
        ops_c, ops_w = operation_counts(frames, nL, nM)
        res["cases"][name] = {"frames": s["F"], "clustered": tc, other: to, "ratio_clustered_to_" + other: tc["median_ms"] / to["median_ms"],
                              "grid": eng.last_clustered_grid(), "refused": int((info < 0).sum()), "infeasible": int((info == 0).sum()),
                              "clusters_median": float(np.median(info[info > 0])) if (info > 0).any() else 0.0,
                              "ops_clustered": ops_c, "ops_whole_frame": ops_w}
        if other == "belief":
            it = s["d_iters"].cpu().numpy()
            res["cases"][name]["belief"].update(sweeps_median=float(np.median(it)), sweeps_max=int(it.max()))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
