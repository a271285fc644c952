"""bench.py's plain line and --dump-outputs: a plain run times exactly --steps steps and carries the headline only; what it dumps
is what the timed path computed, checked against the checker on a few matrices / frames."""
import importlib.util
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol
from probabilisticsemslam_amd import workloads as wl

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"}
FULL_ONLY = {"parity_prune_vs_noprune", "launch", "roofline", "issue", "value_host_inclusive", "cpu_baseline", "configs"}


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("cfg", ["c2", "c3", "c4", "w128"])
def test_dense_dump_fits_and_is_a_fixed_sample(cfg):
    bench = _bench_module()
    B, N, M, k, _ = wl.DENSE_CONFIGS[cfg]
    rng = np.random.default_rng(5)
    m = dict(B=B, N=N, M=M, k=k, nf=np.full(B, k, np.int32), g=rng.random((B, k)),
             r4c=rng.integers(0, N, (B, k, M), dtype=np.int32), c4r=rng.integers(0, M, (B, k, N), dtype=np.int32))
    m["nf"][:: 7] = 3
    out = bench.dense_outputs(m)
    again = bench.dense_outputs(m)
    assert sum(a.nbytes for a in out.values()) <= bench.DUMP_BYTES
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert all(np.array_equal(out[n], again[n]) for n in out)
    idx = out["matrix_index"].astype(np.int64)
    assert (np.diff(idx) > 0).all() and idx[-1] < B
    for j in (0, len(idx) - 1):
        b, n = idx[j], int(m["nf"][idx[j]])
        assert out["nf"][j] == n
        assert np.array_equal(out["gain"][j, :n], m["g"][b, :n]) and (out["gain"][j, n:] == 0).all()
        assert np.array_equal(out["row4col"][j, :n], m["r4c"][b, :n]) and (out["row4col"][j, n:] == 0).all()
        assert np.array_equal(out["col4row"][j, :n], m["c4r"][b, :n]) and (out["col4row"][j, n:] == 0).all()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _plain_run(tmp_path, *args, gpus=1, **env_extra):
    d = tmp_path / "out"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT",
                                                             "KBEST_BENCH_SELF_LAUNCH", "KBEST_BENCH_FORCE_DIST", "KBEST_BENCH_BACKEND")}
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--dump-outputs", str(d)] + list(args),
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-1500:]
    out = json.loads(lines[0])
    assert HEADLINE <= out.keys() and not (FULL_ONLY & out.keys())
    assert out["ms_per_step"] > 0 and out["value"] > 0 and out["higher_is_better"] is True and out["dtype"] == "f64"
    dump = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert all(a.dtype in (np.float32, np.float64) for a in dump.values())
    assert sum((d / f).stat().st_size for f in os.listdir(d)) < 64_000_000
    return out, dump


@pytest.mark.gpu
def test_plain_c4_line_and_dump_match_the_checker(tmp_path):
    out, dump = _plain_run(tmp_path, "--steps", "3", "--warmup", "1")
    assert out["steps"] == 3 and out["warmup"] == 1
    assert set(dump) == {"nf", "gain", "row4col", "col4row", "matrix_index"}
    _, N, M, k, seed = wl.DENSE_CONFIGS["c4"]
    idx = dump["matrix_index"].astype(np.int64)
    assert out["value"] > 0 and len(idx) == len(dump["nf"]) == dump["gain"].shape[0]
    for j in (0, len(idx) // 2, len(idx) - 1):
        onf, or4c, oc4r, og, _ = ol.orc_kbest_batch(wl.dense_batch(1, N, M, seed, first=int(idx[j])), N, M, k)
        n = int(onf[0])
        assert dump["nf"][j] == n
        assert (bits(dump["gain"][j, :n]) == bits(og[0, :n])).all()
        assert (dump["row4col"][j, :n] == or4c[0, :n]).all() and (dump["col4row"][j, :n] == oc4r[0, :n]).all()


@pytest.mark.gpu
def test_plain_c5_line_and_dump_match_the_checker(tmp_path):
    out, dump = _plain_run(tmp_path, "--config", "c5", "--steps", "2", "--warmup", "1")
    assert out["steps"] == 2
    F, nL, nM, k = 1000, 20, 10, 200
    assert set(dump) == {"probs", "nf"} and dump["probs"].shape == (F, nM, nL + 1) and dump["nf"].shape == (F,)
    frames = wl.kitti_like_frames(3, nL=nL, nM=nM)
    for i, f in enumerate(frames):
        c, ridx = ol.condition_costs(f, nL + nM, nM)
        q, _ = ol.assignment_prob(c, len(ridx) - nM, nM, k)
        cl = len(ridx) - nM
        ref = np.zeros((nM, nL + 1))
        ref[:, np.asarray(ridx[:cl], dtype=np.int64)] = q[:, :cl]
        ref[:, nL] = q[:, cl]
        assert np.abs(dump["probs"][i] - ref).max() <= 1e-12, i


@pytest.mark.gpu
def test_plain_world2_over_gloo_dumps_what_one_gpu_computes(tmp_path):
    """A plain run of the world > 1 path (two gloo ranks on GPU 0, weak scaling, int8 tables in the packed slices): headline only,
    and rank 0's dump is the one-GPU run's -- rank 0 solves the same first matrices of the seeded stream."""
    one, d1 = _plain_run(tmp_path / "one", "--steps", "2", "--warmup", "1")
    two, d2 = _plain_run(tmp_path / "two", "--steps", "2", "--warmup", "1", gpus=2, KBEST_BENCH_BACKEND="gloo",
                         MASTER_PORT=str(_free_port()))
    assert two["n_gpus"] == 2 and two["steps"] == 2 and "collective" not in two
    assert d1.keys() == d2.keys() and all(np.array_equal(d1[n], d2[n]) for n in d1)
