"""CPU: the index arithmetic of the asynchronous exact hybrid draws (kbest_hybrid_frontier_sample_assoc_batch_f64_dev) before any GPU
run -- the gather of kbest_hybrid.hip and the key and join kernels of kbest_hybrid_sample.hip compiled for the host
(tests/cpp/hybrid_sample_dev_host.cpp: a stand-alone program under AddressSanitizer and UBSan, exact-size heap buffers, nothing
loaded into python) on descriptors, labels, row lists, the clustered sampler's draws and the list sampler's per-cluster outputs taken
from the restatements frontier_check.hybrid_frontier_probs and frontier_sample_check.hybrid_frontier_sample_assoc / open_row_keys /
sample_cluster; the library exports the new symbols; without a GPU the entry fails loudly.  Everything the kernels only move, or
add in the stated order, must come back with equal bits."""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import cluster_sample_check as csc
import frontier_check as fc
import frontier_sample_check as fsc
import probabilisticsemslam_amd as pk
import test_hybrid_dev_cpu as hd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NL, NM = hd.NL, hd.NM
MAX_EXACT = hd.MAX_EXACT
N_SAMPLE = 5
SEED = fsc.SEED
REFUSED_AT_5 = [8, 10, 12, 15]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_doubles(a, b):
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


@functools.lru_cache(maxsize=None)
def draws(b, max_width, condition=True, max_exact=MAX_EXACT):
    """The restatement of frame b of the sixteen, frame key b.  Computed once; nobody changes it."""
    return fsc.hybrid_frontier_sample_assoc(hd.frames()[b], NL, NM, N_SAMPLE, SEED, condition, b, 0, max_exact, max_width)


@functools.lru_cache(maxsize=None)
def sampled(b, condition=True):
    """What the two samplers leave of frame b at max_exact = 4: (assign with the open columns -1 and logProb over the small clusters
    in label order from 0.0 -- the clustered sampler's second instantiation; per open cluster (o, keys, assignLocal, logTerm, logZ,
    info, W) -- the list sampler, which knows no max_width)."""
    full = draws(b, fc.MAX_WIDTH, condition)
    assert full.method == 0
    parts, _ = csc.cluster_parts(hd.frames()[b], NL, NM, condition)
    roots = {o["root"] for o in full.opens}
    assign = np.full((N_SAMPLE, NM), -1, np.int32)
    logp = np.zeros(N_SAMPLE)
    for p in parts:
        if int(p.cols[0]) not in roots:
            prod, _ = csc.walk_cluster(p, N_SAMPLE, SEED, b, 0, assign)
            logp = logp + (np.log(prod) - np.log(p.Z))
    opens, total = [], logp
    for o in full.opens:
        keys = fsc.open_row_keys(o, NL).astype(np.int32)
        a, lt, lz, info, W, _ = fsc.sample_cluster(o["block"], o["nL"], o["m"], keys, N_SAMPLE, SEED, b, 0)
        assert info == 1 and np.array_equal(a, o["assign_local"]) and same_doubles(lt, o["logterm"])
        opens.append((o, keys, a.astype(np.int32), lt, lz, info, W))
        total = total + lt
    assert same_doubles(total, full.logp)  # (the additions of the join, in its order)
    return assign, logp, opens


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("hybrid_sample_dev_host")
    (tmp / "hip").mkdir()
    (tmp / "hip" / "hip_runtime.h").write_text("")
    out = str(tmp / "hybrid_sample_dev_host")
    csrc = os.path.join(ROOT, "probabilisticsemslam_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", str(tmp), "-I", os.path.join(ROOT, "include"), "-I", csrc, "-x", "c++",
                           os.path.join(ROOT, "tests", "cpp", "hybrid_sample_dev_host.cpp"), "-o", out, "-lpthread"])
    return out


def run_host(exe, tmp_path, index, max_width, maxRawRow=NL + NM, maxCol=NM, condition=True, sampler=False, nothing_open=False):
    """The gather, the key kernel and the join on the frames `index` (indices into the sixteen).  Returns (list items with their
    keys, per frame (method, nFrontier, nOpen, first, logPerm, assign, logProb))."""
    src, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("6iQ", len(index), maxRawRow, maxCol, int(condition), max_width, N_SAMPLE, SEED))
        for b in index:
            info, _, lp, lab, _ = hd.partial(b, condition)
            if nothing_open:  # max_exact = 16: the clustered sampler's own draws and sum, the partial kernel's sum never read
                d = draws(b, fc.MAX_WIDTH, condition, 16)
                assign, logp, opens, lp, draw_lp = d.assign, d.logp, [], -5.0, d.logperm
            else:
                assign, logp, opens = sampled(b, condition)
                draw_lp = -5.0
            f.write(struct.pack("4iQ", NL, NM, info, len(opens), b))
            f.write(np.ascontiguousarray(hd.frames()[b], dtype=np.float64).tobytes() + struct.pack("2d", lp, draw_lp) + lab.tobytes())
            f.write(np.ascontiguousarray(assign, dtype=np.int32).tobytes() + np.ascontiguousarray(logp, dtype=np.float64).tobytes())
            for o, _, a, lt, lz, sinfo, W in opens:
                f.write(struct.pack("4i", o["root"], o["m"], o["nL"], o["R"]) + np.asarray(o["rows"], dtype=np.int32).tobytes())
                f.write(struct.pack("2id", sinfo, W, lz) + np.ascontiguousarray(a).tobytes() + np.ascontiguousarray(lt).tobytes())
                f.write(np.ascontiguousarray(o["block"], dtype=np.float64).tobytes())
    subprocess.check_call([exe, str(src), str(out)] + (["sampler"] if sampler else []))
    buf = out.read_bytes()
    (count,) = struct.unpack_from("i", buf, 0)
    at, items, res = 4, [], []
    for _ in range(count):
        it = struct.unpack_from("6i4qQ", buf, at)
        at += 64
        keys = None
        if it[5]:
            keys = np.frombuffer(buf, dtype=np.int32, count=it[3] + it[2], offset=at)
            at += 4 * (it[3] + it[2])
        items.append((it, keys))
    for _ in index:
        method, nfr, nopen, first, lp = struct.unpack_from("4id", buf, at)
        asg = np.frombuffer(buf, dtype=np.int32, count=N_SAMPLE * NM, offset=at + 24).reshape(N_SAMPLE, NM)
        logp = np.frombuffer(buf, dtype=np.float64, count=N_SAMPLE, offset=at + 24 + 4 * N_SAMPLE * NM)
        at += 24 + 4 * N_SAMPLE * NM + 8 * N_SAMPLE
        res.append((method, nfr, nopen, first, lp, asg, logp))
    assert at == len(buf)
    return items, res


def check(index, items, res, max_width, maxRawRow=NL + NM, maxCol=NM, condition=True):
    k = 0
    for j, b in enumerate(index):
        want = draws(b, max_width, condition)
        method, nfr, nopen, first, lp, asg, logp = res[j]
        opens = sampled(b, condition)[2]
        assert (method, nfr, nopen, first) == (want.method, want.nfrontier, len(opens), k), (b, res[j][:4])
        assert np.array_equal(asg, want.assign), b
        assert same_doubles(logp, want.logp), (b, logp, want.logp)
        assert same_doubles(lp, want.logperm), (b, lp, want.logperm)
        sub = rows = cols = 0
        for o, keys, *_ in opens:  # frame order, then label order; the running sums of the host loop, from the frame's own places
            it, got = items[k]
            assert it == (j, o["root"], o["m"], o["nL"], o["R"], 1, j * (NL + NM) * NM + sub, j * maxRawRow + rows,
                          (j * maxCol + cols) * N_SAMPLE, k * N_SAMPLE, b), (b, it)
            assert np.array_equal(got, keys) and np.array_equal(keys[: o["R"]], o["all_rows"]), (b, got, keys)
            sub += (o["nL"] + o["m"]) * o["m"]
            rows += o["nL"] + o["m"]
            cols += o["m"]
            k += 1
    assert k == len(items)


def test_the_restatement_on_the_sixteen_frames():
    """What the other tests stand on: max_exact = 4 opens 1 .. 3 clusters a frame, every frame drawn at max_width = 16; at
    max_width = 5 frames 8, 10, 12 and 15 are refused (-1s, NaNs) and the other twelve drawn, with the draws of max_width = 16."""
    for b in range(16):
        d = draws(b, 16)
        assert d.method == 0 and 1 <= d.nopen == d.nfrontier <= 3 and (d.assign >= 0).all() and np.isfinite(d.logp).all()
        d5 = draws(b, 5)
        if b in REFUSED_AT_5:
            assert d5.method == -1 and (d5.assign == -1).all() and np.isnan(d5.logp).all() and np.isnan(d5.logperm) and d5.nfrontier == 0
        else:
            assert d5.method == 0 and np.array_equal(d5.assign, d.assign) and same_doubles(d5.logp, d.logp)
    # the open clusters hold miss rows (keys >= nL behind the landmark rows) for the key kernel to find
    opens = [o for b in range(16) for o in draws(b, 16).opens]
    assert all(o["R"] > o["nL"] for o in opens)
    assert all((o["all_rows"][o["nL"]:] >= NL).all() and (o["all_rows"][: o["nL"]] < NL).all() for o in opens)


@pytest.mark.parametrize("condition", [True, False])
def test_gather_keys_and_join_on_the_host_under_sanitizers(exe, tmp_path, condition):
    """max_width = 16: all sixteen frames method 0; the row keys equal open_row_keys (condition = False: the gate on raw costs),
    the list in the host loop's order with its offsets, assign, method and nFrontier equal, logProb and logPerm with the
    restatement's bits (condition = False: m_k times the frame's block minimum, found by the join kernel itself)."""
    index = list(range(16))
    items, res = run_host(exe, tmp_path, index, 16, condition=condition)
    check(index, items, res, 16, condition=condition)
    assert [r[0] for r in res] == [0] * 16
    if not condition:
        assert all(hd.frames()[b].min() != 0.0 for b in index)


@pytest.mark.parametrize("condition", [True, False])
def test_the_refusal_mix_on_the_host(exe, tmp_path, condition):
    """max_width = 5, condition True: exactly frames 8, 10, 12 and 15 are refused (-1s, NaNs, nFrontier 0, logPerm NaN), the other
    twelve drawn.  On raw costs the restatement says which."""
    index = list(range(16))
    items, res = run_host(exe, tmp_path, index, 5, condition=condition)
    check(index, items, res, 5, condition=condition)
    refused = [j for j, r in enumerate(res) if r[0] == -1]
    assert refused == [b for b in index if draws(b, 5, condition).method == -1] and refused
    if condition:
        assert refused == REFUSED_AT_5
    for j in refused:
        assert (res[j][5] == -1).all() and np.isnan(res[j][6]).all() and res[j][1] == 0 and np.isnan(res[j][4])


def test_nothing_open_on_the_host(exe, tmp_path):
    """Frames without an open cluster: the clustered sampler's draws and its own sum pass through the join untouched."""
    index = [0, 8, 15]
    items, res = run_host(exe, tmp_path, index, 16, nothing_open=True)
    assert items == []
    for j, b in enumerate(index):
        d = draws(b, 16, True, 16)
        assert res[j][:4] == (0, 0, 0, 0) and same_doubles(res[j][4], d.logperm)
        assert np.array_equal(res[j][5], d.assign) and same_doubles(res[j][6], d.logp)


def test_max_width_zero_refuses_every_frame_with_an_open_cluster(exe, tmp_path):
    index = [0, 8]
    items, res = run_host(exe, tmp_path, index, 0)
    for j in range(2):
        assert res[j][0] == -1 and res[j][1] == 0 and np.isnan(res[j][4]) and (res[j][5] == -1).all() and np.isnan(res[j][6]).all()


def test_gather_sampler_and_join_end_to_end_on_the_host(exe, tmp_path):
    """The device path behind the two clustered kernels with nothing taken from the restatement but its inputs: the gather, the key
    kernel, then frontier_sample_list_kernel itself on the gathered list (two workgroups, slots of the default size), then the
    join, raw costs.  The rules of tests/test_gpu_frontier_sample.py: the restatement's margin >= 1e-10 first, then assign exact
    and logProb within 1e-12; logPerm within 1e-12 relative."""
    index = [0, 8, 15]
    for max_width in (16, 5):
        items, res = run_host(exe, tmp_path, index, max_width, condition=False, sampler=True)
        worst = worst_lp = 0.0
        for j, b in enumerate(index):
            want = draws(b, max_width, False)
            method, nfr, nopen, first, lp, asg, logp = res[j]
            assert (method, nfr, nopen) == (want.method, want.nfrontier, want.nopen), (b, res[j][:4])
            assert np.array_equal(asg, want.assign), b
            if method == 0:
                assert want.margin >= 1e-10
                worst = max(worst, np.abs(logp - want.logp).max())
                worst_lp = max(worst_lp, abs(lp - want.logperm) / max(1.0, abs(want.logperm)))
            else:
                assert np.isnan(lp) and np.isnan(logp).all()
        print(f"max_width {max_width}: logProb {worst:.3g}, logPerm {worst_lp:.3g}")
        assert worst <= 1e-12 and worst_lp <= 1e-12


def test_more_frames_than_one_workgroup_of_the_gather(exe, tmp_path):
    """260 frames (the sixteen, again and again, reversed) and larger strides than the frames need: the places in the row keys,
    the local draws and the terms follow from the frame index and the list index."""
    index = [15 - (j % 16) for j in range(260)]
    items, res = run_host(exe, tmp_path, index, 16, maxRawRow=NL + NM + 3, maxCol=NM + 5)
    check(index, items, res, 16, maxRawRow=NL + NM + 3, maxCol=NM + 5)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pk.lib_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "probabilisticsemslam_amd", "csrc")])
    return pk.load_library()


def test_library_exports_hybrid_sample_dev_entries(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pk.lib_path()], text=True)
    from probabilisticsemslam_amd import engine
    for sym in ("kbest_reserve_hybrid_sample_dev", "kbest_hybrid_frontier_sample_assoc_batch_f64_dev"):
        assert sym in engine.C_ABI_SYMBOLS and f" T {sym}\n" in out and hasattr(lib, sym), sym
        assert getattr(lib, sym).argtypes is not None, sym
    assert len(lib.kbest_reserve_hybrid_sample_dev.argtypes) == 5
    assert len(lib.kbest_hybrid_frontier_sample_assoc_batch_f64_dev.argtypes) == 26
    for name in ("reserve_hybrid_sample_dev", "hybrid_frontier_sample_assoc_dev"):
        assert callable(getattr(pk.KBestEngine, name)), name
    header = open(os.path.join(ROOT, "include", "kbest_c.h")).read()
    assert "int kbest_reserve_hybrid_sample_dev(kbest_ctx *ctx, int B, int maxRawRow, int maxCol, int nSample);" in header
    assert "int kbest_hybrid_frontier_sample_assoc_batch_f64_dev(" in header


def test_hybrid_sample_dev_without_gpu_fails_loudly(lib):
    if lib.kbest_device_count() > 0:
        return  # (a GPU is present: tests/test_gpu_hybrid_sample_dev.py has the rest)
    with pytest.raises(pk.KBestError):
        pk.KBestEngine(0).reserve_hybrid_sample_dev(1, NL + NM, NM, N_SAMPLE)
