"""CPU: the index arithmetic of the asynchronous exact hybrid entry (kbest_hybrid_frontier_probs_batch_f64_dev) before any GPU run --
kbest_hybrid.hip's gather and scatter kernels compiled for the host (tests/cpp/hybrid_dev_host.cpp: a stand-alone program under
AddressSanitizer and UBSan, exact-size heap buffers, nothing loaded into python) on descriptors, labels, row lists and per-cluster
blocks taken from the restatement frontier_check.hybrid_frontier_probs; the library exports the new symbols; without a GPU the
entry fails loudly.  Everything the scatter only moves, or adds in the stated order, must come back with equal bits."""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import cluster_check as cc
import frontier_check as fc
import hybrid_check as hc
import permanent_check as pc
import probabilisticsemslam_amd as pk
from probabilisticsemslam_amd import workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = (200, 40, 24, 24)  # README.md: F, nL, nM, side
NL, NM = SMALL[1], SMALL[2]
MAX_EXACT = 4


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def frames():
    return wl.scene_frames(*SMALL)[:16]


@functools.lru_cache(maxsize=None)
def restated(b, max_width, condition=True):
    """The restatement of frame b with k = 0 and no big-cluster tier.  Computed once; nobody changes it."""
    return fc.hybrid_frontier_probs(frames()[b], NL, NM, 0, condition=condition, max_exact=MAX_EXACT, max_big=0, max_width=max_width)


@functools.lru_cache(maxsize=None)
def partial(b, condition=True):
    """What the partial kernel leaves of frame b: (info, probs with the open columns 0.0, logPerm over the answered clusters in
    cluster order -- the loop of the restatement --, labels, the open clusters' dicts with the sweep's own outputs)."""
    X, A = hc.gated_block(frames()[b], NL, NM, condition)
    clusters, lab = cc.clusters_of(A)
    full = restated(b, fc.MAX_WIDTH, condition)
    assert full[1] == 0
    probs = full[0].copy()
    lp = 0.0
    for cols, rows in clusters:
        if len(cols) > MAX_EXACT:
            probs[cols] = 0.0
        else:
            lp = lp + float(np.log(pc.subset_sums(A[np.ix_(rows, cols)])[1]))
    opens = []
    for o in full[2]:
        p, lz, info, W = fc.frontier_cluster(o["block"], o["nL"], o["m"])  # (the kernel knows no max_width: the scatter applies it)
        assert info == 1 and [int(c) for c in np.flatnonzero(lab == o["root"])] == [int(c) for c in o["cols"]]
        opens.append(dict(o, sweep=(info, W, lz, p)))
    return len(clusters), probs, lp, lab.astype(np.int32), opens


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("hybrid_dev_host")
    (tmp / "hip").mkdir()
    (tmp / "hip" / "hip_runtime.h").write_text("")
    out = str(tmp / "hybrid_dev_host")
    csrc = os.path.join(ROOT, "probabilisticsemslam_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", str(tmp), "-I", os.path.join(ROOT, "include"), "-I", csrc, "-x", "c++",
                           os.path.join(ROOT, "tests", "cpp", "hybrid_dev_host.cpp"), "-o", out, "-lpthread"])
    return out


def run_host(exe, tmp_path, index, max_width, maxRawRow=NL + NM, maxCol=NM, condition=True, sweep=False):
    """The gather and the scatter on the frames `index` (indices into frames()).  Returns (list items, per frame (method,
    nFrontier, nOpen, first, logPerm, slice))."""
    src, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("5i", len(index), maxRawRow, maxCol, int(condition), max_width))
        for b in index:
            info, probs, lp, lab, opens = partial(b, condition)
            f.write(struct.pack("4i", NL, NM, info, len(opens)))
            f.write(np.ascontiguousarray(frames()[b], dtype=np.float64).tobytes() + probs.tobytes() + struct.pack("d", lp) + lab.tobytes())
            for o in opens:
                sinfo, W, lz, p = o["sweep"]
                f.write(struct.pack("4i", o["root"], o["m"], o["nL"], o["R"]) + np.asarray(o["rows"], dtype=np.int32).tobytes())
                f.write(struct.pack("2id", sinfo, W, lz) + np.ascontiguousarray(p, dtype=np.float64).tobytes())
                f.write(np.ascontiguousarray(o["block"], dtype=np.float64).tobytes())
    subprocess.check_call([exe, str(src), str(out)] + (["sweep"] if sweep else []))
    buf = out.read_bytes()
    (count,) = struct.unpack_from("i", buf, 0)
    at, items, res = 4, [], []
    for _ in range(count):
        items.append(struct.unpack_from("6i3q", buf, at))
        at += 48
    for _ in index:
        method, nfr, nopen, first, lp = struct.unpack_from("4id", buf, at)
        p = np.frombuffer(buf, dtype=np.float64, count=NM * (NL + 1), offset=at + 24).reshape(NM, NL + 1)
        at += 24 + 8 * NM * (NL + 1)
        res.append((method, nfr, nopen, first, lp, p))
    assert at == len(buf)
    return items, res


def check(index, items, res, max_width, maxRawRow=NL + NM, maxCol=NM, condition=True):
    k = 0
    for j, b in enumerate(index):
        want = restated(b, max_width, condition)
        method, nfr, nopen, first, lp, p = res[j]
        opens = partial(b, condition)[4]
        assert (method, nfr, nopen, first) == (want[1], want[3], len(opens), k), (b, res[j][:4])
        assert np.array_equal(bits(p), bits(want[0])), b
        assert bits(lp) == bits(want[6]) or (np.isnan(lp) and np.isnan(want[6])), (b, lp, want[6])
        sub = rows = prob = 0
        for o in opens:  # frame order, then label order; the running sums of hybrid_impl
            assert items[k] == (j, o["root"], o["m"], o["nL"], k, 1, j * (NL + NM) * NM + sub, j * maxCol * maxRawRow + prob,
                                j * maxRawRow + rows), (b, items[k])
            sub += (o["nL"] + o["m"]) * o["m"]
            rows += o["nL"]
            prob += o["m"] * (o["nL"] + 1)
            k += 1
    assert k == len(items)


def test_the_restatement_on_the_sixteen_frames():
    """What the other tests stand on: max_exact = 4 opens 1 .. 3 clusters of 5 .. 15 columns a frame, W <= 9, every frame answered
    at max_width = 16; at max_width = 5 frames 8, 10, 12 and 15 are refused and the other twelve answered."""
    opens = [restated(b, 16)[2] for b in range(16)]
    assert {len(o) for o in opens} == {1, 2, 3}
    assert min(o["m"] for f in opens for o in f) == 5 and max(o["m"] for f in opens for o in f) == 15
    assert max(o["W"] for f in opens for o in f) == 9
    assert [restated(b, 16)[1] for b in range(16)] == [0] * 16
    assert [b for b in range(16) if restated(b, 5)[1] == -1] == [8, 10, 12, 15]
    assert all(restated(b, 5)[1] == 0 for b in range(16) if b not in (8, 10, 12, 15))
    for b in (8, 10, 12, 15):
        assert not restated(b, 5)[0].any() and restated(b, 5)[3] == 0 and np.isnan(restated(b, 5)[6])


def test_gather_and_scatter_on_the_host_under_sanitizers(exe, tmp_path):
    """max_width = 16: all sixteen frames method 0, every slice, logPerm, method and nFrontier with the restatement's bits, and the
    list in hybrid_impl's order with its offsets."""
    index = list(range(16))
    items, res = run_host(exe, tmp_path, index, 16)
    check(index, items, res, 16)
    assert [r[0] for r in res] == [0] * 16


def test_the_refusal_mix_on_the_host(exe, tmp_path):
    """max_width = 5: exactly frames 8, 10, 12 and 15 are refused (zeros, nFrontier 0, logPerm NaN), the other twelve answered."""
    index = list(range(16))
    items, res = run_host(exe, tmp_path, index, 5)
    check(index, items, res, 5)
    assert [j for j, r in enumerate(res) if r[0] == -1] == [8, 10, 12, 15]
    for j in (8, 10, 12, 15):
        assert not res[j][5].any() and res[j][1] == 0 and np.isnan(res[j][4])


def test_raw_costs_on_the_host(exe, tmp_path):
    """condition = 0: logPerm takes m_k times the frame's block minimum, found by the scatter kernel itself."""
    index = [0, 3, 8, 15]
    items, res = run_host(exe, tmp_path, index, 16, condition=False)
    check(index, items, res, 16, condition=False)
    assert [r[0] for r in res] == [0] * 4 and all(frames()[b].min() != 0.0 for b in index)


def test_gather_sweep_and_scatter_end_to_end_on_the_host(exe, tmp_path):
    """The device path behind the partial kernel with nothing taken from the restatement but its inputs: the gather, then
    frontier_list_kernel itself on the gathered list (two workgroups, slots of the default size), then the scatter, raw costs.
    Tolerances of tests/test_frontier_cpu.py: 1e-12 on the probabilities, 1e-12 relative on logPerm; the rest equal."""
    index = [0, 8, 15]
    for max_width, refused in ((16, []), (5, [2])):  # (raw, frame 15 has a cluster of W > 5; frames 0 and 8 do not)
        items, res = run_host(exe, tmp_path, index, max_width, condition=False, sweep=True)
        assert [j for j, b in enumerate(index) if restated(b, max_width, False)[1] == -1] == refused
        worst = worst_lp = 0.0
        for j, b in enumerate(index):
            want = restated(b, max_width, False)
            method, nfr, nopen, first, lp, p = res[j]
            assert (method, nfr, nopen) == (want[1], want[3], len(partial(b, False)[4])), (b, res[j][:4])
            worst = max(worst, np.abs(p - want[0]).max())
            if method == 0:
                worst_lp = max(worst_lp, abs(lp - want[6]) / max(1.0, abs(want[6])))
                assert np.abs(p.sum(axis=1) - 1.0).max() <= 1e-12
            else:
                assert np.isnan(lp) and not p.any()
        print(f"max_width {max_width}: probabilities {worst:.3g}, logPerm {worst_lp:.3g}")
        assert [j for j, r in enumerate(res) if r[0] == -1] == refused
        assert worst <= 1e-12 and worst_lp <= 1e-12


def test_more_frames_than_one_workgroup_of_the_gather(exe, tmp_path):
    """260 frames (the sixteen, again and again, reversed): the gather's second workgroup starts behind the clusters of the first
    256 frames, and larger strides than the frames need."""
    index = [15 - (j % 16) for j in range(260)]
    items, res = run_host(exe, tmp_path, index, 16, maxRawRow=NL + NM + 3, maxCol=NM + 5)
    check(index, items, res, 16, maxRawRow=NL + NM + 3, maxCol=NM + 5)


def test_more_frames_than_the_grid_of_the_scatter(exe, tmp_path):
    """4 100 frames (the sixteen in an order that does not repeat every 256 frames): the scatter's launcher caps its grid at 4 096
    workgroups, so frames 4 096 .. 4 099 are the second pass of its frame loop, on the ctl, colOf and waveMin the first pass left;
    the gather runs seventeen workgroups.  Raw costs at max_width = 5: workgroups 2 and 3 take a refused frame (10, 15: zeros, no
    barrier between reading ctl and the end of the pass) and then an answered one (1, 6: colOf, and the block minimum through
    waveMin) -- the pair of passes that the barrier at the end of the loop keeps apart."""
    index = [(5 * j + j // 16 + 3 * (j // 256) + 7 * (j // 4096)) % 16 for j in range(4100)]
    assert index[:240] != index[256:496] and index[:4] == [0, 5, 10, 15] and index[4096:] == [7, 12, 1, 6]
    assert [restated(b, 5, False)[1] for b in (10, 15, 1, 6)] == [-1, -1, 0, 0]
    items, res = run_host(exe, tmp_path, index, 5, condition=False)
    check(index, items, res, 5, condition=False)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pk.lib_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "probabilisticsemslam_amd", "csrc")])
    return pk.load_library()


def test_library_exports_hybrid_dev_entries(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pk.lib_path()], text=True)
    from probabilisticsemslam_amd import engine
    for sym in ("kbest_reserve_hybrid_dev", "kbest_hybrid_frontier_probs_batch_f64_dev"):
        assert sym in engine.C_ABI_SYMBOLS and f" T {sym}\n" in out and hasattr(lib, sym), sym
    for name in ("reserve_hybrid_dev", "hybrid_frontier_probs_dev"):
        assert callable(getattr(pk.KBestEngine, name)), name
    header = open(os.path.join(ROOT, "include", "kbest_c.h")).read()
    assert "int kbest_reserve_hybrid_dev(kbest_ctx *ctx, int B, int maxRawRow, int maxCol);" in header
    assert "int kbest_hybrid_frontier_probs_batch_f64_dev(" in header


def test_hybrid_dev_without_gpu_fails_loudly(lib):
    if lib.kbest_device_count() > 0:
        return  # (a GPU is present: tests/test_gpu_hybrid_dev.py has the rest)
    with pytest.raises(pk.KBestError):
        pk.KBestEngine(0).reserve_hybrid_dev(1, NL + NM, NM)
