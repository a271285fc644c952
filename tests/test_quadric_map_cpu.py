"""CPU: exact getAssignmentProbs from quadrics against a map of any size (kbest_quadric_map.hip) before any GPU run -- the conditions
of the scenes the GPU tests stand on, from the numpy restatement alone; the passes over the map compiled for the host
(tests/cpp/quadric_map_host.cpp: a stand-alone program under AddressSanitizer and UBSan, -ffp-contract=off, exact-size heap buffers,
nothing loaded into python) on the smallest shapes at which they can go wrong, with the restatement's BITS for nKeep, rowIdx and the
compact block; the library exports the new symbols; without a GPU the entries fail loudly."""
import os
import struct
import subprocess

import numpy as np
import pytest

import probabilisticsemslam_amd as pk
import quadric_map_lib as qm
from quadric_map_lib import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = qm.TILE


# ---- 1. the inputs -------------------------------------------------------------------------------------------------------------------------
chain = qm.chain_restated


def test_conditions_of_the_chain_frames():
    """What tests/test_gpu_quadric_map.py stands on, recomputed: every frame keeps at most 256 of the 5 000 landmarks; at k = 0 at
    least one frame is answered by the frontier tier, at least one is all-exact without an open cluster, and at least one is refused
    and then answered at k = 50."""
    r0 = [chain(f, 0) for f in range(6)]
    kept = [len(r["rows"]) for r in r0]
    print("kept", kept, "method", [r["method"] for r in r0], "nFrontier", [r["nFrontier"] for r in r0],
          "maxCluster", [r["maxCluster"] for r in r0])
    assert max(kept) <= 256 and min(kept) >= 30
    assert any(r["method"] == 0 and r["nFrontier"] >= 1 for r in r0)
    assert any(r["method"] == 0 and not r["opens"] for r in r0)
    refused = [f for f in range(6) if r0[f]["method"] == -1]
    assert refused and all(chain(f, 50)["method"] in (1, 2) for f in refused)
    for r in r0:
        assert (np.diff(r["rows"]) > 0).all() and (r["method"] != 0 or np.abs(r["probs"].sum(axis=1) - 1.0).max() <= 1e-12)


def test_compact_path_has_the_bits_of_the_raw_path():
    """Compact block with condition = 0 against the raw block with condition = 1 (the parent's path), wherever the raw block is small
    enough to form: the six chain frames at k = 50 (k-best leg included) and eight frames of a map of 300 at k = 0."""
    mean, cov = qm.make_map(*qm.CHAIN["map"])
    cases = [(mean, cov, qm.chain_frame(f), qm.CHAIN["gate"], 50) for f in range(6)]
    m3, c3, small, gate3 = qm.parity_batch()
    cases += [(m3, c3, fr[2:], gate3, 0) for fr in small[:8]]
    for j, (lm, lc, (mm, mc), gate, k) in enumerate(cases):
        got = chain(j, 50) if j < 6 else qm.restated(lm, lc, mm, mc, gate, k=k)
        want = qm.restated_raw(lm, lc, mm, mc, gate, k=k)
        assert np.array_equal(bits(got["probs"]), bits(want[0])), j
        assert (got["method"], got["nFrontier"], got["maxCluster"], len(got["opens"])) == (want[1], want[3], want[5], len(want[2])), j
        assert bits(got["logPerm"]) == bits(want[6]) or (np.isnan(got["logPerm"]) and np.isnan(want[6])), j


def test_sparse_scenes_keep_a_few_dozen_rows():
    mean, cov = qm.make_map(1, 5000, 200.0, 3.0)
    mm, mc = qm.make_frame(300, mean, 24, 24, 1)
    r = qm.restated(mean, cov, mm, mc, 10.0)
    print("sparse: kept", len(r["rows"]), "method", r["method"])
    assert 1 <= len(r["rows"]) <= 64 and r["method"] == 0


# ---- 2. the passes over the map, compiled for the host -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("quadric_map_host")
    (tmp / "hip").mkdir()
    (tmp / "hip" / "hip_runtime.h").write_text("")
    out = str(tmp / "quadric_map_host")
    csrc = os.path.join(ROOT, "probabilisticsemslam_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-ffp-contract=off", "-I", str(tmp), "-I", os.path.join(ROOT, "include"), "-I", csrc, "-x", "c++",
                           os.path.join(ROOT, "tests", "cpp", "quadric_map_host.cpp"), "-o", out, "-lpthread"])
    return out


def run_host(exe, tmp_path, map_mean, map_cov, frames, gate, maxMap, maxKeep, maxCol):
    """frames: (landOff, nL, measMean, measCov).  Returns per frame (nKeep, nLh, costOff, cprobOff, rowIdx[maxKeep], the frame's
    stretch of the compact buffer) and the list of dense stretches (pad of 8, slice) with the last pad."""
    src, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("<5id", len(frames), maxMap, maxKeep, maxCol, len(map_mean), gate))
        f.write(np.ascontiguousarray(map_mean, dtype=np.float64).tobytes() + np.ascontiguousarray(map_cov, dtype=np.float64).tobytes())
        for off, nL, mm, mc in frames:
            f.write(struct.pack("<qii", off, nL, len(mm)))
            f.write(np.ascontiguousarray(mm, dtype=np.float64).tobytes() + np.ascontiguousarray(mc, dtype=np.float64).tobytes())
    subprocess.check_call([exe, str(src), str(out)])
    buf = out.read_bytes()
    at, res, stride = 0, [], (maxKeep + maxCol) * maxCol
    for _ in frames:
        nk, nlh, co, po = struct.unpack_from("<iiqq", buf, at)
        rows = np.frombuffer(buf, dtype=np.int32, count=maxKeep, offset=at + 24)
        cc = np.frombuffer(buf, dtype=np.float64, count=stride, offset=at + 24 + 4 * maxKeep)
        at += 24 + 4 * maxKeep + 8 * stride
        res.append((nk, nlh, co, po, rows, cc))
    dense = np.frombuffer(buf, dtype=np.float64, offset=at)
    return res, dense


def check_frame(j, res, dense, dense_at, map_mean, map_cov, frame, gate, maxKeep, maxCol):
    """Frame j of a run against the restatement; returns where the next frame's dense stretch begins."""
    off, nL, mm, mc = frame
    nM = len(mm)
    rows, cc, _ = qm.compact(map_mean[off:off + nL], map_cov[off:off + nL], mm, mc, gate)
    nk, nlh, co, po, got_rows, got_cc = res[j]
    assert (nk, nlh, co, po) == (len(rows), len(rows), j * (maxKeep + maxCol) * maxCol, j * maxCol * (maxKeep + 1)), (j, res[j][:4])
    assert np.array_equal(got_rows[:nk], rows) and (got_rows[nk:] == -77).all(), j
    assert np.array_equal(bits(got_cc[:cc.size]), bits(cc)), j
    assert (got_cc[cc.size:] == -7.0).all(), j
    # the expansion of compact probabilities that are their own index + 1
    cp = po + 1.0 + np.arange(nM * (nk + 1)).reshape(nM, nk + 1)
    want = qm.expand(cp, rows, nL)
    assert (dense[dense_at:dense_at + 8] == -5.0).all(), j
    got = dense[dense_at + 8:dense_at + 8 + want.size].reshape(nM, nL + 1)
    assert np.array_equal(bits(got), bits(want)), j
    return dense_at + 8 + want.size


def test_edge_shapes_on_the_host_under_sanitizers(exe, tmp_path):
    """One map, every frame a window of it: nL in {0, 1, T-1, T, T+1, 2T+3} x nM in {1, 128} with identity covariances, the kept rows
    exactly the first and the last landmark and the two either side of every tile boundary; nothing kept; cost 0 / 42 (kept: <=) /
    43 (dropped) in one column; two windows of a random map (the LDL^T solve on real covariances).  Bounds larger than any frame
    needs: maxMap four tiles, maxKeep 300, maxCol 128."""
    map_mean, map_cov, frames, gate = qm.edge_batch()
    res, dense = run_host(exe, tmp_path, map_mean, map_cov, frames, gate, 4 * T, 300, 128)
    dense_at = 0
    for j, fr in enumerate(frames):
        dense_at = check_frame(j, res, dense, dense_at, map_mean, map_cov, fr, gate, 300, 128)
    assert dense_at + 8 == dense.size and (dense[dense_at:] == -5.0).all()
    kept = [r[0] for r in res]
    print("kept rows", kept)
    assert kept[:12] == [0, 0, 1, 1, 2, 2, 2, 2, 3, 3, 6, 6] and kept[12] == 0 and kept[13] == 2
    assert res[13][4][:2].tolist() == [0, 1]           # cost 0 and cost 42 kept, 43 dropped
    assert res[10][4][:6].tolist() == [0, T - 1, T, 2 * T - 1, 2 * T, 2 * T + 2]
    assert min(kept[14:]) >= 20                        # the random windows keep a real set


def test_full_refused_and_untaken_frames_on_the_host(exe, tmp_path):
    """maxKeep = 8: a frame that keeps exactly 8 rows is answered; one that keeps 9 has the true nKeep, nLh = -1, nothing in its
    rowIdx and compact block, zeros in its dense slice; a frame with nL > maxMap and one with nM > maxCol are not touched at all."""
    map_mean, map_cov, frames, gate = qm.limit_batch()
    res, dense = run_host(exe, tmp_path, map_mean, map_cov, frames, gate, 300, 8, 4)
    at = check_frame(0, res, dense, 0, map_mean, map_cov, frames[0], gate, 8, 4)
    assert res[0][0] == 8
    nk, nlh, _, _, rows, cc = res[1]
    assert (nk, nlh) == (9, -1) and (rows == -77).all() and (cc == -7.0).all()
    assert (dense[at:at + 8] == -5.0).all() and not dense[at + 8:at + 8 + 3 * 301].any()
    at += 8 + 3 * 301
    for j in (2, 3):
        nk, nlh, _, _, rows, cc = res[j]
        assert (nk, nlh) == (-77, -1) and (rows == -77).all() and (cc == -7.0).all(), j
    assert (dense[at:] == -5.0).all() and dense.size - at == 8 + 2 * 302 + 8 + 5 * 11 + 8


# ---- 3. the library ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pk.lib_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "probabilisticsemslam_amd", "csrc")])
    return pk.load_library()


def test_library_exports_quadric_map_entries(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pk.lib_path()], text=True)
    from probabilisticsemslam_amd import engine
    for sym in ("kbest_reserve_quadric_map_dev", "kbest_quadric_map_probs_batch_f64_dev", "kbest_quadric_map_probs_batch_f64"):
        assert sym in engine.C_ABI_SYMBOLS and f" T {sym}\n" in out and hasattr(lib, sym), sym
    for name in ("reserve_quadric_map_dev", "quadric_map_probs_dev", "quadric_map_probs"):
        assert callable(getattr(pk.KBestEngine, name)), name
    header = open(os.path.join(ROOT, "include", "kbest_c.h")).read()
    assert "int kbest_reserve_quadric_map_dev(kbest_ctx *ctx, int B, int maxMap, int maxKeep, int maxCol);" in header
    assert "int kbest_quadric_map_probs_batch_f64_dev(" in header and "int kbest_quadric_map_probs_batch_f64(" in header
    assert engine.KBEST_QUADRIC_MAP_TILE == T and f"#define KBEST_QUADRIC_MAP_TILE {T}" in header


def test_quadric_map_without_gpu_fails_loudly(lib):
    if lib.kbest_device_count() > 0:
        return  # (a GPU is present: tests/test_gpu_quadric_map.py has the rest)
    with pytest.raises(pk.KBestError):
        pk.KBestEngine(0).reserve_quadric_map_dev(1, 1000, 64, 24)
