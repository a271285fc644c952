"""CPU: joint associations from quadrics against a map of any size (kbest_quadric_map_sample.hip) before any GPU run -- the
conditions of the scenes the GPU tests stand on, from the numpy restatement alone (tests/quadric_map_sample_lib.py); the kernel that
maps compact rows to raw rows compiled for the host (tests/cpp/quadric_map_sample_host.cpp: a stand-alone program under
AddressSanitizer and UBSan, exact-size heap buffers, nothing loaded into python) against the restated map; the statistical check of
the GPU test on the restatement's own draws; the library exports the new symbols; without a GPU the entries fail loudly."""
import os
import struct
import subprocess

import numpy as np
import pytest

import probabilisticsemslam_amd as pk
import quadric_map_lib as qm
import quadric_map_sample_lib as qs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "probabilisticsemslam_amd", "csrc")


# ---- 1. the scenes -----------------------------------------------------------------------------------------------------------------------
def test_conditions_of_the_chain_frames():
    """What tests/test_gpu_quadric_map_sample.py stands on: at k = 0 chain frames 0 .. 3 are drawn (method 0), some of them through
    a frontier cluster and some without an open cluster, and frames 4 and 5 are refused because of an open cluster; at k = 50 the
    methods are 0, 0, 0, 0, 2, 2, and EVERY sub-block that is then enumerated has more than 32 rows (the k-best batch of the host
    entry never has the shape of the lane-per-child kernel); with max_width = 0 exactly the frames with an open cluster are
    refused."""
    r0 = [qm.chain_restated(f, 0) for f in range(6)]
    r50 = [qm.chain_restated(f, 50) for f in range(6)]
    print("k = 0: method", [r["method"] for r in r0], "opens", [len(r["opens"]) for r in r0], "nFrontier", [r["nFrontier"] for r in r0])
    assert [r["method"] for r in r0] == [0, 0, 0, 0, -1, -1] and [r["method"] for r in r50] == [0, 0, 0, 0, 2, 2]
    assert any(r["nFrontier"] >= 1 for r in r0[:4]) and all(len(r["opens"]) >= 1 for r in r0[4:])
    rows = [qs.enumerated_rows(f) for f in range(6)]
    print("k = 50: rows of the enumerated sub-blocks", rows)
    assert rows[:4] == [[], [], [], []] and all(rows[f] and min(rows[f]) > 32 for f in (4, 5))
    d = [qs.chain_draws(f) for f in range(4)]
    assert all(x["method"] == 0 and (x["assign"] >= 0).all() for x in d)
    assert any(x["nFrontier"] >= 1 for x in d)
    for f in range(6):  # max_width = 0: the frames with an open cluster, and only those
        assert (qs.chain_draws(f, max_width=0)["method"] == -1) == (len(r0[f]["opens"]) > 0), f
    assert any(not r["opens"] for r in r0) or any(not qm.window_restated("parity", j)["opens"] for j in range(16))


def test_conditions_of_the_parity_and_far_frames():
    """The sixteen parity frames hold frames without an open cluster (equal bits with the older path) and frames with a frontier
    cluster (valid draws); the frame against 100 000 landmarks keeps rows beyond 65 535 and is drawn."""
    re = [qm.window_restated("parity", j) for j in range(16)]
    closed = [j for j in range(16) if not re[j]["opens"]]
    frontier = [j for j in range(16) if re[j]["nFrontier"] >= 1 and re[j]["method"] == 0]
    print("parity: without an open cluster", closed, "with a frontier cluster", frontier, "method", [r["method"] for r in re])
    assert closed and frontier
    far = qm.window_restated("far", 6)
    assert far["method"] == 0 and far["rows"].max() > 65535


def test_restated_map_on_a_chain_frame():
    """The restatement maps every draw to a kept landmark or to the column's own miss row, no landmark twice, and logProb is the sum
    over the chosen entries of the compact block: -sum_c ccost[row_c][c] - logPerm within 1e-9."""
    for f in range(4):
        d, r = qs.chain_draws(f), qm.chain_restated(f, 0)
        nk, nM = len(d["rows"]), 40
        X = d["ccost"].reshape(nM, nk + nM).T
        comp = d["compact"].assign
        for s in range(qs.N):
            land = d["assign"][s][d["assign"][s] < 5000]
            assert len(set(land.tolist())) == len(land) and set(land.tolist()) <= set(d["rows"].tolist()), (f, s)
            assert (d["assign"][s][d["assign"][s] >= 5000] == 5000 + np.flatnonzero(d["assign"][s] >= 5000)).all(), (f, s)
            chosen = X[comp[s], np.arange(nM)]
            assert np.isfinite(chosen).all() and abs(d["logp"][s] - (-chosen.sum() - r["logPerm"])) <= 1e-9, (f, s)


# ---- 2. the statistical check, on the restatement first ----------------------------------------------------------------------------------------
def test_frequencies_of_the_restated_draws_meet_the_exact_marginals():
    """Four sparse frames (a few dozen kept rows, clusters of at most 6 measurements), 8 192 draws each under one fixed seed: every
    frequency of (measurement -> landmark or miss) within 5 sqrt(p (1 - p) / n) + 1 / n of the restated exact marginal p."""
    mean, cov, frames, gate = qs.sparse_batch()
    for f in range(4):
        re = qs.sparse_restated(f)
        assert re["method"] == 0 and 20 <= len(re["rows"]) <= 40 and re["maxCluster"] <= 6, (f, len(re["rows"]), re["maxCluster"])
        d = qs.restated(mean, cov, frames[f][2], frames[f][3], gate, qs.STAT_DRAWS, seed=qs.STAT_SEED, frame_key=f)
        assert d["method"] == 0
        freq = qs.frequencies(d["assign"], 5000)
        worst = qs.worst_excess(freq, re["probs"], qs.STAT_DRAWS)
        print(f"sparse frame {f}: kept {len(re['rows'])}, largest cluster {re['maxCluster']}, worst excess over the bound {worst:.3g}, "
              f"largest deviation {qs.worst_sigmas(freq, re['probs'], qs.STAT_DRAWS):.2f} sigma")
        assert worst <= 0.0, f


# ---- 3. the kernel, compiled for the host ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("quadric_map_sample_host")
    (tmp / "hip").mkdir()
    (tmp / "hip" / "hip_runtime.h").write_text("")
    out = str(tmp / "quadric_map_sample_host")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-I", str(tmp), "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-x", "c++",
                           os.path.join(ROOT, "tests", "cpp", "quadric_map_sample_host.cpp"), "-o", out, "-lpthread"])
    return out


PAD, INT_PAD, LP_PAD = 8, -77, -5.0


def run_rows(exe, tmp_path, frames, maxMap, maxKeep, maxCol, nSample, nTiles, adjacent=()):
    """frames: dicts landOff, measOff, nL, nM, nKeep, rows (<= maxKeep of them), assign [nSample, max(nM, 0)] as the sampler left
    it.  Every slice lies between pads of sentinels, but frame j + 1 follows frame j directly for j in adjacent.  Returns (the
    assign buffer after the launch, logProb after it, asgOff, lpOff)."""
    B = len(frames)
    asg, lp, asgOff, lpOff = [np.full(PAD, INT_PAD, np.int32)], [np.full(PAD, LP_PAD)], [], []
    rows = np.full((B, maxKeep), INT_PAD, np.int32)
    for j, fr in enumerate(frames):
        asgOff.append(sum(len(a) for a in asg))
        lpOff.append(sum(len(a) for a in lp))
        asg.append(np.ascontiguousarray(fr["assign"], dtype=np.int32).reshape(-1))
        lp.append(np.full(nSample, 0.25 + j))
        if j not in adjacent:
            asg.append(np.full(PAD, INT_PAD, np.int32))
            lp.append(np.full(PAD, LP_PAD))
        rows[j, :len(fr["rows"])] = fr["rows"]
    asg, lp = np.concatenate(asg), np.concatenate(lp)
    src, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("<6i2q", B, maxMap, maxKeep, maxCol, nSample, nTiles, len(asg), len(lp)))
        for j, fr in enumerate(frames):
            f.write(struct.pack("<4q4i", fr["landOff"], fr["measOff"], fr.get("asgOff", asgOff[j]), lpOff[j], fr["nL"], fr["nM"],
                                fr["nKeep"], 0))
        f.write(rows.tobytes() + asg.tobytes() + lp.tobytes())
    subprocess.check_call([exe, str(src), str(out)])
    buf = out.read_bytes()
    got_asg = np.frombuffer(buf, dtype=np.int32, count=len(asg))
    got_lp = np.frombuffer(buf, dtype=np.float64, offset=4 * len(asg))
    assert got_lp.size == len(lp)
    return (asg, got_asg), (lp, got_lp), asgOff, lpOff


MAXMAP, MAXKEEP, MAXCOL = 70000, 40, 128


def taken_frame(rng, nSample, nM, nKeep, nL=MAXMAP):
    """A frame the launch takes: rows ascending with the last one beyond 65 535 where there is one; the draws cycle through -1, 0,
    nKeep - 1, nKeep, nKeep + nM - 1 and go on at random in -1 .. nKeep + nM - 1."""
    rows = np.sort(rng.choice(nL - 1, size=nKeep, replace=False)).astype(np.int32) if nKeep else np.zeros(0, np.int32)
    if nKeep:
        rows[-1] = nL - 1
    edge = [v for v in (-1, 0, nKeep - 1, nKeep, nKeep + nM - 1) if -1 <= v < nKeep + nM]
    a = rng.integers(-1, nKeep + nM, size=nSample * nM)
    a[:len(edge)] = edge[:len(a)]
    if nSample * nM >= 2 * len(edge):
        a[-len(edge):] = edge
    return dict(landOff=0, measOff=0, nL=nL, nM=nM, nKeep=nKeep, rows=rows, assign=a.reshape(nSample, nM))


@pytest.mark.parametrize("nSample,nTiles", [(1, 1), (5, 2), (300, 7)])
def test_rows_kernel_on_the_host_under_sanitizers(exe, tmp_path, nSample, nTiles):
    """nSample below, no multiple of and above one workgroup of 256; nM in {1, 128} x nKeep in {0, 1, maxKeep}; the values -1, 0,
    nKeep - 1, nKeep, nKeep + nM - 1; kept row 69 999 (beyond 65 535); a frame with nKeep = maxKeep + 1 (every assign -1, every
    logProb NaN, nothing beyond its slices, its rowIdx never read: it holds sentinels); frames beyond maxMap and maxCol, with
    nM = 0, nL = -1 and a negative offset of either kind, untouched between sentinels; frames 0 | 1 and the refused frame and its
    neighbour adjacent.  The expected values are quadric_map_sample_lib.map_rows, the restated map."""
    rng = np.random.default_rng(1000 + nSample)
    frames = [taken_frame(rng, nSample, nM, nk) for nM in (1, 128) for nk in (0, 1, MAXKEEP)]
    frames.append(taken_frame(rng, nSample, 3, 5, nL=7))
    refused = len(frames)
    frames.append(dict(landOff=0, measOff=0, nL=MAXMAP, nM=7, nKeep=MAXKEEP + 1, rows=[], assign=np.full((nSample, 7), INT_PAD)))
    frames.append(taken_frame(rng, nSample, 128, MAXKEEP))
    beyond = len(frames)
    for kw in (dict(nL=MAXMAP + 1), dict(nM=MAXCOL + 1), dict(nM=0), dict(nL=-1), dict(landOff=-1), dict(measOff=-3)):
        fr = dict(landOff=0, measOff=0, nL=100, nM=4, nKeep=2, rows=[3, 9])
        fr.update(kw)
        fr["assign"] = rng.integers(-1, 2 + max(fr["nM"], 1), size=(nSample, max(fr["nM"], 0)))
        frames.append(fr)
    (asg, got_asg), (lp, got_lp), asgOff, lpOff = run_rows(exe, tmp_path, frames, MAXMAP, MAXKEEP, MAXCOL, nSample, nTiles,
                                                           adjacent=(0, refused))
    want_asg, want_lp = asg.copy(), lp.copy()
    for j, fr in enumerate(frames[:beyond]):
        n = nSample * fr["nM"]
        if j == refused:
            want_asg[asgOff[j]:asgOff[j] + n] = -1
            want_lp[lpOff[j]:lpOff[j] + nSample] = np.nan
        else:
            want_asg[asgOff[j]:asgOff[j] + n] = qs.map_rows(fr["assign"], fr["rows"], fr["nL"]).reshape(-1)
    assert np.array_equal(got_asg, want_asg)
    assert np.array_equal(np.isnan(got_lp), np.isnan(want_lp)) and np.array_equal(got_lp[~np.isnan(want_lp)], want_lp[~np.isnan(want_lp)])
    assert (got_asg == MAXMAP - 1).any() and np.isnan(got_lp).sum() == nSample and (got_asg[asgOff[refused]:][:7 * nSample] == -1).all()


def test_rows_kernel_leaves_a_frame_with_a_negative_draw_offset_alone(exe, tmp_path):
    rng = np.random.default_rng(5)
    frames = [taken_frame(rng, 5, 3, 2, nL=50), taken_frame(rng, 5, 3, 2, nL=50)]
    frames[1]["asgOff"] = -1
    (asg, got_asg), (lp, got_lp), asgOff, _ = run_rows(exe, tmp_path, frames, 50, 4, 3, 5, 1)
    want = asg.copy()
    want[asgOff[0]:asgOff[0] + 15] = qs.map_rows(frames[0]["assign"], frames[0]["rows"], 50).reshape(-1)
    assert np.array_equal(got_asg, want) and np.array_equal(got_lp, lp)


# ---- 4. the library ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pk.lib_path()):
        subprocess.check_call(["make", "-C", CSRC])
    return pk.load_library()


def test_library_exports_quadric_map_sample_entries(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pk.lib_path()], text=True)
    from probabilisticsemslam_amd import engine
    for sym in ("kbest_reserve_quadric_map_sample_dev", "kbest_quadric_map_sample_assoc_batch_f64_dev",
                "kbest_quadric_map_sample_assoc_batch_f64", "kbest_quadric_map_sample_kernel_usage"):
        assert sym in engine.C_ABI_SYMBOLS and f" T {sym}\n" in out and hasattr(lib, sym), sym
    for name in ("reserve_quadric_map_sample_dev", "quadric_map_sample_assoc_dev", "quadric_map_sample_assoc"):
        assert callable(getattr(pk.KBestEngine, name)), name
    header = open(os.path.join(ROOT, "include", "kbest_c.h")).read()
    assert "int kbest_reserve_quadric_map_sample_dev(kbest_ctx *ctx, int B, int maxMap, int maxKeep, int maxCol, int nSample);" in header
    assert "int kbest_quadric_map_sample_assoc_batch_f64_dev(" in header and "int kbest_quadric_map_sample_assoc_batch_f64(" in header
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "kbest_quadric_map_sample.hip" in make.split("SRCS", 1)[1].split("\n", 1)[0]
    assert os.path.exists(os.path.join(CSRC, "kbest_quadric_map_sample.hip"))


def test_quadric_map_sample_without_gpu_fails_loudly(lib):
    if lib.kbest_device_count() > 0:
        return  # (a GPU is present: tests/test_gpu_quadric_map_sample.py has the rest)
    with pytest.raises(pk.KBestError):
        pk.KBestEngine(0).reserve_quadric_map_sample_dev(1, 1000, 64, 24, 5)
