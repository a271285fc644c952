"""CPU: the restatement of the draws by gated clusters (tests/cluster_sample_check.py) -- its draws against the whole-frame
restatement (tests/sample_check.py) on the frames both take, against the exact clustered marginals beyond them, the consistency of
every part of an assembled frame; the plain C++ of the kernel (the walk and the index arithmetic around it) on the host under
sanitizers against the restatement; without a GPU the entries fail loudly."""
import os
import struct
import subprocess

import numpy as np
import pytest

import cluster_check as cc
import cluster_sample_check as cs
import oracle_lib as ol
import permanent_check as pc
import probabilisticsemslam_amd as pk
import sample_check as sc
from probabilisticsemslam_amd import workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pk.lib_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "probabilisticsemslam_amd", "csrc")])
    return pk.load_library()


@pytest.mark.parametrize("condition", [False, True])
def test_same_draws_as_the_whole_frame_walk_on_scene_frames(condition):
    """scene_frames(6, 20, 10, 12.0): 2 to 4 clusters a frame.  The uniform of a row is indexed by the frame's active rows, the
    whole-frame layers factorise: the clustered walk makes the whole-frame walk's decisions."""
    worst, margin, sizes = 0.0, np.inf, []
    for b, (f, got) in enumerate(zip(wl.scene_frames(6, 20, 10, 12.0), cs.scene_draws(6, 20, 10, 12.0, 1024, condition))):
        asg, lp, Z, mg = sc.sample_assoc(f, 20, 10, 1024, seed=sc.SEED, condition=condition, frame_key=b)
        assert got.info >= 2 and np.array_equal(asg, got.assign), b
        worst, margin = max(worst, np.abs(lp - got.logp).max(), abs(np.log(Z) - got.logperm)), min(margin, got.margin, mg)
        sizes.append((got.info, got.maxc))
    print(f"condition {condition}: (clusters, largest) {sizes}, logProb differs by {worst:.3g}, smallest margin {margin:.3g}")
    assert worst <= 1e-13 and margin >= 1e-10


def test_same_draws_as_the_whole_frame_walk_on_the_frame_sets():
    for (F, nL, nM) in sc.FRAME_SETS:
        for b, (f, want) in enumerate(zip(wl.kitti_like_frames(F, nL=nL, nM=nM), sc.reference_draws(F, nL, nM))):
            got = cs.clustered_sample_assoc(f, nL, nM, sc.N_DRAWS, seed=sc.SEED, condition=True, frame_key=b)
            assert got.info > 0 and np.array_equal(got.assign, want.assign), (F, b)
            assert np.abs(got.logp - want.logp).max() <= 1e-13 and abs(got.logperm - np.log(want.Z)) <= 1e-13
            # sample_base continues a sequence
            tail = cs.clustered_sample_assoc(f, nL, nM, 96, seed=sc.SEED, condition=True, frame_key=b, sample_base=4000)
            assert np.array_equal(tail.assign, got.assign[4000:]) and np.array_equal(tail.logp, got.logp[4000:])


def test_assembled_frame_follows_the_exact_marginals():
    """cluster_check.assembled_frame() (36 x 18, three interleaved parts of 6 measurements), 4 096 draws: the empirical marginals
    within 4 / sqrt(N) of cluster_check.clustered_probs (the bound of tests/test_sample_cpu.py); every part's draws are consistent:
    no landmark twice, no gated entry ever; logPerm is the clustered restatement's."""
    N = sc.N_DRAWS
    f, nL, nM, parts, got = cs.assembled_draws(N)
    want, logperm, info, maxc, lab = cc.clustered_probs(f, nL, nM)
    assert (got.info, got.maxc) == (info, maxc) == (3, 6) and got.logperm == logperm
    emp = np.zeros((nM, nL + 1))
    for c in range(nM):
        np.add.at(emp[c], np.minimum(got.assign[:, c], nL), 1.0 / N)
    worst = np.abs(emp - want).max() * np.sqrt(N)
    print(f"worst marginal error {worst:.3g} / sqrt(N), smallest margin {got.margin:.3g}")
    assert worst <= 4.0
    a = pc.to_probs(f).reshape(nM, nL + nM)
    assert (a[np.arange(nM), got.assign] > 0.0).all()  # no gated entry is ever drawn
    for p in range(3):
        rows = got.assign[:, p::3]  # the part's 6 measurements
        assert (rows % 3 == p).all()  # ... stay on the part's own rows
        for s in range(0, N, 37):
            lm = rows[s][rows[s] < nL]
            assert len(set(lm.tolist())) == len(lm)  # no landmark is taken twice
    srt = np.sort(np.where(got.assign < nL, got.assign, -1 - np.arange(nM)), axis=1)  # (misses made distinct)
    assert (srt[:, 1:] != srt[:, :-1]).all()  # ... in any draw, over the whole frame


def test_margins_beyond_sixteen_measurements():
    for shape, n, most in (((6, 40, 24, 24.0), 512, 9), ((4, 60, 40, 30.0), 256, 14)):
        got = cs.scene_draws(*shape, n)
        frames = wl.scene_frames(*shape)
        print(f"{shape}: clusters {[g.info for g in got]}, largest {[g.maxc for g in got]}, smallest margin {min(g.margin for g in got):.3g}")
        assert max(g.maxc for g in got) == most and min(g.margin for g in got) >= 1e-10
        for f, g in zip(frames, got):
            assert g.logperm == cc.clustered_probs(f, shape[1], shape[2])[1]
            assert (g.assign >= 0).all() and np.isfinite(g.logp).all()


def test_refusals_and_infeasible_frames_of_the_restatement():
    dense = wl.dense_batch(1, 20, 17, 17)[0] * 10.0
    r = cs.clustered_sample_assoc(dense, 3, 17, 5)
    assert r.info == -2 and r.maxc == 17 and (r.assign == -1).all() and np.isnan(r.logp).all() and np.isnan(r.logperm)
    f = wl.scene_frames(1, 20, 10, 12.0)[0]
    r = cs.clustered_sample_assoc(f, 20, 10, 5, slot_bytes=1024)
    assert r.info == -3 and (r.assign == -1).all() and np.isnan(r.logperm)
    bad = np.array(f)
    bad[9 * 30:] = np.inf  # the last column without a finite entry
    r = cs.clustered_sample_assoc(bad, 20, 10, 5)
    assert r.info == 0 and r.logperm == -np.inf and (r.assign == -1).all() and np.isnan(r.logp).all()


def test_walk_on_the_host_under_sanitizers(tmp_path):
    """tests/cpp/cluster_sample_host.cpp: kbest_cluster_sample.h -- the generator, cs_small, cs_place, cs_layer_entry, cs_walk --
    with AddressSanitizer and UBSan on heap blocks of exactly the planned size.  Frame 0 of scene_frames(6, 20, 10, 12.0) has
    small-tier clusters and one of 8 measurements and 23 rows for the workgroup tier; arenas of 64 KiB, 2 048 and 256 bytes put that cluster's layers in the arena,
    its layers in the slot, and its entries in the slot too.  Draws equal to the restatement, logProb 1e-12, Z 1e-12 relative."""
    exe = str(tmp_path / "cluster_sample_host")
    csrc = os.path.join(ROOT, "probabilisticsemslam_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", csrc, os.path.join(ROOT, "tests", "cpp", "cluster_sample_host.cpp"), "-o", exe])
    n, key = 1024, 0
    f = wl.scene_frames(6, 20, 10, 12.0)[0]
    want = cs.scene_draws(6, 20, 10, 12.0, n)[0]
    parts, _ = cs.cluster_parts(f, 20, 10)
    assert want.margin >= 1e-10 and [len(p.cols) for p in parts].count(8) == 1
    tiers = set()
    for arena in (64 << 10, 2048, 256):
        src, out = tmp_path / f"in{arena}.bin", tmp_path / f"out{arena}.bin"
        with open(src, "wb") as fh:
            fh.write(struct.pack("=iiiiIQQ", len(parts), n, 10, arena, 0, sc.SEED, key))
            for p in parts:
                R, m = p.a.shape
                fh.write(struct.pack("ii", m, R) + np.asarray(p.cols, np.int32).tobytes() + np.asarray(p.gidx, np.uint16).tobytes() +
                         np.asarray(p.raw, np.uint16).tobytes() + np.ascontiguousarray(p.a, dtype=np.float64).tobytes())
        subprocess.check_call([exe, str(src), str(out)])
        buf = out.read_bytes()
        k = len(parts)
        Z = np.frombuffer(buf, np.float64, k, 0)
        tier = np.frombuffer(buf, np.int32, k, 8 * k)
        asg = np.frombuffer(buf, np.int32, n * 10, 12 * k).reshape(n, 10)
        lp = np.frombuffer(buf, np.float64, n, 12 * k + 40 * n)
        assert len(buf) == 12 * k + 48 * n
        assert np.array_equal(asg, want.assign), arena
        assert np.abs(lp - want.logp).max() <= 1e-12
        assert all(abs(z - p.Z) <= 1e-12 * p.Z for z, p in zip(Z, parts))
        assert [t == 0 for t in tier] == [cc_small(p) for p in parts]
        tiers |= set(tier.tolist())
    assert tiers == {0, 1, 2}


def cc_small(part):
    R, m = part.a.shape
    return m <= 6 and (R * (1 << m) + R * m) * 8 <= 4096  # cl_small of kbest_cluster.hip


def test_cluster_sample_without_gpu_fails_loudly(lib):
    if lib.kbest_device_count() > 0:
        return  # (a GPU is present: tests/test_gpu_cluster_sample.py has the rest)
    with pytest.raises(pk.KBestError):
        pk.clusterSampleAssoc(np.random.rand(12), 2, 3, 4)
