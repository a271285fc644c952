"""CPU: the restatement of the draws from the exact posterior (tests/sample_check.py) -- its generator against the published known
answers, its draws against the plain permutation sum (chi-square on the joints, the marginals, the log-probabilities), its
invariance under conditioning; the kernel source itself on the host under sanitizers against the restatement; the library exports
sampleAssoc and its C entries; without a GPU they fail loudly."""
import os
import struct
import subprocess

import numpy as np
import pytest

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


def test_philox_known_answers():
    """Philox4x32-10 of Salmon et al.: counter and key all zero, all ones, and the digits of pi."""
    ones = 0xFFFFFFFF
    for ctr, key, want in (((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
                           ((ones,) * 4, (ones,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
                           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
                            (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))):
        assert sc.philox4x32_10(ctr, key) == want
        got = sc.philox4x32_10(tuple(np.array([w], np.uint64) for w in ctr), key)  # the array form the walk uses
        assert tuple(int(w[0]) for w in got) == want
    # u: words 0, 1 for even rows, words 2, 3 for odd rows of the same block; seed and frame key split into their words
    seed, fkey = 0x299F31D0A4093822, 0x0370734413198A2E
    w = (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)
    draw = np.array([0x243F6A88], np.uint64)
    assert sc.uniforms(seed, draw, 2 * 0x85A308D3, fkey)[0] == (((w[1] << 32) | w[0]) >> 11) * 2.0 ** -53
    assert sc.uniforms(seed, draw, 2 * 0x85A308D3 + 1, fkey)[0] == (((w[3] << 32) | w[2]) >> 11) * 2.0 ** -53


def test_raw_and_preconditioned_blocks_draw_the_same_joints():
    """condition = 1 on a raw block and condition = 0 on its conditioned block: the same rows (in the caller's numbering through
    rowIdx), the same log-probabilities; no gated entry and no row conditionCosts drops is ever drawn."""
    for (F, nL, nM) in sc.FRAME_SETS:
        for b, (f, want) in enumerate(zip(wl.kitti_like_frames(F, nL=nL, nM=nM), sc.reference_draws(F, nL, nM))):
            cond, idx = ol.condition_costs(f, nL + nM, nM)
            asg, lp, Z, _ = sc.sample_assoc(cond, len(idx) - nM, nM, 512, seed=sc.SEED, frame_key=b)
            assert np.array_equal(np.asarray(idx)[asg], want.assign[:512]) and np.array_equal(lp, want.logp[:512]) and Z == want.Z
            a = pc.to_probs(cond).reshape(nM, len(idx))
            assert (a[np.arange(nM), asg] > 0.0).all()  # every drawn entry passes the gate
            assert np.isin(want.assign, idx).all()


def test_log_prob_is_the_joints_weight_over_z():
    """Against the plain permutation sum over the conditioned block: 1e-12."""
    worst = 0.0
    for (F, nL, nM) in sc.FRAME_SETS:
        for b, (f, got) in enumerate(zip(wl.kitti_like_frames(F, nL=nL, nM=nM), sc.reference_draws(F, nL, nM))):
            cond, idx = ol.condition_costs(f, nL + nM, nM)
            joint, Z = sc.joint_probabilities(cond, len(idx) - nM, nM)
            back = {int(r): i for i, r in enumerate(idx)}
            want = np.array([np.log(joint[tuple(back[int(r)] for r in row)]) for row in got.assign])
            worst = max(worst, np.abs(got.logp - want).max(), abs(got.Z - Z) / Z)
    print(f"logProb vs permutation sum {worst:.3g}")
    assert worst <= 1e-12


def test_draws_follow_the_exact_posterior():
    """4 096 draws per frame, seed 2024, frameKey = b, conditioned: the histogram of joints against the permutation sum's joint
    probabilities over the cells with expectation >= 5, z = (chi2 - n) / sqrt(2 n) <= 4 (n: those cells); the empirical marginals
    against permanent_probs within 4 / sqrt(N)."""
    N = sc.N_DRAWS
    worst_z = worst_m = 0.0
    margin = np.inf
    for (F, nL, nM) in sc.FRAME_SETS:
        for b, (f, got) in enumerate(zip(wl.kitti_like_frames(F, nL=nL, nM=nM), sc.reference_draws(F, nL, nM))):
            cond, idx = ol.condition_costs(f, nL + nM, nM)
            joint, _ = sc.joint_probabilities(cond, len(idx) - nM, nM)
            seen = {}
            for row in got.assign.tolist():
                seen[tuple(row)] = seen.get(tuple(row), 0) + 1
            chi2 = n = 0
            for rows, pr in joint.items():
                if N * pr >= 5.0:
                    obs = seen.get(tuple(int(idx[r]) for r in rows), 0)
                    chi2 += (obs - N * pr) ** 2 / (N * pr)
                    n += 1
            assert n >= 2, (F, b)
            z = (chi2 - n) / np.sqrt(2.0 * n)
            cp, _ = pc.permanent_probs(cond, len(idx) - nM, nM)
            want = pc.scatter_back(cp, idx, nL, nM)
            emp = np.zeros((nM, nL + 1))
            for c in range(nM):
                np.add.at(emp[c], np.minimum(got.assign[:, c], nL), 1.0 / N)
            worst_z, worst_m, margin = max(worst_z, z), max(worst_m, np.abs(emp - want).max() * np.sqrt(N)), min(margin, got.margin)
    print(f"worst z {worst_z:.3g}, worst marginal error {worst_m:.3g} / sqrt(N), smallest margin {margin:.3g}")
    assert worst_z <= 4.0 and worst_m <= 4.0


def test_degenerate_frames_of_the_restatement():
    cost = wl.dense_batch(1, 9, 3, 5)[0] * 10.0
    cost[9:18] = np.inf  # a column without a finite entry
    asg, lp, Z, _ = sc.sample_assoc(cost, 6, 3, 8)
    assert Z == 0.0 and (asg == -1).all() and np.isnan(lp).all()
    one = np.array([0.5, 43.0, 2.0])  # 3 x 1: row 1 is gated
    asg, lp, Z, _ = sc.sample_assoc(one, 2, 1, 2000, seed=3)
    w = np.exp(0.5 - one) * np.array([1.0, 0.0, 1.0])
    assert set(asg[:, 0].tolist()) == {0, 2} and abs((asg[:, 0] == 0).mean() - w[0] / w.sum()) <= 4 / np.sqrt(2000)
    np.testing.assert_allclose(lp, np.log(w[asg[:, 0]] / w.sum()), rtol=0, atol=1e-15)
    # sample_base continues a sequence
    f = wl.kitti_like_frames(1, nL=6, nM=3)[0]
    whole = sc.sample_assoc(f, 6, 3, 96, seed=9, condition=True, frame_key=5)
    tail = sc.sample_assoc(f, 6, 3, 32, seed=9, condition=True, frame_key=5, sample_base=64)
    assert np.array_equal(whole[0][64:], tail[0]) and np.array_equal(whole[1][64:], tail[1])


def test_kernel_source_on_the_host_under_sanitizers(tmp_path):
    """tests/cpp/sample_host.cpp: the kernel's own source as host threads, AddressSanitizer and UBSan on, exact-size buffers, two
    workgroups striding over the frames: the two frame sets (raw, conditioned while loading) with every layer in LDS (mode 0) and
    with the layers in the work space (mode 1), one 13-column frame with everything there (mode 2).  Draws equal to the restatement
    (whose margins are far above the last bits of exp), logProb 1e-12, perm 1e-12 relative."""
    (tmp_path / "hip").mkdir()
    (tmp_path / "hip" / "hip_runtime.h").write_text("")
    exe = str(tmp_path / "sample_host")
    csrc = os.path.join(ROOT, "probabilisticsemslam_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", str(tmp_path), "-I", os.path.join(ROOT, "include"), "-I", csrc, "-x", "c++",
                           os.path.join(ROOT, "tests", "cpp", "sample_host.cpp"), "-o", exe, "-lpthread"])
    small = [(f, nL, nM, b, w) for (F, nL, nM) in sc.FRAME_SETS
             for b, (f, w) in enumerate(zip(wl.kitti_like_frames(F, nL=nL, nM=nM), sc.reference_draws(F, nL, nM)))]
    wide = sc.wide_frame()
    runs = [(0, sc.N_DRAWS, sc.SEED, 1, small), (1, 256, sc.SEED, 1, small), (2, wide[4].n, sc.SEED, 0, [wide])]
    for mode, n_sample, seed, condition, frames in runs:
        src, out = tmp_path / f"in{mode}.bin", tmp_path / f"out{mode}.bin"
        with open(src, "wb") as fh:
            fh.write(struct.pack("iiiiiIQ", len(frames), mode, n_sample, condition, 2, 0, seed))
            for f, nL, nM, key, _ in frames:
                fh.write(struct.pack("iiQ", nL, nM, key) + np.asarray(f, dtype=np.float64).tobytes())
        subprocess.check_call([exe, str(src), str(out)])
        buf, at = out.read_bytes(), 0
        for f, nL, nM, key, want in frames:
            assert want.margin >= 1e-10
            (perm,) = struct.unpack_from("d", buf, at)
            asg = np.frombuffer(buf, dtype=np.int32, count=n_sample * nM, offset=at + 8).reshape(n_sample, nM)
            lp = np.frombuffer(buf, dtype=np.float64, count=n_sample, offset=at + 8 + 4 * n_sample * nM)
            at += 8 + 4 * n_sample * nM + 8 * n_sample
            assert np.array_equal(asg, want.assign[:n_sample]), (mode, nM, key)
            assert np.abs(lp - want.logp[:n_sample]).max() <= 1e-12 and abs(perm - want.Z) <= 1e-12 * want.Z, (mode, nM, key)
        assert at == len(buf)


def test_library_exports_sample_entries(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pk.lib_path()], text=True)
    assert "_Z11sampleAssocRKSt6vectorIdSaIdEEmmmm" in out
    from probabilisticsemslam_amd import engine
    for sym in ("kbest_sample_assoc_batch_f64", "kbest_sample_assoc_batch_f64_dev", "kbest_reserve_sample"):
        assert sym in engine.C_ABI_SYMBOLS and f" T {sym}\n" in out and hasattr(lib, sym), sym
    assert callable(pk.sampleAssoc)
    for name in ("sample_assoc", "sample_assoc_dev", "reserve_sample"):
        assert callable(getattr(pk.KBestEngine, name)), name
    header = open(os.path.join(ROOT, "include", "kbest_c.h")).read()
    assert "u = (((hi << 32) | lo) >> 11) * 2^-53" in header and "(sampleBase + s, i >> 1, frameKey[b] low word," in header


def test_sample_without_gpu_fails_loudly(lib):
    if lib.kbest_device_count() > 0:
        return  # (a GPU is present: tests/test_gpu_sample.py has the rest)
    with pytest.raises(pk.KBestError):
        pk.sampleAssoc(np.random.rand(12), 2, 3, 4)
