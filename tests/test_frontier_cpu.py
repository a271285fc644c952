"""CPU: the restatement of the frontier tier (tests/frontier_check.py) against the project's other restatements -- the plain subset
sums where they are affordable, the column-scaled sums of the big-cluster tier on the scene clusters of 17, 18 and 20 measurements
-- its invariances, the clusters of 22, 23 and 25 measurements that have no other exact answer, and the widths of every oversized
cluster of the three scene families; the kernel source itself on the host under sanitizers; the library exports hybridFrontierProb and its C entries; without a GPU they fail loudly."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bigcluster_check as bc
import frontier_check as fc
import permanent_check as pc
import probabilisticsemslam_amd as pk
import range_lib as rl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES, scene, oversized, raw_cluster = fc.FAMILIES, fc.scene, fc.oversized, fc.raw_cluster


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pk.lib_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "probabilisticsemslam_amd", "csrc")])
    return pk.load_library()


def sparse_block(rng, R, C, density):
    a = rng.random((R, C)) * (rng.random((R, C)) < density)
    return a[(a > 0.0).any(axis=1)]


def test_against_the_plain_subset_sums():
    """Random sparse blocks of at most 12 columns: Z within 1e-15 relative, probabilities within 1e-12."""
    rng = np.random.default_rng(2024)
    seen = worst_z = worst_p = 0
    for R, C, density in ((14, 9, 0.3), (20, 12, 0.2), (16, 12, 0.3), (9, 9, 0.5), (12, 5, 1.0), (1, 1, 1.0), (6, 7, 0.6), (24, 10, 0.15)):
        for _ in range(3):
            a = sparse_block(rng, R, C, density)
            if len(a) == 0:
                continue
            w, Z = fc.frontier_sums(a)
            pw, pZ = pc.subset_sums(a)
            if not pZ > 0.0:
                assert Z == 0.0 and not w.any()
                continue
            seen += 1
            worst_z = max(worst_z, abs(Z - pZ) / pZ)
            worst_p = max(worst_p, np.abs(w / Z - pw / pZ).max())
    print(f"{seen} feasible blocks: Z {worst_z:.3g} relative, probabilities {worst_p:.3g}")
    assert seen >= 12
    assert worst_z <= 1e-15 and worst_p <= 1e-12


@pytest.mark.parametrize("shape,index,cluster", [((75, 60, 40, 30), 1, (17, 40)), ((75, 60, 40, 30), 38, (18, 43)),
                                                 ((6, 200, 128, 60), 5, (20, 46))])
def test_against_the_big_cluster_restatement(shape, index, cluster):
    """The scene clusters tests/test_gpu_bigcluster.py uses (conditioned while loading): 1e-12 on the probabilities, 1e-12 relative
    on log Z."""
    _, nL, nM, _ = shape
    want = fc.hybrid_frontier_probs(scene(*shape)[index], nL, nM, condition=True)
    (o,) = want[2]
    assert (o["m"], o["R"]) == cluster and o["tier"] == "frontier" and want[1] == 0 and want[3] == 1 and want[4] == 0
    p, logZ, info = bc.big_cluster(o["block"], o["nL"], o["m"])
    err = np.abs(o["probs"] - p).max()
    print(f"cluster {cluster}: W {o['W']}, vs big_cluster {err:.3g}, log Z {o['logZ']!r} vs {logZ!r}")
    assert info == 1 and err <= 1e-12 and abs(o["logZ"] - logZ) <= 1e-12 * max(1.0, abs(logZ))
    assert np.abs(want[0].sum(axis=1) - 1.0).max() <= 1e-12


def test_permutations_leave_z_alone():
    """Rows and columns in another order: another greedy order, other layers, the same Z (1e-12 relative: sums of non-negative
    terms) -- and the widths are those of the pattern, whatever the values."""
    rng = np.random.default_rng(5)
    for _ in range(6):
        a = sparse_block(rng, 18, 11, 0.25)
        _, Z = fc.frontier_sums(a)
        rp, cp = rng.permutation(a.shape[0]), rng.permutation(a.shape[1])
        w2, Z2 = fc.frontier_sums(a[rp][:, cp])
        w1, _ = fc.frontier_sums(a)
        assert abs(Z2 - Z) <= 1e-12 * Z
        if Z > 0.0:
            assert np.abs(w2 - w1[rp][:, cp]).max() <= 1e-12 * Z
        assert fc.greedy_plan(fc.row_masks(a), a.shape[1])[1] == fc.greedy_plan(fc.row_masks(a * 0.5 + (a > 0)), a.shape[1])[1]


@pytest.mark.parametrize("shape,frame,size", [(FAMILIES[1], 89, (58, 25)), (FAMILIES[2], 54, (51, 22)), (FAMILIES[2], 8, (61, 23))])
def test_columns_sum_to_z_beyond_twenty(shape, frame, size):
    """The clusters no other tier answers: every column's marginals sum to Z (1e-12 relative)."""
    A = raw_cluster(shape, frame, size)
    w, Z = fc.frontier_sums(A)
    err = np.abs(w.sum(axis=0) / Z - 1.0).max()
    steps, W, layers = fc.greedy_plan(fc.row_masks(A), A.shape[1])
    print(f"{size[1]} x {size[0]}: W {W}, {layers} doubles of layers, Z' {Z!r}, columns - 1 {err:.3g}")
    assert Z > 0.0 and err <= 1e-12 and (w >= 0.0).all()


def test_every_oversized_scene_cluster_fits_the_tier():
    """Every cluster of more than 16 columns of the three families: W <= 16 and the layers inside the default slot, raw and
    conditioned; the widest of the raw ones has W = 12."""
    widths = []
    for shape in FAMILIES:
        for condition in (False, True):
            for b, A in oversized(shape, condition):
                steps, W, layers = fc.greedy_plan(fc.row_masks(A), A.shape[1])
                assert W <= fc.MAX_WIDTH and layers * 8 <= fc.SLOT, (shape, condition, b, W, layers)
                assert W == max(fc.popcount(s["psi"]) for s in steps) and len(steps) == A.shape[0]
                if not condition:
                    widths.append(W)
    assert len(widths) == 20 and max(widths) == 12


def test_edges_of_the_restatement():
    inf = np.inf
    flat = lambda blk: np.ascontiguousarray(np.asarray(blk, dtype=np.float64).T).reshape(-1)  # noqa: E731
    p, lz, info, W = fc.frontier_cluster(flat([[1.5]]), 0, 1)  # one miss row
    assert info == 1 and W == 1 and p.tolist() == [[1.0]] and lz == -1.5
    same_row = flat([[1.0, 2.0], [inf, inf], [inf, inf], [inf, inf]])  # both columns can only take row 0
    p, lz, info, W = fc.frontier_cluster(same_row, 2, 2)
    assert info == 0 and not p.any() and lz == -inf and W == 2
    wide = np.full((2 + 17, 17), inf)  # two landmark rows over 17 columns and a miss row each
    wide[:2] = 1.0
    wide[2:] = np.where(np.eye(17, dtype=bool), 0.5, inf)
    assert fc.frontier_cluster(flat(wide), 2, 17)[2:] == (fc.REFUSED_WIDTH, 17)
    p, lz, info, W = fc.frontier_cluster(flat(wide[:18, :16]), 2, 16)
    assert info == 1 and W == 16
    need = fc.layers_bytes(fc.row_masks(np.isfinite(wide[:18, :16]).astype(float)), 16)
    assert fc.frontier_cluster(flat(wide[:18, :16]), 2, 16, slot_bytes=need - 8)[2] == fc.REFUSED_SLOT
    assert fc.frontier_cluster(flat(wide[:18, :16]), 2, 16, slot_bytes=need)[2] == 1
    # without the tier the frame function is bigcluster_check's
    f = scene(75, 60, 40, 30)[1]
    a, b = fc.hybrid_frontier_probs(f, 60, 40, condition=True, max_width=0), bc.hybrid_exact_probs(f, 60, 40, condition=True)
    assert np.array_equal(a[0].view(np.int64), b[0].view(np.int64)) and (a[1], a[3], a[4], a[5], a[6]) == (b[1], 0, b[3], b[4], b[5])


def test_kernel_source_on_the_host_under_sanitizers(tmp_path):
    """tests/cpp/frontier_host.cpp: the kernel's own source as 256 host threads per workgroup, AddressSanitizer and UBSan on,
    two workgroups striding over the clusters, against the restatement (1e-12).  Then the slot at exactly the need of the largest
    cluster of the run: the same answers, nothing beyond the buffers."""
    (tmp_path / "hip").mkdir()
    (tmp_path / "hip" / "hip_runtime.h").write_text("")
    exe = str(tmp_path / "frontier_host")
    csrc = os.path.join(ROOT, "probabilisticsemslam_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", str(tmp_path), "-I", os.path.join(ROOT, "include"), "-I", csrc, "-x", "c++",
                           os.path.join(ROOT, "tests", "cpp", "frontier_host.cpp"), "-o", exe, "-lpthread"])
    names = ["one_by_one", "two_by_one", "fewer_states_than_a_wave", "opens_and_closes_in_one_row", "band_of_24", "same_only_row",
             "width_17"]
    blocks = [fc.edge_clusters()[n] for n in names]
    want = [fc.frontier_cluster(*b) for b in blocks]
    A = raw_cluster(FAMILIES[1], 89, (58, 25))  # the 25 x 58 scene cluster, as costs: 58 landmark rows, the miss rows all zeros
    with np.errstate(divide="ignore"):
        blk = np.full((58 + 25, 25), np.inf)
        blk[:58] = -np.log(A)
    blocks.append((np.ascontiguousarray(blk.T).reshape(-1), 58, 25))
    want.append(fc.frontier_cluster(*blocks[-1]))
    # beyond the range (tests/range_lib.py): a deep pair chain of 64 columns is declined, a cluster without a matching stays 0
    for c in (rl.pair_chain(32, 25), rl.no_matching()["three_columns_two_rows"]):
        blocks.append((c.block, c.nLk, c.m))
        want.append(fc.frontier_cluster(*blocks[-1]))
        names.append(c.name)
    names.insert(7, "25 x 58")
    assert [w[2] for w in want] == [1, 1, 1, 1, 1, 0, fc.REFUSED_WIDTH, 1, bc.OUT_OF_RANGE, 0]
    src = tmp_path / "in.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("i", len(blocks)))
        for b, l, m in blocks:
            f.write(struct.pack("ii", m, l) + np.asarray(b, dtype=np.float64).tobytes())
    need = max(fc.layers_bytes(fc.row_masks(fc.scaled_block(*b)[0]), b[2]) for b, w in zip(blocks, want) if w[2] >= 0) // 8
    for args in ([], [str(need), "1"]):
        out = tmp_path / "out.bin"
        subprocess.check_call([exe, str(src), str(out)] + args)
        buf, at = out.read_bytes(), 0
        for (b, l, m), (wp, wlz, winfo, wW), name in zip(blocks, want, names):
            info, width, lz = struct.unpack_from("iid", buf, at)
            p = np.frombuffer(buf, dtype=np.float64, count=m * (l + 1), offset=at + 16).reshape(m, l + 1)
            at += 16 + 8 * m * (l + 1)
            assert (info, width) == (winfo, wW), name
            if winfo < 0:
                assert (p == -5.0).all() and lz == -5.0, name
            else:
                assert np.abs(p - wp).max() <= 1e-12 and (lz == wlz or abs(lz - wlz) <= 1e-12 * max(1.0, abs(wlz))), name
        assert at == len(buf)


def test_library_exports_frontier_entries(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pk.lib_path()], text=True)
    assert "_Z18hybridFrontierProbRKSt6vectorIdSaIdEEmmm" in out
    from probabilisticsemslam_amd import engine
    for sym in ("kbest_reserve_frontier", "kbest_set_frontier_work_cap", "kbest_set_frontier_slot", "kbest_frontier_probs_f64_dev",
                "kbest_hybrid_frontier_probs_batch_f64"):
        assert sym in engine.C_ABI_SYMBOLS and f" T {sym}\n" in out and hasattr(lib, sym), sym
    assert callable(pk.hybridFrontierProb)
    for name in ("hybrid_frontier_probs", "frontier_probs_dev", "reserve_frontier", "set_frontier_work_cap", "set_frontier_slot"):
        assert callable(getattr(pk.KBestEngine, name)), name
    header = open(os.path.join(ROOT, "include", "kbest_c.h")).read()
    assert "#define KBEST_FRONTIER_MAX_COLS 64" in header and "#define KBEST_FRONTIER_MAX_WIDTH 16" in header
    assert "KBEST_FRONTIER_SLOT ((size_t)4 << 20)" in header and "KBEST_FRONTIER_WORK_CAP ((size_t)1 << 30)" in header
    assert (engine.KBEST_FRONTIER_MAX_COLS, engine.KBEST_FRONTIER_MAX_WIDTH, engine.KBEST_FRONTIER_SLOT) == (fc.MAX_COLS, fc.MAX_WIDTH, fc.SLOT)


def test_frontier_without_gpu_fails_loudly(lib):
    if lib.kbest_device_count() > 0:
        return  # (a GPU is present: tests/test_gpu_frontier.py has the rest)
    with pytest.raises(pk.KBestError):
        pk.hybridFrontierProb(np.random.rand(12), 2, 3, 0)
