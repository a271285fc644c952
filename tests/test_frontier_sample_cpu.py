"""CPU: the restatement of the frontier sampler (tests/frontier_sample_check.py) against the truth -- the plain permutation sum of
every open cluster of at most 10 measurements of the sixteen scene frames (chi-square on the joints, the marginals of
frontier_check, the log-probabilities) --, its small clusters against cluster_sample_check, the validity of every draw, the
disjointness of the two counter domains; the kernel source itself on the host under sanitizers; without a GPU the entries fail
loudly."""
import os
import struct
import subprocess

import numpy as np
import pytest

import cluster_sample_check as csc
import frontier_check as fc
import frontier_sample_check as fsc
import probabilisticsemslam_amd as pk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIXTEEN = tuple(range(16))
N = 4096


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pk.lib_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "probabilisticsemslam_amd", "csrc")])
    return pk.load_library()


def joints_of(L):
    """{tuple of the sub-block row of every column: weight} of a cluster by the plain permutation sum over its non-zero entries."""
    R, m = L.A.shape
    options = [[r for r in range(R) if L.A[r, c] > 0.0] for c in range(m)]
    out = {}

    def rec(c, used, rows, w):
        if c == m:
            out[tuple(rows)] = w
            return
        for r in options[c]:
            if not (used >> r) & 1:
                rec(c + 1, used | (1 << r), rows + [int(L.rows[r])], w * L.A[r, c])

    rec(0, 0, [], 1.0)
    return out


def test_open_clusters_follow_the_truth():
    """Frames 0 .. 15 of scene_frames(200, 40, 24, 24.0), conditioned, max_exact = 4: open clusters of 5 .. 15 columns, W <= 9.
    Every open cluster of at most 10 columns: 4 096 draws against its permutation sum -- z = (chi2 - n) / sqrt(2 n) < 4 over the
    joints with expectation >= 5, the empirical marginals within 4 / sqrt(N) of frontier_check's, logTerm within 1e-12 of
    log(weight / Z)."""
    worst_z = worst_m = worst_l = 0.0
    margin, seen_clusters, sizes, widths = np.inf, 0, [], []
    for b, o in fsc.open_clusters(fsc.SMALL, SIXTEEN):
        sizes.append(o["m"])
        L = fsc.cluster_layers(o["block"], o["nL"], o["m"])
        widths.append(L.W)
        assert L.info == 1
        if o["m"] > 10:
            continue
        seen_clusters += 1
        asg, lt, mg = fsc.walk(L, o["keys"], N, fsc.SEED, b)
        joint = joints_of(L)
        Z = sum(joint.values())
        assert abs(Z - L.Z) <= 1e-12 * Z
        seen = {}
        for row in asg.tolist():
            seen[tuple(row)] = seen.get(tuple(row), 0) + 1
        assert set(seen) <= set(joint)  # no gated entry is drawn, no row twice: every draw is a term of the sum
        chi2 = n = 0
        for rows, w in joint.items():
            if N * w / Z >= 5.0:
                chi2 += (seen.get(rows, 0) - N * w / Z) ** 2 / (N * w / Z)
                n += 1
        assert n >= 2, (b, o["m"])
        z = (chi2 - n) / np.sqrt(2.0 * n)
        want, _, info, _ = fc.frontier_cluster(o["block"], o["nL"], o["m"])
        emp = np.zeros((o["m"], o["nL"] + 1))
        for c in range(o["m"]):
            np.add.at(emp[c], np.minimum(asg[:, c], o["nL"]), 1.0 / N)
        truth = np.log(np.array([joint[tuple(r)] for r in asg.tolist()]) / Z)
        worst_z, worst_m = max(worst_z, z), max(worst_m, np.abs(emp - want).max() * np.sqrt(N))
        worst_l, margin = max(worst_l, np.abs(lt - truth).max()), min(margin, mg)
    print(f"{seen_clusters} clusters of {sorted(sizes)} columns (W up to {max(widths)}): worst z {worst_z:.3g}, worst marginal error "
          f"{worst_m:.3g} / sqrt(N), logTerm {worst_l:.3g}, smallest margin {margin:.3g}")
    assert min(sizes) == 5 and max(sizes) == 15 and max(widths) <= 9 and seen_clusters >= 20
    assert worst_z < 4.0 and worst_m <= 4.0 and worst_l <= 1e-12


def test_small_clusters_are_the_clustered_samplers():
    """A frame with small and open clusters: the small clusters' columns EQUAL cluster_sample_check's (the clustered sampler takes
    the whole frame at its own limit of 16), every column is assigned, no row is taken twice, no gated entry is drawn."""
    import hybrid_check as hc
    _, nL, nM, _ = fsc.SMALL
    for b in (0, 2, 10):
        d = fsc.frame_draws(fsc.SMALL, b, 512)
        f = fsc.scene(*fsc.SMALL)[b]
        whole = csc.clustered_sample_assoc(f, nL, nM, 512, seed=fsc.SEED, condition=True, frame_key=b)
        assert d.method == 0 and d.nopen >= 1 and len(d.small_cols) >= 1 and whole.info > 0
        assert np.array_equal(d.assign[:, d.small_cols], whole.assign[:, d.small_cols]), b
        assert (d.assign >= 0).all()
        _, A = hc.gated_block(f, nL, nM, True)
        for row in d.assign:
            assert len(set(row.tolist())) == nM and (A[row, np.arange(nM)] > 0.0).all(), b
        # the frame's log-probability: the product of the drawn entries over the product of the clusters' Z
        parts, _ = csc.cluster_parts(f, nL, nM, True)
        small_z = sum(np.log(p.Z) for p in parts if int(p.cols[0]) in set(d.small_cols.tolist()))
        open_z = sum(np.log(fsc.cluster_layers(o["block"], o["nL"], o["m"]).Z) for o in d.opens)
        colscale = sum(fsc.cluster_layers(o["block"], o["nL"], o["m"]).colmin.sum() for o in d.opens)
        want = np.log(A[d.assign, np.arange(nM)]).sum(axis=1) + colscale - small_z - open_z
        assert np.abs(d.logp - want).max() <= 1e-11, b
    # nothing open: the clustered sampler's draws, bit for bit
    d = fsc.frame_draws(fsc.SMALL, 0, 64, max_exact=16)
    whole = csc.clustered_sample_assoc(fsc.scene(*fsc.SMALL)[0], nL, nM, 64, seed=fsc.SEED, condition=True, frame_key=0)
    assert d.nopen == 0 and np.array_equal(d.assign, whole.assign)
    assert np.array_equal(d.logp.view(np.int64), whole.logp.view(np.int64)) and d.logperm == whole.logperm


def test_counter_domains_are_disjoint():
    """The counters themselves: the clustered sampler's second word is (active row) >> 1 <= 511, the frontier sampler's has bit 31
    set -- for every row key a frame can hold."""
    small = {i >> 1 for i in range(1024)}
    big = {fsc.counter(q)[0] for q in range(1024 + 128)}
    assert max(small) == 511 and min(big) >= 1 << 31 and not small & big
    assert fsc.counter(6) == (0x80000003, 0) and fsc.counter(7) == (0x80000003, 1)
    draw = np.arange(4, dtype=np.uint64)
    import sample_check as sc
    assert not np.array_equal(fsc.uniforms(7, draw, 6, 3), sc.uniforms(7, draw, 6, 3))
    assert not np.array_equal(fsc.uniforms(7, draw, 6, 3), fsc.uniforms(7, draw, 7, 3))


def test_refusals_of_the_restatement():
    _, nL, nM, _ = fsc.SMALL
    # max_width = 5 refuses the frames whose open cluster is wider, and no other
    refused = [b for b in SIXTEEN if fsc.frame_draws(fsc.SMALL, b, 4, max_width=5).method == -1]
    assert refused == [8, 10, 12, 15]
    d = fsc.frame_draws(fsc.SMALL, 8, 4, max_width=5)
    assert (d.assign == -1).all() and np.isnan(d.logp).all() and np.isnan(d.logperm)
    blk = fc.edge_clusters()["same_only_row"]
    a, lt, lz, info, W, _ = fsc.sample_cluster(*blk, np.arange(4), 3)
    assert info == 0 and (a == -1).all() and np.isnan(lt).all() and lz == -np.inf
    assert fsc.sample_cluster(*fc.edge_clusters()["width_17"], np.arange(19), 3)[3] == fc.REFUSED_WIDTH


def host_cases():
    """Three clusters of the sixteen frames: the widest (W = 9, 15 columns), the one of 12 columns, and one of 5."""
    oc = fsc.open_clusters(fsc.SMALL, SIXTEEN)
    pick = [next((b, o) for b, o in oc if o["m"] == m) for m in (15, 12, 5)]
    assert fsc.cluster_layers(pick[0][1]["block"], pick[0][1]["nL"], 15).W == max(
        fsc.cluster_layers(o["block"], o["nL"], o["m"]).W for _, o in oc)
    return pick


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    """The two host programs under AddressSanitizer and UBSan, built once for the module."""
    tmp_path = tmp_path_factory.mktemp("host")
    (tmp_path / "hip").mkdir()
    (tmp_path / "hip" / "hip_runtime.h").write_text("")
    csrc = os.path.join(ROOT, "probabilisticsemslam_amd", "csrc")
    out = {}
    for name in ("frontier_sample_host", "frontier_host"):
        out[name] = str(tmp_path / name)
        subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-I", str(tmp_path), "-I", os.path.join(ROOT, "include"), "-I", csrc, "-x", "c++",
                               os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", out[name], "-lpthread"])
    return out


def test_kernel_source_on_the_host_under_sanitizers(tmp_path, exes):
    """tests/cpp/frontier_sample_host.cpp: the kernel's own source as 256 host threads per workgroup, AddressSanitizer and UBSan on,
    heap blocks of exactly the planned sizes; 256 draws of three clusters equal the restatement (margin >= 1e-10 asserted first),
    logTerm within 1e-12, log Z equal to the frontier tier's host program."""
    cases, n_sample, seed, base = host_cases(), 256, fsc.SEED, 7
    want = [fsc.sample_cluster(o["block"], o["nL"], o["m"], o["keys"], n_sample, seed, b, base) for b, o in cases]
    assert all(w[3] == 1 and w[5] >= 1e-10 for w in want), [w[5] for w in want]
    need = max(fc.layers_bytes(fc.row_masks(fc.scaled_block(o["block"], o["nL"], o["m"])[0]), o["m"]) for _, o in cases) // 8
    src, plain = tmp_path / "in.bin", tmp_path / "plain.bin"
    with open(src, "wb") as f, open(plain, "wb") as g:
        f.write(struct.pack("iiQII", len(cases), n_sample, seed, base, 0))
        g.write(struct.pack("i", len(cases)))
        for b, o in cases:
            blk = np.asarray(o["block"], dtype=np.float64).tobytes()
            f.write(struct.pack("iiQ", o["m"], o["nL"], b) + blk + np.asarray(o["keys"], dtype=np.int32).tobytes())
            g.write(struct.pack("ii", o["m"], o["nL"]) + blk)
    ref = tmp_path / "ref.bin"
    subprocess.check_call([exes["frontier_host"], str(plain), str(ref)])
    rbuf, rat, ref_logz = ref.read_bytes(), 0, []
    for b, o in cases:
        info, width, lz = struct.unpack_from("iid", rbuf, rat)
        rat += 16 + 8 * o["m"] * (o["nL"] + 1)
        ref_logz.append((info, width, lz))
    for args in ([], [str(need), "1"]):  # two workgroups striding; then one, its slot exactly the need of the largest cluster
        out = tmp_path / "out.bin"
        subprocess.check_call([exes["frontier_sample_host"], str(src), str(out)] + args)
        buf, at = out.read_bytes(), 0
        for (b, o), w, r in zip(cases, want, ref_logz):
            info, width, lz = struct.unpack_from("iid", buf, at)
            asg = np.frombuffer(buf, dtype=np.int32, count=n_sample * o["m"], offset=at + 16).reshape(n_sample, o["m"])
            lt = np.frombuffer(buf, dtype=np.float64, count=n_sample, offset=at + 16 + 4 * n_sample * o["m"])
            at += 16 + 4 * n_sample * o["m"] + 8 * n_sample
            assert (info, width) == (1, w[4]) == r[:2] and lz == r[2], (b, o["m"])
            assert abs(lz - w[2]) <= 1e-12 * max(1.0, abs(w[2]))
            assert np.array_equal(asg, w[0]), (b, o["m"])
            assert np.abs(lt - w[1]).max() <= 1e-12, (b, o["m"])
        assert at == len(buf)


def shared_forward_cases():
    """[(name, block, nL, m)]: the inputs of the two host tests, the smallest shapes of frontier_check (widths 16 and 17 among
    them), and the shapes of tests/range_lib.py: hubs, two hubs, pair chains down to a declined one, clusters without a matching."""
    import range_lib as rl
    out = [(f"frame {b}, {o['m']} columns", o["block"], o["nL"], o["m"]) for b, o in host_cases()]
    out += [(n, *fc.edge_clusters()[n]) for n in ("one_by_one", "two_by_one", "fewer_states_than_a_wave", "opens_and_closes_in_one_row",
                                                  "band_of_24", "same_only_row", "width_16", "width_17")]
    A = fc.raw_cluster(fc.FAMILIES[1], 89, (58, 25))
    with np.errstate(divide="ignore"):
        blk = np.full((58 + 25, 25), np.inf)
        blk[:58] = -np.log(A)
    out.append(("25 x 58", np.ascontiguousarray(blk.T).reshape(-1), 58, 25))
    cases = [rl.hub(17, 36), rl.two_hubs(16, 41), rl.pair_chain(9, 41), rl.pair_chain(32, 20), rl.pair_chain(32, 25)]
    cases += list(rl.no_matching().values())
    return out + [(c.name, c.block, c.nLk, c.m) for c in cases]


def test_tier_and_sampler_write_the_same_info_width_and_log_z(tmp_path, exes):
    """The sampler restates the tier's plan and forward sweep: on the same clusters frontier_host and frontier_sample_host
    write the same (info, width, logZ), byte for byte -- answered, without a matching, refused for its width,
    declined below the range, and, the width-16 cluster alone in a slot one double below its need, refused for the slot."""
    every, n_sample = shared_forward_cases(), 2
    (wide,) = [c for c in every if c[0] == "width_16"]
    need = fc.layers_bytes(fc.row_masks(fc.scaled_block(*wide[1:])[0]), wide[3]) // 8
    seen = set()
    for cases, args in ((every, []), ([wide], [str(need - 1), "1"])):
        src, plain, tier, draw = (tmp_path / n for n in ("in.bin", "plain.bin", "tier.bin", "draw.bin"))
        with open(src, "wb") as f, open(plain, "wb") as g:
            f.write(struct.pack("iiQII", len(cases), n_sample, fsc.SEED, 0, 0))
            g.write(struct.pack("i", len(cases)))
            for k, (_, block, nL, m) in enumerate(cases):
                blk = np.asarray(block, dtype=np.float64).tobytes()
                f.write(struct.pack("iiQ", m, nL, k) + blk + np.arange(nL + m, dtype=np.int32).tobytes())
                g.write(struct.pack("ii", m, nL) + blk)
        subprocess.check_call([exes["frontier_host"], str(plain), str(tier)] + args)
        subprocess.check_call([exes["frontier_sample_host"], str(src), str(draw)] + args)
        tbuf, dbuf, tat, dat = tier.read_bytes(), draw.read_bytes(), 0, 0
        for name, _, nL, m in cases:
            assert tbuf[tat:tat + 16] == dbuf[dat:dat + 16], (name, struct.unpack_from("iid", tbuf, tat), struct.unpack_from("iid", dbuf, dat))
            seen.add(struct.unpack_from("i", tbuf, tat)[0])
            tat += 16 + 8 * m * (nL + 1)
            dat += 16 + 4 * n_sample * m + 8 * n_sample
        assert tat == len(tbuf) and dat == len(dbuf)
    assert seen == {1, 0, fc.REFUSED_SLOT, fc.REFUSED_WIDTH, -5}, seen


def test_frontier_sample_without_gpu_fails_loudly(lib):
    if lib.kbest_device_count() > 0:
        return  # (a GPU is present: tests/test_gpu_frontier_sample.py has the rest)
    with pytest.raises(pk.KBestError):
        pk.hybridFrontierSampleAssoc(np.random.rand(12), 2, 3, 4)
