"""CPU: the restatement of the table sampler (tests/table_sample_check.py) against the truth -- a chi-square of its draws against
the weights of one enumerated cluster, its weights against oracle_lib.weights_from_solutions on every open cluster of the sixteen
scene frames --, the disjointness of the three counter domains, k = 0 against frontier_sample_check, the margins of every case the
GPU tests use, and the selection of kbest_table_sample.h itself on the host under sanitizers."""
import os
import struct
import subprocess

import numpy as np

import frontier_sample_check as fsc
import oracle_lib as ol
import sample_check as sc
import table_sample_check as tsc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_MARGIN = 1e-10
K = 50


def test_draws_follow_the_tables_weights():
    """20 000 restated draws of one enumerated cluster (k = 50) against w / total: z = (chi2 - n) / sqrt(2 n) < 4 over the slots
    with expectation >= 5, as tests/test_sample_cpu.py has it for its joints; logTerm is log(w_j / total) within 1e-12."""
    N = 20000
    b, o = fsc.open_clusters(fsc.SMALL, tsc.SIXTEEN)[0]
    nf, r4c, g = tsc.enumerate_cluster(o, K)
    w, P, last = tsc.table_weights(g, nf)
    assert nf >= 10 and last == nf - 1
    asg, pick, lt, margin = tsc.sample_tables(r4c, g, nf, N, tsc.SEED, o["root"], b)
    assert margin >= MIN_MARGIN
    total = P[-1]
    seen = np.bincount(pick, minlength=nf)
    chi2 = n = 0
    for j in range(nf):
        if N * w[j] / total >= 5.0:
            chi2 += (seen[j] - N * w[j] / total) ** 2 / (N * w[j] / total)
            n += 1
    assert n >= 2
    z = (chi2 - n) / np.sqrt(2.0 * n)
    print(f"{nf} slots, {n} with expectation >= 5: z {z:.3g}, smallest margin {margin:.3g}")
    assert z < 4.0
    assert np.array_equal(asg, r4c[pick]) and np.abs(lt - np.log(w[pick] / total)).max() <= 1e-12


def test_weights_are_assignment_probs():
    """Every open cluster of frames 0 .. 15 of SMALL at max_exact = 4: the restatement's weights accumulated over the solutions are
    oracle_lib.weights_from_solutions within 1e-12 -- and with it assignment_prob, which hybrid_check.hybrid_probs uses."""
    worst = 0.0
    count = 0
    for b, o in fsc.open_clusters(fsc.SMALL, tsc.SIXTEEN):
        nLk, m = o["nL"], o["m"]
        nf, r4c, g = tsc.enumerate_cluster(o, K)
        assert nf >= 1
        w, P, _ = tsc.table_weights(g, nf)
        probs = np.zeros((m, nLk + 1))
        for j in range(nf):
            probs[np.arange(m), np.minimum(r4c[j], nLk)] += w[j]
        probs = probs / P[-1]
        want = ol.weights_from_solutions(r4c, g, nLk, m)
        direct, dnf = ol.assignment_prob(o["block"], nLk, m, K)
        assert dnf == nf
        worst = max(worst, np.abs(probs - want).max(), np.abs(probs - direct).max())
        count += 1
    print(f"{count} open clusters: largest difference {worst:.3g}")
    assert count == 25 and worst <= 1e-12


def test_counter_domains_are_disjoint():
    """The second word of the counter: the clustered sampler's is (active row) >> 1 <= 511, the frontier sampler's has bit 31 set,
    the table sampler's has bit 30 set and bit 31 clear -- for every key a frame can hold, and for the largest key."""
    small = {i >> 1 for i in range(1024)}
    frontier = {fsc.counter(q)[0] for q in range(1024 + 128)}
    table = {tsc.counter(c) for c in list(range(128)) + [tsc.MAX_KEY - 1]}
    assert all((w >> 30) == 1 for w in table) and all((w >> 31) == 1 for w in frontier) and max(small) == 511
    assert not small & table and not frontier & table and not small & frontier
    assert tsc.counter(5) == 0x40000005 and tsc.counter(tsc.MAX_KEY - 1) == 0x7FFFFFFF
    draw = np.arange(4, dtype=np.uint64)
    assert not np.array_equal(tsc.uniform(7, draw, 6, 3), sc.uniforms(7, draw, 6, 3))
    assert not np.array_equal(tsc.uniform(7, draw, 6, 3), fsc.uniforms(7, draw, 6, 3))
    assert not np.array_equal(tsc.uniform(7, draw, 6, 3), tsc.uniform(7, draw, 7, 3))
    assert not np.array_equal(tsc.uniform(7, draw, 6, 3), tsc.uniform(7, draw, 6, 4))


def test_k_0_is_the_frontier_restatement():
    for b, width in ((0, 16), (8, 5), (9, 5)):
        d = tsc.frame_draws(tsc.SMALL, b, 16, 0, max_width=width)
        w = fsc.frame_draws(fsc.SMALL, b, 16, max_width=width)
        assert d.method == w.method and d.nenum == 0 and (d.nopen, d.nfrontier, d.maxc) == (w.nopen, w.nfrontier, w.maxc)
        assert np.array_equal(d.assign, w.assign) and np.array_equal(d.logp.view(np.int64), w.logp.view(np.int64))
        assert d.logperm == w.logperm or (np.isnan(d.logperm) and np.isnan(w.logperm))
    assert tsc.frame_draws(tsc.SMALL, 8, 16, 0, max_width=5).method == -1


def test_every_gpu_case_has_its_margin():
    """What tests/test_gpu_table_sample.py compares exactly: the restatement alone decides every draw by at least 1e-10."""
    worst = np.inf
    for name in tsc.handcrafted():
        mg = tsc.handcrafted_draws(name)[3]
        assert mg >= MIN_MARGIN, (name, mg)
        worst = min(worst, mg)
    for i in range(len(tsc.pack_problems())):
        d = tsc.pack_draws(i)
        assert d is None or d[3] >= MIN_MARGIN, (i, d[3])
        worst = min(worst, np.inf if d is None else d[3])
    cases = tsc.gpu_frame_cases()
    for name, d in cases.items():
        assert d.method in (0, 1, 2) and d.margin >= MIN_MARGIN, (name, d.method, d.margin)
        worst = min(worst, d.margin)
    print(f"smallest margin of the GPU cases {worst:.3g}")
    # what the cases are there for
    assert sum(cases[f"all_enumerated_{b}"].nenum for b in tsc.SIXTEEN) == 25
    assert all(cases[f"all_enumerated_{b}"].nfrontier == 0 for b in tsc.SIXTEEN)
    assert [b for b in tsc.SIXTEEN if cases[f"width_5_{b}"].nenum >= 1] == [8, 10, 12, 15]
    assert cases["dense"].nenum == 1 and cases["dense"].maxc == 18 and cases["dense"].method == 2
    assert cases["blocks"].method == 2 and cases["blocks_complete"].method == 1
    assert [o["nf"] for o in cases["blocks_complete"].opens] == [501, 501, 501]
    assert cases["blocks"].nenum == 3 and tsc.block_draws(False).method == -2 and tsc.block_draws(False).logperm == -np.inf
    edge = tsc.handcrafted()["cutoff_edge"]
    w, _, last = tsc.table_weights(edge[1], edge[2])
    assert w[3] > 0.0 and w[4] == 0.0 and w[5] == 0.0 and last == 3  # one ulp below the cutoff is kept, the cutoff itself is not
    assert not (tsc.handcrafted_draws("cutoff_edge")[1] >= 4).any()
    assert (tsc.handcrafted_draws("nf_1")[1] == 0).all() and (tsc.handcrafted_draws("nf_1")[2] == 0.0).all()


def test_selection_on_the_host_under_sanitizers(tmp_path):
    """tests/cpp/table_sample_host.cpp: the selection of kbest_table_sample.h on the host, AddressSanitizer and UBSan on, heap
    blocks of exactly the needed sizes: the picks and rows of the handcrafted tables and of three enumerated clusters equal the
    restatement (margins asserted first), logTerm within 1e-12; the pick with T = total and beyond is the last slot with a weight."""
    (tmp_path / "hip").mkdir()
    (tmp_path / "hip" / "hip_runtime.h").write_text("")
    csrc = os.path.join(ROOT, "probabilisticsemslam_amd", "csrc")
    exe = str(tmp_path / "table_sample_host")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", str(tmp_path), "-I", os.path.join(ROOT, "include"), "-I", csrc, "-x", "c++",
                           os.path.join(ROOT, "tests", "cpp", "table_sample_host.cpp"), "-o", exe])
    n_sample, seed, base = 64, tsc.HAND_SEED, 3
    problems = []  # (row4col, gain, nf, m, cluster key, frame key)
    hand = tsc.handcrafted()
    for key, (name, (r4c, g, nf, m)) in enumerate(hand.items()):
        problems.append((r4c, g, nf, m, key, 5))
    for b, o in fsc.open_clusters(fsc.SMALL, tsc.SIXTEEN)[:3]:
        nf, r4c, g = tsc.enumerate_cluster(o, K)
        problems.append((np.ascontiguousarray(r4c), g, nf, o["m"], o["root"], b))
    want = [tsc.sample_tables(r4c, g, nf, n_sample, seed, ck, fk, base, m=m) for r4c, g, nf, m, ck, fk in problems]
    assert all(w[3] >= MIN_MARGIN for w in want), [w[3] for w in want]
    src, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("iiQII", len(problems), n_sample, seed, base, 0))
        for r4c, g, nf, m, ck, fk in problems:
            k, max_col = r4c.shape
            gk = np.full(k, np.nan)
            gk[: len(g)] = g
            f.write(struct.pack("iiiiIIQd", k, max_col, m, nf, ck, 0, fk, tsc.CUTOFF))
            f.write(np.ascontiguousarray(r4c, dtype=np.int32).tobytes() + gk.tobytes())
    subprocess.check_call([exe, str(src), str(out)])
    buf, at = out.read_bytes(), 0
    for (r4c, g, nf, m, ck, fk), w in zip(problems, want):
        info, last, total = struct.unpack_from("iid", buf, at)
        asg = np.frombuffer(buf, dtype=np.int32, count=n_sample * m, offset=at + 16).reshape(n_sample, m)
        pick = np.frombuffer(buf, dtype=np.int32, count=n_sample, offset=at + 16 + 4 * n_sample * m)
        lt = np.frombuffer(buf, dtype=np.float64, count=n_sample, offset=at + 16 + 4 * n_sample * (m + 1))
        edge = struct.unpack_from("iiii", buf, at + 16 + 4 * n_sample * (m + 1) + 8 * n_sample)
        at += 16 + 4 * n_sample * (m + 1) + 8 * n_sample + 16
        assert np.array_equal(pick, w[1]) and np.array_equal(asg, w[0]), ck
        if min(nf, r4c.shape[0]) <= 0:
            assert info == 0 and last == -1 and np.isnan(lt).all() and (pick == -1).all()
            continue
        _, P, wlast = tsc.table_weights(g, min(nf, r4c.shape[0]))
        assert info == 1 and last == wlast and abs(total - P[-1]) <= 1e-12 * P[-1]
        assert np.abs(lt - w[2]).max() <= 1e-12
        assert edge[:3] == (wlast, wlast, 0), ck  # T = total, T beyond it: the fall-through; T = 0: the first slot
    assert at == len(buf)
