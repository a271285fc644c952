"""GPU: joint associations drawn from tables of k best assignments (kbest_table_sample.hip, kbest_table_sample_f64_dev,
kbest_hybrid_sample_assoc_batch_f64, the hybridSampleAssoc shim) against the numpy restatement of tests/table_sample_check.py --
never against the kernel's own output.  The draws are compared for EXACT equality: the two sides differ by the last bits of exp, so
every case first asserts that the smallest relative margin of its restatement, min |T - P_j| / total over every slot, is at least
1e-10 (tests/test_table_sample_cpu.py asserts the same without a GPU); then assign and pick exactly and logTerm / logProb within
1e-12.  With k = 0 the frame entry is compared with kbest_hybrid_frontier_sample_assoc_batch_f64 bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import frontier_sample_check as fsc
import probabilisticsemslam_amd as pk
import table_sample_check as tsc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_MARGIN = 1e-10
BAD_ARG = -2  # KBEST_ERR_BAD_ARG
PAD = 64
SMALL, SEED, SIXTEEN, K = tsc.SMALL, tsc.SEED, tsc.SIXTEEN, tsc.K_GPU


@pytest.fixture(scope="module")
def eng():
    e = pk.KBestEngine(0)
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(x, y):
    """Every output of two calls of the frame entries, bit for bit (lists of arrays, float arrays, integer arrays)."""
    for a, b in zip(x, y):
        if isinstance(a, list):
            assert len(a) == len(b)
            for p, q in zip(a, b):
                assert np.array_equal(bits(p), bits(q)) if p.dtype == np.float64 else np.array_equal(p, q)
        else:
            assert np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b)


def run_tables(eng, problems, n, cluster_key, frame_key, seed=tsc.HAND_SEED, base=3, with_pick=True):
    """kbest_table_sample_f64_dev on [(row4col [k, maxCol], gain [k], nf, m)] of one shape, sentinels between and around
    everything.  Returns one (assignLocal [n, m], pick [n], logTerm [n], info) per problem; untouched: -5 / -5 / -5.0 / -77."""
    dev = torch.device("cuda", 0)
    k, max_col = problems[0][0].shape
    P = len(problems)
    tab = np.stack([np.asarray(p[0], dtype=np.int32) for p in problems])
    gain = np.stack([np.asarray(p[1], dtype=np.float64) for p in problems])
    nf = np.array([p[2] for p in problems], np.int32)
    ms = [max(int(p[3]), 0) for p in problems]
    asgOff, ltOff = [], []
    aat = lat = PAD
    for m in ms:
        asgOff.append(aat)
        ltOff.append(lat)
        aat += n * min(m, max_col) + PAD
        lat += n + PAD
    d_tab, d_gain, d_nf = (torch.from_numpy(x).to(dev) for x in (tab, gain, nf))
    d_asg = torch.full((aat,), -5, dtype=torch.int32, device=dev)
    d_lt = torch.full((lat,), -5.0, dtype=torch.float64, device=dev)
    d_pick = torch.full((P + 2, n), -5, dtype=torch.int32, device=dev)
    d_info = torch.full((P + 2,), -77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    eng.table_sample_dev(k, max_col, [p[3] for p in problems], d_tab, d_gain, d_nf, n, d_asg, asgOff, d_lt, ltOff,
                         d_pick[1:] if with_pick else None, d_info[1:], cluster_key=cluster_key, frame_key=frame_key, seed=seed,
                         sample_base=base)
    torch.cuda.synchronize()
    assert np.array_equal(d_tab.cpu().numpy(), tab) and np.array_equal(bits(d_gain.cpu().numpy()), bits(gain))
    asg, lt, pick, info = d_asg.cpu().numpy(), d_lt.cpu().numpy(), d_pick.cpu().numpy(), d_info.cpu().numpy()
    assert (pick[0] == -5).all() and (pick[-1] == -5).all() and info[0] == -77 and info[-1] == -77
    if not with_pick:
        assert (pick == -5).all()
    out, aend, lend = [], 0, 0
    for j, m in enumerate(ms):
        assert (asg[aend: asgOff[j]] == -5).all() and (lt[lend: ltOff[j]] == -5.0).all(), j  # nothing between the problems
        mm = min(m, max_col)
        aend, lend = asgOff[j] + n * mm, ltOff[j] + n
        out.append((asg[asgOff[j]: aend].reshape(n, mm), pick[1 + j], lt[ltOff[j]: lend], int(info[1 + j])))
    assert (asg[aend:] == -5).all() and (lt[lend:] == -5.0).all()
    return out


def check_problem(got, want, name):
    assert want[3] >= MIN_MARGIN, (name, want[3])
    assert got[3] == 1, name
    assert np.array_equal(got[1], want[1]), name
    assert np.array_equal(got[0], want[0]), name
    assert np.abs(got[2] - want[2]).max() <= 1e-12, name


# ---- 1. the low-level entry -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tsc.handcrafted()))
def test_handcrafted_tables(eng, name):
    cases = tsc.handcrafted()
    r4c, g, nf, m = cases[name]
    n = tsc.HAND_DRAWS.get(name, 64)
    got = run_tables(eng, [cases[name]], n, [list(cases).index(name)], [5])[0]
    want = tsc.handcrafted_draws(name)
    if name == "nf_0":
        assert got[3] == 0 and (got[0] == -1).all() and (got[1] == -1).all() and np.isnan(got[2]).all()
        return
    check_problem(got, want, name)
    if name == "nf_1":
        assert (got[1] == 0).all() and (bits(got[2]) == 0).all()  # every pick is 0, logTerm is exactly 0.0
    if name == "cutoff_edge":
        assert not (got[1] >= 3).any()  # gain_0 + 42 is never picked (and its neighbour weighs exp(-42))
    if name == "equal_gains":
        assert {1, 2} <= set(got[1].tolist())
    if name == "k_4096":
        assert len(set(got[1].tolist())) >= 32 and got[1].max() >= 256


def test_more_than_one_pack_and_shapes_out_of_range(eng):
    probs = tsc.pack_problems()
    P = len(probs)
    got = run_tables(eng, list(probs), tsc.PACK_N, list(range(P)), [1000 + i for i in range(P)])
    drawn = 0
    for i, (r4c, g, nf, m) in enumerate(probs):
        want = tsc.pack_draws(i)
        if want is None:  # m outside 1 .. maxCol: nothing is touched
            assert got[i][3] == -1 and (got[i][0] == -5).all() and (got[i][1] == -5).all() and (got[i][2] == -5.0).all(), i
        elif nf == 0:
            assert got[i][3] == 0 and (got[i][0] == -1).all() and (got[i][1] == -1).all() and np.isnan(got[i][2]).all(), i
        else:
            check_problem(got[i], want, i)
            drawn += 1
    assert drawn >= 60
    # without a pick array: the same rows
    again = run_tables(eng, list(probs[:5]), tsc.PACK_N, list(range(5)), [1000 + i for i in range(5)], with_pick=False)
    for i in range(1, 5):
        assert np.array_equal(again[i][0], got[i][0]) and np.array_equal(bits(again[i][2]), bits(got[i][2]))


def test_bad_arguments_of_the_low_level_entry(eng):
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    one, off = np.array([3], np.int32), np.zeros(1, np.int64)
    neg = np.array([-1], np.int64)
    key, big = np.array([5], np.uint32), np.array([1 << 30], np.uint32)
    dummy = C.c_void_p(8)

    def call(k=8, max_col=4, n_sample=4, base=0, ck=key, ao=off, lo=off):
        return eng.lib.kbest_table_sample_f64_dev(eng.ctx, 1, k, max_col, vp(one), dummy, dummy, dummy, 42.0, vp(ck), None, n_sample, 0,
                                                  base, dummy, vp(ao), dummy, vp(lo), None, None, None)

    # (every one of these returns before anything is launched: the dummy pointers are never used)
    assert call(k=4097) == BAD_ARG and call(k=0) == BAD_ARG and call(max_col=0) == BAD_ARG
    assert call(n_sample=0) == BAD_ARG and call(n_sample=2, base=2 ** 32 - 1) == BAD_ARG
    assert call(ck=big) == BAD_ARG and call(ao=neg) == BAD_ARG and call(lo=neg) == BAD_ARG
    assert eng.lib.kbest_table_sample_f64_dev(eng.ctx, 0, 8, 4, None, None, None, None, 42.0, None, None, 4, 0, 0, None, None, None, None,
                                              None, None, None) == 0
    # k = 4096 is accepted: the handcrafted case k_4096 draws from it


# ---- 2. the frame entry ------------------------------------------------------------------------------------------------------------------
def sixteen(eng, n, k, **kw):
    _, nL, nM, _ = SMALL
    frames = [fsc.scene(*SMALL)[b] for b in SIXTEEN]
    return eng.hybrid_sample_assoc(frames, [nL] * 16, [nM] * 16, n, k, seed=SEED, condition=True, max_exact=4, **kw)


def check_frame(got, j, want, name):
    asg, lp, logPerm, method, nOpen, nFr, nEn, maxc = got
    assert want.margin >= MIN_MARGIN, (name, want.margin)
    assert (method[j], nOpen[j], nFr[j], nEn[j], maxc[j]) == (want.method, want.nopen, want.nfrontier, want.nenum, want.maxc), name
    assert np.array_equal(asg[j], want.assign), name
    diff = np.abs(lp[j] - want.logp).max()
    assert diff <= 1e-12, (name, diff)
    assert abs(logPerm[j] - want.logperm) <= 1e-12 * max(1.0, abs(want.logperm)), name
    return diff


def test_every_open_cluster_enumerated(eng):
    """max_width = 0: all 25 open clusters of the sixteen frames go through the k-best engine in one batch and the table sampler."""
    got = sixteen(eng, tsc.N_GPU, K, max_width=0)
    worst, margins = 0.0, []
    for b in SIXTEEN:
        want = tsc.frame_draws(SMALL, b, tsc.N_GPU, K, max_width=0)
        worst = max(worst, check_frame(got, b, want, b))
        margins.append(want.margin)
        assert want.method in (1, 2) and want.nfrontier == 0
    print(f"enumerated clusters {got[6].tolist()}, methods {got[3].tolist()}, smallest margin {min(margins):.3g}, "
          f"largest logProb difference {worst:.3g}")
    assert got[6].sum() == 25 and (got[5] == 0).all()


def test_width_5_enumerates_what_the_frontier_tier_leaves(eng):
    n = 128
    _, nL, nM, _ = SMALL
    frames = [fsc.scene(*SMALL)[b] for b in SIXTEEN]
    got = sixteen(eng, n, K, max_width=5)
    old = eng.hybrid_frontier_sample_assoc(frames, [nL] * 16, [nM] * 16, n, seed=SEED, condition=True, max_exact=4, max_width=5)
    full = eng.hybrid_frontier_sample_assoc(frames, [nL] * 16, [nM] * 16, n, seed=SEED, condition=True, max_exact=4)
    assert np.flatnonzero(old[3] == -1).tolist() == [8, 10, 12, 15] and (full[3] == 0).all()
    for b in SIXTEEN:
        want = tsc.frame_draws(SMALL, b, n, K, max_width=5)
        check_frame(got, b, want, b)
        if b in (8, 10, 12, 15):
            assert got[3][b] in (1, 2) and got[6][b] >= 1
            # the columns of its small clusters and of the clusters the frontier tier still takes: what those samplers draw
            cols = list(want.small_cols) + [c for o in want.opens if o["tier"] == "frontier" for c in o["cols"]]
            assert len(cols) >= 1 and np.array_equal(got[0][b][:, cols], full[0][b][:, cols]), b
            assert any(o["tier"] == "kbest" for o in want.opens)
        else:  # the bits of the existing entry
            assert got[6][b] == 0 and got[3][b] == 0
            assert np.array_equal(got[0][b], old[0][b]) and np.array_equal(bits(got[1][b]), bits(old[1][b]))
            assert bits(got[2])[b] == bits(old[2])[b] and (got[4][b], got[5][b], got[7][b]) == (old[4][b], old[5][b], old[6][b])


def test_k_0_is_the_existing_entry(eng):
    _, nL, nM, _ = SMALL
    frames = [fsc.scene(*SMALL)[b] for b in SIXTEEN]
    for kw in (dict(max_width=5), dict(max_width=16), dict(max_width=0), dict(max_width=16, sample_base=9, frame_key=list(range(50, 66)))):
        a = sixteen(eng, 32, 0, **kw)
        b = eng.hybrid_frontier_sample_assoc(frames, [nL] * 16, [nM] * 16, 32, seed=SEED, condition=True, max_exact=4, **kw)
        same(a[:6] + a[7:], b)
        assert not a[6].any()
    a = sixteen(eng, 32, 0, max_width=5)
    assert np.flatnonzero(a[3] == -1).tolist() == [8, 10, 12, 15] and np.isnan(a[2][8]) and (a[0][8] == -1).all()


def test_a_frame_alone_first_and_last_in_a_batch_of_forty(eng):
    _, nL, nM, _ = SMALL
    b, key, n = tsc.BATCH_FRAME, tsc.BATCH_KEY, tsc.BATCH_N
    frames = [fsc.scene(*SMALL)[i] for i in range(40)]
    frames[0] = frames[39] = frames[b]
    keys = [key] + list(range(1, 39)) + [key]
    batch = eng.hybrid_sample_assoc(frames, [nL] * 40, [nM] * 40, n, K, seed=SEED, condition=True, max_exact=4, max_width=5, frame_key=keys)
    alone = eng.hybrid_sample_assoc([frames[b]], [nL], [nM], n, K, seed=SEED, condition=True, max_exact=4, max_width=5, frame_key=[key])
    want = tsc.frame_draws(SMALL, b, n, K, frame_key=key, max_width=5)
    assert want.nenum >= 1 and want.nfrontier + want.nenum == want.nopen
    check_frame(alone, 0, want, "alone")
    for j in (0, 39):
        assert np.array_equal(alone[0][0], batch[0][j]) and np.array_equal(bits(alone[1][0]), bits(batch[1][j]))
        assert bits(alone[2])[0] == bits(batch[2])[j] and [int(x[0]) for x in alone[3:]] == [int(x[j]) for x in batch[3:]]
    # sample_base continues a sequence
    half = n // 2
    for lo in (0, half):
        part = eng.hybrid_sample_assoc([frames[b]], [nL], [nM], half, K, seed=SEED, condition=True, max_exact=4, max_width=5,
                                       frame_key=[key], sample_base=lo)
        assert np.array_equal(part[0][0], alone[0][0][lo: lo + half]) and np.array_equal(bits(part[1][0]), bits(alone[1][0][lo: lo + half]))


def test_an_infeasible_enumerated_cluster_between_two_answered(eng):
    nL, nM = tsc.BLOCKS
    got = eng.hybrid_sample_assoc([tsc.block_frame(True), tsc.block_frame(False), tsc.block_frame(True)], [nL] * 3, [nM] * 3, 64, K,
                                  seed=SEED, max_exact=4, max_width=0, frame_key=[7, 7, 7])
    asg, lp, logPerm, method, nOpen, nFr, nEn, _ = got
    want = tsc.block_draws(True)
    assert tsc.block_draws(False).method == -2 and want.nenum == 3
    assert method[1] == -2 and (asg[1] == -1).all() and np.isnan(lp[1]).all() and logPerm[1] == -np.inf and nEn[1] == 0 and nOpen[1] == 3
    for j in (0, 2):
        check_frame(got, j, want, j)
    # a k beyond every cluster's assignments: each enumeration is complete within the cutoff, method 1
    whole = eng.hybrid_sample_assoc([tsc.block_frame(True)], [nL], [nM], 64, tsc.BLOCKS_ALL, seed=SEED, max_exact=4, max_width=0,
                                    frame_key=[7])
    assert method[0] == 2 and whole[3][0] == 1
    check_frame(whole, 0, tsc.block_draws(True, tsc.BLOCKS_ALL), "complete")


def test_cpp_shim_module_function_and_bad_arguments(eng, tmp_path):
    exe = str(tmp_path / "shim_table_sample")
    libdir = os.path.join(ROOT, "probabilisticsemslam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_table_sample.cpp"), "-o", exe,
                           "-L", libdir, "-l:libkbest_amd.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
                           "-L/opt/rocm/lib", "-lamdhip64"])
    nL, nM = tsc.DENSE
    frame, n, k = tsc.dense_frame(), tsc.DENSE_N, tsc.DENSE_K
    want = tsc.dense_draws()
    assert want.method == 2 and want.nenum == 1 and want.maxc == 18 and want.margin >= MIN_MARGIN
    path = tmp_path / "scene.txt"
    path.write_text(f"{nL} {nM}\n" + "\n".join("inf" if np.isinf(v) else float.hex(float(v)) for v in frame) + "\n")
    lines = subprocess.check_output([exe, str(path), str(n), str(k), str(SEED)], text=True).splitlines()
    assert len(lines) == n + 2
    for s in range(n):
        tok = lines[s].split()
        assert tok[:2] == ["s", str(s)] and [int(v) for v in tok[2:]] == want.assign[s].tolist(), s
    assert lines[-2].startswith("k = 0: runtime_error hybridSampleAssoc: frame refused")
    assert lines[-1].startswith("empty column: runtime_error hybridSampleAssoc") and "no consistent association" in lines[-1]
    assert np.array_equal(pk.hybridSampleAssoc(frame, nL, nM, n, k, SEED), want.assign)
    got = eng.hybrid_sample_assoc([frame], [nL], [nM], n, k, seed=SEED, frame_key=[0])
    check_frame(got, 0, want, "dense")
    with pytest.raises(RuntimeError, match="refused"):
        pk.hybridFrontierSampleAssoc(frame, nL, nM, 1)
    with pytest.raises(RuntimeError, match="refused"):
        pk.hybridSampleAssoc(frame, nL, nM, 1, 0)
    for kw in (dict(k=-1), dict(k=4097), dict(max_exact=17), dict(max_width=17), dict(max_width=-1), dict(sample_base=2 ** 32 - 1)):
        args = dict(k=10)
        args.update(kw)
        with pytest.raises(pk.KBestError):
            eng.hybrid_sample_assoc([frame], [nL], [nM], 2, args.pop("k"), **args)
    out = eng.hybrid_sample_assoc([], [], [], 4, 10)
    assert out[0] == [] and out[3].size == 0
