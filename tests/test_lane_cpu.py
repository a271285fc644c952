"""CPU: the lane-per-child k-best kernel (kbest_lane.hip) and the launch behind it (finish_tables_kernel) compiled for the host from
their own text -- tests/cpp/lane_host.cpp, a stand-alone program under AddressSanitizer and UBSan, -ffp-contract=off, nothing loaded
into python.  The work space, every output table and each workgroup's LDS are exact-size heap blocks PREFILLED with 0x00, 0xFF or
seeded random bytes: each case runs with all three and must (a) end clean under both sanitizers and (b) give, with every fill, the
checker's answer (oracle_lib: k + 1 solutions where the kernel enumerates one more for the tie check) -- nf, the bits of the gains and of
tieGain, the tie flags, the tables up to nf -- with every slotSid[s], s < nf, inside the problem's state slots.  An index read from
memory that nobody wrote fails one of the two.  Three mutants of the kernel's text prove that the detector detects.

All runs are started together, once (the thread emulation waits more than it computes); the tests read the results."""
import concurrent.futures
import os

import numpy as np
import pytest

import lane_host_lib as lh
import oracle_lib as ol

F_I8, F_NO_REORDER = 64, 128
INF = np.inf


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def uniform(seed, B, N, M):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (B, N * M))


def faulted16():
    """Problems 0-7 and 692-699 of the launch that faulted on the GPU (tests/test_gpu_round3.py, shape1), as one batch."""
    c = np.random.default_rng(16016).uniform(0, 1, (700, 256))
    return np.concatenate([c[:8], c[692:]])


def with_inf(seed, N, frac):
    """N x N with a fraction of +inf entries, the diagonal finite (a feasible root)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.0, 1.0, (N, N))
    c[rng.uniform(size=(N, N)) < frac] = INF
    c[np.arange(N), np.arange(N)] = rng.uniform(0.0, 1.0, N)
    return c.T.reshape(1, N * N)  # column-major


def one_inf_column(seed, N, col):
    c = uniform(seed, 1, N, N)
    c[0, col * N:(col + 1) * N] = INF
    return c


def one_inf_row(seed, N, row):
    c = uniform(seed, 1, N, N)
    c[0, row::N] = INF
    return c


def ragged12():
    """maxRow = maxCol = 12 with shape arrays: full, N < maxRow square, M < N (padded columns), an empty frame, N < M (nf = -1)."""
    rng = np.random.default_rng(1212)
    shapes = [(12, 12), (9, 9), (10, 6), (0, 0), (5, 8), (1, 1)]
    costs = np.zeros((len(shapes), 144))
    for b, (n, m) in enumerate(shapes):
        costs[b, :n * m] = rng.uniform(0.0, 1.0, n * m)
    return costs, [s[0] for s in shapes], [s[1] for s in shapes]


# name -> (costs, maxRow, maxCol, k, options of lane_host_lib.run, options of the check)
def make_cases():
    C = {}
    C["faulted16"] = (faulted16(), 16, 16, 30, dict(spec=12, waves=4), {})
    C["faulted_first2"] = (faulted16()[:2], 16, 16, 30, dict(spec=12, waves=4), {})  # (what mutant 2 is run on)
    for n in (1, 2, 3, 15, 16):        # 4 rows per lane
        C["rows4_n%d" % n] = (uniform(40 + n, 1, n, n), n, n, 6, dict(spec=4, waves=2), {})
    for n in (17, 31, 32):             # 8 rows per lane
        C["rows8_n%d" % n] = (uniform(80 + n, 1, n, n), n, n, 5, dict(spec=4, waves=4), {})
    for w in (1, 2, 4):
        C["waves%d" % w] = (uniform(300 + w, 2, 8, 8), 8, 8, 12, dict(spec=4, waves=w), {})
    # the in-place merge: one pool entry per thread (kernel-side k = 64 on one wave) and four (65)
    C["merge_k64"] = (uniform(64, 1, 7, 7), 7, 7, 64, dict(spec=8, waves=1, tie=False), {})
    C["merge_k65"] = (uniform(65, 1, 7, 7), 7, 7, 65, dict(spec=8, waves=1, tie=False), {})
    for s in (1, 4, 12, 16):
        C["spec%d" % s] = (uniform(500 + s, 1, 10, 10), 10, 10, 12, dict(spec=s, waves=2), {})
    C["keys_dijkstra_32"] = (uniform(3201, 1, 32, 32), 32, 32, 4, dict(spec=1, waves=4), dict(closure=False))
    C["keys_closure_32"] = (uniform(3208, 1, 32, 32), 32, 32, 4, dict(spec=8, waves=4), dict(closure=True))
    rc, rn, rm = ragged12()
    C["ragged12"] = (rc, 12, 12, 8, dict(spec=4, waves=2, nRow=rn, nCol=rm), {})
    C["padded_10x6"] = (uniform(106, 2, 10, 6), 10, 6, 9, dict(spec=4, waves=2), {})
    C["k1_root_only"] = (uniform(11, 2, 6, 6), 6, 6, 1, dict(spec=4, waves=1, tie=False), {})
    C["k1_and_one_behind"] = (uniform(12, 2, 6, 6), 6, 6, 1, dict(spec=4, waves=1), {})
    C["k2"] = (uniform(13, 2, 6, 6), 6, 6, 2, dict(spec=4, waves=1, tie=False), dict(reorder=False))
    C["k3_m3_reorder"] = (uniform(14, 2, 3, 3), 3, 3, 3, dict(spec=4, waves=1, tie=False), dict(reorder=True))
    C["pool_runs_dry"] = (uniform(15, 2, 3, 3), 3, 3, 10, dict(spec=4, waves=1), dict(nf=6))
    C["inf_column"] = (one_inf_column(21, 6, 2), 6, 6, 5, dict(spec=4, waves=1), dict(nf=0))
    C["inf_row"] = (one_inf_row(22, 6, 4), 6, 6, 5, dict(spec=4, waves=1), dict(nf=0))
    C["inf_scattered"] = (np.concatenate([with_inf(23, 8, 0.3), with_inf(24, 8, 0.5)]), 8, 8, 14, dict(spec=4, waves=2), {})
    C["maximize"] = (uniform(31, 2, 9, 9), 9, 9, 10, dict(spec=4, waves=2, maximize=True), {})
    C["cutoff_inside"] = (uniform(32, 2, 9, 9), 9, 9, 12, dict(spec=4, waves=2), dict(cut_between=(4, 5)))
    C["tables_i8"] = (uniform(33, 2, 9, 9), 9, 9, 10, dict(spec=4, waves=2, flags=F_I8), {})
    C["no_reorder"] = (uniform(34, 2, 9, 9), 9, 9, 10, dict(spec=4, waves=2, flags=F_NO_REORDER), {})
    C["shard0of2"] = (uniform(35, 2, 7, 7), 7, 7, 10, dict(spec=4, waves=2, tie=False, root=(0, 2)), dict(shard=True))
    C["shard1of2"] = (uniform(35, 2, 7, 7), 7, 7, 10, dict(spec=4, waves=2, tie=False, root=(1, 2)), dict(shard=True))
    C["ties_int_8x8"] = (np.floor(uniform(36, 2, 8, 8) * 4.0), 8, 8, 40, dict(spec=12, waves=2), dict(ties=True))
    return C


CASES = make_cases()
# (mutant, the case it is run on)
MUTANT_RUNS = [(1, "waves1"), (2, "faulted_first2"), (3, "waves1")]


def resolve_cutoff(name):
    """cut_between = (i, j): a cutoff half way between the i-th and the j-th best gain of problem 0, relative to its best."""
    costs, N, M, k, opts, chk = CASES[name]
    if "cut_between" in chk and "cutoff" not in opts:
        i, j = chk["cut_between"]
        _, _, _, g = ol.orc_kbest(costs[0], N, M, k)
        opts["cutoff"] = float(0.5 * (g[i] + g[j]) - g[0])
    return opts


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Builds the program (and the three mutants) and runs every case with every fill, all at once."""
    tmp = tmp_path_factory.mktemp("lane_host")
    jobs = {}
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(2, min(8, os.cpu_count() or 2))) as pool:
        builds = {m: pool.submit(lh.build, tmp, lh.ASAN, m, "-O0") for m in (0, 1, 2, 3)}
        exe = {m: b.result() for m, b in builds.items()}
        n = 0
        for name in CASES:
            costs, N, M, k, _, _ = CASES[name]
            opts = resolve_cutoff(name)
            for fill in lh.FILLS:
                d = tmp / ("job%d" % n)
                d.mkdir()
                n += 1
                jobs[(0, name, fill)] = pool.submit(lh.run, exe[0], d, costs, N, M, k, fill=fill, seed=1000 + n, check=False, **opts)
        for m, name in MUTANT_RUNS:
            costs, N, M, k, _, _ = CASES[name]
            for fill in lh.FILLS:
                d = tmp / ("job%d" % n)
                d.mkdir()
                n += 1
                jobs[(m, name, fill)] = pool.submit(lh.run, exe[m], d, costs, N, M, k, fill=fill, seed=1000 + n, check=False, **CASES[name][4])
        return {key: j.result() for key, j in jobs.items()}


def canon(c4r, M):
    c = np.array(c4r, copy=True)
    c[c >= M] = -1  # rows on zero-padded columns: which padded column is a tie artefact
    return c


def truth_of(name, b):
    """The checker's answer for problem b of a case: (nf, row4col, col4row, gain, the gain behind the tables or NaN)."""
    costs, N, M, k, opts, chk = CASES[name]
    n = opts["nRow"][b] if "nRow" in opts else N
    m = opts["nCol"][b] if "nCol" in opts else M
    if n < 1 or m < 1:
        return 0, None, None, None, np.nan
    if n < m:
        return -1, None, None, None, np.nan
    ke = k + 1 if opts.get("tie", True) else k
    onf, r4c, c4r, g = ol.orc_kbest(costs[b, :n * m], n, m, ke, maximize=opts.get("maximize", False), cutoff=opts.get("cutoff"))
    behind = g[k] if onf > k else np.nan
    return min(onf, k), r4c, c4r, g, behind


def mismatch(name, res):
    """None if the run's result is the truth, else a description of the first difference."""
    costs, N, M, k, opts, chk = CASES[name]
    tie = opts.get("tie", True)
    if res is None:
        return "no result"
    for b in range(costs.shape[0]):
        nf, r4c, c4r, g, behind = truth_of(name, b)
        if int(res["nf"][b]) != nf:
            return "problem %d: nf %d, truth %d" % (b, res["nf"][b], nf)
        if nf <= 0:
            continue
        n = opts["nRow"][b] if "nRow" in opts else N
        m = opts["nCol"][b] if "nCol" in opts else M
        sid = res["slotSid"][b, :nf]
        if sid.min() < 0 or sid.max() >= res["statesPerProblem"]:
            return "problem %d: slotSid outside [0, %d): %s" % (b, res["statesPerProblem"], sid)
        if chk.get("shard"):
            continue  # (a shard's own list: test_root_shards_merge_to_the_unsharded_answer)
        if not np.array_equal(bits(res["gain"][b, :nf]), bits(g[:nf])):
            return "problem %d: gains" % b
        if tie:
            if not (np.isnan(behind) and np.isnan(res["tieGain"][b])) and bits(res["tieGain"][b]) != bits(behind):
                return "problem %d: tieGain %r, truth %r" % (b, res["tieGain"][b], behind)
        if chk.get("ties"):
            why = mismatch_with_ties(name, b, res, nf, behind)
            if why:
                return why
            continue
        if tie and int(res["flags"][b]) != 0:
            return "problem %d: tie flags %d on tie-free costs" % (b, res["flags"][b])
        if not np.array_equal(res["row4col"][b, :nf, :m], r4c[:nf]):
            return "problem %d: row4col" % b
        if not np.array_equal(canon(res["col4row"][b, :nf, :n], m), canon(c4r[:nf], m)):
            return "problem %d: col4row" % b
    return None


def mismatch_with_ties(name, b, res, nf, behind):
    """Integer costs: per gain level the kernel's assignments against the checker's complete level, in the order of kbest_ties.h
    (row4col lexicographic in the reference's column order).  A level that ends inside the tables has exactly the checker's members;
    the level that straddles slot k has nf - (its start) distinct members of the checker's."""
    costs, N, M, k, opts, chk = CASES[name]
    cn, cr4c, cg, boundary, _ = ol.canonical_kbest(costs[b], N, M, k)
    got, gg = res["row4col"][b, :nf], res["gain"][b, :nf]
    if cn != nf or not np.array_equal(bits(gg), bits(cg)):
        return "problem %d: gains against the canonical order" % b
    want_flags = (1 if (np.diff(cg) == 0).any() else 0) | (2 if boundary else 0)
    if int(res["flags"][b]) != want_flags or boundary != (behind == cg[-1]):
        return "problem %d: tie flags %d, truth %d" % (b, res["flags"][b], want_flags)
    C = costs[b].reshape(M, N)  # [column][row]
    for level in np.unique(cg):
        idx = np.nonzero(cg == level)[0]
        rows = [tuple(r) for r in got[idx]]
        if rows != sorted(rows) or len(set(rows)) != len(rows):
            return "problem %d: level %r not in lexicographic order" % (b, level)
        if boundary and level == cg[-1]:
            for r in rows:  # any members of the level: a permutation with that gain (integer costs: the sum is exact)
                if sorted(r) != list(range(N)) or sum(C[c, r[c]] for c in range(M)) != level:
                    return "problem %d: level %r holds a row that is not of it" % (b, level)
        elif rows != [tuple(r) for r in cr4c[idx]]:
            return "problem %d: level %r" % (b, level)
        inv = res["col4row"][b, idx]
        for j, r in enumerate(rows):
            if [int(inv[j, r[c]]) for c in range(M)] != list(range(M)):
                return "problem %d: col4row is not the inverse of row4col" % b
    return None


@pytest.mark.parametrize("name", list(CASES))
def test_clean_under_sanitizers_and_the_truth_with_every_fill(runs, name):
    for fill in lh.FILLS:
        rc, err, res = runs[(0, name, fill)]
        assert rc == 0 and res is not None and res["status"] == 0, (name, fill, rc, err[-4000:])
        why = mismatch(name, res)
        assert why is None, (name, fill, why)
    a = runs[(0, name, lh.FILLS[0])][2]
    for fill in lh.FILLS[1:]:
        c = runs[(0, name, fill)][2]
        assert np.array_equal(a["nf"], c["nf"]) and np.array_equal(a["flags"], c["flags"]), (name, fill)
        opts = CASES[name][4]
        if CASES[name][5].get("ties"):
            continue  # (which members of the gain level that straddles slot k come out is not defined: KBEST_TIE_BOUNDARY says so)
        for b in range(len(a["nf"])):
            n = max(int(a["nf"][b]), 0)
            rows = opts["nRow"][b] if "nRow" in opts else CASES[name][1]
            cols = opts["nCol"][b] if "nCol" in opts else CASES[name][2]
            assert np.array_equal(bits(a["gain"][b, :n]), bits(c["gain"][b, :n])), (name, fill, b)
            assert np.array_equal(a["row4col"][b, :n, :cols], c["row4col"][b, :n, :cols]), (name, fill, b)
            assert np.array_equal(a["col4row"][b, :n, :rows], c["col4row"][b, :n, :rows]), (name, fill, b)


def test_column_keys_take_the_path_the_layout_says(runs):
    """32 x 32: with one hypothesis per round the closure's matrix (Dp * Dp floats) does not fit the lists it borrows and the keys come
    from one search per column; with eight it fits.  Both cases reorder (k >= 3, M >= 3)."""
    for name in ("keys_dijkstra_32", "keys_closure_32"):
        res = runs[(0, name, 1)][2]
        assert res["kernelK"] >= 3
        assert (32 * 32 * 4 <= res["offFree"] - res["offFreshG"]) == CASES[name][5]["closure"], name


def test_kernel_side_k_is_what_the_case_is_about(runs):
    assert runs[(0, "merge_k64", 1)][2]["kernelK"] == 64 and runs[(0, "merge_k65", 1)][2]["kernelK"] == 65
    assert runs[(0, "k1_root_only", 1)][2]["kernelK"] == 1 and runs[(0, "k1_and_one_behind", 1)][2]["kernelK"] == 2
    assert runs[(0, "k2", 1)][2]["kernelK"] == 2 and runs[(0, "k3_m3_reorder", 1)][2]["kernelK"] == 3
    assert runs[(0, "faulted16", 1)][2]["kernelK"] == 31 and runs[(0, "faulted16", 1)][2]["statesPerProblem"] == 31 + 12 * 16 + 2
    for name in ("pool_runs_dry", "inf_column", "inf_row"):
        assert (runs[(0, name, 1)][2]["nf"] == CASES[name][5]["nf"]).all(), name
    assert runs[(0, "ragged12", 1)][2]["nf"].tolist()[3:5] == [0, -1]
    assert (runs[(0, "cutoff_inside", 1)][2]["nf"][0] == 5)  # the cutoff cuts inside the k best


def test_root_shards_merge_to_the_unsharded_answer(runs):
    """Stride 2, offsets 0 and 1: slot 0 of both shards is the root, the rest of the two lists merged by gain are the checker's k best."""
    costs, N, M, k, _, _ = CASES["shard0of2"]
    for fill in lh.FILLS:
        s0, s1 = runs[(0, "shard0of2", fill)][2], runs[(0, "shard1of2", fill)][2]
        for b in range(costs.shape[0]):
            onf, r4c, _, g = ol.orc_kbest(costs[b], N, M, k)
            cand = [(s["gain"][b, i], tuple(s["row4col"][b, i])) for s in (s0, s1) for i in range(1, int(s["nf"][b]))]
            cand.sort()
            merged = [(s0["gain"][b, 0], tuple(s0["row4col"][b, 0]))] + cand[:k - 1]
            assert tuple(s1["row4col"][b, 0]) == merged[0][1] and bits(s1["gain"][b, 0]) == bits(s0["gain"][b, 0])
            assert len(merged) == onf and [m[1] for m in merged] == [tuple(r) for r in r4c[:onf]], (fill, b)
            assert np.array_equal(bits([m[0] for m in merged]), bits(g[:onf])), (fill, b)


@pytest.mark.parametrize("mutant", [1, 2, 3])
def test_mutant_is_caught(runs, mutant):
    """The detector detects: 1 -- the entry that ends an emission run never reaches the slot table; 2 -- a refilled lane group keeps
    the child before's shortestPathCost; 3 -- the free-slot stack is sized without the children of a round, so that its upper entries
    lie in the finishing pass's scratch (lane_host_lib.MUTANTS says why ONE entry short can not be caught).  Each must fail some run:
    a sanitizer report, or an answer that is not the truth with some fill."""
    caught = []
    for (m, name) in MUTANT_RUNS:
        if m != mutant:
            continue
        for fill in lh.FILLS:
            rc, err, res = runs[(m, name, fill)]
            if rc != 0 or res is None:
                caught.append((name, fill, "sanitizer" if "Sanitizer" in err or "runtime error" in err else "exit %d" % rc))
            else:
                why = mismatch(name, res)
                if why:
                    caught.append((name, fill, why))
    print("mutant", mutant, "caught by", caught)
    assert caught, mutant
