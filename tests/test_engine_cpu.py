"""CPU: the 64-row k-best kernel (kbest_engine.hip: kbest_kernel<NW, EPT, RELAY>, condition_kernel, weights_kernel) and the launches
behind it (merge_topk_kernel, finish_tables_kernel, fill_unused_kernel) compiled for the host from their own text --
tests/cpp/engine_host.cpp, a stand-alone program under AddressSanitizer and UBSan, -ffp-contract=off, nothing loaded into python.
The state work space with its slot table, every output table, the split buffer, the relay images and each workgroup's LDS are
exact-size heap blocks PREFILLED with 0x00, 0xFF or seeded random bytes: each case runs with all three and must (a) end clean under
both sanitizers and (b) give, with every fill, the checker's answer (oracle_lib: k + 1 solutions where the kernel enumerates one more
for the tie check) -- nf, the bits of the gains and of tieGain, the tie flags, the tables up to nf, -1 and gain 0 beyond -- with every
slotSid[s], s < nf, inside the problem's state slots.  An index read from memory that nobody wrote fails one of the two.  Four
mutants of the kernel's text prove that the detector detects.

All runs are started together, once (the thread emulation waits more than it computes); the tests read the results."""
import concurrent.futures
import os

import numpy as np
import pytest

import engine_host_lib as eh
import oracle_lib as ol

F_NO_PRUNE, F_COUNT_PUSHED, F_RECT_ROOT, F_NO_SHIFT, F_EXACT_ROOT, F_NO_T0, F_I8, F_NO_REORDER = 1, 2, 4, 8, 16, 32, 64, 128
INF = np.inf
OPT_ENTRY = (0.85, 0.85, 1.0, 0.25, 8)  # optRho0, optRho1, optPhi, optKappa, optMinPool as batch_dev_impl sets them
T0_SCRATCH = 160                        # kbest_engine.hip


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def uniform(seed, B, N, M):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (B, N * M))


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


def ragged12(seed=1212, first=0):
    """maxRow = maxCol = 12 with shape arrays: full, N < maxRow square, M < N (padded columns), an empty frame, N < M (nf = -1)."""
    rng = np.random.default_rng(seed)
    shapes = [(12, 12), (9, 9), (10, 6), (0, 0), (5, 8)][first:]
    costs = np.zeros((len(shapes), 144))
    for b, (n, m) in enumerate(shapes):
        costs[b, :n * m] = rng.uniform(0.0, 1.0, n * m)
    return costs, [s[0] for s in shapes], [s[1] for s in shapes]


def even_relay(P):
    first = 1024 // P
    return (P, first, (1024 - first) // (P - 1))


# name -> (costs, maxRow, maxCol, k, options of engine_host_lib.run, options of the check)
def make_cases():
    C = {}
    # -- instantiations
    for w in (1, 2, 4, 8, 12, 16):
        C["waves%d" % w] = (uniform(300 + w, 2 if w <= 8 else 1, 8, 8), 8, 8, 10, dict(spec=min(w, 12), waves=w), {})
    C["ept1_k64"] = (uniform(64, 1, 7, 7), 7, 7, 64, dict(spec=1, waves=1, tie=False), {})
    C["ept4_k65"] = (uniform(65, 1, 7, 7), 7, 7, 65, dict(spec=1, waves=1, tie=False), {})
    # -- lane = row edges (64: the only size that takes the D >= 64 arm of allRows)
    for n in (1, 2, 3, 31, 32, 33, 63, 64):
        C["rows_n%d" % n] = (uniform(40 + n, 1, n, n), n, n, 6 if n >= 3 else 3, dict(spec=2, waves=2), {})
    # -- rectangular
    C["padded_10x6"] = (uniform(106, 2, 10, 6), 10, 6, 9, dict(spec=4, waves=4), {})
    C["park_64x3"] = (uniform(643, 1, 64, 3), 64, 3, 6, dict(spec=4, waves=4), {})
    rc, rn, rm = ragged12()
    C["ragged12"] = (rc, 12, 12, 8, dict(spec=4, waves=4, nRow=rn, nCol=rm), {})
    # -- short lists
    C["k1_root_only"] = (uniform(11, 2, 3, 3), 3, 3, 1, dict(spec=1, waves=1, tie=False), {})
    C["k2"] = (uniform(13, 2, 3, 3), 3, 3, 2, dict(spec=2, waves=2, tie=False), {})
    C["k3"] = (uniform(14, 2, 3, 3), 3, 3, 3, dict(spec=2, waves=2, tie=False), {})
    C["pool_runs_dry"] = (uniform(15, 2, 3, 3), 3, 3, 10, dict(spec=2, waves=2), dict(nf=6))
    C["inf_column"] = (one_inf_column(21, 6, 2), 6, 6, 5, dict(spec=2, waves=2), dict(nf=0))
    C["inf_row"] = (one_inf_row(22, 6, 4), 6, 6, 5, dict(spec=2, waves=2), dict(nf=0))
    C["inf_scattered_12"] = (with_inf(23, 12, 0.3), 12, 12, 14, dict(spec=4, waves=4), {})
    # -- a-priori thresholds (8 waves, 8 hypotheses per round)
    for M, tag in ((12, "12x12"), (9, "12x9")):
        C["t0_off_k2_" + tag] = (uniform(120 + M, 1, 12, M), 12, M, 2, dict(tie=False), dict(t0=False, t1=False))
        C["t0_on_k3_" + tag] = (uniform(121 + M, 1, 12, M), 12, M, 3, dict(tie=False), dict(t0=True, t1=M == 12))
        C["t0_on_k40_" + tag] = (uniform(122 + M, 1, 12, M), 12, M, 40, dict(), dict(t0=True, t1=M == 12))
    C["t0_no_room"] = (uniform(123, 1, 12, 12), 12, 12, 40, dict(eager=8), dict(t0=False, t1=False))  # maxSid == nSlots
    # -- optimistic bounds (4 waves)
    C["opt_entry_28"] = (uniform(2828, 1, 28, 28), 28, 28, 100, dict(spec=4, waves=4, opt=OPT_ENTRY), {})
    C["opt_forced_10"] = (uniform(1010, 1, 10, 10), 10, 10, 40, dict(spec=4, waves=4, opt=OPT_ENTRY), {})
    C["opt_off_cutoff"] = (uniform(1011, 1, 10, 10), 10, 10, 40, dict(spec=4, waves=4, opt=OPT_ENTRY), dict(cut_between=(20, 21)))
    # -- lazy and eager states (0: every selected candidate is re-solved)
    for w in (4, 8):
        for e in (0, 1, 64):
            C["eager%d_w%d" % (e, w)] = (uniform(700 + w + e, 1, 12, 12), 12, 12, 40, dict(spec=min(w, 8), waves=w, eager=e), {})
    # -- relay
    C["relay_w4_p2"] = (uniform(801, 1, 12, 12), 12, 12, 40, dict(spec=4, waves=4, relay=even_relay(2)), {})
    C["relay_w8_p3"] = (uniform(802, 1, 12, 12), 12, 12, 40, dict(relay=even_relay(3)), {})
    C["relay_w12_p5"] = (uniform(803, 1, 12, 12), 12, 12, 40, dict(spec=12, waves=12, relay=even_relay(5)), {})
    C["relay_done_in_first"] = (uniform(804, 1, 12, 12), 12, 12, 40, dict(relay=even_relay(3)), dict(cut_between=(4, 5)))
    rc2, rn2, rm2 = ragged12(1313, first=1)
    C["relay_ragged_refused"] = (rc2, 12, 12, 16, dict(spec=4, waves=4, nRow=rn2, nCol=rm2, relay=even_relay(3)), {})
    # -- internal split (sharedT is used), merged by launch_merge_topk
    for s in (2, 3):
        C["split%d" % s] = (uniform(900 + s, 1, 12, 12), 12, 12, 20, dict(split=s, tie=False), {})
    # -- the caller's root sharding (t0On is off there)
    C["shard0of2"] = (uniform(35, 1, 10, 10), 10, 10, 12, dict(tie=False, root=(0, 2)), dict(shard=True, t0=False))
    C["shard1of2"] = (uniform(35, 1, 10, 10), 10, 10, 12, dict(tie=False, root=(1, 2)), dict(shard=True, t0=False))
    # -- flags
    C["rect_root_10x6"] = (uniform(41, 2, 10, 6) * 5 - 1, 10, 6, 1, dict(spec=4, waves=4, tie=False, flags=F_RECT_ROOT, duals=True), dict(assign=(True, 0)))
    C["rect_root_noshift"] = (uniform(42, 2, 10, 6) + 0.5, 10, 6, 1, dict(spec=4, waves=4, tie=False, flags=F_RECT_ROOT | F_NO_SHIFT, duals=True),
                              dict(assign=(False, 0)))
    C["rect_root_gaincols"] = (uniform(43, 2, 10, 6), 10, 6, 1, dict(spec=4, waves=4, tie=False, flags=F_RECT_ROOT, duals=True, gainCols=4),
                               dict(assign=(True, 4)))
    C["exact_root"] = (uniform(44, 2, 9, 9), 9, 9, 10, dict(spec=4, waves=4, flags=F_EXACT_ROOT), {})
    C["no_prune_count_pushed"] = (uniform(45, 2, 7, 7), 7, 7, 10, dict(spec=1, waves=4, tie=False, flags=F_NO_PRUNE | F_COUNT_PUSHED, pushed=True),
                                  dict(pushed=True))
    C["no_t0"] = (uniform(46, 1, 12, 12), 12, 12, 20, dict(flags=F_NO_T0), dict(t0=False))
    C["no_reorder"] = (uniform(47, 2, 9, 9), 9, 9, 10, dict(spec=4, waves=4, flags=F_NO_REORDER), {})
    C["tables_i8"] = (uniform(48, 2, 9, 9), 9, 9, 10, dict(spec=4, waves=4, flags=F_I8), {})
    C["tables_host"] = (uniform(49, 2, 9, 9), 9, 9, 10, dict(spec=4, waves=4, tablesHost=True), {})
    C["maximize"] = (uniform(50, 2, 9, 9), 9, 9, 10, dict(spec=4, waves=4, maximize=True), {})
    C["cutoff_inside"] = (uniform(51, 2, 9, 9), 9, 9, 12, dict(spec=4, waves=4), dict(cut_between=(4, 5)))
    # -- exact ties, the finishing kernel behind them
    for w in (4, 8):
        C["ties_int_8x8_w%d" % w] = (np.floor(uniform(36, 1, 8, 8) * 4.0), 8, 8, 40, dict(spec=min(w, 8), waves=w), dict(ties=True))
    # every assignment costs 0: the fresh list holds gains of exactly 0.0 where the filter's minima live in the next round (mutant 4)
    C["zeros_4x4"] = (np.zeros((1, 16)), 4, 4, 10, dict(spec=4, waves=4), dict(ties=True))
    return C


CASES = make_cases()
# (mutant, the case it is run on)
MUTANT_RUNS = [(1, "waves8"), (2, "waves8"), (3, "eager64_w8"), (4, "zeros_4x4")]


def resolve_cutoff(name):
    """cut_between = (i, j): a cutoff half way between the i-th and the j-th best gain of problem 0, relative to its best."""
    costs, N, M, k, opts, chk = CASES[name]
    if "cut_between" in chk and "cutoff" not in opts:
        i, j = chk["cut_between"]
        _, _, _, g = ol.orc_kbest(costs[0], N, M, max(k, j + 1))
        opts["cutoff"] = float(0.5 * (g[i] + g[j]) - g[0])
    return opts


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Builds the program (and the four mutants) and runs every case with every fill, all at once."""
    tmp = tmp_path_factory.mktemp("engine_host")
    jobs = {}
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(2, min(8, os.cpu_count() or 2))) as pool:
        builds = {m: pool.submit(eh.build, tmp, eh.ASAN, m, "-O0") for m in (0, 1, 2, 3, 4)}
        exe = {m: b.result() for m, b in builds.items()}
        n = 0
        for name in CASES:
            costs, N, M, k, _, _ = CASES[name]
            opts = resolve_cutoff(name)
            for fill in eh.FILLS:
                d = tmp / ("job%d" % n)
                d.mkdir()
                n += 1
                jobs[(0, name, fill)] = pool.submit(eh.run, exe[0], d, costs, N, M, k, fill=fill, seed=1000 + n, check=False, **opts)
        for m, name in MUTANT_RUNS:
            costs, N, M, k, _, _ = CASES[name]
            for fill in eh.FILLS:
                d = tmp / ("job%d" % n)
                d.mkdir()
                n += 1
                jobs[(m, name, fill)] = pool.submit(eh.run, exe[m], d, costs, N, M, k, fill=fill, seed=1000 + n, check=False, **CASES[name][4])
        for fill in eh.FILLS:
            d = tmp / ("cond%d" % fill)
            d.mkdir()
            jobs[("condition", fill)] = pool.submit(eh.run_condition, exe[0], d, CONDITION_BLOCKS, 130, fill=fill, seed=3000 + fill)
            for acc in (True, False):
                d = tmp / ("weights%d_%d" % (fill, acc))
                d.mkdir()
                W = weights_input()
                jobs[("weights", acc, fill)] = pool.submit(eh.run_weights, exe[0], d, W["nL"], W["nM"], W["nf"], W["cost"], W["gain"], W["r4c"], k=W["k"],
                                                           maxCol=32, maxRow=W["maxRow"], gate=1, solveRows=10 if acc else 300, rowIdx=W["rowIdx"],
                                                           nLout=W["nLout"], fill=fill, seed=4000 + fill)
        out = {key: j.result() for key, j in jobs.items()}
    print("seconds per case (fills 1, 2, 3):", {name: [round(out[(0, name, f)][2]["seconds"], 1) if out[(0, name, f)][2] else None for f in eh.FILLS]
                                                for name in CASES})
    return out


# ---- condition_kernel: nR in {1, 63, 64, 65, 130} x nC in {1, 5}, a row kept by exactly 42.0 and rows beyond the gate
def condition_blocks():
    rng = np.random.default_rng(4242)
    blocks = [rng.uniform(0.0, 90.0, (nR, nC)) for nR in (1, 63, 64, 65, 130) for nC in (1, 5)]  # (about half the entries beyond the gate)
    edge = np.full((5, 2), 100.0)
    edge[0] = [0.0, 0.0]                         # the column minima
    edge[1] = [42.0, 100.0]                      # kept by exactly 42.0
    edge[2] = [np.nextafter(42.0, 50.0), 100.0]  # one ulp beyond: dropped
    edge[3] = [5.0, 200.0]
    edge[4] = [43.0, 43.0]                       # beyond the gate in every column: dropped
    return blocks + [edge]


CONDITION_BLOCKS = condition_blocks()


def test_condition_kernel_is_the_restatement_bit_for_bit(runs):
    """conditionCosts on the host build against the oracle's restatement (as tests/test_gpu_parity.py::test_condition_costs_device
    compares the device's): the kept rows, their map, the conditioned block -- on exact-size prefilled blocks, every fill."""
    for fill in eh.FILLS:
        rc, err, res = runs[("condition", fill)]
        assert rc == 0 and res is not None, (fill, rc, err[-3000:])
        for b, blk in enumerate(CONDITION_BLOCKS):
            nR, nC = blk.shape
            oc, orx = ol.condition_costs(blk.T.reshape(-1), nR, nC)
            g = int(res["goodRows"][b])
            assert g == len(orx) and int(res["condL"][b]) == g - nC, (fill, b)
            assert np.array_equal(res["rowIdx"][b, :g], orx), (fill, b)
            assert np.array_equal(bits(res["out"][res["off"][b]:res["off"][b] + g * nC]), bits(oc)), (fill, b)
    edge = runs[("condition", 1)][2]
    assert edge["rowIdx"][len(CONDITION_BLOCKS) - 1, :3].tolist() == [0, 1, 3] and edge["goodRows"][len(CONDITION_BLOCKS) - 1] == 3


# ---- weights_kernel: the single-column path, nf = 0, nf = chunk and chunk + 1 at maxCol = 32, a row map; accumulators in LDS and not
_weights = {}


def weights_input():
    """Problems of 6 landmarks x 3 measurements (504 assignments) weighed from the checker's own k-best lists; maxCol = 32: 256
    solutions per chunk.  0: nf = 256 = chunk; 1: nf = 257 = chunk + 1; 2: nf = 0 (an infeasible frame); 3: one column; 4: nf = 40
    of a frame whose rows go back through a row map."""
    if _weights:
        return _weights
    rng = np.random.default_rng(777)
    k, nLr, nMr = 257, 6, 3
    conds = [rng.uniform(0.0, 3.0, (nLr + nMr) * nMr) for _ in range(5)]
    conds[2][(nLr + nMr):2 * (nLr + nMr)] = INF
    conds[3] = np.array([0.5, 43.0, 2.0, 10.0, 42.0, 41.5, 1.0])  # nL = 6, one column
    nfGiven = [256, 257, 0, 7, 40]
    nL, nM = [nLr] * 5, [nMr, nMr, nMr, 1, nMr]
    gain = np.zeros((5, k)); r4c = np.zeros((5, k, 32), np.int32)
    for b in (0, 1, 2, 4):
        onf, orow, _, og = ol.orc_kbest(conds[b], nLr + nMr, nMr, k, cutoff=42.0)
        assert onf == (0 if b == 2 else k)
        gain[b, :onf] = og[:onf]
        r4c[b, :onf, :nMr] = orow[:onf]
    rowIdx = np.tile(np.arange(16, dtype=np.int32), (5, 1))
    rowIdx[4, :nLr + nMr] = [1, 2, 4, 7, 8, 9, 11, 12, 13]  # problem 4: kept rows of a frame with 10 landmarks
    nLout = [nLr, nLr, nLr, nLr, 10]
    _weights.update(k=k, nL=nL, nM=nM, nf=nfGiven, cost=conds, gain=gain, r4c=r4c, rowIdx=rowIdx, nLout=nLout, maxRow=16)
    return _weights


@pytest.mark.parametrize("acc", [True, False])
def test_weights_kernel_against_the_oracle(runs, acc):
    """assignmentProb's accumulate / normalise against the oracle's, with the bounds of the GPU tests of this kernel
    (tests/test_gpu_parity.py: rtol 1e-12, atol 1e-15 on the tables, rtol 1e-14 on the single-column path; only exp() can differ)."""
    W = weights_input()
    for fill in eh.FILLS:
        rc, err, res = runs[("weights", acc, fill)]
        assert rc == 0 and res is not None, (acc, fill, rc, err[-3000:])
        assert res["chunk"] == 256 and res["ldsAcc"] == int(acc)
        for b in range(5):
            got = res["probs"][b]
            if W["nM"][b] == 1:
                po, _ = ol.assignment_prob(W["cost"][b], W["nL"][b], 1, W["k"])
                np.testing.assert_allclose(got, po, rtol=1e-14)
                assert res["nf"][b] == 5  # the entries below 42 (the entry of exactly 42 weighs nothing)
                continue
            po, onf = ol.assignment_prob(W["cost"][b], W["nL"][b], W["nM"][b], W["nf"][b] if W["nf"][b] else W["k"])
            want = po
            if b == 4:  # scatter back through the row map (getAssignmentProbs, assignment.cpp:68-74)
                want = np.zeros((W["nM"][b], W["nLout"][b] + 1))
                want[:, W["rowIdx"][b, :W["nL"][b]]] = po[:, :W["nL"][b]]
                want[:, W["nLout"][b]] = po[:, W["nL"][b]]
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-15, equal_nan=True, err_msg=str((acc, fill, b)))
            assert np.isnan(got).all() == (b == 2)


def canon(c4r, M):
    c = np.array(c4r, copy=True)
    c[c >= M] = -1  # rows on zero-padded columns: which padded column is a tie artefact
    return c


def shape_of(name, b):
    costs, N, M, k, opts, chk = CASES[name]
    return (opts["nRow"][b] if "nRow" in opts else N), (opts["nCol"][b] if "nCol" in opts else M)


def truth_of(name, b):
    """The checker's answer for problem b of a case: (nf, row4col, col4row, gain, the gain behind the tables or NaN)."""
    costs, N, M, k, opts, chk = CASES[name]
    n, m = shape_of(name, b)
    if n < 1 or m < 1:
        return 0, None, None, None, np.nan
    if n < m:
        return -1, None, None, None, np.nan
    ke = k + 1 if opts.get("tie", True) else k
    onf, r4c, c4r, g = ol.orc_kbest(costs[b, :n * m], n, m, ke, maximize=opts.get("maximize", False), cutoff=opts.get("cutoff"))
    behind = g[k] if onf > k else np.nan
    return min(onf, k), r4c, c4r, g, behind


def unused_slots_are_cleared(name, b, res, nf):
    """Slots beyond nf after the fill kernel: -1 in the problem's own columns and rows, gain 0."""
    n, m = shape_of(name, b)
    lo = max(nf, 0)
    if (res["gain"][b, lo:] != 0.0).any() or (res["row4col"][b, lo:, :m] != -1).any() or (res["col4row"][b, lo:, :n] != -1).any():
        return "problem %d: slots beyond nf are not cleared" % b
    return None


def mismatch(name, res):
    """None if the run's result is the truth, else a description of the first difference."""
    costs, N, M, k, opts, chk = CASES[name]
    tie = opts.get("tie", True)
    S = opts.get("split", 1)
    if res is None:
        return "no result"
    B = costs.shape[0]
    # (hypotheses live below maxSid, the atoms of the a-priori threshold from there; the program reports maxSid for maxRow rows -- a
    #  smaller problem of a ragged batch has fewer atoms and a larger one)
    top = res["statesPerProblem"] if "nRow" in opts else res["maxSid"]
    for w in range(B * S):  # every workgroup's slot table, up to its own count
        wn = min(int(res["wgNf"][w]), k)
        if wn > 0:
            sid = res["slotSid"][w, :wn]
            if sid.min() < 0 or sid.max() >= top:
                return "workgroup %d: slotSid outside [0, %d): %s" % (w, top, sid)
    if "assign" in chk:
        return mismatch_assign(name, res)
    for b in range(B):
        nf, r4c, c4r, g, behind = truth_of(name, b)
        n, m = shape_of(name, b)
        if chk.get("shard"):
            continue  # (a shard's own list: test_root_shards_merge_to_the_unsharded_answer)
        if int(res["nf"][b]) != nf:
            return "problem %d: nf %d, truth %d" % (b, res["nf"][b], nf)
        why = unused_slots_are_cleared(name, b, res, nf)
        if why:
            return why
        if nf <= 0:
            continue
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
        if chk.get("pushed"):  # (tests/test_gpu_parity.py: the oracle's push count, unpruned)
            st = ol.orc_kbest(costs[b], n, m, k, opts.get("maximize", False), opts.get("cutoff"), want_stats=True)[4]
            if int(res["pushed"][b]) != st.children_pushed:
                return "problem %d: pushed %d, truth %d" % (b, res["pushed"][b], st.children_pushed)
    return None


def mismatch_assign(name, res):
    """The assign2D / shortestPathCPP launch (RECT_ROOT, k = 1, duals), as tests/test_gpu_setup_loads.py compares it with the oracle:
    the tables with -1 for an unassigned row, the gain, u and v, all exactly."""
    costs, N, M, k, opts, chk = CASES[name]
    shift, gc = chk["assign"]
    for b in range(costs.shape[0]):
        o = ol.orc_assign2d_ex(costs[b], N, M, opts.get("maximize", False), shift, gc)
        if int(res["nf"][b]) != o[0]:
            return "problem %d: feasible %d, truth %d" % (b, res["nf"][b], o[0])
        if res["row4col"][b, 0].tolist() != o[1].tolist() or res["col4row"][b, 0].tolist() != o[2].tolist():
            return "problem %d: tables" % b
        if N > M and not (res["col4row"][b, 0] == -1).any():
            return "problem %d: no unassigned row" % b
        if res["gain"][b, 0] != o[3] or res["dualU"][b].tolist() != o[4].tolist() or res["dualV"][b].tolist() != o[5].tolist():
            return "problem %d: gain or duals" % b
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
    Cm = costs[b].reshape(M, N)  # [column][row]
    for level in np.unique(cg):
        idx = np.nonzero(cg == level)[0]
        rows = [tuple(r) for r in got[idx]]
        if rows != sorted(rows) or len(set(rows)) != len(rows):
            return "problem %d: level %r not in lexicographic order" % (b, level)
        if boundary and level == cg[-1]:
            for r in rows:  # any members of the level: a permutation with that gain (integer costs: the sum is exact)
                if sorted(r) != list(range(N)) or sum(Cm[c, r[c]] for c in range(M)) != level:
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
    costs, N, M, k, opts, chk = CASES[name]
    for fill in eh.FILLS:
        rc, err, res = runs[(0, name, fill)]
        assert rc == 0 and res is not None and res["status"] == 0, (name, fill, rc, err[-4000:])
        why = mismatch(name, res)
        assert why is None, (name, fill, why)
        if "relay" in opts:  # the last workgroup of every matrix to leave has put its three words back
            assert not res["relayWords"].any(), (name, fill, res["relayWords"])
    a = runs[(0, name, eh.FILLS[0])][2]
    for fill in eh.FILLS[1:]:
        c = runs[(0, name, fill)][2]
        assert np.array_equal(a["nf"], c["nf"]) and np.array_equal(a["flags"], c["flags"]), (name, fill)
        if chk.get("ties"):
            continue  # (which members of the gain level that straddles slot k come out is not defined: KBEST_TIE_BOUNDARY says so)
        for b in range(len(a["nf"])):
            n = max(int(a["nf"][b]), 0)
            rows, cols = shape_of(name, b)
            assert np.array_equal(bits(a["gain"][b, :n]), bits(c["gain"][b, :n])), (name, fill, b)
            assert np.array_equal(a["row4col"][b, :n, :cols], c["row4col"][b, :n, :cols]), (name, fill, b)
            assert np.array_equal(canon(a["col4row"][b, :n, :rows], cols), canon(c["col4row"][b, :n, :rows], cols)), (name, fill, b)


def test_a_priori_thresholds_take_the_arm_the_layout_says(runs):
    """t0On (kbest_engine.hip): pruning, kernel-side k >= 3, no root sharding by the caller, no push counting, not NO_T0, not RECT_ROOT,
    8 waves or more, 3 hypotheses per round or more, and room for the atoms behind the eager slots (maxSid < nSlots); t1On: t0On, a
    square problem and spec * 64 >= T0_SCRATCH + 64.  What the cases are about, from the sizes the program launched with."""
    for name, (costs, N, M, k, opts, chk) in CASES.items():
        if "t0" not in chk:
            continue
        res = runs[(0, name, 1)][2]
        waves, spec, flags = opts.get("waves", 8), opts.get("spec", 8), opts.get("flags", 0)
        room = res["maxSid"] < res["statesPerProblem"]
        assert room == (res["statesPerProblem"] - res["atomSlots"] > res["lazyStates"]), name
        t0 = (not flags & F_NO_PRUNE and res["kernelK"] >= 3 and (opts.get("root", (0, 1))[1] <= 1 or opts.get("split", 1) > 1)
              and not flags & (F_COUNT_PUSHED | F_NO_T0 | F_RECT_ROOT) and waves >= 8 and min(spec, waves) >= 3 and room)
        assert bool(t0) == chk["t0"], (name, res["kernelK"], room)
        if "t1" in chk:
            assert bool(t0 and N == M and min(spec, waves) * 64 >= T0_SCRATCH + 64) == chk["t1"], name
    assert runs[(0, "t0_no_room", 1)][2]["maxSid"] == runs[(0, "t0_no_room", 1)][2]["statesPerProblem"]


def test_the_entry_still_sizes_as_the_header_restates():
    """The program sizes its blocks from kbest_engine.h (engine_states_need, engine_states_per_problem, SplitLayout,
    relay_image_bytes, relay_words_bytes), which restates what kbest_capi.cpp computes for the 64-row route.  Until the entry calls
    the header, the entry's own lines are pinned here: whoever changes one of them is sent to the other."""
    capi = open(os.path.join(eh.CSRC, "kbest_capi.cpp")).read()
    head = open(os.path.join(eh.CSRC, "kbest_engine.h")).read()
    for line in ("    const size_t nStates = (size_t)B * (size_t)(k + ctx->extraStates + eager_states(ctx, B, maxRow, k)) * (size_t)kb::state_stride(maxRow);\n",
                 "    if (slotOff) *slotOff = (nStates + 127) & ~(size_t)127;\n",
                 "    return nStates + (size_t)B * (size_t)kb::slot_table_stride(k) * 2 + 256;\n",
                 "        p.statesPerProblem = k + ctx->extraStates + eager_states(ctx, PB, fastRow, k);\n",
                 "        p.lazyStates = k + ctx->extraStates;\n",
                 "    if (imgOut) *imgOut = ((size_t)ldsB + 16 + 127) & ~(size_t)127;\n",
                 "    const size_t need = (size_t)B * img, needF = (size_t)B * 16;"):
        assert capi.count(line) == 1, line
    for line in ("    const size_t nStates = (size_t)B * (size_t)engine_states_per_problem(k, extraStates, eagerStates) * (size_t)state_stride(maxRow);\n",
                 "inline int engine_states_per_problem(int k, int extraStates, int eagerStates) { return k + extraStates + eagerStates; }\n",
                 "inline size_t relay_image_bytes(int ldsBytes) { return ((size_t)ldsBytes + 16 + 127) & ~(size_t)127; }\n",
                 "inline size_t relay_words_bytes(int B) { return (size_t)B * 16; }\n"):
        assert head.count(line) == 1, line
    body = """    SplitLayout(int B, int S, int k, int maxCol)
    {
        auto up = [](size_t x) { return (x + 127) & ~(size_t)127; };
        offGain = 0;
        offR4C = up((size_t)S * B * k * 8);
        offNf = offR4C + up((size_t)S * B * k * maxCol * 4);
        offT = offNf + up((size_t)S * B * 4);
        bytes = offT + up((size_t)B * 8);
    }
"""
    assert capi.count(body) == 1 and head.count(body) == 1


def test_the_cases_are_what_they_are_about(runs):
    assert runs[(0, "ept1_k64", 1)][2]["kernelK"] == 64 and runs[(0, "ept4_k65", 1)][2]["kernelK"] == 65  # k <= NW * 64: one entry per thread
    assert runs[(0, "k1_root_only", 1)][2]["kernelK"] == 1 and runs[(0, "k2", 1)][2]["kernelK"] == 2 and runs[(0, "k3", 1)][2]["kernelK"] == 3
    for name in ("pool_runs_dry", "inf_column", "inf_row"):
        assert (runs[(0, name, 1)][2]["nf"] == CASES[name][5]["nf"]).all(), name
    assert runs[(0, "ragged12", 1)][2]["nf"].tolist()[3:5] == [0, -1]
    assert runs[(0, "relay_ragged_refused", 1)][2]["nf"].tolist()[2:4] == [0, -1]
    assert runs[(0, "cutoff_inside", 1)][2]["nf"][0] == 5 and runs[(0, "relay_done_in_first", 1)][2]["nf"][0] == 5
    assert runs[(0, "opt_off_cutoff", 1)][2]["nf"][0] == 21
    for w in (4, 8):  # eager 0: no child is kept in full, every selected candidate is re-solved; the slots are the lazy ones
        r = runs[(0, "eager0_w%d" % w, 1)][2]
        assert r["statesPerProblem"] == r["lazyStates"] == 41 + 8
    for name in ("relay_w4_p2", "relay_w8_p3", "relay_w12_p5"):  # the image is an exact-size block of whole 128-byte lines
        r = runs[(0, name, 1)][2]
        assert r["relayImage"] >= r["lds"] + 16 and r["relayImage"] % 128 == 0 and r["relayImage"] - r["lds"] < 16 + 128


def test_root_shards_merge_to_the_unsharded_answer(runs):
    """Stride 2, offsets 0 and 1: slot 0 of both shards is the root, the rest of the two lists merged by gain are the checker's k best."""
    costs, N, M, k, _, _ = CASES["shard0of2"]
    for fill in eh.FILLS:
        s0, s1 = runs[(0, "shard0of2", fill)][2], runs[(0, "shard1of2", fill)][2]
        for b in range(costs.shape[0]):
            onf, r4c, _, g = ol.orc_kbest(costs[b], N, M, k)
            cand = [(s["gain"][b, i], tuple(s["row4col"][b, i])) for s in (s0, s1) for i in range(1, int(s["nf"][b]))]
            cand.sort()
            merged = [(s0["gain"][b, 0], tuple(s0["row4col"][b, 0]))] + cand[:k - 1]
            assert tuple(s1["row4col"][b, 0]) == merged[0][1] and bits(s1["gain"][b, 0]) == bits(s0["gain"][b, 0])
            assert len(merged) == onf and [m[1] for m in merged] == [tuple(r) for r in r4c[:onf]], (fill, b)
            assert np.array_equal(bits([m[0] for m in merged]), bits(g[:onf])), (fill, b)


@pytest.mark.parametrize("mutant", [1, 2, 3, 4])
def test_mutant_is_caught(runs, mutant):
    """The detector detects (engine_host_lib.MUTANTS): 1 -- the entry that ends an emission run never reaches the slot table; 2 -- a
    node's counter of finished filter parts is not put back to zero; 3 -- the eager slots are handed out over the atoms of the
    a-priori threshold; 4 -- the filter's minima, which share their LDS with the fresh list, are not re-armed behind the merge.  Each
    must fail some run: a sanitizer report, or an answer that is not the truth with some fill."""
    caught = []
    for (m, name) in MUTANT_RUNS:
        if m != mutant:
            continue
        for fill in eh.FILLS:
            rc, err, res = runs[(m, name, fill)]
            if rc != 0 or res is None:
                caught.append((name, fill, "sanitizer" if "Sanitizer" in err or "runtime error" in err else "exit %d" % rc))
            else:
                why = mismatch(name, res)
                if why:
                    caught.append((name, fill, why))
    print("mutant", mutant, "caught by", caught)
    assert caught, mutant
