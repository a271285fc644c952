"""GPU tests added in round 5: the HIP engine inside a real process group (world 2, gloo, both ranks on GPU 0),
bench.py's self-launch failing fast on a node with too few GPUs."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol
import probabilisticsemslam_amd as pk
from probabilisticsemslam_amd import workloads as wl

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_engine_in_a_process_group_world2(engine, tmp_path):
    """SURVEY 8(e) with the product on every rank: two child processes, one gloo group, each rank a KBestEngine on
    GPU 0.  Batch mode (contiguous shards + ONE packed all-gather) and subtree mode (root_shard + k-way merge to the
    global k-best heap) must give, on every rank, the single-rank engine's tables, which are the checker's."""
    B, Bsub, world = 13, 3, 2  # 13: uneven shards
    out = str(tmp_path / "dist")
    port = _free_port()
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "dist_engine_worker.py"), out, str(B), str(Bsub)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o)
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)

    cases = {"batch": wl.dense_config("c2", B=B), "sub": wl.dense_config("c2", B=Bsub),
             "sub64": (wl.dense_config("c4", B=2)[0], 64, 64, 60)}
    for tag, (costs, N, M, k) in cases.items():
        nf, r4c, c4r, g = engine.kbest(costs, N, M, k)            # the single-rank engine
        onf, or4c, oc4r, og, _ = ol.orc_kbest_batch(costs, N, M, k)  # the checker
        assert (nf == onf).all() and (r4c == or4c).all() and (bits(g) == bits(og)).all(), tag
        for rank in range(world):
            z = np.load(f"{out}.rank{rank}.npz")
            assert (z[f"{tag}_nf"] == nf).all(), (tag, rank)
            assert (z[f"{tag}_r"] == r4c).all(), (tag, rank)
            assert (bits(z[f"{tag}_g"]) == bits(g)).all(), (tag, rank)


def test_bench_self_launch_refuses_more_gpus_than_the_node_has():
    """`python bench.py --gpus N` without WORLD_SIZE is the launcher: with fewer than N GPUs it says so in one line and
    exits 2 at once -- no rank is spawned, nothing hangs."""
    import torch
    n = torch.cuda.device_count() + 1
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n)], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 2
    assert f"--gpus {n}" in r.stderr and "nothing launched" in r.stderr
    assert r.stdout.strip() == ""


def test_bench_launches_its_own_rank_and_steps_over_rccl():
    """The driver's multi-GPU command on the one GPU there is: `bench.py --gpus 1` made to take the launcher path
    (KBEST_BENCH_SELF_LAUNCH) and the distributed step (KBEST_BENCH_FORCE_DIST: a 1-rank RCCL communicator, one packed all-gather per
    step overlapped with the next step's kernel).  One JSON line, parity flag set, the headline's launches are relays."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(KBEST_BENCH_SELF_LAUNCH="1", KBEST_BENCH_FORCE_DIST="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--full", "--no-cpu", "--no-extra", "--no-host"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-1500:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-1500:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 1 and out["steps"] == 4 and out["parity_prune_vs_noprune"] is True
    assert "all-gather" in out["config"]["collective"]
    assert out["launch"]["relay_launches"] == out["launch"]["of"] == 10  # (K + W steps without the exchange, then K + W with it)
    assert out["collective"]["row4col_dtype"] == "int8" and out["collective"]["bytes_per_rank_per_step"] == 1024 * 200 * (8 + 64) + 1024 * 4
    assert out["collective"]["exposed_ms"] is not None
    assert out["roofline"]["frac"] > 0.5 and out["value"] > 5e7


def test_reference_caller_object_runs_on_the_engine(tmp_path):
    """Link-level drop-in with the reference's OWN caller code: oracle/_ref/ref_caller_on_engine holds the verbatim
    slices of assignment.cpp (conditionCosts, assignmentProb :547-683, bruteForceProb :835-964) compiled against the
    reference's own shortestPathCPP.hpp and linked to libkbest_amd.so in place of shortestPathCPP.cpp -- so the call
    sites assignment.cpp:594 (kBest2DCutoff) and :880 (kBest2D) run unchanged on the GPU.  Its probabilities must be the
    goldens recorded from the all-reference build (same host libm, bit-identical assignments and gains from the engine:
    tolerance 1e-12 relative, far inside the north star's 1e-6)."""
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_caller_on_engine")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/ref_caller_on_engine not built (needs /root/reference at build time)")
    syms = subprocess.check_output(["nm", "-D", "--undefined-only", exe], text=True)
    assert "kBest2DCutoff" in syms and "_Z7kBest2Dmmmb" in syms  # the solver is NOT in the binary: it comes from the engine
    z = np.load(os.path.join(HERE, "golden", "weights_golden.npz"))
    names = [str(n) for n in z["names"]]
    req = [np.array([len(names)], np.int32).tobytes()]
    for n in names:
        nL, nM, k, good, brute = (int(x) for x in z[n + "/meta"])
        req.append(np.array([brute, nL, nM, k], np.int32).tobytes())
        req.append(np.ascontiguousarray(z[n + "/raw"], np.float64).tobytes())
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(b"".join(req))
    subprocess.check_call([exe, str(fin), str(fout)], timeout=600)
    buf = fout.read_bytes()
    o = 0
    for n in names:
        nL, nM, k, good, brute = (int(x) for x in z[n + "/meta"])
        g, w = np.frombuffer(buf, np.int32, 2, o)
        o += 8
        assert g == good, n
        want = z[n + "/probs"]
        p = np.frombuffer(buf, np.float64, nM * w, o).reshape(nM, w)
        o += 8 * nM * w
        assert p.shape == want.shape, n
        np.testing.assert_allclose(p, want, rtol=1e-12, atol=1e-300, err_msg=n)
        if brute:
            w2 = int(np.frombuffer(buf, np.int32, 1, o)[0])
            o += 4
            q = np.frombuffer(buf, np.float64, nM * w2, o).reshape(nM, w2)
            o += 8 * nM * w2
            np.testing.assert_allclose(q, z[n + "/brute"], rtol=1e-12, atol=1e-300, err_msg=n)
    assert o == len(buf)


# ---------------------------------------------------------------------------------------------- exact ties
def _int_costs(rng, B, N, M, hi):
    return rng.integers(0, hi, size=(B, N * M)).astype(np.float64)


def engine_with(monkeypatch, **env):
    for key, val in env.items():
        monkeypatch.setenv(key, str(val))
    eng = pk.KBestEngine(0)
    for key in env:
        monkeypatch.delenv(key)
    return eng


TIE_ROUTES = [{}, {"KBEST_NO_LANE": 1, "KBEST_NO_SMALL": 1}, {"KBEST_FORCE_SMALL": 1}, {"KBEST_FORCE_LANE": 1}, {"KBEST_FORCE_WIDE": 1}]


@pytest.mark.parametrize("shape", [(10, 10, 30, 3), (8, 8, 20, 40), (16, 16, 50, 30), (12, 7, 30, 25), (40, 40, 60, 200), (20, 20, 100, 1000)])
def test_exact_ties_one_answer_whatever_the_kernel(monkeypatch, shape):
    """Integer costs: masses of exactly equal gains.  Every kernel the batch can be routed to returns the SAME tables --
    solutions in (gain, row4col lexicographic) order, and where the k-th and (k+1)-th gains are equal the lexicographically
    first assignments of that gain level (completed by the synchronous entry up to KBEST_TIE_CAP beyond k) -- and they are
    the checker's k best brought into that order.  A level larger than the cap is flagged KBEST_TIE_UNRESOLVED: there the
    gains (a multiset) and the validity of every assignment are checked.  shortestPathCPP.cpp:30-42, 574."""
    N, M, k, hi = shape
    rng = np.random.default_rng(1000 * N + k)
    B = 12
    costs = _int_costs(rng, B, N, M, hi)
    want = [ol.canonical_kbest(costs[b], N, M, k, cap=pk.engine.KBEST_TIE_CAP) for b in range(B)]
    seen_boundary = seen_resolved = 0
    first = None
    for knobs in TIE_ROUTES:
        if knobs.get("KBEST_FORCE_SMALL") and N > 32 or knobs.get("KBEST_FORCE_LANE") and N > 32:
            continue
        eng = engine_with(monkeypatch, **knobs)
        nf, r4c, c4r, g, fl = eng.kbest(costs, N, M, k, tie_flags=True, canonical_ties=True)
        for b in range(B):
            wn, wr, wg, boundary, resolved = want[b]
            assert nf[b] == wn, (knobs, b)
            assert bool(fl[b] & pk.engine.KBEST_TIE_BOUNDARY) == boundary, (knobs, b, fl[b])
            assert (bits(g[b, :wn]) == bits(wg)).all(), (knobs, b)          # gains: always the checker's, bit for bit
            if boundary and not resolved:
                assert fl[b] & pk.engine.KBEST_TIE_UNRESOLVED, (knobs, b)
                for s in range(wn):                                           # valid, distinct assignments with the gain they claim
                    assert len(set(r4c[b, s])) == M
                    assert costs[b].reshape(M, N)[np.arange(M), r4c[b, s]].sum() == g[b, s]
                assert len({tuple(r) for r in r4c[b, :wn]}) == wn
                continue
            assert not (fl[b] & pk.engine.KBEST_TIE_UNRESOLVED), (knobs, b)
            assert bool(fl[b] & pk.engine.KBEST_TIE_RESOLVED) == boundary, (knobs, b)
            assert (r4c[b, :wn] == wr).all(), (knobs, b, np.argwhere(r4c[b, :wn] != wr)[:3])
            inv = np.full(N, -1)
            for s in range(wn):                                               # col4row is the inverse on the real columns
                inv[:] = -1
                inv[r4c[b, s]] = np.arange(M)
                got = c4r[b, s].copy()
                got[got >= M] = -1
                assert (got == inv).all(), (knobs, b, s)
            seen_boundary += boundary
            seen_resolved += resolved
        if first is None:
            first = (nf.copy(), r4c.copy(), g.copy(), fl.copy())
        else:  # bit-identical tables across routings wherever the answer is defined
            ok = (first[3] & pk.engine.KBEST_TIE_UNRESOLVED) == 0
            assert (first[1][ok] == r4c[ok]).all() and (bits(first[2][ok]) == bits(g[ok])).all() and (first[3][ok] == fl[ok]).all(), knobs
    assert seen_boundary > 0 or hi >= 1000  # (the generator does produce ties at slot k in the small-range cases)


def _int_frames(rng, F, nL, nM, hi, gate=10.0):
    """KITTI-like raw blocks (SURVEY 8(d) C5 layout) with INTEGER landmark costs: conditionCosts turns them into integer-valued
    conditioned blocks -- masses of exactly equal gains."""
    nR = nL + nM
    out = []
    for _ in range(F):
        C_ = np.full(nR * nM, np.inf)
        for c in range(nM):
            near = rng.random(nL) < 4.0 / nL
            near[c % nL] = True
            C_[c * nR: c * nR + nL] = np.where(near, rng.integers(0, hi, nL), 60 + rng.integers(0, 400, nL)).astype(np.float64)
            C_[c * nR + nL + c] = gate
        out.append(C_)
    return out


@pytest.mark.parametrize("shape", [(6, 3, 20, 6), (12, 5, 100, 8), (20, 10, 200, 12), (20, 10, 50, 4), (30, 12, 200, 10)])
def test_exact_ties_association_one_answer_whatever_the_batch(monkeypatch, shape):
    """The judge's case: an integer-cost frame alone, in a 2-frame batch and in a 600-frame batch -- and through every
    association kernel (exhaustive, bounded walk, fused enumeration, general pipeline) -- gives the SAME probabilities, bit
    for bit, and they are the checker's: the canonical k best (gain, row4col lexicographic; the lexicographically first
    assignments of a gain level that straddles slot k) weighed by assignmentProb's own accumulation (assignment.cpp:616-648).
    Frames whose tied level is larger than KBEST_TIE_CAP on a route that cannot see it whole are flagged KBEST_TIE_UNRESOLVED
    there (and only checked to be proper distributions)."""
    nL, nM, k, hi = shape
    rng = np.random.default_rng(77 * nL + k)
    F = 600
    frames = _int_frames(rng, F, nL, nM, hi)
    E = pk.engine
    probe = list(range(0, F, 37))  # the frames that are also solved alone / in pairs and by the checker
    want = {}
    for f in probe:
        cond, idx = ol.condition_costs(frames[f], nL + nM, nM)
        condL = len(idx) - nM
        p, n, boundary, resolved = ol.canonical_assignment_prob(cond, condL, nM, k, cap=E.KBEST_TIE_CAP)
        full = np.zeros((nM, nL + 1))
        full[:, idx[:condL]] = p[:, :condL]   # getAssignmentProbs' scatter (assignment.cpp:68-74)
        full[:, nL] = p[:, condL]
        want[f] = (full, boundary, resolved)
    assert sum(1 for f in probe if want[f][1]) > 0, "the generator must produce ties at slot k"
    routes = [{}, {"KBEST_NO_TINY": 1}, {"KBEST_NO_TINY": 1, "KBEST_NO_BNB": 1}, {"KBEST_NO_TINY": 1, "KBEST_NO_BNB": 1, "KBEST_NO_SMALL": 1}]
    results = {}
    for ri, knobs in enumerate(routes):
        eng = engine_with(monkeypatch, **knobs)
        runs = {"all": (list(range(F)),)}
        P, nf = eng.weights(frames, [nL] * F, [nM] * F, k, condition=True)
        fl = eng.last_tie_flags()
        assert len(fl) == F
        got = {f: (P[f], int(fl[f])) for f in probe}
        results[(ri, "600")] = got
        alone, pair = {}, {}
        for f in probe[:6]:
            p1, _ = eng.weights([frames[f]], [nL], [nM], k, condition=True)
            alone[f] = (p1[0], int(eng.last_tie_flags()[0]))
            p2, _ = eng.weights([frames[f], frames[(f + 1) % F]], [nL] * 2, [nM] * 2, k, condition=True)
            pair[f] = (p2[0], int(eng.last_tie_flags()[0]))
        results[(ri, "1")] = alone
        results[(ri, "2")] = pair
    n_checked = 0
    for key, got in results.items():
        for f, (p, flag) in got.items():
            full, boundary, resolved = want[f]
            assert bool(flag & E.KBEST_TIE_BOUNDARY) == boundary, (key, f, flag)
            np.testing.assert_allclose(p.sum(axis=1), 1.0, rtol=1e-12)
            if flag & E.KBEST_TIE_UNRESOLVED:
                assert boundary and not resolved, (key, f)  # only a level beyond the cap may stay open
                continue
            assert bits(p).tolist() == bits(results[(0, "600")][f][0]).tolist() or (results[(0, "600")][f][1] & E.KBEST_TIE_UNRESOLVED), (key, f)
            np.testing.assert_allclose(p, full, rtol=1e-12, atol=1e-300, err_msg=str((key, f)))
            n_checked += 1
    assert n_checked > len(probe)


def test_apriori_threshold_scratch_is_not_rearmed_early(monkeypatch):
    """Regression (round 5): 700 ragged 2-column frames at k = 1 025 through the 64-row kernel's 8-wave shape -- the shape with
    the a-priori threshold, whose LDS scratch the caller re-arms afterwards.  Without a barrier between the two, one problem
    in ten thousand came back with nf = 2 (non-deterministically); the checker's counts are required on every problem of
    every repetition."""
    eng = engine_with(monkeypatch, KBEST_NO_SMALL=1, KBEST_NO_LANE=1)
    rng = np.random.default_rng(11)
    F = 700
    for rep in range(40):
        nL0 = int(rng.integers(3, 40))
        conds = []
        for _ in range(F):
            nL = nL0 - int(rng.integers(0, 3))
            nR = nL + 2
            C_ = np.full(nR * 2, np.inf)
            for c in range(2):
                col = 60.0 + 400.0 * rng.random(nL)
                pick = rng.random(nL) < 3.0 / max(nL, 1)
                col[pick] = 12.0 * rng.random(pick.sum()) * rng.random(pick.sum())
                C_[c * nR: c * nR + nL] = col
                C_[c * nR + nL + c] = 10.0
            conds.append(ol.condition_costs(C_, nR, 2)[0])
        nRow = np.array([len(c) // 2 for c in conds], np.int32)
        nCol = np.full(F, 2, np.int32)
        off = np.zeros(F, np.int64)
        off[1:] = np.cumsum(nRow[:-1].astype(np.int64) * 2)
        flat = np.concatenate(conds)
        nf, r4c, c4r, g = eng.kbest(flat, int(nRow.max()), 2, 1025, cutoff=42.0, nRow=nRow, nCol=nCol, costOff=off)
        want = np.array([ol.orc_kbest(conds[f], int(nRow[f]), 2, 1025, cutoff=42.0)[0] for f in range(F)])
        assert (nf == want).all(), (rep, np.nonzero(nf != want)[0][:5], nf[nf != want][:5], want[nf != want][:5])


def dev_kbest(eng, costs, N, M, k, **kw):
    """The asynchronous device entry (the one that launches relays: the host entries write their tables into host memory and
    never do) on fresh device buffers; returns numpy (nf, row4col, col4row, gain)."""
    import torch
    dev = torch.device("cuda", 0)
    B = costs.shape[0]
    d_cost = torch.from_numpy(np.ascontiguousarray(costs)).to(dev)
    d_r = torch.full((B, k, M), -7, dtype=torch.int32, device=dev)
    d_c = torch.full((B, k, N), -7, dtype=torch.int32, device=dev)
    d_g = torch.full((B, k), float("nan"), dtype=torch.float64, device=dev)
    d_n = torch.full((B,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # (the fills above ran on torch's stream; a NULL stream means the context's own to the engine)
    eng.kbest_dev(d_cost, B, N, M, k, d_r, d_c, d_g, d_n, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    return d_n.cpu().numpy(), d_r.cpu().numpy(), d_c.cpu().numpy(), d_g.cpu().numpy()


@pytest.mark.parametrize("pieces,nwaves", [(2, 4), (3, 4), (3, 8), (5, 8), (3, 12), (8, 12)])
def test_relay_pieces_leave_the_tables_unchanged(monkeypatch, pieces, nwaves):
    """Relay launches (round 5): a matrix is enumerated by `pieces` workgroups one after the other, the LDS handed on through
    HBM.  Forced (KBEST_RELAY) on small batches of every shape the 64-row kernel runs the relay in -- 4, 8 and 12 waves; square,
    rectangular, ragged; with a cutoff; maximising; k above and below the pieces' shares -- the tables are the checker's, bit
    for bit (shortestPathCPP.cpp:574-760 order)."""
    eng = engine_with(monkeypatch, KBEST_RELAY=pieces, KBEST_NWAVES=nwaves, KBEST_NO_SMALL=1, KBEST_NO_LANE=1, KBEST_NO_TINY=1, KBEST_NO_BNB=1)
    rng = np.random.default_rng(77 + pieces + nwaves)
    relayed = 0
    cases = [(24, 24, 200, 300, {}), (33, 33, 200, 40, {}), (64, 64, 200, 24, {}), (48, 40, 100, 30, {}),
             (64, 64, 17, 20, {}), (40, 40, 120, 20, {"maximize": True}), (30, 10, 200, 64, {"cutoff": 3.0}),
             (20, 20, 256, 20, {}), (64, 3, 150, 20, {}), (24, 24, 700, 12, {}), (64, 64, 900, 6, {}), (40, 40, 600, 300, {})]
    for N, M, k, B, kw in cases:
        costs = rng.random((B, N * M))
        before = eng.relay_launches()
        nf, r4c, c4r, g = dev_kbest(eng, costs, N, M, k, **kw)
        relayed += eng.relay_launches() > before
        wn, wr, wc, wg, _ = ol.orc_kbest_batch(costs, N, M, k, **kw)
        assert (nf == wn).all(), (N, M, k)
        for b in range(B):
            n = int(wn[b])
            assert (bits(g[b, :n]) == bits(wg[b, :n])).all(), (N, M, k, b)
            assert (r4c[b, :n] == wr[b, :n]).all(), (N, M, k, b)
            assert (c4r[b, :n, :][wc[b, :n, :] < M] == wc[b, :n, :][wc[b, :n, :] < M]).all(), (N, M, k, b)
    assert relayed >= len(cases) - 2, relayed  # (the launches WERE relays: all but the shapes the forced wave count cannot take)


def test_relay_is_chosen_for_batches_of_several_generations_and_changes_nothing(monkeypatch):
    """The launch plan itself: 1 024 dense 64x64 (two generations of resident workgroups) and 2 048 dense 32x32 run as relays
    by default; the same engine with KBEST_RELAY=0 runs them plain.  Identical tables, same context used twice in a row
    (the progress words are never cleared: the epoch moves on)."""
    plain = engine_with(monkeypatch, KBEST_RELAY=0)
    auto = pk.KBestEngine(0)
    for name, B in (("c4", 1024), ("c3", 2048), ("c4", 700)):
        costs, N, M, k = wl.dense_config(name, B=B)
        a = dev_kbest(plain, costs, N, M, k)
        assert plain.relay_launches() == 0
        for _ in range(2):
            before = auto.relay_launches()
            b = dev_kbest(auto, costs, N, M, k)
            assert auto.relay_launches() == before + 1, name
            assert (a[0] == b[0]).all()
            assert (a[1] == b[1]).all() and (a[2] == b[2]).all()
            assert (bits(a[3]) == bits(b[3])).all()


def test_relay_launch_inside_a_graph_is_replayable(monkeypatch):
    """A captured relay launch replays as it is: the three words of a matrix (pieces claimed / done / workgroups gone) are put
    back to zero by the last of its workgroups to leave, nothing outside the kernel clears them (a memset node in front of the kernel
    did not reach the claim words, which live in L2: the second replay hung).  96 x 64x64, k = 200 as a forced relay of three
    pieces (every piece resident from the start), captured once, replayed four times -- back to back and with another relay launch
    of the same context in between; every replay equals a plain launch (KBEST_RELAY=0) of the same input."""
    import torch
    dev = torch.device("cuda", 0)
    plain = engine_with(monkeypatch, KBEST_RELAY=0)
    eng = engine_with(monkeypatch, KBEST_RELAY=3, KBEST_NWAVES=12)  # (the shape of large batches: small ones run 16 waves, never relayed)
    _, N, M, k, seed = wl.DENSE_CONFIGS["c4"]
    B = 96
    costs = wl.dense_batch(B, N, M, seed)
    d_cost = torch.from_numpy(costs).to(dev)
    d_other = torch.from_numpy(wl.dense_batch(B, N, M, seed, first=200)).to(dev)
    d_r4c = torch.empty((B, k, M), dtype=torch.int32, device=dev)
    d_c4r = torch.empty((B, k, N), dtype=torch.int32, device=dev)
    d_g = torch.empty((B, k), dtype=torch.float64, device=dev)
    d_nf = torch.empty(B, dtype=torch.int32, device=dev)
    d_r2, d_c2, d_g2, d_n2 = torch.empty_like(d_r4c), torch.empty_like(d_c4r), torch.empty_like(d_g), torch.empty_like(d_nf)
    eng.reserve(B, N, k)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eng.kbest_dev(d_cost, B, N, M, k, d_r4c, d_c4r, d_g, d_nf, stream=s.cuda_stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        eng.kbest_dev(d_cost, B, N, M, k, d_r4c, d_c4r, d_g, d_nf, stream=s.cuda_stream)
    for it, first in enumerate((5000, 9000, 13000, 17000)):
        c2 = wl.dense_batch(B, N, M, seed, first=first)
        d_cost.copy_(torch.from_numpy(c2))
        d_g.zero_(); d_nf.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want = plain.kbest(c2, N, M, k)
        assert eng.relay_launches() >= 2
        assert (d_nf.cpu().numpy() == want[0]).all(), first
        assert (d_r4c.cpu().numpy() == want[1]).all() and (bits(d_g.cpu().numpy()) == bits(want[3])).all(), first
        if it % 2 == 0:
            continue  # (the next replay follows this one directly: it finds the words as this one left them)
        with torch.cuda.stream(s):  # a relay launch of the same context outside the graph
            eng.kbest_dev(d_other, B, N, M, k, d_r2, d_c2, d_g2, d_n2, stream=s.cuda_stream)
        torch.cuda.synchronize()
        assert (d_n2.cpu().numpy() == k).all()


@pytest.mark.parametrize("nwaves", [4, 8, 12])
def test_relay_ragged_batch_with_infeasible_and_empty_frames(monkeypatch, nwaves):
    """A forced relay over a RAGGED batch (per-problem numRow / numCol, packed cost blocks) that also holds infeasible problems
    (a column of +inf: kBest2D returns 0, shortestPathCPP.cpp:588-593), problems with fewer than k assignments, and problems
    whose shape is undefined in the reference (numRow < numCol: nf = -1) -- every later piece of those must find the matrix
    finished and leave.  Against the checker, problem by problem."""
    import torch
    dev = torch.device("cuda", 0)
    eng = engine_with(monkeypatch, KBEST_RELAY=3, KBEST_NWAVES=nwaves, KBEST_NO_SMALL=1, KBEST_NO_LANE=1, KBEST_NO_TINY=1, KBEST_NO_BNB=1)
    rng = np.random.default_rng(900 + nwaves)
    B, maxRow, maxCol, k = 90, 40, 40, 120
    nRow = rng.integers(1, maxRow + 1, B).astype(np.int32)
    nCol = np.array([int(rng.integers(1, r + 1)) for r in nRow], np.int32)
    nRow[5], nCol[5] = 3, 7            # undefined shape
    nRow[11], nCol[11] = 3, 3          # 6 assignments in all: fewer than k
    blocks = [rng.random(int(r) * int(c)) for r, c in zip(nRow, nCol)]
    blocks[17][: int(nRow[17])] = np.inf   # first column all +inf: infeasible
    blocks[23][:] = np.inf
    off = np.zeros(B, np.int64)
    off[1:] = np.cumsum([len(b_) for b_ in blocks[:-1]])
    flat = np.concatenate(blocks)
    d_cost = torch.from_numpy(flat).to(dev)
    d_nR, d_nC, d_off = torch.from_numpy(nRow).to(dev), torch.from_numpy(nCol).to(dev), torch.from_numpy(off).to(dev)
    d_r = torch.full((B, k, maxCol), -7, dtype=torch.int32, device=dev)
    d_c = torch.full((B, k, maxRow), -7, dtype=torch.int32, device=dev)
    d_g = torch.full((B, k), float("nan"), dtype=torch.float64, device=dev)
    d_n = torch.full((B,), -7, dtype=torch.int32, device=dev)
    before = eng.relay_launches()
    torch.cuda.synchronize()
    eng.kbest_dev(d_cost, B, maxRow, maxCol, k, d_r, d_c, d_g, d_n, stream=torch.cuda.current_stream().cuda_stream,
                  d_nRow=d_nR, d_nCol=d_nC, d_costOff=d_off)
    torch.cuda.synchronize()
    assert eng.relay_launches() == before + 1
    nf, r4c, g = d_n.cpu().numpy(), d_r.cpu().numpy(), d_g.cpu().numpy()
    for b in range(B):
        N, M = int(nRow[b]), int(nCol[b])
        if N < M:
            assert nf[b] == -1, b
            continue
        wn, wr, wc, wg = ol.orc_kbest(blocks[b], N, M, k)
        assert nf[b] == wn, (b, N, M, nf[b], wn)
        assert (bits(g[b, :wn]) == bits(wg[:wn])).all(), b
        assert (r4c[b, :wn, :M] == wr[:wn]).all(), b
    assert nf[17] == 0 and nf[23] == 0 and nf[11] == 6


def test_relay_under_load_equals_plain_launches():
    """A bounded slice of tests/dev/relay_stress.py: batches of 1.2 - 4 generations (every slot busy, pieces of different matrices
    sharing CUs, warm L1s -- where a sloppy hand-over would go stale), the plan's relay and 2 / 5 / 8 forced pieces against plain
    launches of the same build, every word of every table compared on the device."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "dev", "relay_stress.py"), "10", "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "relay stress ok" in r.stdout, (r.stdout[-800:], r.stderr[-800:])


@pytest.mark.parametrize("shape", [(70, 70, 12, 1000), (80, 30, 25, 1300)])
def test_general_size_kernel_takes_a_large_batch_as_a_queue(monkeypatch, shape):
    """More problems than the general-size kernel has workgroups (768 at up to 128 rows): a workgroup that finishes a problem takes the
    next one off a queue (kbest_wide.hip); the fixed stride (KBEST_NO_WIDE_QUEUE) gives the same tables, and both the checker's."""
    N, M, k, B = shape
    rng = np.random.default_rng(N * 1000 + B)
    costs = rng.random((B, N * M))
    want = ol.orc_kbest_batch(costs, N, M, k)
    for knobs in ({}, {"KBEST_NO_WIDE_QUEUE": 1}):
        eng = engine_with(monkeypatch, **knobs)
        for rep in range(2):  # (the queue's words are back at zero after a launch)
            nf, r4c, c4r, g = eng.kbest(costs, N, M, k)
            assert (nf == want[0]).all(), knobs
            assert (r4c == want[1]).all() and (bits(g) == bits(want[3])).all(), knobs
            assert (c4r[want[2] < M] == want[2][want[2] < M]).all(), knobs
