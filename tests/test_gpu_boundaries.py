"""GPU: problems exactly on the cutoff and gate comparisons (tests/boundary_lib.py, tests/golden/boundary_golden.npz) through
every k-best route and every association kernel.  k-best: nf and gains bit for bit, row4col slot for slot, col4row up to the
names of padded columns, against the checker (and the compiled reference where it was built).  Association: nf exactly, every
probability within (2 nf + 8) 2^-53 of the high-precision value and exactly 0 where that is 0 (oracle_lib.hp_mismatch).  Every
leg asserts how many problems it put on a boundary and which kernel ran."""
import os

import numpy as np
import pytest

import boundary_lib as bl
import oracle_lib as ol
import probabilisticsemslam_amd as pk
import soak_lib

pytestmark = pytest.mark.gpu

E = pk.engine
HERE = os.path.dirname(os.path.abspath(__file__))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def engine_with(monkeypatch, **env):
    """A fresh context whose launch knobs come from the environment at creation (kbest_create reads them once)."""
    for key, val in env.items():
        monkeypatch.setenv(key, str(val))
    eng = pk.KBestEngine(0)
    for key in env:
        monkeypatch.delenv(key)
    return eng


def golden_cases(max_rows=64, B=2):
    """The k-best cases of boundary_golden.npz as one-problem cases (the same matrix B times)."""
    z = np.load(os.path.join(HERE, "golden", "boundary_golden.npz"))
    out = []
    for name in (str(n) for n in z["kbest_names"]):
        N, M, k, mx, _ = (int(x) for x in z[name + "/meta"])
        if N <= max_rows:
            out.append(dict(N=N, M=M, k=k, B=B, maximize=bool(mx), cutoff=float(z[name + "/cutoff"][0]), kind="golden-" + name,
                            C=np.tile(z[name + "/cost"], (B, 1))))
    return out


def expect(case):
    """The checker's tables of a case (and the compiled reference's, where it exists, must be the same)."""
    onf, or4c, oc4r, og, _ = ol.orc_kbest_batch(case["C"], case["N"], case["M"], case["k"], case["maximize"], case["cutoff"])
    if ol.have_ref():
        for b in range(0, case["B"], 3):
            rn, rr, _, rg = ol.ref_kbest(case["C"][b], case["N"], case["M"], case["k"], case["maximize"], case["cutoff"])
            assert rn == onf[b] and (rr[:rn] == or4c[b, :rn]).all() and (bits(rg[:rn]) == bits(og[b, :rn])).all(), case["kind"]
    return onf, or4c, oc4r, og


def same_tables(got, want, case, what):
    nf, r4c, c4r, g = got[:4]
    onf, or4c, oc4r, og = want
    M = case["M"]
    assert (nf == onf).all(), (what, case["kind"], case["N"], M, case["k"], case["cutoff"], nf, onf)
    for b in range(case["B"]):
        n = int(onf[b])
        assert (bits(g[b, :n]) == bits(og[b, :n])).all(), (what, case["kind"], b)
        assert (r4c[b, :n] == or4c[b, :n]).all(), (what, case["kind"], b)
        real = oc4r[b, :n] < M
        assert (c4r[b, :n][real] == oc4r[b, :n][real]).all(), (what, case["kind"], b)


def same_canonical(got, case, what):
    """KBEST_FLAG_CANONICAL_TIES against the checker's canonical k best (the fast kernels' own answer on ties)."""
    nf, r4c, _, g = got[:4]
    for b in range(case["B"]):
        n, cr, cg, _, resolved = ol.canonical_kbest(case["C"][b], case["N"], case["M"], case["k"], case["maximize"], case["cutoff"])
        assert nf[b] == n, (what, case["kind"], b, nf[b], n)
        assert (bits(g[b, :n]) == bits(cg)).all(), (what, case["kind"], b)
        assert (r4c[b, :n] == cr).all(), (what, case["kind"], b)


# ---------------------------------------------------------------- k-best routes

ROUTES = {
    "lane": (dict(KBEST_FORCE_LANE=1), E.KBEST_ROUTE_LANE, 32, True),
    "small": (dict(KBEST_FORCE_SMALL=1), E.KBEST_ROUTE_SMALL, 32, False),
    "fast": (dict(KBEST_NO_SMALL=1, KBEST_NO_LANE=1), E.KBEST_ROUTE_FAST, 64, False),
    "wide": (dict(KBEST_FORCE_WIDE=1), E.KBEST_ROUTE_WIDE, 64, False),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_kbest_routes_on_the_cutoff(monkeypatch, route):
    """B1 (tie-free: the kernel's own answer, slot for slot), B2 (integer ties on the boundary: the default entry's reference
    ties and KBEST_FLAG_CANONICAL_TIES against the canonical list), B3 (0.1 grids: the default entry) and the golden cases on one
    forced route.  Every third B1 case takes int8 tables.  B1 calls must report the route's kernel alone (no tie re-run happens
    without ties); B2 / B3 calls that re-run tied problems on the reference-order kernel report that kernel instead.  (B3 is not
    held to canonical_kbest: on a grid that is not exact in binary, which solutions a cutHyp keeps depends on the tree the
    enumeration split, and the checker's canonical list is cut from the reference's tree.)"""
    knobs, bit, max_rows, square = ROUTES[route]
    eng = engine_with(monkeypatch, **knobs)
    seed = 0xB1 + sorted(ROUTES).index(route)
    b1, on1 = bl.b1_cases(seed, 36, rows=(2, max_rows), square=square)
    b2, on2 = bl.b2_cases(seed + 10, 30)
    b3, on3 = bl.b3_cases(seed + 20, 30)
    assert on1 >= 140 and on2 >= 40 and on3 >= 20, (on1, on2, on3)
    for i, case in enumerate(b1 + golden_cases(max_rows)):
        want = expect(case)
        i8 = i % 3 == 0
        got = eng.kbest(case["C"], case["N"], case["M"], case["k"], case["maximize"], case["cutoff"], tables_i8=i8)
        r = eng.last_route()
        if case["kind"].startswith("b1"):
            assert r & bit and not (r & E.KBEST_ROUTE_EXACT), (route, r)
        same_tables([np.asarray(x, dtype=np.float64 if j == 3 else np.int64) for j, x in enumerate(got)], want, case, route)
    direct = 0
    for case in b2 + b3:
        want = expect(case)
        got = eng.kbest(case["C"], case["N"], case["M"], case["k"], case["maximize"], case["cutoff"])
        r = eng.last_route()
        assert r & (bit | E.KBEST_ROUTE_EXACT), (route, r)
        direct += bool(r & bit)
        same_tables(got, want, case, route + " default")
        if case["kind"].startswith("b2"):
            got = eng.kbest(case["C"], case["N"], case["M"], case["k"], case["maximize"], case["cutoff"], canonical_ties=True)
            assert eng.last_route() & bit, (route, eng.last_route())
            same_canonical(got, case, route + " canonical")
    assert direct >= 5, direct
    eng.close()


def test_kbest_general_size_rows_on_the_cutoff(engine):
    """65 - 200 rows: the general-size kernel without any knob."""
    cases, on = bl.b1_cases(0x65, 10, rows=(65, 200), k=(3, 20, 60), B=2)
    assert on >= 20
    for case in cases:
        want = expect(case)
        got = engine.kbest(case["C"], case["N"], case["M"], case["k"], case["maximize"], case["cutoff"])
        assert engine.last_route() & E.KBEST_ROUTE_WIDE, engine.last_route()
        same_tables(got, want, case, "wide natural")


@pytest.mark.parametrize("rows", [(2, 64), (65, 300), (513, 1024)])
def test_kbest_reference_order_on_the_cutoff(engine, rows):
    """KBEST_FLAG_REFERENCE_ORDER: everything the checker's, slot for slot, col4row on padded columns included; up to 64 rows,
    65 - 1 024 rows (at most 24 columns above 512 rows)."""
    big = rows[0] > 512
    cases, on = bl.b1_cases(0xE0 + rows[0], 3 if big else 12, rows=rows, k=(3, 20), B=2, max_cols=24 if big else None)
    if rows[1] <= 64:
        more, on2 = bl.b2_cases(0xE1, 20)
        more3, on3 = bl.b3_cases(0xE2, 20)
        assert on2 >= 20 and on3 >= 10
        cases += more + more3 + golden_cases()
    assert on >= (6 if big else 24)
    for case in cases:
        assert soak_lib.check_case(engine, case, reference_order=True) is None, case["kind"]
        assert engine.last_route() == E.KBEST_ROUTE_EXACT


def _dev(eng, case, **kw):
    import torch
    dev = torch.device("cuda", 0)
    B, N, M, k = case["B"], case["N"], case["M"], case["k"]
    i8 = kw.pop("tables_i8", False)
    tdt = torch.int8 if i8 else torch.int32
    d_cost = torch.from_numpy(np.ascontiguousarray(case["C"])).to(dev)
    d_r = torch.full((B, k, M), -7, dtype=tdt, device=dev)
    d_c = torch.full((B, k, N), -7, dtype=tdt, device=dev)
    d_g = torch.full((B, k), float("nan"), dtype=torch.float64, device=dev)
    d_n = torch.full((B,), -7, dtype=torch.int32, device=dev)
    d_f = torch.zeros(B, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    eng.kbest_dev(d_cost, B, N, M, k, d_r, d_c, d_g, d_n, maximize=case["maximize"], cutoff=case["cutoff"], stream=st, tables_i8=i8,
                  d_tie_flags=d_f, **kw)
    torch.cuda.synchronize()
    route = eng.last_route()
    return d_cost, d_r, d_c, d_g, d_n, d_f, st, route


def test_kbest_device_entry_and_tie_resolution_on_the_cutoff(engine):
    """kbest_dev, then kbest_resolve_ties_dev: tie-free B1 as launched; B2, B3 and the golden cases after the resolution, the
    default (reference ties) slot for slot, int8 tables too.  nf included: the b3nf golden cases keep fewer solutions on the
    reference-order kernel than in the first pass, and the re-run's count must reach the device's nf."""
    b1, on1 = bl.b1_cases(0xDE, 16, rows=(2, 48))
    b2, on2 = bl.b2_cases(0xDF, 24)
    b3, on3 = bl.b3_cases(0xE3, 24)
    assert on1 >= 60 and on2 >= 30 and on3 >= 15
    for i, case in enumerate(b1 + b2 + b3 + golden_cases()):
        i8 = i % 2 == 1
        d_cost, d_r, d_c, d_g, d_n, d_f, st, _ = _dev(engine, case, tables_i8=i8)
        engine.resolve_ties_dev(d_cost, case["B"], case["N"], case["M"], case["k"], d_r, d_c, d_g, d_f, maximize=case["maximize"],
                                cutoff=case["cutoff"], stream=st, tables_i8=i8, d_nf=d_n)
        import torch
        torch.cuda.synchronize()
        got = (d_n.cpu().numpy(), d_r.cpu().numpy().astype(np.int64), d_c.cpu().numpy().astype(np.int64), d_g.cpu().numpy())
        same_tables(got, expect(case), case, "dev + resolve")


def test_kbest_relay_on_the_cutoff(monkeypatch):
    """Relay launches of the 64-row kernel (KBEST_RELAY=3) through the device entry on B1 batches of 24 row permutations."""
    eng = engine_with(monkeypatch, KBEST_RELAY=3, KBEST_NWAVES=12, KBEST_NO_SMALL=1, KBEST_NO_LANE=1, KBEST_NO_TINY=1, KBEST_NO_BNB=1)
    cases, on = bl.b1_cases(0x3E, 10, rows=(24, 64), k=(40, 200), B=24, square=True)
    assert on >= 200
    relayed = 0
    for case in cases:
        before = eng.relay_launches()
        _, d_r, d_c, d_g, d_n, _, _, route = _dev(eng, case)
        relayed += eng.relay_launches() > before and bool(route & E.KBEST_ROUTE_RELAY)
        got = (d_n.cpu().numpy(), d_r.cpu().numpy(), d_c.cpu().numpy(), d_g.cpu().numpy())
        same_tables(got, expect(case), case, "relay")
    assert relayed >= 5, relayed
    eng.close()


@pytest.mark.parametrize("split", [2, 4])
def test_kbest_split_on_the_cutoff(monkeypatch, split):
    """KBEST_SPLIT: 2 or 4 workgroups per matrix and the merge (KBEST_ROUTE_SPLIT).  The split applies only without the tie check
    (tie_check=False: kbest_capi.cpp, batch_dev_impl runs tie mode unsplit), square 33 - 64 rows, k >= 50."""
    eng = engine_with(monkeypatch, KBEST_SPLIT=split)
    cases, on = bl.b1_cases(0x5B + split, 10, rows=(33, 64), k=(50, 120), B=3, square=True)
    assert on >= 30
    for case in cases:
        got = eng.kbest(case["C"], case["N"], case["M"], case["k"], case["maximize"], case["cutoff"], tie_check=False)
        assert eng.last_route() & E.KBEST_ROUTE_FAST and eng.last_route() & E.KBEST_ROUTE_SPLIT, eng.last_route()
        same_tables(got, expect(case), case, f"split {split}")
    eng.close()


@pytest.mark.parametrize("G,S", [(0, 0), (2, 2), (3, 8)])
def test_kbest_multi_entry_on_the_cutoff(G, S):
    """KBestMulti on logical devices: G = 0 is batch mode over two of them (B1, B2, B3 and the golden cases), (G, S) subtree mode
    with G devices and S shards (B1: square, tie-free)."""
    subtree = G > 0
    multi = pk.KBestMulti([0] * (G or 2))
    cases, on = bl.b1_cases(0x3C + S, 8, rows=(8, 48), k=(10, 40, 120), B=3, square=True)
    if not subtree:
        more, on2 = bl.b2_cases(0x3D, 12)
        more3, on3 = bl.b3_cases(0x3E, 12)
        assert on2 >= 10 and on3 >= 6
        cases += more + more3 + golden_cases(B=3)
    assert on >= 24
    for case in cases:
        got = multi.kbest(case["C"], case["N"], case["M"], case["k"], case["maximize"], case["cutoff"], subtree=subtree, n_shard=S)
        assert multi.tables_agree()
        same_tables(got, expect(case), case, f"multi G={G} S={S}")
    multi.close()


# ---------------------------------------------------------------- association

TINY = [(6, 3), (12, 5), (40, 2)]
BNB = [(20, 10), (30, 16), (50, 8)]


def _chain(f, k, canonical):
    """The checker's getAssignmentProbs on a raw block and its high-precision probabilities: (want nf, hp [nM, nL + 1])."""
    nL, nM = f["nL"], f["nM"]
    cond, idx = ol.condition_costs(f["cost"], nL + nM, nM)
    cl = len(idx) - nM
    hp, nf = ol.hp_assignment_prob(cond, cl, nM, k, canonical=canonical)
    full = np.array([[0] * (nL + 1) for _ in range(nM)], dtype=object)
    full[:, idx[:cl]] = hp[:, :cl]
    full[:, nL] = hp[:, cl]
    if nM > 1:
        _, onf = ol.assignment_prob(cond, cl, nM, k)
        assert onf == nf
    else:
        # one column: the reference enumerates nothing (assignment.cpp:554-570); the engine reports the entries it weighs, x < 42,
        # at most k
        nf = min(int((cond[: cl + 1] < 42.0).sum()), k)
    return nf, full, cond, cl


def _check_frames(out, nf, frames, k, canonical, what):
    for i, f in enumerate(frames):
        want_nf, hp, _, _ = _chain(f, k, canonical)
        assert nf[i] == want_nf, (what, i, f["nL"], f["nM"], nf[i], want_nf)
        bad = ol.hp_mismatch(out[i], hp, want_nf)
        assert bad is None, (what, i, f["nL"], f["nM"], bad)


@pytest.mark.parametrize("family", ["tiny", "bnb", "bnb256"])
def test_assoc_kernels_on_the_gate(monkeypatch, family):
    """A1 frames on the kernel of their shape (kbest_tiny.hip: nM <= 8, <= 64 rows; kbest_bnb.hip: up to 16 measurements,
    1 024-thread workgroups, and 256-thread ones with KBEST_BNB_SMALL_FROM=1), shown to have run by comparing bit for bit with a
    context that has that kernel switched off (which must differ from it nowhere, yet is not the same code), and both against
    the high-precision probabilities: weights(condition=True) one frame per call and as a batch, weights() on the conditioned
    blocks, set_reference_order(2) against the reference's list, brute_force on the smaller conditioned blocks."""
    shapes = TINY if family == "tiny" else BNB
    knobs = dict(KBEST_BNB_SMALL_FROM=1) if family == "bnb256" else {}
    off = dict(KBEST_NO_TINY=1) if family == "tiny" else dict(KBEST_NO_BNB=1, KBEST_NO_TINY=1)
    fast = engine_with(monkeypatch, **knobs)
    plain = engine_with(monkeypatch, **off)
    frames, on = bl.a1_frames(0xA1 + len(family), 18, shapes)
    assert on >= 12, on
    k = 200
    nLs, nMs = [f["nL"] for f in frames], [f["nM"] for f in frames]
    costs = [f["cost"] for f in frames]
    for i, f in enumerate(frames):
        o1, n1 = fast.weights([f["cost"]], [f["nL"]], [f["nM"]], k, condition=True)
        o2, n2 = plain.weights([f["cost"]], [f["nL"]], [f["nM"]], k, condition=True)
        assert n1[0] == n2[0] and np.array_equal(o1[0], o2[0]), (family, i)
        _check_frames(o1, n1, [f], k, True, family)
    out, nf = fast.weights(costs, nLs, nMs, k, condition=True)
    ref, nfr = plain.weights(costs, nLs, nMs, k, condition=True)
    assert (nf == nfr).all() and all(np.array_equal(a, b) for a, b in zip(out, ref))
    _check_frames(out, nf, frames, k, True, family + " batch")
    # conditioned blocks through assignmentProb alone
    conds, cls, cms = [], [], []
    for f in frames:
        _, _, cond, cl = _chain(f, k, True)
        conds.append(cond)
        cls.append(cl)
        cms.append(f["nM"])
    out, nf = fast.weights(conds, cls, cms, k)
    ref, nfr = plain.weights(conds, cls, cms, k)
    assert (nf == nfr).all() and all(np.array_equal(a, b) for a, b in zip(out, ref))
    for i in range(len(conds)):
        hp, hnf = ol.hp_assignment_prob(conds[i], cls[i], cms[i], k, canonical=True)
        assert nf[i] == hnf, (family, i)
        assert ol.hp_mismatch(out[i], hp, hnf) is None, (family, "conditioned", i, ol.hp_mismatch(out[i], hp, hnf))
    # the reference's own list (set_reference_order(2): frames with a tie at slot k on the reference-order kernel)
    fast.set_reference_order(2)
    out, nf = fast.weights(costs, nLs, nMs, k, condition=True)
    fast.set_reference_order(0)
    _check_frames(out, nf, frames, k, False, family + " reference order")
    # bruteForceProb on the conditioned blocks of few assignments
    small = [i for i in range(len(conds)) if cms[i] <= 5 and cls[i] + cms[i] <= 12]
    assert len(small) >= (3 if family == "tiny" else 0)
    for i in small:
        _, _, uk = ol.brute_force_prob(conds[i], cls[i], cms[i])
        out, nf = fast.weights([conds[i]], [cls[i]], [cms[i]], uk, brute_force=True)  # the reference's own k (its bound)
        hb, hbn = ol.hp_brute_force_prob(conds[i], cls[i], cms[i])
        assert hbn is None or nf[0] == hbn, (family, "brute", i, nf[0], hbn)
        assert ol.hp_mismatch(out[0], hb, hbn) is None, (family, "brute", i)
    fast.close()
    plain.close()


def test_assoc_general_pipeline_and_fused_small_on_the_gate(engine):
    """Raw blocks beyond the fused kernels' shapes: more than 64 raw rows with at most 32 kept (fused kbest_small.hip) and more
    than 32 kept rows (the general pipeline).  The association entries report no route; which kernel takes these shapes follows
    from the routing limits of kbest_capi.cpp and is not shown here."""
    fused, on1 = bl.a1_frames(0xF5, 12, [(80, 4), (70, 3), (66, 6)], inf_frac=0.88)
    fused = [f for f in fused if len(ol.condition_costs(f["cost"], f["nL"] + f["nM"], f["nM"])[1]) <= 32]
    general, on2 = bl.a1_frames(0x6E, 10, [(50, 20), (60, 24)], inf_frac=0.1)
    assert len(fused) >= 8 and on1 >= 6 and on2 >= 6
    for frames, what in ((fused, "fused small"), (general, "general")):
        out, nf = engine.weights([f["cost"] for f in frames], [f["nL"] for f in frames], [f["nM"] for f in frames], 200, condition=True)
        _check_frames(out, nf, frames, 200, True, what)


@pytest.mark.parametrize("knobs", [{}, {"KBEST_NO_TINY": 1, "KBEST_NO_BNB": 1}])
def test_assoc_single_column_on_the_gate(monkeypatch, knobs):
    """A2: nM == 1 -- exp(-x) over the conditioned entries x < 42, the entry of exactly 42 weighs nothing; nf = the entries
    weighed.  Up to 64 raw rows and beyond (70 - 120), on the fused kernels and with them switched off."""
    eng = engine_with(monkeypatch, **knobs)
    frames, on = bl.a2_frames(0xA2, 20)
    more, on2 = bl.a2_frames(0xA3, 8, nLs=(70, 95, 120))
    assert on == 20 and on2 == 8
    frames += more
    out, nf = eng.weights([f["cost"] for f in frames], [f["nL"] for f in frames], [1] * len(frames), 200, condition=True)
    _check_frames(out, nf, frames, 200, True, "nM = 1")
    for f, o in zip(frames, out):
        cond, idx = ol.condition_costs(f["cost"], f["nL"] + 1, 1)
        at42 = idx[: len(idx) - 1][cond[: len(idx) - 1] == 42.0]
        assert (o[0, at42] == 0).all()
    eng.close()


def test_assoc_device_entry_and_conditioning_on_the_gate(engine):
    """assoc_probs_dev on A1 frames of every fused shape, and condition_costs on the device bit for bit (entries of exactly 42
    kept, one ulp beyond dropped)."""
    import torch
    frames, on = bl.a1_frames(0xDA, 24, TINY + BNB + [(4, 4)])
    assert on >= 16
    conds, idxs = engine.condition_costs([f["cost"] for f in frames], [f["nL"] + f["nM"] for f in frames], [f["nM"] for f in frames])
    for f, c, ix in zip(frames, conds, idxs):
        wc, wi = ol.condition_costs(f["cost"], f["nL"] + f["nM"], f["nM"])
        assert (ix == wi).all() and (bits(c) == bits(wc)).all()
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    F = len(frames)
    nL = np.array([f["nL"] for f in frames], np.int32)
    nM = np.array([f["nM"] for f in frames], np.int32)
    nR = nL + nM
    coff = np.concatenate([[0], np.cumsum(nR.astype(np.int64) * nM)[:-1]])
    poff = np.concatenate([[0], np.cumsum(nM.astype(np.int64) * (nL + 1))[:-1]])
    k = 200
    d_probs = torch.zeros(int((nM.astype(np.int64) * (nL + 1)).sum()), dtype=torch.float64, device=dev)
    d_nf = torch.zeros(F, dtype=torch.int32, device=dev)
    engine.reserve_assoc(F, int(nR.max()), int(nM.max()), k)
    engine.assoc_probs_dev(F, int(nR.max()), int(nM.max()), t(nL), t(nM), t(nR.astype(np.int32)), t(np.concatenate([f["cost"] for f in frames])),
                           t(coff), k, d_probs, t(poff), d_nf, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    p = d_probs.cpu().numpy()
    out = [p[poff[i]: poff[i] + nM[i] * (nL[i] + 1)].reshape(nM[i], nL[i] + 1) for i in range(F)]
    _check_frames(out, d_nf.cpu().numpy(), frames, k, True, "assoc_probs_dev")


def test_assoc_k_ending_on_the_gate_level(monkeypatch):
    """kbest_tiny.hip's pass 2 collects the assignments up to the k-th one's bucket and none beyond the cutoff best + 42 (kept when
    equal: cpp:709-719).  With k one past the assignments strictly inside the gate, the k-th one lies exactly on best + 42: it
    counts in nf (weight 0).  nf exactly, the probabilities within the high-precision bound, bit for bit the enumeration's."""
    fast = pk.KBestEngine(0)
    plain = engine_with(monkeypatch, KBEST_NO_TINY=1)
    frames, _ = bl.a1_frames(0x6A7E, 40, TINY + [(4, 4), (8, 3)])
    used = 0
    for f in frames:
        nL, nM = f["nL"], f["nM"]
        cond, idx = ol.condition_costs(f["cost"], nL + nM, nM)
        nf, _, _, g = ol.orc_kbest(cond, len(idx), nM, 4096, cutoff=42.0)
        inside = int((g[:nf] < g[0] + 42.0).sum())
        if nf >= 4096 or nf == inside or inside + 1 > 1024:
            continue
        k = inside + 1
        used += 1
        o1, n1 = fast.weights([f["cost"]], [nL], [nM], k, condition=True)
        o2, n2 = plain.weights([f["cost"]], [nL], [nM], k, condition=True)
        assert n1[0] == n2[0] == k and np.array_equal(o1[0], o2[0]), (nL, nM, k, n1, n2)
        _check_frames(o1, n1, [f], k, True, "k on the gate level")
    assert used >= 30, used
    fast.close()
    plain.close()
