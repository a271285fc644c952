"""CPU: problems exactly on the cutoff and gate comparisons (tests/boundary_lib.py).  The checker against the fixture the compiled
reference wrote (tests/golden/boundary_golden.npz, runs everywhere), against the compiled reference itself on the live generators
(where oracle/_ref exists), and the high-precision probabilities of oracle_lib against both."""
import os

import numpy as np
import pytest

import boundary_lib as bl
import oracle_lib as ol

HERE = os.path.dirname(os.path.abspath(__file__))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def bgold():
    return np.load(os.path.join(HERE, "golden", "boundary_golden.npz"))


def test_golden_kbest_on_the_cutoff(bgold):
    z = bgold
    names = [str(n) for n in z["kbest_names"]]
    assert len(names) >= 40
    cut_short = 0
    for name in names:
        N, M, k, mx, nf = (int(x) for x in z[name + "/meta"])
        cut = float(z[name + "/cutoff"][0])
        onf, r4c, c4r, g = ol.orc_kbest(z[name + "/cost"], N, M, k, bool(mx), cut)
        assert onf == nf, name
        assert (r4c[:nf] == z[name + "/row4col"]).all() and (c4r[:nf] == z[name + "/col4row"]).all(), name
        assert (bits(g[:nf]) == bits(z[name + "/gain"])).all(), name
        cut_short += nf < k
    assert cut_short >= len(names) // 2  # the cutoff, not k, ends most of these lists


def test_golden_frames_on_the_gate(bgold):
    z = bgold
    names = [str(n) for n in z["frame_names"]]
    assert len(names) >= 30
    fortytwo = 0
    for name in names:
        nL, nM, k, kept, brute = (int(x) for x in z[name + "/meta"])
        cond, idx = ol.condition_costs(z[name + "/raw"], nL + nM, nM)
        assert len(idx) == kept and (idx == z[name + "/rowIdx"]).all(), name
        assert (bits(cond) == bits(z[name + "/cond"])).all(), name
        fortytwo += int((cond == 42.0).any())
        cl = kept - nM
        p, nf = ol.assignment_prob(cond, cl, nM, k)
        want = z[name + "/probs"]
        assert (bits(p.reshape(-1)[: want.size]) == bits(want.reshape(-1))).all(), name
        # the reference's own float64 probabilities are within the high-precision bound of the GPU tests
        hp, hnf = ol.hp_assignment_prob(cond, cl, nM, k)
        assert hnf is None or hnf == nf, name
        assert ol.hp_mismatch(want.reshape(hp.shape), hp, hnf) is None, name
        if brute:
            pb, nfb, _ = ol.brute_force_prob(cond, cl, nM)
            assert (bits(pb.reshape(-1)) == bits(z[name + "/brute"].reshape(-1)[: pb.size])).all(), name
            hb, hbn = ol.hp_brute_force_prob(cond, cl, nM)
            assert ol.hp_mismatch(pb, hb, hbn) is None, name
    assert fortytwo >= 25


def test_generators_reach_their_boundaries():
    """The floors the GPU legs rely on: every family puts problems exactly (B3: within 2 ulps) on a boundary, B1 tie-free with
    the cutoff on the slot it chose."""
    cases, on = bl.b1_cases(11, 30)
    assert on == sum(c["B"] for c in cases)
    for c in cases:
        nf, _, _, g = ol.orc_kbest(c["C"][0], c["N"], c["M"], c["k"] + 1, c["maximize"])
        j = c["slot"]
        e = g[0] - c["cutoff"] if c["maximize"] else g[0] + c["cutoff"]
        assert (np.diff(g[:nf]) != 0).all() and e == bl.b1_target(g[j], c["which"], c["maximize"])
    assert bl.b2_cases(12, 30)[1] >= 40
    assert bl.b3_cases(13, 30)[1] >= 25
    frames, on = bl.a1_frames(14, 30, [(6, 3), (20, 10)])
    assert on >= 25
    frames, on = bl.a2_frames(15, 20)
    assert on == 20


@pytest.mark.skipif(not (ol.have_ref() and ol.have_ref_assign()), reason="oracle/_ref not built (no reference sources here)")
def test_generators_against_the_compiled_reference():
    """Live generators: the checker equals the compiled reference bit for bit on every boundary problem (nf, gains, both
    tables; conditioned blocks, row indices, probabilities)."""
    on = 0
    for cases, n_on in (bl.b1_cases(21, 60), bl.b1_cases(22, 4, rows=(65, 140), k=(3, 20), B=2), bl.b2_cases(23, 120),
                        bl.b3_cases(24, 120)):
        on += n_on
        for c in cases:
            for b in range(c["B"]):
                a = ol.orc_kbest(c["C"][b], c["N"], c["M"], c["k"], c["maximize"], c["cutoff"])
                r = ol.ref_kbest(c["C"][b], c["N"], c["M"], c["k"], c["maximize"], c["cutoff"])
                nf = a[0]
                assert nf == r[0], (c["kind"], c["N"], c["M"])
                assert (a[1][:nf] == r[1][:nf]).all() and (a[2][:nf] == r[2][:nf]).all() and (bits(a[3][:nf]) == bits(r[3][:nf])).all()
    assert on >= 400
    on = 0
    for frames, n_on in (bl.a1_frames(25, 80, [(6, 3), (12, 5), (40, 2), (20, 10), (30, 16), (50, 8)]), bl.a2_frames(26, 30)):
        on += n_on
        for f in frames:
            nL, nM = f["nL"], f["nM"]
            cond, idx = ol.condition_costs(f["cost"], nL + nM, nM)
            rc, ri = ol.ref_condition_costs(f["cost"], nL + nM, nM)
            assert (idx == ri).all() and (bits(cond) == bits(rc)).all()
            cl = len(idx) - nM
            p, _ = ol.assignment_prob(cond, cl, nM, 200)
            rp = ol.ref_assignment_prob(cond, cl, nM, 200)
            assert (bits(p.reshape(-1)) == bits(rp.reshape(-1)[: p.size])).all()
    assert on >= 90
