"""GPU: the column-scaled exact tiers (kbest_bigcluster.hip, kbest_frontier.hip, kbest_frontier_sample.hip) and the frame entries
above them where Z' leaves the normal doubles.  Every comparison is against the long-double truth of tests/range_lib.py, never
against another kernel or a float64 restatement; the contract is the one of tests/test_range_cpu.py:
    A  answered (info 1; method 0 with the cluster counted; draws with their terms): within 1e-12 of the truth, log Z and logPerm
       within 1e-12 max(1, |.|)
    B  infeasible (info 0, method -2, logPerm -inf, assign -1) only without a complete assignment, and always then
    C  declined (info -5): outputs untouched; in a frame the cluster goes on to the next tier, at last to the enumeration (k >= 1:
       its columns are assignmentProb's within 1e-9, method 1 or 2) or refuses the frame (k = 0 and the device entries: method -1)
    D  never declined with log Z' >= -660
Equal bits where the project promises them: the device entries against the host entries, a cluster alone against in a batch.  The
truths are computed once per module; the kernels take milliseconds."""
import numpy as np
import pytest
import torch

import frontier_sample_check as fsc
import probabilisticsemslam_amd as pk
import range_lib as rl
from test_gpu_frontier_sample import run_dev as sampler_dev
from test_gpu_hybrid_dev import host as probs_host, run_dev as probs_dev, same_bits as same_prob_bits
from test_gpu_hybrid_sample_dev import host as draws_host, run_dev as draws_dev, same_bits as same_draw_bits
from test_gpu_permanent import bits

pytestmark = pytest.mark.gpu

PAD, UNTOUCHED, INT_PAD = 64, -5.0, -77
N_DRAW = 4096
SEED = fsc.SEED
MAX_EXACT = 4   # every generated cluster is open; the ordinary cluster of two columns beside it is the partial kernel's
K = 200


@pytest.fixture(scope="module")
def eng():
    e = pk.KBestEngine(0)
    yield e
    e.close()


def unique(cases):
    seen, out = set(), []
    for c in cases:
        if c.name not in seen:
            seen.add(c.name)
            out.append(c)
    return out


NONE = tuple(rl.no_matching().values())
NONE_FRAMES = tuple(c for k, c in rl.no_matching().items() if k != "empty_column")
BIG, FRONTIER = rl.big_family(), rl.frontier_family()


def run_cluster_entry(eng, cases, tier):
    """kbest_bigcluster_probs_f64_dev / kbest_frontier_probs_f64_dev on the sub-blocks of `cases` in one call, sentinels between and
    around everything.  Returns one (probs or None, logZ or None, info) per case: None where the sentinels came back."""
    dev = torch.device("cuda", 0)
    sub, subOff, probOff, at, pat = [np.full(PAD, -7.0)], [], [], PAD, PAD
    for c in cases:
        subOff.append(at)
        probOff.append(pat)
        sub += [c.block, np.full(PAD, -7.0)]
        at += len(c.block) + PAD
        pat += c.m * (c.nLk + 1) + PAD
    sub = np.concatenate(sub)
    d_sub = torch.from_numpy(sub).to(dev)
    d_probs = torch.full((pat,), UNTOUCHED, dtype=torch.float64, device=dev)
    d_logZ = torch.full((len(cases) + 2,), UNTOUCHED, dtype=torch.float64, device=dev)
    d_int = torch.full((2, len(cases) + 2), INT_PAD, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    m, nLk = [c.m for c in cases], [c.nLk for c in cases]
    if tier == "big":
        eng.bigcluster_probs_dev(m, nLk, subOff, probOff, d_sub, d_probs, d_logZ[1:], d_int[0, 1:])
    else:
        eng.frontier_probs_dev(m, nLk, subOff, probOff, d_sub, d_probs, d_logZ[1:], d_int[0, 1:], d_int[1, 1:])
    torch.cuda.synchronize()
    hp, hz, hi = d_probs.cpu().numpy(), d_logZ.cpu().numpy(), d_int.cpu().numpy()
    assert np.array_equal(bits(d_sub.cpu().numpy()), bits(sub))
    assert hz[0] == hz[-1] == UNTOUCHED and (hi[:, 0] == INT_PAD).all() and (hi[:, -1] == INT_PAD).all()
    out, end = [], 0
    for j, c in enumerate(cases):
        assert (hp[end:probOff[j]] == UNTOUCHED).all(), c.name
        end = probOff[j] + c.m * (c.nLk + 1)
        p, lz = hp[probOff[j]:end].reshape(c.m, c.nLk + 1).copy(), float(hz[1 + j])
        out.append((None if (p == UNTOUCHED).all() else p, None if lz == UNTOUCHED else lz, int(hi[0, 1 + j])))
    assert (hp[end:] == UNTOUCHED).all()
    return out


def report(what, cases, infos):
    print(f"{what}: " + ", ".join(f"{c.name} ({rl.truth_of(c).logZprime:.1f}): {i}" for c, i in zip(cases, infos)))


# ---- 1. the per-cluster entries --------------------------------------------------------------------------------------------------------
def test_bigcluster_tier(eng):
    """hub(17 .. 20) and two_hubs on both sides of the range, and the clusters without a complete assignment, in one call."""
    cases = BIG + NONE
    got = run_cluster_entry(eng, cases, "big")
    report("kbest_bigcluster_probs_f64_dev info", cases, [g[2] for g in got])
    safe, deep = rl.counts(BIG)
    assert safe >= 6 and deep >= 4
    for c, g in zip(cases, got):
        rl.check_cluster(c, *g)


def test_frontier_tier(eng):
    """two_hubs and pair chains of 9 .. 32 pairs on both sides of the range, and the clusters without a complete assignment."""
    cases = FRONTIER + NONE
    got = run_cluster_entry(eng, cases, "frontier")
    report("kbest_frontier_probs_f64_dev info", cases, [g[2] for g in got])
    safe, deep = rl.counts(FRONTIER)
    assert safe >= 6 and deep >= 4
    for c, g in zip(cases, got):
        rl.check_cluster(c, *g)


def test_frontier_sampler(eng):
    """The same clusters, 4 096 draws each: info, log Z and the untouched outputs as the tier's; every draw a complete assignment
    whose logTerm is the long-double log-probability of that joint; empirical marginals within 4 / sqrt(N)."""
    cases = FRONTIER + NONE
    clusters = [(j, dict(block=c.block, nL=c.nLk, m=c.m, keys=np.arange(c.nLk + c.m, dtype=np.int32))) for j, c in enumerate(cases)]
    got = sampler_dev(eng, clusters, N_DRAW)
    tier = run_cluster_entry(eng, cases, "frontier")
    report("kbest_frontier_sample_f64_dev info", cases, [g[3] for g in got])
    for c, (a, lt, lz, info, W), (_, tlz, tinfo) in zip(cases, got, tier):
        t = rl.truth_of(c)
        assert info == tinfo, (c.name, info, tinfo)  # (the sampler follows the tier)
        if info == 1:
            assert bits(lz) == bits(tlz), c.name
            rl.close(lz, t.logZ, c.name)
            rl.check_draws(c, a, lt)
        elif info == 0:
            assert t.logZprime == -np.inf and (a == -1).all() and np.isnan(lt).all() and lz == -np.inf, c.name
        else:
            assert info == rl.OUT_OF_RANGE and -np.inf < t.logZprime < rl.SAFE, (c.name, info, t.logZprime)
            assert (a == -5).all() and (lt == UNTOUCHED).all() and lz == UNTOUCHED, (c.name, "a declined cluster's outputs were written")


# ---- 2. the frame entries ----------------------------------------------------------------------------------------------------------------
def frames_of(cases):
    return [c.cost for c in cases], [c.nL for c in cases], [c.nM for c in cases]


@pytest.mark.parametrize("k", [0, K])
def test_hybrid_exact_probs(eng, k):
    cases = BIG + NONE_FRAMES
    out, method, nOpen, nBig, _, lp = eng.hybrid_exact_probs(*frames_of(cases), k, max_exact=MAX_EXACT)
    report(f"hybrid_exact_probs(k = {k}) method", cases, method.tolist())
    for j, c in enumerate(cases):
        assert nOpen[j] == 1, c.name
        rl.check_frame(c, out[j], int(method[j]), float(lp[j]), int(nBig[j]), k)


@pytest.mark.parametrize("k", [0, K])
def test_hybrid_frontier_probs(eng, k):
    """Every case: a hub is wider than 16 and goes frontier -> big-cluster; what both decline goes on to the enumeration."""
    cases = tuple(unique(BIG + FRONTIER)) + NONE_FRAMES
    out, method, nOpen, nBig, _, lp, nFr = eng.hybrid_frontier_probs(*frames_of(cases), k, max_exact=MAX_EXACT)
    report(f"hybrid_frontier_probs(k = {k}) method", cases, method.tolist())
    for j, c in enumerate(cases):
        assert nOpen[j] == 1, c.name
        rl.check_frame(c, out[j], int(method[j]), float(lp[j]), int(nFr[j] + nBig[j]), k)


def test_hybrid_frontier_probs_dev(eng):
    """The one-stream device entry: the host entry's bits (k = 0, no big-cluster tier), and the contract; a declined cluster
    refuses its frame."""
    cases = FRONTIER + NONE_FRAMES
    frames, nL, nM = frames_of(cases)
    want = probs_host(eng, frames, nL, nM, False, MAX_EXACT, 16)
    got = probs_dev(eng, frames, nL, nM, False, MAX_EXACT, 16)
    same_prob_bits(got, want)
    report("hybrid_frontier_probs_dev method", cases, got[1].tolist())
    for j, c in enumerate(cases):
        rl.check_frame(c, got[0][j], int(got[1][j]), float(got[5][j]), int(got[3][j]), 0)


@pytest.mark.parametrize("k", [0, K])
def test_hybrid_sample_assoc(eng, k):
    """hybrid_frontier_sample_assoc (k = 0, also through hybrid_sample_assoc: the same bits) and hybrid_sample_assoc(k = 200)."""
    cases = FRONTIER + NONE_FRAMES
    frames, nL, nM = frames_of(cases)
    asg, lp, logPerm, method, nOpen, nFr, nEnum, _ = eng.hybrid_sample_assoc(frames, nL, nM, N_DRAW, k, seed=SEED, max_exact=MAX_EXACT)
    report(f"hybrid_sample_assoc(k = {k}) method", cases, method.tolist())
    if k == 0:
        a2, l2, p2, m2, _, f2, _ = eng.hybrid_frontier_sample_assoc(frames, nL, nM, N_DRAW, seed=SEED, max_exact=MAX_EXACT)
        for j in range(len(cases)):
            assert np.array_equal(asg[j], a2[j]) and np.array_equal(bits(lp[j]), bits(l2[j])) and method[j] == m2[j] and nFr[j] == f2[j]
            assert bits(logPerm[j:j + 1])[0] == bits(p2[j:j + 1])[0] or (np.isnan(logPerm[j]) and np.isnan(p2[j]))
    for j, c in enumerate(cases):
        assert nOpen[j] == 1, c.name
        rl.check_frame_draws(c, asg[j], lp[j], int(method[j]), float(logPerm[j]), int(nFr[j]), k)
        assert nEnum[j] == (1 if method[j] in (1, 2) else 0), c.name


def test_hybrid_frontier_sample_assoc_dev(eng):
    """The one-stream device entry of the draws: the host entry's bits, and the contract."""
    cases = FRONTIER + NONE_FRAMES
    frames, nL, nM = frames_of(cases)
    n = 1024
    want = draws_host(eng, frames, nL, nM, n, False, MAX_EXACT, 16)
    got = draws_dev(eng, frames, nL, nM, n, False, MAX_EXACT, 16)
    same_draw_bits(got, want)
    report("hybrid_frontier_sample_assoc_dev method", cases, got[3].tolist())
    for j, c in enumerate(cases):
        rl.check_frame_draws(c, got[0][j], got[1][j], int(got[3][j]), float(got[2][j]), int(got[5][j]), 0)


# ---- 3. the tiers of at most 16 measurements: safe by a bound ------------------------------------------------------------------------
def test_guard_for_the_tiers_of_at_most_16(eng):
    """hub(16, 41.9) and a two_hubs of 16 columns, each as a frame of its own: every non-zero entry is above e^-42, every product
    above e^-672.  permanent_probs, clustered_probs, sample_assoc and clustered_sample_assoc against the long-double truth."""
    cases = rl.guard_family()
    frames, nL, nM = [c.block for c in cases], [c.nLk for c in cases], [c.m for c in cases]
    want_lp = [rl.truth_of(c).logZ + c.m * float(np.min(c.block)) for c in cases]  # (the frame's units a = exp(mn - x))
    p, perm = eng.permanent_probs(frames, nL, nM)
    q, logPerm, info, _ = eng.clustered_probs(frames, nL, nM)[:4]
    a1, l1, perm1 = eng.sample_assoc(frames, nL, nM, N_DRAW, seed=SEED)
    a2, l2, logPerm2, info2, _ = eng.clustered_sample_assoc(frames, nL, nM, N_DRAW, seed=SEED)
    for j, c in enumerate(cases):
        t = rl.truth_of(c)
        assert t.logZprime < -550.0
        assert np.abs(p[j] - t.probs).max() <= rl.TOL and np.abs(q[j] - t.probs).max() <= rl.TOL, c.name
        assert info[j] == 1 and info2[j] == 1, c.name
        for lz in (float(np.log(perm[j])), float(logPerm[j]), float(np.log(perm1[j])), float(logPerm2[j])):
            rl.close(lz, want_lp[j], c.name)
        rl.check_draws(c, a1[j], l1[j], "sample_assoc")
        rl.check_draws(c, a2[j], l2[j], "clustered_sample_assoc")


# ---- 4. a deep cluster and its neighbours ------------------------------------------------------------------------------------------------
def test_deep_case_alone_first_and_last_in_a_batch(eng):
    """pair_chain(32, 25), declined, and pair_chain(32, 21), answered just inside the range, each alone, first and last among
    ordinary scene frames: the same bits for every frame everywhere -- a deep cluster does not disturb its neighbours, and the
    neighbours keep the bits they have without it."""
    scene = list(fsc.scene(*fsc.SMALL)[:6])
    sL, sM = [fsc.SMALL[1]] * 6, [fsc.SMALL[2]] * 6

    def run(frames, nL, nM):
        out, method, nOpen, nBig, maxc, lp, nFr = eng.hybrid_frontier_probs(frames, nL, nM, 0, condition=True, max_exact=MAX_EXACT)
        return out, method, nOpen, nFr, maxc, lp

    base = run(scene, sL, sM)
    assert (base[1] == 0).all() and base[2].max() >= 1
    for name in ("pair_chain(32, 25)", "pair_chain(32, 21)"):
        c = next(x for x in FRONTIER if x.name == name)
        alone = run([c.cost], [c.nL], [c.nM])
        assert alone[1][0] == (0 if rl.truth_of(c).logZprime >= rl.SAFE else -1), (name, alone[1])
        first = run([c.cost] + scene, [c.nL] + sL, [c.nM] + sM)
        last = run(scene + [c.cost], sL + [c.nL], sM + [c.nM])
        same_prob_bits(tuple(x[:1] for x in first), alone, what=name + " first")
        same_prob_bits(tuple(x[-1:] for x in last), alone, what=name + " last")
        same_prob_bits(tuple(x[1:] for x in first), base, what="the scene frames behind " + name)
        same_prob_bits(tuple(x[:-1] for x in last), base, what="the scene frames before " + name)
