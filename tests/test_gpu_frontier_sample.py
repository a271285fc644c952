"""GPU: joint associations drawn from the exact posterior of sparse clusters (kbest_frontier_sample.hip,
kbest_frontier_sample_f64_dev, kbest_hybrid_frontier_sample_assoc_batch_f64, the hybridFrontierSampleAssoc shim) against the numpy
restatement of tests/frontier_sample_check.py -- never against the kernel's own output.  The draws are compared for EXACT equality:
the two sides differ by the last bits of exp (about 1e-15 relative), so every case first asserts that the smallest relative margin
of its restatement, min |Tt - boundary| / tot over every decision, is at least 1e-10; then assign exactly and logProb / logTerm
within 1e-12.  log Z, info and width: the bits of the frontier tier's marginal entry."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import frontier_check as fc
import frontier_sample_check as fsc
import probabilisticsemslam_amd as pk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_MARGIN = 1e-10
BAD_ARG, NOT_RESERVED = -2, -6  # KBEST_ERR_BAD_ARG, KBEST_ERR_NOT_RESERVED
SIXTEEN = tuple(range(16))
PAD = 64
SMALL, MID, SEED = fsc.SMALL, fsc.MID, fsc.SEED


@pytest.fixture(scope="module")
def eng():
    e = pk.KBestEngine(0)
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def run_dev(eng, clusters, n, seed=SEED, base=0, stream=None, reserve=True, sync=True, keep=None):
    """kbest_frontier_sample_f64_dev on [(frame key, o)] (o: a dict of frontier_sample_check.open_clusters), sentinels between and
    around everything.  Returns one (assignLocal [n, m], logTerm [n], logZ, info, width) per cluster; untouched: -5 / -5.0 / -77."""
    dev = torch.device("cuda", 0)
    sub, keys, subOff, keyOff, asgOff, ltOff = [np.full(PAD, -7.0)], [np.full(PAD, -9, np.int32)], [], [], [], []
    at = kat = aat = lat = PAD
    for _, o in clusters:
        subOff.append(at)
        keyOff.append(kat)
        asgOff.append(aat)
        ltOff.append(lat)
        sub += [np.asarray(o["block"], dtype=np.float64), np.full(PAD, -7.0)]
        keys += [np.asarray(o["keys"], dtype=np.int32), np.full(PAD, -9, np.int32)]
        at += len(o["block"]) + PAD
        kat += len(o["keys"]) + PAD
        aat += n * o["m"] + PAD
        lat += n + PAD
    sub, keys, k = np.concatenate(sub), np.concatenate(keys), len(clusters)
    d_sub, d_keys = torch.from_numpy(sub).to(dev), torch.from_numpy(keys).to(dev)
    d_asg = torch.full((aat,), -5, dtype=torch.int32, device=dev)
    d_lt = torch.full((lat,), -5.0, dtype=torch.float64, device=dev)
    d_logZ = torch.full((k + 2,), -5.0, dtype=torch.float64, device=dev)
    d_int = torch.full((2, k + 2), -77, dtype=torch.int32, device=dev)
    if sync:  # (else the buffers were filled on the caller's stream, the launch's own)
        torch.cuda.synchronize()
    eng.frontier_sample_dev([o["m"] for _, o in clusters], [o["nL"] for _, o in clusters], subOff, d_sub, d_keys, keyOff, n, d_asg,
                            asgOff, d_lt, ltOff, d_logZ[1:], d_int[0, 1:], d_int[1, 1:], seed=seed, sample_base=base,
                            frame_key=[b for b, _ in clusters], stream=stream, reserve=reserve)
    if keep is not None:
        keep.append((d_sub, d_keys))  # (an asynchronous call: its inputs live until the caller synchronises)
    if not sync:
        return lambda: collect(clusters, n, d_asg, d_lt, d_logZ, d_int, asgOff, ltOff)
    torch.cuda.synchronize()
    assert np.array_equal(d_sub.cpu().numpy(), sub) and np.array_equal(d_keys.cpu().numpy(), keys)
    return collect(clusters, n, d_asg, d_lt, d_logZ, d_int, asgOff, ltOff)


def collect(clusters, n, d_asg, d_lt, d_logZ, d_int, asgOff, ltOff):
    ha, hl, hz, hi = d_asg.cpu().numpy(), d_lt.cpu().numpy(), d_logZ.cpu().numpy(), d_int.cpu().numpy()
    assert hz[0] == hz[-1] == -5.0 and hi[:, 0].tolist() == hi[:, -1].tolist() == [-77, -77]
    out, aend, lend = [], 0, 0
    for j, (_, o) in enumerate(clusters):
        assert (ha[aend:asgOff[j]] == -5).all() and (hl[lend:ltOff[j]] == -5.0).all(), j
        aend, lend = asgOff[j] + n * o["m"], ltOff[j] + n
        out.append((ha[asgOff[j]:aend].reshape(n, o["m"]).copy(), hl[ltOff[j]:lend].copy(), float(hz[1 + j]), int(hi[0, 1 + j]),
                    int(hi[1, 1 + j])))
    assert (ha[aend:] == -5).all() and (hl[lend:] == -5.0).all()
    return out


def marginal_tier(eng, clusters):
    """(logZ, info, width) of kbest_frontier_probs_f64_dev on the same clusters."""
    dev = torch.device("cuda", 0)
    subOff, probOff, at, pat = [], [], 0, 0
    for _, o in clusters:
        subOff.append(at)
        probOff.append(pat)
        at += len(o["block"])
        pat += o["m"] * (o["nL"] + 1)
    d_sub = torch.from_numpy(np.concatenate([np.asarray(o["block"], dtype=np.float64) for _, o in clusters])).to(dev)
    d_probs = torch.zeros(pat, dtype=torch.float64, device=dev)
    d_logZ = torch.full((len(clusters),), -5.0, dtype=torch.float64, device=dev)
    d_int = torch.full((2, len(clusters)), -77, dtype=torch.int32, device=dev)
    eng.frontier_probs_dev([o["m"] for _, o in clusters], [o["nL"] for _, o in clusters], subOff, probOff, d_sub, d_probs, d_logZ, d_int[0],
                           d_int[1])
    torch.cuda.synchronize()
    return d_logZ.cpu().numpy(), d_int[0].cpu().numpy(), d_int[1].cpu().numpy()


def restated(b, o, n, seed=SEED, base=0):
    return fsc.sample_cluster(o["block"], o["nL"], o["m"], o["keys"], n, seed, b, base)


def check_cluster(got, want, name, lo=0):
    a, lt, lz, info, W = got
    wa, wlt, wlz, winfo, wW, margin = want
    assert margin >= MIN_MARGIN, (name, margin)
    assert (info, W) == (winfo, wW), name
    assert np.array_equal(a, wa[lo: lo + len(a)]), name
    assert np.abs(lt - wlt[lo: lo + len(a)]).max() <= 1e-12, name
    assert abs(lz - wlz) <= 1e-12 * max(1.0, abs(wlz)), name
    return margin


def same_bits(x, y):
    return np.array_equal(x[0], y[0]) and np.array_equal(bits(x[1]), bits(y[1])) and bits(x[2]) == bits(y[2]) and x[3:] == y[3:]


# ---- 1. the per-cluster entry ----------------------------------------------------------------------------------------------------------
def test_open_clusters_of_the_sixteen_frames(eng):
    """The 25 open clusters of frames 0 .. 15 at max_exact = 4 (5 .. 15 columns, W <= 9), 512 draws, in one call."""
    oc = list(fsc.open_clusters(SMALL, SIXTEEN))
    got = run_dev(eng, oc, 512)
    margins = [check_cluster(g, restated(b, o, 512), (b, o["m"])) for g, (b, o) in zip(got, oc)]
    lz, info, width = marginal_tier(eng, oc)
    print(f"{len(oc)} clusters of {sorted(o['m'] for _, o in oc)} columns: smallest margin {min(margins):.3g}")
    assert np.array_equal(bits([g[2] for g in got]), bits(lz))
    assert [g[3] for g in got] == info.tolist() == [1] * len(oc) and [g[4] for g in got] == width.tolist()


def test_same_bits_alone_first_last_and_under_a_cap(eng):
    oc = list(fsc.open_clusters(SMALL, SIXTEEN))
    j = next(i for i, (_, o) in enumerate(oc) if o["m"] == 12)
    one = oc[j]
    (alone,) = run_dev(eng, [one], 512)
    first = run_dev(eng, [one] + oc[:j] + oc[j + 1:], 512)[0]
    last = run_dev(eng, ([one] + oc[:j] + oc[j + 1:])[::-1], 512)[-1]
    many = run_dev(eng, (oc * 3)[:70], 64)  # more clusters than one launch takes
    few = run_dev(eng, oc, 64)
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    mine = run_dev(eng, oc, 64, stream=s.cuda_stream)  # (a stream of the caller's)
    try:
        eng.set_frontier_work_cap(fc.SLOT)  # one slot: one cluster at a time
        capped = run_dev(eng, [one] + oc[:j] + oc[j + 1:], 512, reserve=False)[0]
    finally:
        eng.set_frontier_work_cap(0)
    check_cluster(alone, restated(*one, 512), "alone")
    for other in (first, last, capped):
        assert same_bits(alone, other)
    for i in range(70):
        assert same_bits(many[i], few[i % len(oc)]), i
    for a, b in zip(few, mine):
        assert same_bits(a, b)


def test_most_layers_and_largest_width(eng):
    """scene_frames(200, 60, 40, 30.0), conditioned: the cluster of 25 measurements of frame 89 (58 rows: the most layers) and the
    one of 18 of frame 38 (W = 10, the largest of the cases), 64 draws."""
    _, nL, nM, _ = MID
    cases = []
    for b, size in ((89, 25), (38, 18)):
        (o,) = [o for o in fsc.hc_opens(fsc.scene(*MID)[b], nL, nM, True, 16)]
        assert o["m"] == size
        o["keys"] = fsc.open_row_keys(o, nL).astype(np.int32)
        cases.append((b, o))
    got = run_dev(eng, cases, 64)
    want = [restated(b, o, 64) for b, o in cases]
    assert [w[4] for w in want] == [9, 10]
    for g, w, (b, o) in zip(got, want, cases):
        print(f"frame {b}: {o['m']} columns, {o['R']} rows, W {w[4]}, margin {w[5]:.3g}")
        check_cluster(g, w, b)
    lz, info, width = marginal_tier(eng, cases)
    assert np.array_equal(bits([g[2] for g in got]), bits(lz)) and [g[4] for g in got] == width.tolist()


def test_draw_counts_and_continuation(eng):
    """nSample 1, 63 and 5 000 (more than one round of the walk; a round's last thread without a draw), and sampleBase 4 096
    continuing the first 4 096."""
    b, o = next((b, o) for b, o in fsc.open_clusters(SMALL, SIXTEEN) if o["m"] == 9)
    want = restated(b, o, 5000)
    for n in (1, 63, 5000):
        (g,) = run_dev(eng, [(b, o)], n)
        check_cluster(g, want, n)
    (g,) = run_dev(eng, [(b, o)], 904, base=4096)
    check_cluster(g, want, "continued", lo=4096)


# ---- 2. the frame entry ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_exact", [4, 8])
def test_frame_entry_on_the_sixteen_frames(eng, max_exact):
    _, nL, nM, _ = SMALL
    frames = [fsc.scene(*SMALL)[b] for b in SIXTEEN]
    n = 256
    asg, lp, logPerm, method, nOpen, nFr, maxc = eng.hybrid_frontier_sample_assoc(frames, [nL] * 16, [nM] * 16, n, seed=SEED, condition=True,
                                                                                  max_exact=max_exact)
    _, pm, pOpen, _, pmaxc, plp, pFr = eng.hybrid_frontier_probs(frames, [nL] * 16, [nM] * 16, 0, condition=True, max_exact=max_exact,
                                                                 max_big=0)
    assert np.array_equal(method, pm) and np.array_equal(nOpen, pOpen) and np.array_equal(nFr, pFr) and np.array_equal(maxc, pmaxc)
    assert np.array_equal(bits(logPerm), bits(plp))
    margins = []
    for b in SIXTEEN:
        want = fsc.frame_draws(SMALL, b, n, max_exact)
        margins.append(want.margin)
        assert want.margin >= MIN_MARGIN, (b, want.margin)
        assert (method[b], nOpen[b], nFr[b], maxc[b]) == (want.method, want.nopen, want.nfrontier, want.maxc) and want.method == 0
        assert np.array_equal(asg[b][:, want.small_cols], want.assign[:, want.small_cols]), b  # the clustered sampler's columns
        assert np.array_equal(asg[b], want.assign), b
        assert np.abs(lp[b] - want.logp).max() <= 1e-12, b
        assert abs(logPerm[b] - want.logperm) <= 1e-12 * max(1.0, abs(want.logperm))
    print(f"max_exact {max_exact}: open clusters {nOpen.tolist()}, smallest margin {min(margins):.3g}")
    assert nOpen.sum() >= 6


def test_nothing_open_is_the_clustered_sampler(eng):
    from probabilisticsemslam_amd import workloads as wl
    F, nL, nM = 6, 20, 10
    frames = wl.scene_frames(F, nL, nM, 12.0)
    for condition in (False, True):
        a = eng.hybrid_frontier_sample_assoc(frames, [nL] * F, [nM] * F, 300, seed=SEED, condition=condition, max_exact=16)
        b = eng.clustered_sample_assoc(frames, [nL] * F, [nM] * F, 300, seed=SEED, condition=condition)
        assert not a[4].any() and not a[5].any() and (a[3] == 0).all() and (b[3] > 0).all()
        assert np.array_equal(a[6], b[4]) and np.array_equal(bits(a[2]), bits(b[2]))
        for f in range(F):
            assert np.array_equal(a[0][f], b[0][f]) and np.array_equal(bits(a[1][f]), bits(b[1][f])), f


def test_a_frame_alone_and_in_a_batch_of_forty(eng):
    _, nL, nM, _ = SMALL
    frames = [fsc.scene(*SMALL)[b] for b in range(40)]
    order = np.random.default_rng(3).permutation(40)
    batch = eng.hybrid_frontier_sample_assoc([frames[b] for b in order], [nL] * 40, [nM] * 40, 100, seed=SEED, condition=True, max_exact=4,
                                             frame_key=[int(b) for b in order])
    for b in (10, 12, 33):
        alone = eng.hybrid_frontier_sample_assoc([frames[b]], [nL], [nM], 100, seed=SEED, condition=True, max_exact=4, frame_key=[b])
        j = int(np.flatnonzero(order == b)[0])
        assert alone[3][0] == 0 and alone[4][0] >= 1
        assert np.array_equal(alone[0][0], batch[0][j]) and np.array_equal(bits(alone[1][0]), bits(batch[1][j]))
        assert bits(alone[2])[0] == bits(batch[2])[j] and [int(x[0]) for x in alone[3:]] == [int(x[j]) for x in batch[3:]]
    want = fsc.frame_draws(SMALL, 10, 100)
    j = int(np.flatnonzero(order == 10)[0])
    assert want.margin >= MIN_MARGIN and np.array_equal(batch[0][j], want.assign)


# ---- 3. refusals and edges ---------------------------------------------------------------------------------------------------------------
def test_refusals(eng):
    _, nL, nM, _ = SMALL
    frames = [fsc.scene(*SMALL)[b] for b in SIXTEEN]
    args = ([nL] * 16, [nM] * 16, 8)
    asg, lp, logPerm, method, nOpen, nFr, _ = eng.hybrid_frontier_sample_assoc(frames, *args, seed=SEED, condition=True, max_exact=4,
                                                                               max_width=5)
    assert np.flatnonzero(method == -1).tolist() == [8, 10, 12, 15] and (np.delete(method, [8, 10, 12, 15]) == 0).all()
    for b in (8, 10, 12, 15):
        assert (asg[b] == -1).all() and np.isnan(lp[b]).all() and np.isnan(logPerm[b]) and nFr[b] == 0
    want = fsc.frame_draws(SMALL, 9, 8, max_width=5)
    assert want.margin >= MIN_MARGIN and np.array_equal(asg[9], want.assign)
    # a slot 8 bytes below the layers of the largest cluster: -3 for that cluster, -1 for its frame, and no other
    oc = list(fsc.open_clusters(SMALL, SIXTEEN))
    need = [fc.layers_bytes(fc.row_masks(fc.scaled_block(o["block"], o["nL"], o["m"])[0]), o["m"]) for _, o in oc]
    big = int(np.argmax(need))
    assert sorted(need)[-1] > sorted(need)[-2]
    try:
        eng.set_frontier_slot(need[big] - 8)
        low = run_dev(eng, oc, 8)
        out = eng.hybrid_frontier_sample_assoc(frames, *args, seed=SEED, condition=True, max_exact=4)
        eng.set_frontier_slot(need[big])
        fits = run_dev(eng, oc, 8)
    finally:
        eng.set_frontier_slot(0)
    assert [g[3] for g in low] == [fc.REFUSED_SLOT if j == big else 1 for j in range(len(oc))]
    assert (low[big][0] == -5).all() and (low[big][1] == -5.0).all() and low[big][2] == -5.0 and low[big][4] == fits[big][4]
    assert fits[big][3] == 1 and np.array_equal(fits[big][0], restated(*oc[big], 8)[0])
    assert np.flatnonzero(out[3] == -1).tolist() == [oc[big][0]] and (np.delete(out[3], oc[big][0]) == 0).all()


def test_an_infeasible_cluster_between_two_answered(eng):
    oc = list(fsc.open_clusters(SMALL, SIXTEEN))
    blk, l, m = fc.edge_clusters()["same_only_row"]
    dead = dict(block=blk, nL=l, m=m, keys=np.arange(l + m, dtype=np.int32))
    got = run_dev(eng, [oc[0], (5, dead), oc[1]], 16)
    assert [g[3] for g in got] == [1, 0, 1] and (got[1][0] == -1).all() and np.isnan(got[1][1]).all() and got[1][2] == -np.inf
    check_cluster(got[0], restated(*oc[0], 16), 0)
    check_cluster(got[2], restated(*oc[1], 16), 2)
    # the frame entry: both columns of the middle frame can only take landmark row 0
    _, nL, nM, _ = SMALL
    inf = np.inf
    bad = fc.flat([[1.0, 2.0], [inf, inf], [inf, inf], [inf, inf]])
    good = [fsc.scene(*SMALL)[0], fsc.scene(*SMALL)[1]]
    asg, lp, logPerm, method, nOpen, nFr, _ = eng.hybrid_frontier_sample_assoc([good[0], bad, good[1]], [nL, 2, nL], [nM, 2, nM], 16, seed=SEED,
                                                                               max_exact=1, frame_key=[0, 7, 1])
    assert method.tolist() == [0, -2, 0] and (asg[1] == -1).all() and np.isnan(lp[1]).all() and logPerm[1] == -inf and nFr[1] == 0
    for j, b in ((0, 0), (2, 1)):
        want = fsc.frame_draws(SMALL, b, 16, 1, False)
        assert want.margin >= MIN_MARGIN and np.array_equal(asg[j], want.assign) and np.abs(lp[j] - want.logp).max() <= 1e-12


def test_bad_arguments_and_not_reserved(eng):
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    nLa, off = np.array([6], np.int32), np.zeros(1, np.int64)
    dummy = C.c_void_p(8)
    for m, n_sample, base in ((65, 4, 0), (0, 4, 0), (3, 0, 0), (3, 2, 2 ** 32 - 1)):
        one = np.array([m], np.int32)
        rc = eng.lib.kbest_frontier_sample_f64_dev(eng.ctx, 1, vp(one), vp(nLa), vp(off), dummy, dummy, vp(off), None, n_sample, 0, base,
                                                   dummy, vp(off), dummy, vp(off), None, None, None, None)
        assert rc == BAD_ARG, (m, n_sample, base)
    assert eng.lib.kbest_reserve_frontier_sample(eng.ctx, 1, 65, 70) == BAD_ARG
    fresh = pk.KBestEngine(0)
    try:  # the asynchronous entry allocates nothing
        one = np.array([3], np.int32)
        rc = fresh.lib.kbest_frontier_sample_f64_dev(fresh.ctx, 1, vp(one), vp(nLa), vp(off), dummy, dummy, vp(off), None, 4, 0, 0, dummy,
                                                     vp(off), dummy, vp(off), None, None, None, None)
        assert rc == NOT_RESERVED
    finally:
        fresh.close()
    good = fsc.scene(*SMALL)[0]
    _, nL, nM, _ = SMALL
    for kw in (dict(max_exact=17), dict(max_width=17), dict(max_width=-1), dict(sample_base=2 ** 32 - 1)):
        with pytest.raises(pk.KBestError):
            eng.hybrid_frontier_sample_assoc([good], [nL], [nM], 2, **kw)
    out = eng.hybrid_frontier_sample_assoc([], [], [], 4)
    assert out[0] == [] and out[3].size == 0


def test_two_launches_on_a_callers_stream(eng):
    """Without a synchronise between them: the second continues the first; one work space, stream order alone."""
    oc = list(fsc.open_clusters(SMALL, SIXTEEN))[:6]
    eng.reserve_frontier_sample(len(oc), max(o["m"] for _, o in oc), max(o["m"] + o["nL"] for _, o in oc))
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    keep = []
    with torch.cuda.stream(s):
        first = run_dev(eng, oc, 200, stream=s.cuda_stream, reserve=False, sync=False, keep=keep)
        second = run_dev(eng, oc, 56, base=200, stream=s.cuda_stream, reserve=False, sync=False, keep=keep)
    torch.cuda.synchronize()
    for g1, g2, (b, o) in zip(first(), second(), oc):
        want = restated(b, o, 256)
        check_cluster(g1, want, b)
        check_cluster(g2, want, b, lo=200)


def test_cpp_shim_and_module_function(eng, tmp_path):
    exe = str(tmp_path / "shim_frontier_sample")
    libdir = os.path.join(ROOT, "probabilisticsemslam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_frontier_sample.cpp"), "-o", exe,
                           "-L", libdir, "-l:libkbest_amd.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
                           "-L/opt/rocm/lib", "-lamdhip64"])
    _, nL, nM, _ = MID
    frame = fsc.scene(*MID)[89]  # raw: a cluster of twenty-five measurements, refused by clusterSampleAssoc
    path = tmp_path / "scene.txt"
    path.write_text(f"{nL} {nM}\n" + "\n".join("inf" if np.isinf(v) else float.hex(float(v)) for v in frame) + "\n")
    lines = subprocess.check_output([exe, str(path), "32", str(SEED)], text=True).splitlines()
    want = fsc.hybrid_frontier_sample_assoc(frame, nL, nM, 32, SEED, False, 0)
    assert want.method == 0 and want.maxc == 25 and want.nfrontier == 1 and want.margin >= MIN_MARGIN
    assert len(lines) == 33
    for s in range(32):
        tok = lines[s].split()
        assert tok[:2] == ["s", str(s)] and [int(v) for v in tok[2:]] == want.assign[s].tolist(), s
    assert lines[-1].startswith("empty column: runtime_error hybridFrontierSampleAssoc") and "no consistent association" in lines[-1]
    assert np.array_equal(pk.hybridFrontierSampleAssoc(frame, nL, nM, 32, SEED), want.assign)
    with pytest.raises(RuntimeError, match="refused"):
        pk.clusterSampleAssoc(frame, nL, nM, 1)
