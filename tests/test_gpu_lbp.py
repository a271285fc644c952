"""GPU: the belief-propagation association probabilities (kbest_lbp.hip, kbest_belief_probs_batch_f64[_dev], the beliefProb
shim) against the numpy restatement of tests/lbp_check.py and the exact marginals -- never against the kernel's own output.

1e-12 absolute is the project's standing tolerance for probabilities; the iteration's rounding does not accumulate (fp64 against
long double at a fixed sweep count: 3e-16), so nothing looser is needed at a fixed sweep count."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import lbp_check as lc
import oracle_lib as ol
import permanent_check as pc
import probabilisticsemslam_amd as pk
from probabilisticsemslam_amd import workloads as wl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME_SETS = ((40, 6, 3), (20, 5, 4), (6, 6, 5))  # the enumerable sets of test_gpu_permanent.py
BIG_SHAPES = ((3, 60, 24), (2, 200, 48), (2, 400, 64), (1, 896, 128))  # (frames, nL, nM): 24 .. 128 measurements, up to 1 024 rows
DENSE_SHAPES = ((12, 5), (40, 16), (64, 24), (150, 48), (1024, 128))  # (rows, measurements) of the dense u01 * 10 blocks


@pytest.fixture(scope="module")
def eng():
    e = pk.KBestEngine(0)
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def enumerable_sets():
    """Conditioned frames of the enumerable sets: (block, nL, nM)."""
    out = []
    for F, nL, nM in FRAME_SETS:
        for f in wl.kitti_like_frames(F, nL=nL, nM=nM):
            cond, idx = ol.condition_costs(f, nL + nM, nM)
            out.append((cond, len(idx) - nM, nM))
    return out


@functools.lru_cache(maxsize=None)
def big_frames():
    """Raw KITTI-like frames of 24 .. 128 measurements: (block, nL, nM)."""
    out = []
    for F, nL, nM in BIG_SHAPES:
        out += [(f, nL, nM) for f in wl.kitti_like_frames(F, nL=nL, nM=nM, seed=0xB16 + nM)]
    return out


@functools.lru_cache(maxsize=None)
def dense_frames():
    return [(wl.dense_batch(1, nR, nM, 0x5EED0000 + 131 * nR + nM)[0] * 10.0, nR - nM, nM) for nR, nM in DENSE_SHAPES]


@functools.lru_cache(maxsize=None)
def c5_frames(F):
    return wl.kitti_like_frames(F, nL=20, nM=10)


def conditioned_want(raw, nL, nM, tol, max_iter):
    """The restatement on a raw block: conditionCosts on the host, the iteration, scatter back."""
    cond, idx = ol.condition_costs(raw, nL + nM, nM)
    cp, iters, resid = lc.belief_probs(cond, len(idx) - nM, nM, tol, max_iter)
    return pc.scatter_back(cp, idx, nL, nM), iters, resid, cond, idx


def run(eng, frames, **kw):
    return eng.belief_probs([f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames], **kw)


def device_run(eng, frames, tol, max_iter, condition=False, maxRawRow=None, maxCol=None, reserve=True, fill=-1.0):
    """The device entry on a stream of the caller's.  Returns (list of probs, iters, resid)."""
    import torch
    nLs, nMs = [f[1] for f in frames], [f[2] for f in frames]
    sizes = np.array([(l + m) * m for l, m in zip(nLs, nMs)], np.int64)
    psizes = np.array([m * (l + 1) for l, m in zip(nLs, nMs)], np.int64)
    coff = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    poff = np.concatenate([[0], np.cumsum(psizes)[:-1]]).astype(np.int64)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_cost, d_coff, d_poff = t(np.concatenate([f[0] for f in frames])), t(coff), t(poff)
    d_nL, d_nM = t(np.asarray(nLs, np.int32)), t(np.asarray(nMs, np.int32))
    d_probs = torch.full((int(psizes.sum()),), fill, dtype=torch.float64, device=dev)
    d_iters = torch.full((len(frames),), -77, dtype=torch.int32, device=dev)
    d_resid = torch.full((len(frames),), -1.0, dtype=torch.float64, device=dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    eng.belief_probs_dev(len(frames), maxRawRow or max(l + m for l, m in zip(nLs, nMs)), maxCol or max(nMs), d_nL, d_nM, d_cost,
                         d_coff, d_probs, d_poff, d_iters, d_resid, condition=condition, tol=tol, max_iter=max_iter,
                         stream=s.cuda_stream, reserve=reserve)
    s.synchronize()
    hp = d_probs.cpu().numpy()
    out = [hp[poff[b]: poff[b] + psizes[b]].reshape(nMs[b], nLs[b] + 1) for b in range(len(frames))]
    return out, d_iters.cpu().numpy(), d_resid.cpu().numpy()


# ---- 1. parity at a fixed sweep count -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iter", [1, 2, 25, 300])
def test_parity_at_fixed_sweep_count(eng, max_iter):
    worst = {}

    def compare(name, got, iters, resid, want):
        w = 0.0
        for b, (p, (q, wi, wr)) in enumerate(zip(got, want)):
            assert not np.isnan(p).any(), (name, b)
            w = max(w, np.abs(p - q).max())
            assert iters[b] == wi == max_iter, (name, b, iters[b], wi)
            assert abs(resid[b] - wr) <= 1e-12, (name, b, resid[b], wr)
            assert np.abs(p.sum(axis=1) - 1.0).max() <= 1e-12, (name, b)  # every column of a feasible frame sums to 1
        worst[name] = w

    fr = enumerable_sets()
    got, iters, resid = run(eng, fr, tol=0.0, max_iter=max_iter)
    compare("enumerable", got, iters, resid, [lc.belief_probs(c, l, m, 0.0, max_iter) for c, l, m in fr])

    raw = c5_frames(1000)
    got, iters, resid = eng.belief_probs(raw, [20] * 1000, [10] * 1000, condition=True, tol=0.0, max_iter=max_iter)
    compare("1000 x 30x10 conditioned", got, iters, resid, [conditioned_want(f, 20, 10, 0.0, max_iter)[:3] for f in raw])

    fr = big_frames()
    got, iters, resid = run(eng, fr, condition=True, tol=0.0, max_iter=max_iter)
    compare("24 .. 128 measurements", got, iters, resid, [conditioned_want(f, l, m, 0.0, max_iter)[:3] for f, l, m in fr])

    fr = dense_frames()
    got, iters, resid = run(eng, fr, tol=0.0, max_iter=max_iter)
    compare("dense", got, iters, resid, [lc.belief_probs(c, l, m, 0.0, max_iter) for c, l, m in fr])

    print(f"max_iter = {max_iter}: engine vs restatement " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1e-12, (k, v)


# ---- 2. converged runs ---------------------------------------------------------------------------------------------------------
def test_converged_runs(eng):
    tol = 1e-12
    rng = np.random.default_rng(5)
    groups = (("C5", [(f, 20, 10) for f in c5_frames(200)], True),
              ("crowded 8+8", [(lc.crowded_frame(rng), 8, 8) for _ in range(10)], False),
              ("24 .. 128 measurements", big_frames(), True),
              ("dense", dense_frames()[:4], False))
    for name, fr, condition in groups:
        got, iters, resid = run(eng, fr, condition=condition, tol=tol, max_iter=10000)
        worst, dit, its = 0.0, 0, []
        for b, (f, l, m) in enumerate(fr):
            want, wi, wr = conditioned_want(f, l, m, tol, 10000)[:3] if condition else lc.belief_probs(f, l, m, tol, 10000)
            assert 0 < wi < 10000, (name, b, wi)
            worst = max(worst, np.abs(got[b] - want).max())
            dit = max(dit, abs(int(iters[b]) - wi))
            its.append(int(iters[b]))
            assert resid[b] <= tol, (name, b, resid[b])
        print(f"{name}: converged engine vs the restatement's fixed point {worst:.3g}; sweeps {min(its)} .. {max(its)}, "
              f"off the restatement's count by at most {dit}")
        assert dit <= 1, name
        assert worst <= 1e-9, name


# ---- 3. condition = True on raw blocks -----------------------------------------------------------------------------------------
def test_condition_on_raw_blocks_bitwise(eng):
    fr = [(f, 20, 10) for f in c5_frames(64)] + big_frames()
    n_dropped = 0
    for tol, max_iter in ((0.0, 7), (1e-12, 10000)):
        got, iters, resid = run(eng, fr, condition=True, tol=tol, max_iter=max_iter)
        host = [ol.condition_costs(f, l + m, m) for f, l, m in fr]
        cgot, citers, cresid = run(eng, [(c, len(idx) - m, m) for (c, idx), (_, _, m) in zip(host, fr)], tol=tol, max_iter=max_iter)
        for b, (f, l, m) in enumerate(fr):
            cond, idx = host[b]
            want = pc.scatter_back(cgot[b], idx, l, m)
            assert np.array_equal(bits(got[b]), bits(want)), b
            assert iters[b] == citers[b] and bits(resid[b]) == bits(cresid[b]), b
            dropped = np.setdiff1d(np.arange(l), np.asarray(idx, dtype=np.int64))
            n_dropped += len(dropped)
            assert (got[b][:, dropped] == 0.0).all(), b  # exactly 0.0
    assert n_dropped > 0


# ---- 4. accuracy: the reason for the feature ---------------------------------------------------------------------------------------
def test_accuracy_on_c5_frames(eng):
    F, nL, nM = 200, 20, 10
    frames = c5_frames(F)
    truth = json.load(open(os.path.join(ROOT, "profiles", "exact_truth_c5.json")))
    k200 = truth["shapes"]["30x10"]["k"]["200"]["median"]
    exact, _ = eng.permanent_probs(frames, [nL] * F, [nM] * F, condition=True)
    got, iters, resid = eng.belief_probs(frames, [nL] * F, [nM] * F, condition=True)
    err = np.array([np.abs(got[b] - exact[b]).max() for b in range(F)])
    werr = []
    for f in frames:
        cond, idx = ol.condition_costs(f, nL + nM, nM)
        cL = len(idx) - nM
        werr.append(np.abs(lc.belief_probs(cond, cL, nM)[0] - lc.exact_probs(cond, cL, nM)).max())
    werr = np.array(werr)
    stats = lambda e: np.array([np.median(e), np.quantile(e, 0.95), e.max()])  # noqa: E731
    print(f"engine vs exact engine: median {stats(err)[0]:.4g} p95 {stats(err)[1]:.3g} max {stats(err)[2]:.3g} frames > 0.1: "
          f"{(err > 0.1).sum()}; restatement vs subset sums: median {stats(werr)[0]:.4g} p95 {stats(werr)[1]:.3g} max "
          f"{stats(werr)[2]:.3g} frames > 0.1: {(werr > 0.1).sum()}; k = 200 median {k200:.3g}")
    np.testing.assert_allclose(stats(err), stats(werr), rtol=0, atol=1e-9)
    np.testing.assert_allclose(err, werr, rtol=0, atol=1e-9)
    assert (err > 0.1).sum() == (werr > 0.1).sum()
    assert np.median(err) < k200


# ---- 5. exact cases ------------------------------------------------------------------------------------------------------------
def test_exact_cases(eng):
    rng = np.random.default_rng(12)
    fr = []
    for nL in (0, 1, 4, 40):
        fr.append((rng.random(nL + 1) * 50.0, nL, 1))
    for nL, nM in ((6, 3), (12, 5), (20, 10), (30, 12), (40, 16)):
        for _ in range(6):
            nR = nL + nM
            cost = np.full(nR * nM, np.inf)
            for r in range(nL):
                cost[int(rng.integers(0, nM)) * nR + r] = rng.random() * 12.0
            for c in range(nM):
                cost[c * nR + nL + c] = 10.0
            fr.append((cost, nL, nM))
    got, iters, resid = run(eng, fr)
    exact, _ = eng.permanent_probs([f[0] for f in fr], [f[1] for f in fr], [f[2] for f in fr])
    worst = 0.0
    for b, (cost, nL, nM) in enumerate(fr):
        assert iters[b] == 1 and resid[b] == 0.0, b
        worst = max(worst, np.abs(got[b] - exact[b]).max())
        assert np.abs(got[b].sum(axis=1) - 1.0).max() <= 1e-12
    col = fr[2][0]
    w = np.where(col.min() + 42.0 > col, np.exp(col.min() - col), 0.0)
    np.testing.assert_allclose(got[2][0], w / w.sum(), rtol=0, atol=1e-12)
    print(f"single-column and conflict-free frames vs the exact engine {worst:.3g}")
    assert worst <= 1e-12


# ---- 6. invariance, bitwise ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tol,max_iter", [(0.0, 40), (1e-12, 10000)])
def test_invariance_bitwise(eng, tol, max_iter):
    rng = np.random.default_rng(2024)
    others = []
    for i in range(96):
        nM = 1 + (i * 7) % 40
        nL = int(rng.integers(0, 200))
        others.append((rng.random((nL + nM) * nM) * 10.0, nL, nM))
    others.append(dense_frames()[4])  # 1 024 rows: every launch it travels in has 16 waves per workgroup
    xs = []
    f = wl.kitti_like_frames(3, nL=20, nM=10, seed=4242)[2]
    cond, idx = ol.condition_costs(f, 30, 10)
    xs.append((cond, len(idx) - 10, 10))  # one wave
    f = big_frames()[3][0]
    cond, idx = ol.condition_costs(f, 248, 48)
    assert len(idx) > 64
    xs.append((cond, len(idx) - 48, 48))  # several chunks
    xs.append(dense_frames()[3])  # 150 x 48 dense
    for x in xs:
        (alone,), it0, rs0 = run(eng, [x], tol=tol, max_iter=max_iter)
        want, wi, _ = lc.belief_probs(*x, tol, max_iter)
        assert np.abs(alone - want).max() <= (1e-12 if tol == 0.0 else 1e-9) and abs(int(it0[0]) - wi) <= 1
        first = run(eng, [x] + others, tol=tol, max_iter=max_iter)
        last = run(eng, others + [x], tol=tol, max_iter=max_iter)
        mid = device_run(eng, others[:50] + [x] + others[50:], tol, max_iter)
        dalone = device_run(eng, [x], tol, max_iter)
        eng.set_belief_lds_limit(1024)  # nothing of a frame fits: a and nu in the work space
        try:
            hbm = run(eng, [x], tol=tol, max_iter=max_iter)
            hbm_mixed = run(eng, others[:20] + [x], tol=tol, max_iter=max_iter)
            hbm_dev = device_run(eng, [x] + others[:5], tol, max_iter)
        finally:
            eng.set_belief_lds_limit(0)
        for name, (p, it, rs), at in (("first", first, 0), ("last", last, -1), ("device, middle", mid, 50), ("device, alone", dalone, 0),
                                      ("work space", hbm, 0), ("work space, mixed", hbm_mixed, -1), ("work space, device", hbm_dev, 0)):
            assert np.array_equal(bits(alone), bits(p[at])), (name, x[1], x[2])
            assert it[at] == it0[0] and bits(rs[at]) == bits(rs0[0]), (name, x[1], x[2])
    # the neighbours in the mixed batch are right as well
    p, it, _ = run(eng, others, tol=0.0, max_iter=25)
    for b in (0, 17, 60, 95, 96):
        want, _, _ = lc.belief_probs(*others[b], 0.0, 25)
        np.testing.assert_allclose(p[b], want, rtol=0, atol=1e-12, err_msg=str(b))


# ---- 7. edges ------------------------------------------------------------------------------------------------------------------------
def test_infeasible_frames_give_zeros(eng):
    cost = wl.dense_batch(1, 9, 3, 5)[0] * 10.0
    cost[9:18] = np.inf  # a column without a finite entry
    good = wl.dense_batch(1, 9, 3, 6)[0] * 10.0
    forced = np.full(8, np.inf)  # 4 x 2: both columns can only take row 0
    forced[0] = forced[4] = 1.0
    nothing = np.full(12, np.inf)
    for condition in (False, True):
        out, iters, resid = eng.belief_probs([good, cost, forced, nothing, good], [6, 6, 2, 1, 6], [3, 3, 2, 3, 3], condition=condition)
        for b in (1, 2, 3):
            assert iters[b] == -2 and not out[b].any() and not np.isnan(out[b]).any(), (condition, b)
        assert not np.isnan(resid).any()
        assert iters[0] > 0 and np.array_equal(bits(out[0]), bits(out[4]))
        want, wi, _ = lc.belief_probs(good, 6, 3)
        np.testing.assert_allclose(out[0], want, rtol=0, atol=1e-9)


def test_frame_beyond_the_launch_bounds(eng):
    a = (wl.dense_batch(1, 9, 3, 21)[0] * 10.0, 6, 3)
    wide = (wl.dense_batch(1, 9, 5, 22)[0] * 10.0, 4, 5)
    tall = (wl.dense_batch(1, 12, 3, 23)[0] * 10.0, 9, 3)
    out, iters, resid = device_run(eng, [a, wide, tall, a], 1e-12, 10000, maxRawRow=9, maxCol=3, fill=-5.0)
    assert iters[1] == -1 and iters[2] == -1 and iters[0] > 0 and iters[3] == iters[0]
    assert (out[1] == -5.0).all() and (out[2] == -5.0).all()  # untouched
    want, _, _ = lc.belief_probs(*a)
    np.testing.assert_allclose(out[0], want, rtol=0, atol=1e-9)
    assert np.array_equal(bits(out[0]), bits(out[3]))


def test_limits_and_reserve(eng):
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    cost = wl.dense_batch(1, 140, 129, 129)[0] * 10.0
    nL, nM, off = np.array([11], np.int32), np.array([129], np.int32), np.zeros(1, np.int64)
    probs, iters, resid = np.zeros(129 * 12), np.zeros(1, np.int32), np.zeros(1)
    rc = eng.lib.kbest_belief_probs_batch_f64(eng.ctx, 1, vp(nL), vp(nM), vp(cost), vp(off), 0, C.c_double(1e-12), 100, vp(probs),
                                              vp(off), vp(iters), vp(resid))
    assert rc == -3  # KBEST_ERR_UNSUPPORTED
    assert b"128" in eng.lib.kbest_last_error(eng.ctx)
    with pytest.raises(pk.KBestError):
        eng.belief_probs([cost], [11], [129])
    with pytest.raises(pk.KBestError):  # 1 025 rows
        eng.belief_probs([np.zeros(1025 * 2)], [1023], [2])
    # 128 measurements are in; the outputs may be left out
    nL[0], nM[0] = 12, 128
    cost = wl.dense_batch(1, 140, 128, 128)[0] * 10.0
    probs = np.zeros(128 * 13)
    rc = eng.lib.kbest_belief_probs_batch_f64(eng.ctx, 1, vp(nL), vp(nM), vp(cost), vp(off), 0, C.c_double(0.0), 5, vp(probs),
                                              vp(off), None, None)
    assert rc == 0
    want, _, _ = lc.belief_probs(cost, 12, 128, 0.0, 5)
    np.testing.assert_allclose(probs.reshape(128, 13), want, rtol=0, atol=1e-12)
    # the device entry never allocates: a frame that needs the work space on a context that has none
    fresh = pk.KBestEngine(0)
    try:
        big = dense_frames()[4]
        with pytest.raises(pk.KBestError, match="kbest_reserve_belief"):
            device_run(fresh, [big], 0.0, 3, reserve=False)
        assert b"kbest_reserve_belief" in fresh.lib.kbest_last_error(fresh.ctx)
        out, it, _ = device_run(fresh, [big], 0.0, 3, reserve=True)  # the context still answers
        want, _, _ = lc.belief_probs(*big, 0.0, 3)
        np.testing.assert_allclose(out[0], want, rtol=0, atol=1e-12)
    finally:
        fresh.close()


# ---- 8. the shim -----------------------------------------------------------------------------------------------------------------
def test_cpp_shim_belief(eng, tmp_path):
    exe = str(tmp_path / "shim_belief")
    libdir = os.path.join(ROOT, "probabilisticsemslam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_belief.cpp"), "-o", exe,
                           "-L", libdir, "-l:libkbest_amd.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
                           "-L/opt/rocm/lib", "-lamdhip64"])
    f = wl.kitti_like_frames(1, nL=60, nM=24, seed=0xB16 + 24)[0]
    cond, idx = ol.condition_costs(f, 84, 24)
    nL, nM = len(idx) - 24, 24
    path = tmp_path / "frame.txt"
    path.write_text(f"{nL} {nM}\n" + "\n".join("inf" if np.isinf(v) else float.hex(float(v)) for v in cond) + "\n")
    lines = subprocess.check_output([exe, str(path)], text=True).splitlines()
    (want,), iters, _ = eng.belief_probs([cond], [nL], [nM])  # the C entry: the same doubles
    truth, wi, _ = lc.belief_probs(cond, nL, nM)
    assert abs(int(iters[0]) - wi) <= 1
    np.testing.assert_allclose(want, truth, rtol=0, atol=1e-9)
    assert len(lines) == nM + 1
    for c in range(nM):
        tok = lines[c].split()
        assert tok[:2] == ["p", str(c)]
        got = np.array([float.fromhex(v) for v in tok[2:]])
        assert np.array_equal(bits(got), bits(want[c])), c
    assert lines[-1].startswith("permanentProb: runtime_error")  # the exact shim still stops at 16 measurements
    np.testing.assert_array_equal(pk.beliefProb(cond, nL, nM), want)  # the package-level wrapper
