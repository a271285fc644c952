"""The restatement of the factor lists (kbest_factors.hip): the reference's consumer loop (system.cpp:279-346) written literally
over numpy arrays, the prefix sums, the support by np.add.at -- and the generic cases that both the host build of the kernels
(tests/cpp/factors_host.cpp, tests/test_factors_cpu.py) and the GPU test (tests/test_gpu_factors.py) run: small synthetic P with
dyadic values, so that every equality with a threshold is exact and boxSd / p has no rounding to argue about.

A case is a dict: frames (list of dicts P [nM, nSlot + 1] float64, rows None or int32 ascending [nSlot], landOff, method, and
optional overrides nM, nSlot, probOff that push the frame out of the bounds), maxSlot, maxCol, rowStride, ft, nt, sd (the two
thresholds and boxSd), nSupport (None: no support array), landOffNull, methodNull, mapNull."""
import struct

import numpy as np

# the reference's defaults (constsUtils.h:75-78): BOX_SD, NEW_LANDMARK_THRESH, NEW_FACTOR_PROB_THRESH
BOX_SD, NEW_THRESH, FACTOR_THRESH = 3.0, 0.33, 0.05
# the scenes of the GPU tests give non-empty lists at these (test_factors_cpu.test_conditions_of_the_scenes)
SCENE_FACTOR_THRESH, SCENE_NEW_THRESH = FACTOR_THRESH, NEW_THRESH
INT_PAD, F_PAD = -77, -5.0
F_KEYS = ("fFrame", "fMeas", "fLand", "fMap", "fProb", "fSigma")
N_KEYS = ("nFrame", "nMeas", "nProb", "nSigma")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- 1. the reference's loops ------------------------------------------------------------------------------------------------------------
def frame_lists_literal(P, rows, ft, nt, sd):
    """system.cpp:279-346 on one frame, line for line: for m, for q < nL: skip p < thresh, else a factor with noise sd / p
    (constsUtils.h:57-59); then the new landmark where P[m][nL] > thresh.  rows (None: q) names the landmark of slot q."""
    P = np.asarray(P, np.float64)
    nM, nL = P.shape[0], P.shape[1] - 1
    fm, fl, fp, fs, nm, npr, ns = [], [], [], [], [], [], []
    with np.errstate(divide="ignore", invalid="ignore"):
        for m in range(nM):
            for q in range(nL):
                if P[m][q] < ft:
                    continue
                fm.append(m)
                fl.append(int(rows[q]) if rows is not None else q)
                fp.append(P[m][q])
                fs.append(np.float64(sd) / P[m][q])
            if P[m][nL] > nt:
                nm.append(m)
                npr.append(P[m][nL])
                ns.append(np.float64(sd) / P[m][nL])
    return (np.array(fm, np.int32), np.array(fl, np.int32), np.array(fp, np.float64), np.array(fs, np.float64),
            np.array(nm, np.int32), np.array(npr, np.float64), np.array(ns, np.float64))


def frame_lists(P, rows, ft, nt, sd):
    """The same lists with the inner loop over q as one numpy expression (row-major nonzero IS the order m, then q): what the
    large frames use; tests/test_factors_cpu.py holds it against the literal loops."""
    P = np.asarray(P, np.float64)
    nL = P.shape[1] - 1
    with np.errstate(divide="ignore", invalid="ignore"):
        fm, q = np.nonzero(~(P[:, :nL] < ft))
        fp = P[fm, q]
        nm = np.flatnonzero(P[:, nL] > nt)
        npr = P[nm, nL]
        return (fm.astype(np.int32), (np.asarray(rows)[q] if rows is not None else q).astype(np.int32), fp, np.float64(sd) / fp,
                nm.astype(np.int32), npr, np.float64(sd) / npr)


def frame_numbers(fr):
    nM = fr.get("nM", fr["P"].shape[0])
    nSlot = fr.get("nSlot", fr["P"].shape[1] - 1)
    return nM, nSlot


def emits(fr, case):
    """The frames that emit: method >= 0 (where there is one), inside the bounds, no negative offset."""
    nM, nSlot = frame_numbers(fr)
    if not case.get("methodNull") and fr.get("method", 0) < 0:
        return False
    if not case.get("landOffNull") and fr.get("landOff", 0) < 0:
        return False
    return 1 <= nM <= case["maxCol"] and 0 <= nSlot <= case["maxSlot"] and fr.get("probOff", 0) >= 0


def restate(case, lists=frame_lists):
    """Every output of the entry at unbounded capacity: the lists end to end in the order b, m, l, the true counts, their exclusive
    prefix sums, the totals, the support."""
    out = {k: [] for k in F_KEYS + N_KEYS}
    B = len(case["frames"])
    nFactor, nNew = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b, fr in enumerate(case["frames"]):
        if not emits(fr, case):
            continue
        fm, fl, fp, fs, nm, npr, ns = lists(fr["P"], fr.get("rows"), case["ft"], case["nt"], case["sd"])
        land0 = 0 if case.get("landOffNull") else fr.get("landOff", 0)
        for k, v in zip(F_KEYS + N_KEYS, (np.full(len(fm), b, np.int32), fm, fl, fl.astype(np.int64) + land0, fp, fs,
                                          np.full(len(nm), b, np.int32), nm, npr, ns)):
            out[k].append(v)
        nFactor[b], nNew[b] = len(fm), len(nm)
    dt = dict(fFrame=np.int32, fMeas=np.int32, fLand=np.int32, fMap=np.int64, fProb=np.float64, fSigma=np.float64, nFrame=np.int32,
              nMeas=np.int32, nProb=np.float64, nSigma=np.float64)
    out = {k: np.concatenate([np.zeros(0, dt[k])] + v).astype(dt[k]) for k, v in out.items()}
    out.update(nFactor=nFactor, nNew=nNew, factorOff=np.cumsum(nFactor, dtype=np.int64) - nFactor,
               newOff=np.cumsum(nNew, dtype=np.int64) - nNew, total=np.array([nFactor.sum(), nNew.sum()], np.int64))
    if case.get("nSupport") is not None:
        sup = np.zeros(case["nSupport"], np.int32)
        ok = (out["fMap"] >= 0) & (out["fMap"] < case["nSupport"])
        np.add.at(sup, out["fMap"][ok], 1)
        out["support"] = sup
    return out


def same(got, want, maxFactor, maxNew, what=""):
    """got (arrays of the capacities, handed over full of sentinels) against the restatement: the first min(total, capacity) entries
    bit for bit, the sentinels behind them, the counts, offsets, totals and the support (which does not depend on the capacities)."""
    for k in ("nFactor", "nNew", "factorOff", "newOff", "total"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    for keys, cap, tot in ((F_KEYS, maxFactor, int(want["total"][0])), (N_KEYS, maxNew, int(want["total"][1]))):
        n = min(cap, tot)
        for k in keys:
            if k not in got:
                continue
            assert len(got[k]) == cap, (what, k)
            if got[k].dtype == np.float64:
                assert np.array_equal(bits(got[k][:n]), bits(want[k][:n])), (what, k)
                assert (got[k][n:] == F_PAD).all(), (what, k, "beyond the list")
            else:
                assert np.array_equal(got[k][:n], want[k][:n]), (what, k)
                assert (got[k][n:] == INT_PAD).all(), (what, k, "beyond the list")
    assert ("support" in got) == ("support" in want), what
    if "support" in want:
        assert np.array_equal(got["support"], want["support"]), (what, "support")


# ---- 2. packing: one layout for the host program and the GPU test -------------------------------------------------------------------------
def pack(case, pad=0):
    """The input arrays of a case: probs (every frame's slice, `pad` sentinels before, between and behind), probOff, nSlot, nM,
    rowIdx [B][rowStride] (None in dense form), landOff, method."""
    frames = case["frames"]
    B = len(frames)
    parts, probOff, at = [np.full(pad, np.nan)], [], pad
    for fr in frames:
        probOff.append(fr.get("probOff", at))
        parts += [np.ascontiguousarray(fr["P"], dtype=np.float64).reshape(-1), np.full(pad, np.nan)]
        at += fr["P"].size + pad
    compact = any(fr.get("rows") is not None for fr in frames)
    rowIdx = None
    if compact:
        rowIdx = np.full((B, case["rowStride"]), INT_PAD, np.int32)
        for b, fr in enumerate(frames):
            if fr.get("rows") is not None:
                rowIdx[b, :len(fr["rows"])] = fr["rows"]
    nMS = [frame_numbers(fr) for fr in frames]
    return dict(probs=np.concatenate(parts), probOff=np.array(probOff, np.int64).reshape(B), nSlot=np.array([x[1] for x in nMS], np.int32).reshape(B),
                nM=np.array([x[0] for x in nMS], np.int32).reshape(B), rowIdx=rowIdx,
                landOff=np.array([fr.get("landOff", 0) for fr in frames], np.int64).reshape(B),
                method=np.array([fr.get("method", 0) for fr in frames], np.int32).reshape(B))


def write_host_input(path, case, maxFactor, maxNew):
    """The IN file of tests/cpp/factors_host.cpp."""
    k = pack(case)
    B = len(case["frames"])
    flags = (1 if k["rowIdx"] is not None else 0) | (0 if case.get("landOffNull") else 2) | (0 if case.get("methodNull") else 4) | \
        (8 if case.get("nSupport") is not None else 0) | (0 if case.get("mapNull") else 16)
    with open(path, "wb") as f:
        f.write(struct.pack("<4i5q3d", B, case["maxSlot"], case["maxCol"], flags, case.get("rowStride", 0), case.get("nSupport") or 0,
                            maxFactor, maxNew, len(k["probs"]), case["ft"], case["nt"], case["sd"]))
        f.write(k["probOff"].tobytes() + k["landOff"].tobytes() + k["nSlot"].tobytes() + k["nM"].tobytes() + k["method"].tobytes())
        if k["rowIdx"] is not None:
            f.write(k["rowIdx"].tobytes())
        f.write(k["probs"].tobytes())


def read_host_output(path, case, maxFactor, maxNew):
    """The OUT file of tests/cpp/factors_host.cpp as the dict `same` takes."""
    buf = open(path, "rb").read()
    B, at, out = len(case["frames"]), 0, {}

    def take(key, dt, n):
        nonlocal at
        out[key] = np.frombuffer(buf, dtype=dt, count=n, offset=at).copy()
        at += n * np.dtype(dt).itemsize

    take("total", np.int64, 2)
    take("factorOff", np.int64, B)
    take("newOff", np.int64, B)
    take("nFactor", np.int32, B)
    take("nNew", np.int32, B)
    if not case.get("mapNull"):
        take("fMap", np.int64, maxFactor)
    for k in ("fProb", "fSigma"):
        take(k, np.float64, maxFactor)
    for k in ("nProb", "nSigma"):
        take(k, np.float64, maxNew)
    for k in ("fFrame", "fMeas", "fLand"):
        take(k, np.int32, maxFactor)
    for k in ("nFrame", "nMeas"):
        take(k, np.int32, maxNew)
    if case.get("nSupport") is not None:
        take("support", np.int32, case["nSupport"])
    assert at == len(buf)
    return out


# ---- 3. the generic cases ----------------------------------------------------------------------------------------------------------------------
DYADIC = np.array([0.0, 1 / 64, 1 / 32, 1 / 16, 1 / 16, 1 / 8, 1 / 4, 1 / 4, 1 / 2, 1.0])
FT, NT, SD = 1 / 16, 1 / 4, 3.0  # p == FT is kept, p == NT is not new; 3 / p is exact for every dyadic p
SLOTS = (0, 1, 63, 64, 65, 255, 256, 257, 1000)


def dyadic(rng, nM, nSlot):
    return DYADIC[rng.integers(0, len(DYADIC), size=(nM, nSlot + 1))]


def base(frames, maxSlot, maxCol, ft=FT, nt=NT, sd=SD, **kw):
    c = dict(frames=frames, maxSlot=maxSlot, maxCol=maxCol, ft=ft, nt=nt, sd=sd, nSupport=None, rowStride=0)
    c.update(kw)
    return c


def grid_case(maxCol=7, nMs=(1, 2, 5, 7), slots=SLOTS, seed=1):
    """nSlot in {0, 1, 63, 64, 65, 255, 256, 257, 1 000} x nM in {1, 2, 5, maxCol}; the support shorter than the largest map index."""
    rng = np.random.default_rng(seed)
    frames = [dict(P=dyadic(rng, nM, nSlot), landOff=int(rng.integers(0, 500))) for nSlot in slots for nM in nMs]
    return base(frames, 1000, maxCol, nSupport=700)


def pattern_case():
    """Rows with every slot kept, only slot 0, only slot 63, only slot 64, only the last slot, nothing; each with the miss column
    on either side of its threshold."""
    nSlot = 300
    P = np.zeros((12, nSlot + 1))
    for m, keep in enumerate((slice(0, nSlot), [0], [63], [64], [nSlot - 1], [])):
        for half in (0, 1):
            P[2 * m + half, keep] = 0.5
            P[2 * m + half, nSlot] = NT if half == 0 else 0.5
    return base([dict(P=P, landOff=5), dict(P=P[::-1].copy(), landOff=0)], nSlot, 12, nSupport=400)


def refused_case(seed=3):
    """Frames with method -1 and -2 full of NaN, and frames outside the bounds (nM 0, nM > maxCol, nSlot > maxSlot, nSlot < 0, a
    negative probOff, a negative landOff), between frames that emit."""
    rng = np.random.default_rng(seed)
    def good():
        P = dyadic(rng, 3, 70)
        P[:2, 70] = (0.5, 1.0)  # (new landmarks in every frame that emits)
        return dict(P=P, landOff=int(rng.integers(0, 50)))


    nan = lambda **kw: dict(dict(P=np.full((3, 71), np.nan), landOff=1), **kw)  # noqa: E731
    frames = [good(), nan(method=-1), nan(method=-2), good(), nan(nM=0), nan(nM=6), nan(nSlot=101), nan(nSlot=-1), nan(probOff=-8),
              nan(landOff=-1), good()]
    return base(frames, 100, 5, nSupport=200)


def compact_pair(seed=4):
    """(compact, dense): frames with random ascending rowIdx and rowStride > nSlot, and the dense expansion of the same frames --
    the same fLand, the same lists."""
    rng = np.random.default_rng(seed)
    comp, dense = [], []
    for nM, nSlot, nL in ((3, 0, 10), (5, 1, 400), (2, 64, 64), (7, 130, 900), (4, 257, 1000)):
        rows = np.sort(rng.choice(nL, size=nSlot, replace=False)).astype(np.int32)
        P = dyadic(rng, nM, nSlot)
        P[:, :nSlot] = np.maximum(P[:, :nSlot], 1 / 64)  # (a kept 0.0 of the dense form would be every landmark that is not kept)
        D = np.zeros((nM, nL + 1))
        D[:, rows] = P[:, :nSlot]
        D[:, nL] = P[:, nSlot]
        off = int(rng.integers(0, 100))
        comp.append(dict(P=P, rows=rows, landOff=off))
        dense.append(dict(P=D, landOff=off))
    return base(comp, 300, 7, rowStride=300, nSupport=1100, ft=1 / 64), base(dense, 1000, 7, nSupport=1100, ft=1 / 64)


def generic_cases():
    """name -> case.  Every one is run at capacity = total; `capacity_cases` names those that are also run at total - 1, 1 and 0."""
    rng = np.random.default_rng(9)
    small = base([dict(P=dyadic(rng, nM, nSlot), landOff=7 * nM) for nM, nSlot in ((2, 65), (5, 3), (1, 0), (4, 257))], 300, 5, nSupport=150)
    comp, dense = compact_pair()
    wide = base([dict(P=dyadic(rng, 128, nSlot), landOff=3) for nSlot in (65, 1000)], 1000, 128, nSupport=900)
    return dict(
        grid=grid_case(), wide=wide, small=small, pattern=pattern_case(), refused=refused_case(), compact=comp, dense=dense,
        keep_all_zero=dict(small, ft=0.0), keep_all_negative=dict(small, ft=-1.0), keep_none=dict(small, ft=2.0),
        no_support=dict(small, nSupport=None), no_landoff=dict(small, landOffNull=True),
        # (without d_method the frames outside the bounds still emit nothing; the NaN frames with a method are left out)
        no_method=dict(refused_case(), methodNull=True, frames=[f for f in refused_case()["frames"] if f.get("method", 0) >= 0]),
        no_map=dict(small, mapNull=True), short_support=dict(small, nSupport=3))


CAPACITY_CASES = ("small", "refused")


def capacities(total):
    """total, total - 1, 1, 0 (those that are >= 0, once each)."""
    return sorted({c for c in (total, total - 1, 1, 0) if c >= 0}, reverse=True)
