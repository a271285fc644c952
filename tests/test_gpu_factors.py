"""GPU: factor lists from association probabilities (kbest_assoc_factors_f64_dev, kbest_quadric_map_factors_batch_f64_dev and the
host entries).  The yardstick is tests/factors_lib.py -- the reference's consumer loop (system.cpp:279-346) restated -- and every
comparison is bit for bit.  Every output buffer lies between sentinels (-77 / -5.0): nothing is written outside
[0, min(total, capacity)) of a list or outside a count array.  The fused entry is also held against quadric_map_probs_dev alone
(every probability output with equal bits) and against the generic entry on its own d_cprobs (compact form) and d_probs (dense
form).  Nothing here reaches a k-best kernel: the host entries run at k = 0, max_big = 0."""
import numpy as np
import pytest
import torch

import factors_lib as fl
import probabilisticsemslam_amd as pk
import quadric_map_lib as qm
from test_gpu_quadric_map import MapCall, same_frame

pytestmark = pytest.mark.gpu

PAD, INT_PAD, F_PAD = 64, fl.INT_PAD, fl.F_PAD
FT, NT, SD = fl.SCENE_FACTOR_THRESH, fl.SCENE_NEW_THRESH, fl.BOX_SD
T = qm.TILE
I32, I64, F64 = torch.int32, torch.int64, torch.float64


@pytest.fixture(scope="module")
def eng():
    e = pk.KBestEngine(0)
    yield e
    e.close()


def dev():
    return torch.device("cuda", 0)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


class Lists:
    """The output buffers of one call, each between PAD sentinels; kw() are the factor arguments of the engine's entries,
    collect() synchronises, checks the sentinels around every buffer and returns what factors_lib.same takes."""

    KINDS = dict(fFrame=I32, fMeas=I32, fLand=I32, fMap=I64, fProb=F64, fSigma=F64, nFrame=I32, nMeas=I32, nProb=F64, nSigma=F64,
                 nFactor=I32, factorOff=I64, nNew=I32, newOff=I64, total=I64, support=I32)

    def __init__(self, B, maxFactor, maxNew, nSupport=None, with_map=True):
        self.B, self.cf, self.cn, self.nSupport = B, int(maxFactor), int(maxNew), nSupport
        size = dict(nFactor=B, factorOff=B, nNew=B, newOff=B, total=2, support=nSupport)
        size.update({k: self.cf for k in fl.F_KEYS}, **{k: self.cn for k in fl.N_KEYS})
        self.t = {}
        for k, dt in self.KINDS.items():
            if size[k] is None or (k == "fMap" and not with_map):
                continue
            self.t[k] = torch.full((size[k] + 2 * PAD,), F_PAD if dt == F64 else INT_PAD, dtype=dt, device=dev())

    def view(self, k):
        return self.t[k][PAD:] if k in self.t else None

    def kw(self):
        return dict(max_factor=self.cf, d_factors=tuple(self.view(k) for k in fl.F_KEYS) if self.cf else None, max_new=self.cn,
                    d_news=tuple(self.view(k) for k in fl.N_KEYS) if self.cn else None,
                    d_counts=tuple(self.view(k) for k in ("nFactor", "factorOff", "nNew", "newOff")), d_total=self.view("total"),
                    d_support=self.view("support"), n_support=self.nSupport or 0)

    def refill(self):
        for k, t in self.t.items():
            t.fill_(F_PAD if t.dtype == F64 else INT_PAD)

    def collect(self):
        torch.cuda.synchronize()
        out = {}
        for k, t in self.t.items():
            h = t.cpu().numpy()
            pad = F_PAD if t.dtype == F64 else INT_PAD
            assert (h[:PAD] == pad).all() and (h[len(h) - PAD:] == pad).all(), (k, "written outside the buffer")
            out[k] = h[PAD:len(h) - PAD].copy()
        return out


def per_frame(got, b):
    """The entries of frame b: what must be the same alone and in any batch."""
    f = slice(int(got["factorOff"][b]), int(got["factorOff"][b]) + int(got["nFactor"][b]))
    n = slice(int(got["newOff"][b]), int(got["newOff"][b]) + int(got["nNew"][b]))
    return [got[k][f].tobytes() for k in fl.F_KEYS[1:] if k in got] + [got[k][n].tobytes() for k in fl.N_KEYS[1:]]


# ---- 1. the generic cases ------------------------------------------------------------------------------------------------------------------
def run_generic(eng, case, cf, cn, stream=None, reserve=True):
    k = fl.pack(case, pad=PAD)
    B = len(case["frames"])
    d = {key: up(k[key]) for key in ("probs", "probOff", "nSlot", "nM", "landOff", "method")}
    rows = up(k["rowIdx"]) if k["rowIdx"] is not None else None
    out = Lists(B, cf, cn, case.get("nSupport"), not case.get("mapNull"))
    torch.cuda.synchronize()
    eng.assoc_factors_dev(B, case["maxSlot"], case["maxCol"], d["probs"], d["probOff"], d["nSlot"], d["nM"], d_rowIdx=rows,
                          row_stride=case.get("rowStride", 0), d_landOff=None if case.get("landOffNull") else d["landOff"],
                          d_method=None if case.get("methodNull") else d["method"], factor_thresh=case["ft"], new_thresh=case["nt"],
                          box_sd=case["sd"], stream=stream, reserve=reserve, **out.kw())
    return out.collect()


CASES = fl.generic_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_generic_cases(eng, name):
    """Every generic case of factors_lib at capacity = total: nSlot in {0, 1, 63, 64, 65, 255, 256, 257, 1 000} x nM in {1, 2, 5,
    maxCol}, p == factorThresh kept, p == newThresh not new, thresholds that keep everything (sigma +inf at p = 0) and nothing, the
    row patterns, refused and out-of-bounds frames full of NaN, the compact form, NULL support / landOff / method / fMap, a short
    support."""
    case = CASES[name]
    want = fl.restate(case)
    tf, tn = (int(x) for x in want["total"])
    fl.same(run_generic(eng, case, tf, tn), want, tf, tn, name)


def test_compact_and_dense_form_give_the_same_list(eng):
    comp, dense = CASES["compact"], CASES["dense"]
    tf, tn = (int(x) for x in fl.restate(comp)["total"])
    a, b = run_generic(eng, comp, tf, tn), run_generic(eng, dense, tf, tn)
    assert tf > 100 and set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("name", fl.CAPACITY_CASES)
def test_capacities(eng, name):
    case = CASES[name]
    want = fl.restate(case)
    tf, tn = (int(x) for x in want["total"])
    for cf, cn in list(zip(fl.capacities(tf), fl.capacities(tn))) + [(0, tn), (tf, 0)]:
        fl.same(run_generic(eng, case, cf, cn), want, cf, cn, (name, cf, cn))


def test_no_frame(eng):
    case = fl.base([], 10, 4, nSupport=5)
    got = run_generic(eng, case, 2, 2)
    fl.same(got, fl.restate(case), 2, 2, "B = 0")
    assert got["total"].tolist() == [0, 0] and got["support"].tolist() == [0] * 5


def test_bad_arguments(eng):
    case = CASES["small"]
    strerror = lambda rc: eng.lib.kbest_strerror(rc).decode()  # noqa: E731
    for kw in (dict(ft=float("nan")), dict(nt=float("nan")), dict(sd=float("nan")), dict(maxCol=0), dict(maxCol=129), dict(maxSlot=-1),
               dict(maxSlot=(1 << 22) + 1)):
        with pytest.raises(pk.KBestError) as err:
            run_generic(eng, dict(case, **kw), 4, 4)
        assert str(err.value).startswith(strerror(-2)), kw
    for cf, cn in ((-1, 4), (4, -1)):
        out = Lists(4, 4, 4)
        kw = dict(out.kw(), max_factor=cf, max_new=cn)
        with pytest.raises(pk.KBestError) as err:
            eng.assoc_factors_dev(0, 10, 4, None, None, None, None, **kw)
        assert str(err.value).startswith(strerror(-2)), (cf, cn)


# ---- 2. the fused entry ------------------------------------------------------------------------------------------------------------------------
def launch_fused(eng, c, out, stream=None, reserve=True):
    eng.quadric_map_factors_dev(c.B, c.maxMap, c.maxKeep, c.maxCol, c.d_map[0], c.d_map[1], c.d_landOff, c.d_nL, c.d_meas[0], c.d_meas[1],
                                c.d_measOff, c.d_nM, c.gate, c.d_int[0, 1:], c.d_rows[PAD:], c.d_cprobs[PAD:], c.d_int[1, 1:],
                                d_ccost=c.d_ccost[PAD:], d_probs=c.d_probs, d_probOff=c.d_probOff if c.d_probs is not None else None,
                                d_logPerm=c.d_lp[1:], d_nOpen=c.d_int[2, 1:], d_nFrontier=c.d_int[3, 1:], d_maxCluster=c.d_int[4, 1:],
                                factor_thresh=FT, new_thresh=NT, box_sd=SD, stream=stream, reserve=reserve, **out.kw())


def restated_case(c, got, nSupport):
    """The restatement's input from the call's own probability outputs: the compact probabilities, rowIdx and method as collected."""
    frames = []
    for b, g in enumerate(got):
        if g["took"]:
            frames.append(dict(P=g["cprobs"], rows=g["rows"], landOff=c.frames[b][0], method=g["method"]))
        else:
            frames.append(dict(P=np.full((1, 1), np.nan), landOff=c.frames[b][0], method=-1))
    return dict(frames=frames, maxSlot=c.maxKeep, maxCol=c.maxCol, rowStride=c.maxKeep, ft=FT, nt=NT, sd=SD, nSupport=nSupport)


def fused_scene(eng, which, index=None, cap=(20000, 4000), **kw):
    """One fused call on a scene: (the MapCall, its collected frames, the collected lists, the restatement of the lists)."""
    mean, cov, frames, gate = qm.BATCHES[which]()
    c = MapCall(mean, cov, [frames[j] for j in (index if index is not None else range(len(frames)))], gate, **kw)
    out = Lists(c.B, cap[0], cap[1], len(mean))
    torch.cuda.synchronize()
    launch_fused(eng, c, out)
    got, lists = c.collect(), out.collect()
    return c, got, lists, fl.restate(restated_case(c, got, len(mean)))


SCENES = dict(edge=dict(maxMap=4 * T, maxKeep=300, maxCol=128), limit=dict(maxMap=300, maxKeep=8, maxCol=4), parity=dict(maxKeep=300),
              far=dict(index=[6], maxKeep=256))


@pytest.mark.parametrize("which", sorted(SCENES))
def test_fused_entry(eng, which):
    """edge, limit, parity (16 frames of a 300-landmark map) and the one far frame against 100 000 landmarks: every probability
    output with the bits of quadric_map_probs_dev alone; the lists equal to the restatement on the call's own d_cprobs, to
    assoc_factors_dev on that d_cprobs (compact form) and on the same call's dense d_probs (dense form)."""
    kw = dict(SCENES[which])
    c, got, lists, want = fused_scene(eng, which, **kw)
    mean, cov, frames, gate = qm.BATCHES[which]()
    index = kw.pop("index", None)
    alone = MapCall(mean, cov, [frames[j] for j in (index if index is not None else range(len(frames)))], gate, **kw)
    torch.cuda.synchronize()
    alone.launch(eng)
    for b, (g, a) in enumerate(zip(got, alone.collect())):
        same_frame(g, a, f"{which} frame {b}: the probability entry alone")
    cf, cn = lists["fFrame"].size, lists["nFrame"].size
    tf, tn = (int(x) for x in want["total"])
    print(f"{which}: factors {tf}, new landmarks {tn}, largest support {want['support'].max()}")
    assert 0 < tf <= cf and tn <= cn and (tn > 0 or which == "limit")  # (limit: every measurement sits on landmarks, none is new)
    fl.same(lists, want, cf, cn, which)
    # the generic entry on the call's own buffers: compact, then dense
    comp, poff = Lists(c.B, cf, cn, len(mean)), up(np.arange(c.B, dtype=np.int64) * c.pstride)
    torch.cuda.synchronize()
    eng.assoc_factors_dev(c.B, c.maxKeep, c.maxCol, c.d_cprobs[PAD:], poff, c.d_int[0, 1:], c.d_nM,
                          d_rowIdx=c.d_rows[PAD:], row_stride=c.maxKeep, d_landOff=c.d_landOff, d_method=c.d_int[1, 1:],
                          factor_thresh=FT, new_thresh=NT, box_sd=SD, **comp.kw())
    fl.same(comp.collect(), want, cf, cn, which + ", compact form")
    dense = Lists(c.B, cf, cn, len(mean))
    torch.cuda.synchronize()
    eng.assoc_factors_dev(c.B, c.maxMap, c.maxCol, c.d_probs, c.d_probOff, c.d_nL, c.d_nM, d_landOff=c.d_landOff, d_method=c.d_int[1, 1:],
                          factor_thresh=FT, new_thresh=NT, box_sd=SD, **dense.kw())
    fl.same(dense.collect(), want, cf, cn, which + ", dense form")
    if which == "far":
        assert want["fLand"].max() > 65535 and want["fMap"].max() > 70535
    if which == "edge":
        assert want["support"].max() >= 2
    if which == "limit":  # nKeep = maxKeep emits; nKeep = maxKeep + 1 and the frames beyond the bounds do not
        assert got[1]["nKeep"] == 9 and want["nFactor"][0] > 0 and not want["nFactor"][1:].any() and not want["nNew"][1:].any()
    if which == "parity":
        assert np.bincount(want["fFrame"].astype(np.int64) * 24 + want["fMeas"]).max() >= 2


def test_fused_entry_without_the_dense_slice(eng):
    """d_probs = NULL: the same lists."""
    _, _, lists, want = fused_scene(eng, "parity", maxKeep=300, dense=False)
    fl.same(lists, want, lists["fFrame"].size, lists["nFrame"].size, "no dense slice")
    _, _, full, _ = fused_scene(eng, "parity", maxKeep=300)
    for k in lists:
        assert np.array_equal(lists[k], full[k]), k


def test_a_frame_alone_in_a_batch_and_reversed(eng):
    _, _, base, _ = fused_scene(eng, "parity", maxKeep=300)
    _, _, back, _ = fused_scene(eng, "parity", index=list(range(15, -1, -1)), maxKeep=300)
    for j in range(16):
        assert per_frame(back, 15 - j) == per_frame(base, j), j
    for j in (0, 7, 15):
        _, _, one, _ = fused_scene(eng, "parity", index=[j], maxKeep=300)
        assert per_frame(one, 0) == per_frame(base, j) and one["factorOff"][0] == 0 and (one["fFrame"][:int(one["total"][0])] == 0).all(), j
    assert base["total"][0] == back["total"][0] and np.array_equal(base["support"], back["support"])


def test_two_calls_on_one_stream_without_a_synchronise_between(eng):
    mean, cov, frames, gate = qm.parity_batch()
    _, _, base, _ = fused_scene(eng, "parity", maxKeep=300)
    eng.reserve_quadric_map_factors_dev(16, 300, 300, 24)
    a, b = MapCall(mean, cov, frames, gate, maxKeep=300), MapCall(mean, cov, frames[::-1][:9], gate, maxKeep=300)
    oa, ob = Lists(16, 20000, 4000, 300), Lists(9, 20000, 4000, 300)
    s = torch.cuda.Stream(device=dev())
    torch.cuda.synchronize()
    launch_fused(eng, a, oa, stream=s.cuda_stream, reserve=False)
    launch_fused(eng, b, ob, stream=s.cuda_stream, reserve=False)
    ga, gb = oa.collect(), ob.collect()
    for k in base:
        assert np.array_equal(ga[k], base[k]), k
    for j in range(9):
        assert per_frame(gb, j) == per_frame(base, 15 - j), j


def test_beyond_the_reservation_nothing_is_launched():
    """reserve=False on a context that has reserved nothing, the probability entry's work space only, the factor work space only,
    or the factor work space for fewer frames: KBEST_ERR_NOT_RESERVED and every output -- the probability entry's too -- still holds
    its sentinels.  Then the full reservation, and the call answers."""
    mean, cov, frames, gate = qm.parity_batch()
    c, out = MapCall(mean, cov, frames, gate, maxKeep=300), Lists(16, 20000, 4000, 300)
    fresh, other = pk.KBestEngine(0), pk.KBestEngine(0)
    torch.cuda.synchronize()
    try:
        not_reserved = fresh.lib.kbest_strerror(-6).decode()

        def refused(e, call):
            with pytest.raises(pk.KBestError) as err:
                call(e)
            assert str(err.value).startswith(not_reserved), str(err.value)

        fused = lambda e: launch_fused(e, c, out, reserve=False)  # noqa: E731
        refused(fresh, fused)
        refused(fresh, lambda e: run_generic(e, CASES["small"], 4, 4, reserve=False))
        fresh.reserve_quadric_map_dev(16, 300, 300, 24)
        refused(fresh, fused)
        fresh.reserve_assoc_factors_dev(15, 24)
        refused(fresh, fused)
        fresh.reserve_assoc_factors_dev(16, 23)  # (never shrinks: 24 columns stay reserved)
        other.reserve_assoc_factors_dev(16, 24)
        refused(other, fused)
        for g in c.collect():  # nothing of the refused calls was launched: every output still untouched
            assert g["nKeep"] == INT_PAD and g["method"] == INT_PAD and not g["took"]
        assert all((v == (F_PAD if v.dtype == np.float64 else INT_PAD)).all() for v in out.collect().values())
        fused(fresh)
        assert out.collect()["total"][0] > 0 and any(g["method"] == 0 for g in c.collect())
    finally:
        fresh.close()
        other.close()


def test_captured_and_replayed_on_other_data():
    """Reserve, run eagerly, capture the fused entry on one stream, replay on a second data set inside the same bounds (other frames
    of the same map: only the measurement buffers change): the lists of the eager launches on that data."""
    mean, cov, frames, gate = qm.parity_batch()
    own = pk.KBestEngine(0)  # a context of the test's own: a captured launch marks its work spaces for life
    try:
        sets = [list(range(0, 6)), list(range(10, 16))]
        eager = []
        for idx in sets:
            c, o = MapCall(mean, cov, [frames[j] for j in idx], gate, maxKeep=300), Lists(6, 8000, 2000, 300)
            torch.cuda.synchronize()
            launch_fused(own, c, o)
            eager.append((c, c.collect(), o.collect()))
        main, out = MapCall(mean, cov, [frames[j] for j in sets[0]], gate, maxKeep=300), Lists(6, 8000, 2000, 300)
        s = torch.cuda.Stream(device=dev())
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            launch_fused(own, main, out, stream=s.cuda_stream, reserve=False)
        for k in (1, 0):
            with torch.cuda.stream(s):
                main.d_meas[0].copy_(eager[k][0].d_meas[0])
                main.d_meas[1].copy_(eager[k][0].d_meas[1])
                for t in (main.d_rows, main.d_int):
                    t.fill_(INT_PAD)
                main.d_ccost.fill_(-7.0)
                for t in (main.d_cprobs, main.d_probs, main.d_lp):
                    t.fill_(-5.0)
                out.refill()
                graph.replay()
            s.synchronize()
            for i, g in enumerate(main.collect()):
                same_frame(g, eager[k][1][i], f"replay of set {k}, frame {i}")
            got = out.collect()
            assert got["total"][0] > 0 and got["total"][1] > 0
            for key in got:
                assert np.array_equal(got[key], eager[k][2][key]), (k, key)
    finally:
        own.close()


# ---- 3. the host entries ------------------------------------------------------------------------------------------------------------------------
def test_host_entries(eng):
    """assoc_factors on the dense output of quadric_map_probs(k = 0), and quadric_map_factors(k = 0): the restatement on those dense
    slices, per frame and flat, and the support over the map."""
    mean, cov, frames, gate = qm.parity_batch()
    frames = [(f[0] + 3 * j, f[1] - 3 * j) + tuple(f[2:]) for j, f in enumerate(frames[:6])]  # (windows 3j .. 299 of the map)
    out = eng.quadric_map_probs(mean, cov, frames, gate, k=0, max_big=0)
    case = dict(frames=[dict(P=out[0][b], landOff=frames[b][0], method=int(out[1][b])) for b in range(6)], maxSlot=300, maxCol=24, ft=FT,
                nt=NT, sd=SD, nSupport=300)
    want = fl.restate(case)
    tf, tn = (int(x) for x in want["total"])
    assert tf > 0 and tn > 0 and (out[1] >= 0).any()
    got = eng.assoc_factors(out[0], land_off=[f[0] for f in frames], method=out[1], n_support=300)
    fused = eng.quadric_map_factors(mean, cov, frames, gate, k=0, max_big=0)
    for r in (got, fused):
        flat = dict(r["flat"], **{k: r[k] for k in ("nFactor", "factorOff", "nNew", "newOff", "total", "support")})
        for k, v in flat.items():
            assert np.array_equal(v, want[k]) and (v.dtype != np.float64 or np.array_equal(fl.bits(v), fl.bits(want[k]))), k
        for b in range(6):
            f = slice(int(want["factorOff"][b]), int(want["factorOff"][b]) + int(want["nFactor"][b]))
            assert np.array_equal(r["factors"][b]["land"], want["fLand"][f]) and np.array_equal(fl.bits(r["factors"][b]["sigma"]), fl.bits(want["fSigma"][f]))
            assert len(r["new"][b]["meas"]) == want["nNew"][b]
    assert np.array_equal(fused["method"], out[1])
    short = eng.assoc_factors(out[0], land_off=[f[0] for f in frames], method=out[1], max_factor=tf - 1, max_new=1)  # total > capacity
    assert short["total"].tolist() == [tf, tn] and len(short["flat"]["fLand"]) == tf - 1 and len(short["flat"]["nMeas"]) == 1
    assert np.array_equal(short["flat"]["fLand"], want["fLand"][:tf - 1])
