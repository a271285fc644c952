"""What tests/test_gpu_graph_capture.py captures and replays, without a GPU: the data sets of every case, their references (always the
restatement the entry's own GPU test file uses), the launch bounds, and the work-space needs by the formulas of include/kbest_c.h that
the growth step of a case relies on.  tests/test_graph_capture_cpu.py asserts the conditions of the inputs from this module alone.

A frame case has four data sets inside the SAME launch bounds (B, maxRawRow, maxCol) -- the capture bakes those in --: A (heavy: the
eager launch and the capture), H1 and H2 (heavy, other frames, H2 laid out in reverse order in the buffers), and L (light: smaller
frames, one infeasible frame, one frame beyond the bounds).  Shapes, offsets and keys are device data and differ between the sets.
Cost blocks are column-major (nL+nM) x nM, as everywhere in this project."""
from __future__ import annotations

import functools
import types

import numpy as np

import cluster_check as cc
import cluster_sample_check as csc
import hybrid_check as hc
import lbp_check as lc
import oracle_lib as ol
import permanent_check as pc
import sample_check as sc
from probabilisticsemslam_amd import workloads as wl

MIN_MARGIN = 1e-10          # tests/test_gpu_sample.py
RAW_RESERVE_FLOOR = 1 << 16  # the smallest work space the context allocates (raw_reserve): a need below it does not show as growth
ORDER = ("H1", "L", "H2", "A")  # the replays: heavy, light, heavy, heavy -- the last two back to back


def dense_frame(nR, nM, seed):
    return wl.dense_batch(1, nR, nM, seed)[0] * 10.0


def infeasible(block, nL, nM):
    """The frame with columns 0 and 1 finite in row 0 only: two measurements, one row -- no assignment, whatever conditioning does."""
    nR = nL + nM
    out = np.array(block, dtype=np.float64)
    for c in (0, 1):
        keep = out[c * nR]
        out[c * nR: (c + 1) * nR] = np.inf
        out[c * nR] = keep if np.isfinite(keep) else 1.0 + c
    return out


class DataSet:
    """frames: [(block, nL, nM)]; keys: one uint64 per frame (samplers); reverse: the slices lie in reverse frame order in the buffers;
    infeasible / beyond: the index of that frame, or None."""

    def __init__(self, name, frames, keys=None, reverse=False, infeasible=None, beyond=None, seed=0):
        self.name, self.frames, self.reverse, self.infeasible, self.beyond, self.seed = name, frames, reverse, infeasible, beyond, seed
        self.keys = list(range(len(frames))) if keys is None else keys
        self.B = len(frames)
        self.nL = np.array([f[1] for f in frames], np.int32)
        self.nM = np.array([f[2] for f in frames], np.int32)

    def offsets(self, sizes):
        """Where every frame's slice of `sizes` doubles / ints starts: end to end, in frame order or in reverse."""
        sizes = np.asarray(sizes, np.int64)
        order = np.arange(self.B)[::-1] if self.reverse else np.arange(self.B)
        off = np.zeros(self.B, np.int64)
        at = 0
        for b in order:
            off[b] = at
            at += int(sizes[b])
        return off

    @property
    def cost_sizes(self):
        return (self.nL.astype(np.int64) + self.nM) * self.nM

    @property
    def prob_sizes(self):
        return self.nM.astype(np.int64) * (self.nL.astype(np.int64) + 1)

    def flat_cost(self, cap):
        out = np.zeros(cap, np.float64)
        off = self.offsets(self.cost_sizes)
        for b, f in enumerate(self.frames):
            out[off[b]: off[b] + f[0].size] = f[0]
        return out

    def inside(self, b, maxRawRow, maxCol):
        return 1 <= self.nM[b] <= maxCol and self.nL[b] >= 0 and self.nL[b] + self.nM[b] <= maxRawRow


def pow2_at_least(n):
    cap = RAW_RESERVE_FLOOR
    while cap < n:
        cap <<= 1
    return cap


class FrameCase:
    """Base of the cases whose entry takes a frame batch.  Subclasses: the data sets, the reference, the needs."""
    name = ""
    n_sample = 0
    holds_work_space = True   # False: the captured launch plans without a work space of the context -- nothing to refuse
    condition = False

    def __init__(self):
        self._want = {}

    # -- data ---------------------------------------------------------------------------------------------------------------------
    def sets(self):
        raise NotImplementedError

    @functools.cached_property
    def data(self):
        d = self.sets()
        assert set(d) == {"A", "H1", "H2", "L", "O"}  # O: the eager launch between two replays, in buffers of its own
        assert len({s.B for s in d.values()}) == 1
        return d

    @property
    def B(self):
        return self.data["A"].B

    @functools.cached_property
    def bounds(self):
        """(maxRawRow, maxCol): the heavy sets decide; L's `beyond` frame lies outside."""
        heavy = [self.data[n] for n in ("A", "H1", "H2", "O")]
        return (int(max((s.nL + s.nM).max() for s in heavy)), int(max(s.nM.max() for s in heavy)))

    def caps(self):
        """Doubles of cost / probabilities and ints of draws the buffers must hold: the largest set."""
        n = max(self.n_sample, 1)
        return dict(cost=max(int(s.cost_sizes.sum()) for s in self.data.values()),
                    prob=max(int(s.prob_sizes.sum()) for s in self.data.values()),
                    asg=max(int(s.nM.sum()) * n for s in self.data.values()))

    # -- reference ----------------------------------------------------------------------------------------------------------------
    def reference(self, ds, b):
        raise NotImplementedError

    def want(self, ds):
        """The reference of every frame of the set inside the bounds (None beyond).  Computed once per set, never changed."""
        if ds.name not in self._want:
            R, Cm = self.bounds
            self._want[ds.name] = [self.reference(ds, b) if ds.inside(b, R, Cm) else None for b in range(ds.B)]
        return self._want[ds.name]

    def margins(self):
        """Samplers: the smallest relative margin of every data set's restatement."""
        return {}

    def light_conditions(self):
        """(the light set's infeasible frame IS infeasible by the reference, its refused frame IS beyond the bounds)."""
        L = self.data["L"]
        R, Cm = self.bounds
        return self.is_infeasible(self.want(L)[L.infeasible]), not L.inside(L.beyond, R, Cm)

    def is_infeasible(self, w):
        raise NotImplementedError

    # -- needs by the header's formulas -----------------------------------------------------------------------------------------------
    def need_before(self):
        raise NotImplementedError

    def need_after(self):
        raise NotImplementedError

    def growth_premise(self):
        """The growth request at least quadruples the need, and lies beyond what was allocated for the capture."""
        before, after = self.need_before(), self.need_after()
        return after >= 4 * before and after > pow2_at_least(before)


def light_frames(shapes, seed, maxRawRow):
    """Dense frames of `shapes` [(nR, nM)], the second infeasible, the last beyond the bounds: one row too many."""
    frames = [(dense_frame(nR, nM, seed + i), nR - nM, nM) for i, (nR, nM) in enumerate(shapes)]
    f, nL, nM = frames[1]
    frames[1] = (infeasible(f, nL, nM), nL, nM)
    frames[-1] = (dense_frame(maxRawRow + 1, 2, seed + 99), maxRawRow - 1, 2)
    return frames


# ---- the permanent and its sampler ----------------------------------------------------------------------------------------------------
class PermanentWide(FrameCase):
    """Frames of sample_check.wide_frame()'s size, 20 x 13: the layers lie in the context's work space (mode 2 of the plan)."""
    name = "permanent_wide"
    grow_to = (22, 15)   # (maxRawRow, maxCol) of the growth request: exponential in maxCol

    def sets(self):
        heavy = lambda s: [(dense_frame(20, 13, s + i), 7, 13) for i in range(3)]  # noqa: E731
        return dict(A=DataSet("A", heavy(1313)), H1=DataSet("H1", heavy(2313)), H2=DataSet("H2", heavy(3313), reverse=True),
                    O=DataSet("O", heavy(4313)),
                    L=DataSet("L", light_frames([(12, 8), (14, 9), (0, 0)], 513, 20), reverse=True, infeasible=1, beyond=2))

    def reference(self, ds, b):
        return pc.permanent_probs(*ds.frames[b])

    def is_infeasible(self, w):
        return w[1] == 0.0 and not w[0].any()

    def slot(self, R, Cm):
        return (R + 2) * (1 << Cm) * 8  # kbest_c.h at kbest_permanent_probs_batch_f64_dev: per frame in flight

    def need_before(self):
        return self.B * self.slot(*self.bounds)

    def need_after(self):
        return self.B * self.slot(*self.grow_to)

    def grow_frames(self):
        R, Cm = self.grow_to
        return [(dense_frame(R, Cm, 7000 + i), R - Cm, Cm) for i in range(self.B)]


class PermanentRagged(PermanentWide):
    """12 ragged frames of 1 .. 12 columns under a work cap of one slot: one workgroup takes them in turn."""
    name = "permanent_ragged"
    grow_to = (20, 14)

    def sets(self):
        def heavy(seed, rows):
            return [(dense_frame(rows[i], i + 1, seed + i), rows[i] - (i + 1), i + 1) for i in range(12)]
        rA = [20, 8, 9, 20, 12, 14, 20, 16, 18, 19, 20, 20]
        rB = [3, 20, 5, 9, 20, 11, 13, 20, 15, 17, 18, 20]
        rC = [20, 2, 20, 4, 6, 20, 7, 9, 20, 10, 20, 12]  # (the last: no landmark at all)
        light = [(dense_frame(6 + i, 1 + i % 5, 900 + i), 6 + i - (1 + i % 5), 1 + i % 5) for i in range(12)]
        f, nL, nM = light[4]  # (10 x 5)
        light[4] = (infeasible(f, nL, nM), nL, nM)
        light[7] = (dense_frame(21, 2, 977), 19, 2)
        return dict(A=DataSet("A", heavy(100, rA)), H1=DataSet("H1", heavy(200, rB)), H2=DataSet("H2", heavy(300, rC), reverse=True),
                    O=DataSet("O", heavy(400, rA)), L=DataSet("L", light, reverse=True, infeasible=4, beyond=7))

    def work_cap(self):
        R, Cm = self.bounds
        return (R * Cm + ((R + 2) << Cm)) * 8 + 64  # one frame in flight (tests/test_gpu_permanent.py)

    def need_before(self):
        return self.slot(*self.bounds)  # (the cap: one frame in flight, and at least one)

    def need_after(self):
        return self.slot(*self.grow_to)


class SampleWide(PermanentWide):
    """The 20 x 13 frame, 256 draws, other keys per data set."""
    name = "sample_wide"
    n_sample = 256

    def sets(self):
        d = super().sets()
        for i, n in enumerate(("A", "H1", "H2", "L", "O")):
            d[n].keys = [(0x9E3779B97F4A7C15 * (7 * i + b + 1)) & (2 ** 63 - 1) for b in range(d[n].B)]
            d[n].seed = sc.SEED  # (a host argument: the capture bakes it in)
        return d

    def reference(self, ds, b):
        f, nL, nM = ds.frames[b]
        return sc.Draws(*sc.sample_assoc(f, nL, nM, self.n_sample, seed=ds.seed, frame_key=ds.keys[b]), self.n_sample)

    def is_infeasible(self, w):
        return w.Z == 0.0 and (w.assign == -1).all()

    def margins(self):
        return {n: min(w.margin for w in self.want(s) if w is not None) for n, s in self.data.items()}


# ---- belief propagation ---------------------------------------------------------------------------------------------------------------
class Belief(FrameCase):
    """30 x 10 frames, tol = 0, 25 sweeps.  lds_limit = 0: a and nu in LDS, no work space of the context in the launch;
    lds_limit = 1024 (tests/test_gpu_lbp.py): a and nu in the work space."""
    tol, max_iter = 0.0, 25
    grow_to = (120, 10)  # linear in maxRawRow * maxCol

    def __init__(self, lds_limit):
        super().__init__()
        self.lds_limit = lds_limit
        self.name = "belief_hbm" if lds_limit else "belief_lds"
        self.holds_work_space = bool(lds_limit)

    def sets(self):
        heavy = lambda s: [(f, 20, 10) for f in wl.kitti_like_frames(4, nL=20, nM=10, seed=s)]  # noqa: E731
        light = [(f, 8, 4) for f in wl.kitti_like_frames(2, nL=8, nM=4, seed=61)] + [None, None]
        light[2] = (infeasible(dense_frame(9, 3, 62), 6, 3), 6, 3)
        light[3] = (dense_frame(31, 2, 63), 29, 2)
        light[1], light[2] = light[2], light[1]
        return dict(A=DataSet("A", heavy(0xC0FFEE)), H1=DataSet("H1", heavy(0xBEEF)), H2=DataSet("H2", heavy(0xF00D), reverse=True),
                    O=DataSet("O", heavy(0xABCD)), L=DataSet("L", light, reverse=True, infeasible=1, beyond=3))

    def reference(self, ds, b):
        return lc.belief_probs(*ds.frames[b], self.tol, self.max_iter)

    def is_infeasible(self, w):
        return w[1] == lc.INFEASIBLE and not w[0].any()

    def slot(self, R, Cm):
        return 32 * R * Cm  # kbest_c.h at kbest_belief_probs_batch_f64_dev: per frame in flight

    def need_before(self):
        return self.B * self.slot(*self.bounds)

    def need_after(self):
        return self.B * self.slot(*self.grow_to)

    def grow_frames(self):
        R, Cm = self.grow_to
        return [(f, R - Cm, Cm) for f in wl.kitti_like_frames(self.B, nL=R - Cm, nM=Cm, seed=77)]


# ---- the clustered tiers ---------------------------------------------------------------------------------------------------------------
SCENE = (40, 24, 24)  # nL, nM, side of workloads.scene_frames: clusters of up to 15 measurements


@functools.lru_cache(maxsize=None)
def scene(F):
    return wl.scene_frames(F, *SCENE)


def scene_light(seed):
    """Five frames for the light set of the clustered cases: small scenes, the second infeasible, the last beyond the bounds."""
    small = wl.scene_frames(3, 12, 6, 8, seed=seed)
    frames = [(f, 12, 6) for f in small] + [(dense_frame(9, 3, seed), 6, 3)]
    f, nL, nM = frames[1]
    frames[1] = (infeasible(f, nL, nM), nL, nM)
    frames.append((dense_frame(SCENE[0] + SCENE[1] + 1, 2, seed + 1), SCENE[0] + SCENE[1] - 1, 2))
    return frames


class Clustered(FrameCase):
    """cluster_check.assembled_frame() plus four scene frames, raw blocks with condition = 1."""
    name = "clustered"
    condition = True
    grow_B = 4  # the growth request: four times the frames in flight (the slot itself is at its largest: 2^16 subsets)

    def sets(self):
        f, nL, nM, _ = cc.assembled_frame()
        asm = (f, nL, nM)
        sc_ = [(x, SCENE[0], SCENE[1]) for x in scene(16)]
        return dict(A=DataSet("A", [asm] + sc_[0:4]), H1=DataSet("H1", sc_[4:6] + [asm] + sc_[6:8]),
                    H2=DataSet("H2", sc_[8:12] + [asm], reverse=True), O=DataSet("O", [asm] + sc_[12:16]),
                    L=DataSet("L", scene_light(31), reverse=True, infeasible=1, beyond=4))

    def reference(self, ds, b):
        f, nL, nM = ds.frames[b]
        cond, idx = ol.condition_costs(f, nL + nM, nM)
        p, lp, info, maxc, lab = cc.clustered_probs(cond, len(idx) - nM, nM)
        return pc.scatter_back(p, idx, nL, nM), lp, info, maxc, lab

    def is_infeasible(self, w):
        return w[2] == 0 and not w[0].any()

    def slot(self, R, Cm):
        return min(cc.SLOT_CAP, (R + 2) * (1 << min(Cm, 16)) * 8) + R * 128  # kbest_c.h at kbest_clustered_probs_batch_f64_dev

    def need_before(self):
        return self.B * self.slot(*self.bounds)

    def need_after(self):
        return self.grow_B * self.B * self.slot(*self.bounds)

    def grow_frames(self):
        return [(x, SCENE[0], SCENE[1]) for x in scene(self.grow_B * self.B)]


class ClusteredSample(Clustered):
    name = "clustered_sample"
    n_sample = 64

    def sets(self):
        d = super().sets()
        for i, n in enumerate(("A", "H1", "H2", "L", "O")):
            d[n].keys = [(0xD1B54A32D192ED03 * (5 * i + b + 1)) & (2 ** 63 - 1) for b in range(d[n].B)]
            d[n].seed = sc.SEED  # (a host argument: the capture bakes it in)
        return d

    def reference(self, ds, b):
        f, nL, nM = ds.frames[b]
        return csc.clustered_sample_assoc(f, nL, nM, self.n_sample, seed=ds.seed, condition=True, frame_key=ds.keys[b])

    def is_infeasible(self, w):
        return w.info == 0 and (w.assign == -1).all()

    def margins(self):
        return {n: min(w.margin for w in self.want(s) if w is not None) for n, s in self.data.items()}


class Partial(Clustered):
    """Four scene frames at max_exact = 4: descriptors, row lists and sub-blocks."""
    name = "clustered_partial"
    max_exact = 4

    def sets(self):
        sc_ = [(x, SCENE[0], SCENE[1]) for x in scene(16)]
        light = scene_light(47)
        del light[3]
        return dict(A=DataSet("A", sc_[0:4]), H1=DataSet("H1", sc_[4:8]), H2=DataSet("H2", sc_[8:12], reverse=True),
                    O=DataSet("O", sc_[12:16]), L=DataSet("L", light, reverse=True, infeasible=1, beyond=3))

    def reference(self, ds, b):
        f, nL, nM = ds.frames[b]
        return hc.hybrid_probs(f, nL, nM, 1, condition=True, max_exact=self.max_exact)

    def is_infeasible(self, w):
        return w[1] == -2 or w[3] == 0

    def open_clusters(self):
        return {n: sum(len(w[2]) for w in self.want(s) if w is not None) for n, s in self.data.items()}


def frame_cases():
    return [PermanentWide(), PermanentRagged(), SampleWide(), Belief(0), Belief(1024), Clustered(), ClusteredSample(), Partial()]


# ---- the one-stream hybrid entries ------------------------------------------------------------------------------------------------------
def open_widths(frame, nL, nM, max_exact):
    """The frontier width W of every open cluster (more than max_exact measurements) of a raw frame under condition = 1, by the
    plan of frontier_check.greedy_plan alone -- no sums."""
    import frontier_check as fc
    X, A = hc.gated_block(frame, nL, nM, True)
    out = []
    for cols, rows in cc.clusters_of(A)[0]:
        if len(cols) > max_exact:
            sub = A[np.ix_(rows, cols)]
            out.append(fc.greedy_plan(fc.row_masks(sub), len(cols))[1])
    return out


class Hybrid(FrameCase):
    """16 scene frames at max_exact = 4: heavy and light are disjoint slices of scene_frames(200, 40, 24, 24); the light set ends
    with an infeasible frame and three frames beyond the bounds.  The clustered work space is capped at two frames in flight for the
    capture: the growth request lifts the cap, so sixteen want a slot."""
    condition = True
    max_exact = 4
    in_flight = 2
    n_sample = 0

    def __init__(self, max_width, name="hybrid_probs"):
        super().__init__()
        self.max_width = max_width
        self.name = f"{name}_w{max_width}"

    def sets(self):
        fr = [(x, SCENE[0], SCENE[1]) for x in wl.scene_frames(200, *SCENE)[:80]]
        light = fr[64:76]
        f, nL, nM = fr[77]  # (its one open cluster has W = 4: at max_width = 5 the frame is infeasible still, not refused)
        light.append((infeasible(f, nL, nM), nL, nM))
        light += [(dense_frame(SCENE[0] + SCENE[1] + 1, 2, 900 + i), SCENE[0] + SCENE[1] - 1, 2) for i in range(3)]
        keys = lambda i: [(0xA0761D6478BD642F * (3 * i + b + 1)) & (2 ** 63 - 1) for b in range(16)]  # noqa: E731
        return dict(A=DataSet("A", fr[0:16], keys(0)), H1=DataSet("H1", fr[16:32], keys(1)),
                    H2=DataSet("H2", fr[32:48], keys(2), reverse=True), O=DataSet("O", fr[48:64], keys(3)),
                    L=DataSet("L", light, keys(4), reverse=True, infeasible=12, beyond=13))

    def widths(self):
        """{set: one list of open-cluster widths per frame inside the bounds}"""
        R, Cm = self.bounds
        return {n: [open_widths(*s.frames[b], self.max_exact) for b in range(s.B) if s.inside(b, R, Cm)] for n, s in self.data.items()}

    def open_clusters(self):
        return {n: sum(len(w) for w in ws) for n, ws in self.widths().items()}

    def light_refused_at(self, max_width):
        """Frames of the light set that hold an open cluster wider than max_width: refused there (method -1)."""
        return [b for b, w in enumerate(self.widths()["L"]) if w and max(w) > max_width]

    def light_conditions(self):
        L = self.data["L"]
        R, Cm = self.bounds
        f, nL, nM = L.frames[L.infeasible]
        return hc.hybrid_probs(f, nL, nM, 1, condition=True, max_exact=self.max_exact)[1] == -2, not L.inside(L.beyond, R, Cm)

    def slot(self, R, Cm):
        return min(cc.SLOT_CAP, (R + 2) * (1 << min(Cm, 16)) * 8) + R * 128  # kbest_c.h at kbest_clustered_probs_batch_f64_dev

    def work_cap(self):
        return self.in_flight * self.slot(*self.bounds) + 64

    def need_before(self):
        return self.in_flight * self.slot(*self.bounds)

    def need_after(self):
        return self.B * self.slot(*self.bounds)

    def grow_frames(self):
        return self.data["O"].frames


class HybridSample(Hybrid):
    n_sample = 16

    def __init__(self, max_width):
        super().__init__(max_width, "hybrid_sample")


# ---- kbest_batch_f64_dev: three more routes ------------------------------------------------------------------------------------------
class KBestRoute:
    """Uniform batches: the shapes are host arguments, the data sets differ in the costs.  The light set: problem 1 infeasible (a column
    of +inf: nf = 0), problem 2 with fewer than k assignments, the rest with a third of the entries at +inf."""

    def __init__(self, name, B, N, M, k, integer=0, reference_order=False, grow=(64, 4)):
        self.name, self.Bn, self.N, self.M, self.k, self.integer, self.reference_order, self.grow = name, B, N, M, k, integer, reference_order, grow
        self._want = {}

    @functools.cached_property
    def data(self):
        out = {}
        for i, n in enumerate(("A", "H1", "H2", "L", "O")):
            rng = np.random.default_rng(1000 * self.N + 10 * self.k + i)
            c = rng.integers(0, self.integer, (self.Bn, self.N * self.M)).astype(np.float64) if self.integer else rng.random((self.Bn, self.N * self.M)) * 10.0
            if n == "L":
                c[rng.random(c.shape) < 1.0 / 3.0] = np.inf
                c[1, : self.N] = np.inf  # column-major N x M: the first column
                few = np.full((self.N, self.M), np.inf)
                few[: self.M, :] = np.where(np.eye(self.M, dtype=bool), 1.0, np.inf)
                few[0, 1], few[1, 0] = 2.0, 3.0  # two assignments in all
                c[2] = np.ascontiguousarray(few.T).reshape(-1)
            out[n] = types.SimpleNamespace(name=n, costs=c, seed=0)
        return out

    def want(self, ds):
        """(nf, row4col, col4row, gain) of the checker.  Computed once per set, never changed."""
        if ds.name not in self._want:
            self._want[ds.name] = ol.orc_kbest_batch(ds.costs, self.N, self.M, self.k)[:4]
        return self._want[ds.name]

    def light_conditions(self):
        nf = self.want(self.data["L"])[0]
        return nf[1] == 0, 0 < nf[2] < self.k

    def record(self):
        return 18 * self.N + 24  # kbest_c.h at kbest_reserve: bytes of one hypothesis record

    def need_before(self):
        """The most the header lets the hypothesis states of the capture's reservation be; the reference-order route: its own work space."""
        if self.reference_order:
            return self.Bn * (8 * self.N * self.N + (2 + (self.k - 1) * self.M) * 25 * self.N)
        return self.Bn * (self.k + 1 + 64 + 1024) * self.record()

    def need_after(self):
        """The least the growth request (grow[0] x the batch, grow[1] x k) needs."""
        B, k = self.grow[0] * self.Bn, self.grow[1] * self.k
        if self.reference_order:
            return B * (8 * self.N * self.N + (2 + (k - 1) * self.M) * 25 * self.N)
        return B * (k + 64) * self.record()

    def growth_premise(self):
        before, after = self.need_before(), self.need_after()
        allocated = -(-before // (2 << 20)) * (2 << 20) if self.reference_order else before + before // 64  # (+ the slot tables)
        return after >= 4 * before and after > allocated


def kbest_cases():
    return [KBestRoute("kbest_general_size", 6, 80, 80, 20), KBestRoute("kbest_small_problem", 50, 24, 9, 20),
            KBestRoute("kbest_reference_order", 4, 12, 12, 20, integer=6, reference_order=True, grow=(16, 8))]


# ---- the fused association entry ---------------------------------------------------------------------------------------------------------
class Assoc(FrameCase):
    """kbest_assoc_probs_batch_f64_dev, k = 200.  4 frames of 10 + 10: the bounded walk, with the all-equal frame of
    tests/test_gpu_round4.py in every heavy set so that the second launch has work.  4 frames of 20 + 20: the fused kernel; there the
    light set's last frame keeps more than 32 rows under conditionCosts (d_nf = -2, zeros: the entry's documented limit)."""
    condition = True
    k = 200

    def __init__(self, n):
        super().__init__()
        self.n = n
        self.name = f"assoc_{n}_{n}"

    def all_equal(self):
        n = self.n
        flat = np.full(2 * n * n, np.inf)
        for c in range(n):
            flat[c * 2 * n: c * 2 * n + n] = 1.0
            flat[c * 2 * n + n + c] = 1.0
        return flat

    def sets(self):
        n = self.n

        def heavy(seed, at):
            fr = [(f, n, n) for f in wl.kitti_like_frames(4, nL=n, nM=n, seed=seed)]
            if n == 10:
                fr[at] = (self.all_equal(), n, n)
            return fr
        small = n // 2
        light = [(f, small + 1, small) for f in wl.kitti_like_frames(3, nL=small + 1, nM=small, seed=71)]
        f, nL, nM = light[1]
        light[1] = (infeasible(f, nL, nM), nL, nM)
        light.append((dense_frame(2 * n, n, 72), n, n) if n == 20 else (wl.kitti_like_frames(1, nL=3, nM=2, seed=73)[0], 3, 2))
        return dict(A=DataSet("A", heavy(5, 1)), H1=DataSet("H1", heavy(6, 3)), H2=DataSet("H2", heavy(7, 0), reverse=True),
                    O=DataSet("O", heavy(8, 2)), L=DataSet("L", light, reverse=True, infeasible=1, beyond=3 if n == 20 else None))

    def reference(self, ds, b):
        f, nL, nM = ds.frames[b]
        if n_equal(f):
            return None  # (all costs equal: the columns sum to 1 and nf = k -- tests/test_gpu_round4.py)
        cond, idx = ol.condition_costs(f, nL + nM, nM)
        if len(idx) > 32:
            return "beyond"
        po, nf = ol.assignment_prob(cond, len(idx) - nM, nM, self.k)
        return pc.scatter_back(po, idx, nL, nM), int(nf)

    def light_conditions(self):
        L = self.data["L"]
        w = self.want(L)
        return w[L.infeasible][1] == 0, L.beyond is None or w[L.beyond] == "beyond"

    grow = (64, 4)  # x the frames, x k

    def need_before(self):
        """kbest_c.h at kbest_reserve (the same work space): [B][k + 1 + 64 + up to 1 024] records; the most B frames take."""
        return self.B * (self.k + 1 + 64 + 1024) * (18 * 32 + 24)

    def need_after(self):
        """The least the growth request takes: records of the same size (the same frame shape), none of the up-to-1 024."""
        return self.grow[0] * self.B * (self.grow[1] * self.k + 64) * (18 * 32 + 24)

    def growth_premise(self):
        return self.need_after() >= 4 * self.need_before()

    def grow_frames(self):
        return [(f, self.n, self.n) for f in wl.kitti_like_frames(self.grow[0] * self.B, nL=self.n, nM=self.n, seed=74)]


def n_equal(f):
    fin = f[np.isfinite(f)]
    return fin.size > 0 and (fin == fin[0]).all()


def assoc_cases():
    return [Assoc(10), Assoc(20)]


def hybrid_cases():
    return [Hybrid(16), Hybrid(5), HybridSample(16)]


# ---- the entries that take their shapes, offsets and keys from host arrays at enqueue time -------------------------------------------
class ClusterList:
    """A list of clusters of FIXED shapes [(nL_k, m)] (host arguments, baked into the capture): the data sets differ in the sub-blocks
    -- which entries are finite and what they cost -- and, for the sampler, in the row keys.  The light set is sparser (smaller
    frontiers) and its cluster `dead` has a column without a finite entry: infeasible."""
    shapes = ()
    dead = 0
    n_sample = 0
    holds_work_space = True

    def __init__(self):
        self._want = {}

    def block(self, j, seed, p, dead=False):
        import frontier_check as fc
        nLk, m = self.shapes[j]
        rng = np.random.default_rng(seed)
        land = np.where(rng.random((nLk, m)) < p, 0.1 + rng.random((nLk, m)) * 3.0, np.inf)
        miss = np.ones(m, bool)
        if dead:
            land[:, 0] = np.inf
            miss[0] = False
        return fc.with_miss_rows(land, rng, miss=miss)[0]

    def first_set(self):
        return [self.block(j, 11 + j, 1.0) for j in range(len(self.shapes))]

    @functools.cached_property
    def data(self):
        n = len(self.shapes)
        out = {"A": self.first_set()}
        for i, name in enumerate(("H1", "H2", "O")):
            out[name] = [self.block(j, 100 * (i + 1) + j, 1.0) for j in range(n)]
        out["L"] = [self.block(j, 900 + j, 0.5, dead=j == self.dead) for j in range(n)]
        return {name: types.SimpleNamespace(name=name, blocks=b, seed=0, keys=[np.arange(nLk + m, dtype=np.int32) + 7 * (i + 1)
                                                                                for nLk, m in self.shapes])
                for i, (name, b) in enumerate(out.items())}

    def reference(self, ds, j):
        raise NotImplementedError

    def want(self, ds):
        if ds.name not in self._want:
            self._want[ds.name] = [self.reference(ds, j) for j in range(len(self.shapes))]
        return self._want[ds.name]

    def margins(self):
        return {}

    def growth_premise(self):
        before, after = self.need_before(), self.need_after()
        return after >= 4 * before and after > pow2_at_least(before)


class BigCluster(ClusterList):
    """Two clusters of 10 and 12 measurements: one launch per row each way, a long chain."""
    name = "bigcluster"
    shapes = ((8, 10), (9, 12))
    dead = 1
    grow_to = (14, 23)  # (maxM, maxRows): exponential in maxM

    def reference(self, ds, j):
        import bigcluster_check as bc
        return bc.big_cluster(ds.blocks[j], *self.shapes[j])

    def is_infeasible(self, w):
        return w[2] == 0 and not w[0].any()

    def layers(self, maxM, maxRows):
        return (maxRows + 3) * (1 << maxM) * 8  # kbest_c.h at kbest_bigcluster_probs_f64_dev

    def need_before(self):
        return self.layers(max(m for _, m in self.shapes), max(l + m for l, m in self.shapes))

    def need_after(self):
        return self.layers(*self.grow_to)


class Frontier(ClusterList):
    """tests/test_gpu_frontier.py's "fewer_states_than_a_wave" and "more_states_than_the_workgroup" as one list of clusters."""
    name = "frontier"
    shapes = ((5, 4), (2, 12))
    grow_n = 4  # the growth request: four times the clusters in flight

    def first_set(self):
        import frontier_check as fc
        e = fc.edge_clusters()
        got = [e["fewer_states_than_a_wave"], e["more_states_than_the_workgroup"]]
        assert tuple((l, m) for _, l, m in got) == self.shapes
        return [b for b, _, _ in got]

    def block(self, j, seed, p, dead=False):
        return super().block(j, seed, 0.6 * p if j == 0 else p, dead)

    def reference(self, ds, j):
        import frontier_check as fc
        return fc.frontier_cluster(ds.blocks[j], *self.shapes[j])

    def is_infeasible(self, w):
        return w[2] == 0 and not w[0].any()

    def widths(self):
        return {n: [w[3] for w in self.want(s)] for n, s in self.data.items()}

    def need(self, n):
        import frontier_check as fc
        return n * fc.SLOT  # kbest_c.h at kbest_frontier_probs_f64_dev: a slot for each of the clusters in flight (the plans are small)

    def need_before(self):
        return self.need(len(self.shapes))

    def need_after(self):
        return self.need(self.grow_n * len(self.shapes))


class FrontierSample(Frontier):
    name = "frontier_sample"
    n_sample = 16
    frame_keys = (0x9E3779B97F4A7C15, 0x0123456789ABCDEF)

    def reference(self, ds, j):
        import frontier_sample_check as fsc
        return fsc.sample_cluster(ds.blocks[j], *self.shapes[j], ds.keys[j], self.n_sample, sc.SEED, self.frame_keys[j], 0)

    def is_infeasible(self, w):
        return w[3] == 0 and (w[0] == -1).all()

    def widths(self):
        return {n: [w[4] for w in self.want(s)] for n, s in self.data.items()}

    def margins(self):
        return {n: min(w[5] for w in self.want(s)) for n, s in self.data.items()}


class TableSample:
    """3 tables of the k = 50 best assignments (the checker's, within the cutoff 42), 64 draws, with d_pick.  The tables are device
    data; the light set's tables are short (small problems) and its second one is empty (nf = 0).  No work space, no reservation."""
    name = "table_sample"
    k, n_sample, max_col = 50, 64, 6
    m = (4, 5, 6)
    cluster_key, frame_key = (3, 70000, 5), (11, 0x0123456789ABCDEF, 13)
    holds_work_space = False

    def __init__(self):
        self._want = {}

    def table(self, j, seed, rows):
        m = self.m[j]
        rng = np.random.default_rng(seed)
        blk = rng.random(rows * m) * 8.0
        nf, r4c, _, g = ol.orc_kbest(blk, rows, m, self.k, cutoff=42.0)
        tab = np.full((self.k, self.max_col), -1, np.int32)
        gain = np.full(self.k, np.nan)
        tab[:nf, :m] = np.asarray(r4c)[:nf, :m]
        gain[:nf] = np.asarray(g)[:nf]
        return tab, gain, int(nf)

    @functools.cached_property
    def data(self):
        out = {}
        for i, name in enumerate(("A", "H1", "H2", "O", "L")):
            t = [self.table(j, 50 * i + j, (self.m[j] if name == "L" else self.m[j] + 3)) for j in range(3)]
            if name == "L":
                t[1] = (t[1][0], t[1][1], 0)
            out[name] = types.SimpleNamespace(name=name, seed=0, tab=np.stack([x[0] for x in t]), gain=np.stack([x[1] for x in t]),
                                              nf=np.array([x[2] for x in t], np.int32))
        return out

    def want(self, ds):
        import table_sample_check as tsc
        if ds.name not in self._want:
            self._want[ds.name] = [tsc.sample_tables(ds.tab[j], ds.gain[j], ds.nf[j], self.n_sample, sc.SEED, self.cluster_key[j],
                                                     self.frame_key[j], 0, m=self.m[j]) for j in range(3)]
        return self._want[ds.name]

    def margins(self):
        return {n: min(w[3] for w in self.want(s)) for n, s in self.data.items()}


def list_cases():
    return [BigCluster(), Frontier(), FrontierSample(), TableSample()]
