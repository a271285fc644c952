"""GPU: every asynchronous device entry inside a graph capture -- captured once on one stream, replayed on new data in the same
buffers, against the restatement the entry's own GPU test file uses (tests/graph_capture_lib.py holds data and references), never
against an eager launch of the code under test.

The protocol of a case (run_protocol): a fresh context; every device tensor allocated and the work space reserved before the capture;
data set A launched eagerly on a side stream and compared; the identical call captured; replays on H1 (heavy), L (light: smaller frames,
an infeasible one, one beyond the launch bounds), H2 (heavy, slices in reverse order) and A again, the last two back to back with
nothing but the input copy in between; before every other replay every output is filled with the sentinel of the entry's own test
file.  Between L and H2 one eager launch of the same entry and context into other buffers.  Then the growth step: the entry's own
reservation and its host-buffer entry are asked for a work space that must grow (graph_capture_lib asserts that premise from the
header's formulas); both must be refused with KBEST_ERR_BAD_ARG and a text that says "captured", and only then the graph is replayed
once more.  A case whose captured launch holds no work space of the context (belief propagation with a and nu in LDS) has nothing
to refuse: there the reservation must succeed, and the replay behind it must still be right."""
import numpy as np
import pytest

import graph_capture_lib as gl
import probabilisticsemslam_amd as pk

BAD_ARG_TEXT = "bad argument"  # kbest_strerror(KBEST_ERR_BAD_ARG): the wrapper raises it in front of kbest_last_error


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


class Buffers:
    """The device tensors of one frame batch: inputs sized for the largest data set, outputs with their sentinels."""

    def __init__(self, case, outputs):
        import torch
        self.torch, self.case = torch, case
        dev = torch.device("cuda", 0)
        caps, B = case.caps(), case.B
        z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
        self.nL, self.nM, self.nRow = z(B, torch.int32), z(B, torch.int32), z(B, torch.int32)
        self.coff, self.poff, self.aoff, self.loff, self.key = (z(B, torch.int64) for _ in range(5))
        self.cost = z(caps["cost"], torch.float64)
        self.caps = caps
        self.out, self.sentinel = {}, {}
        for name, (shape, dt, fill) in outputs(case, caps).items():
            self.out[name] = torch.full(shape, fill, dtype=dt, device=dev)
            self.sentinel[name] = fill

    def load(self, ds):
        """The input copy: the data set into the input tensors (on the current stream)."""
        t = self.torch.from_numpy
        n = max(self.case.n_sample, 1)
        self.nL.copy_(t(ds.nL)); self.nM.copy_(t(ds.nM)); self.nRow.copy_(t(ds.nL + ds.nM))
        self.coff.copy_(t(ds.offsets(ds.cost_sizes))); self.poff.copy_(t(ds.offsets(ds.prob_sizes)))
        self.aoff.copy_(t(ds.offsets(ds.nM.astype(np.int64) * n))); self.loff.copy_(t(ds.offsets(np.full(ds.B, n, np.int64))))
        self.key.copy_(t(np.asarray(ds.keys, np.uint64).view(np.int64)))
        self.cost.copy_(t(ds.flat_cost(self.caps["cost"])))

    def fill(self):
        for name, tns in self.out.items():
            tns.fill_(self.sentinel[name])

    def read(self):
        return {name: tns.cpu().numpy() for name, tns in self.out.items()}


def slices(ds, flat, sizes, shape_of):
    off = ds.offsets(sizes)
    return [flat[off[b]: off[b] + int(sizes[b])].reshape(shape_of(b)) for b in range(ds.B)]


def untouched_outside(ds, case, flat, sizes, fill):
    """Everything of `flat` outside the slices of the frames inside the bounds still holds the sentinel."""
    R, Cm = case.bounds
    mask = np.ones(flat.size, bool)
    off = ds.offsets(sizes)
    for b in range(ds.B):
        if ds.inside(b, R, Cm):
            mask[off[b]: off[b] + int(sizes[b])] = False
    rest = flat[mask]
    assert (rest == fill).all() or (np.isnan(fill) and np.isnan(rest).all()), ds.name


# ---- the entries: outputs with the sentinels of their own test files, the launch, the comparison ------------------------------------------
class PermanentEntry:
    @staticmethod
    def outputs(case, caps):
        import torch
        return dict(probs=((caps["prob"],), torch.float64, -1.0), perm=((case.B,), torch.float64, -1.0))

    @staticmethod
    def setup(eng, case):
        if hasattr(case, "work_cap"):
            eng.set_permanent_work_cap(case.work_cap())

    @staticmethod
    def reserve(eng, case, B, R, Cm):
        eng.reserve_permanent(B, R, Cm)

    @staticmethod
    def launch(eng, case, b, stream):
        R, Cm = case.bounds
        eng.permanent_probs_dev(case.B, R, Cm, b.nL, b.nM, b.cost, b.coff, b.out["probs"], b.poff, b.out["perm"], condition=case.condition,
                                stream=stream, reserve=False)
        if hasattr(case, "work_cap"):
            assert eng.last_permanent_grid() == 1  # the cap took effect: one workgroup takes the frames in turn

    @staticmethod
    def host(eng, case, frames):
        eng.permanent_probs([f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames])

    @staticmethod
    def check(case, ds, got, filled):
        want = case.want(ds)
        probs = slices(ds, got["probs"], ds.prob_sizes, lambda b: (int(ds.nM[b]), int(ds.nL[b]) + 1))
        for b, w in enumerate(want):
            if w is None:  # beyond the bounds: perm = 0, its probs are left alone (kbest_c.h)
                assert got["perm"][b] == 0.0, (ds.name, b)
                continue
            np.testing.assert_allclose(probs[b], w[0], rtol=0, atol=1e-12, err_msg=f"{ds.name} {b}")
            np.testing.assert_allclose(got["perm"][b], w[1], rtol=1e-12, atol=0, err_msg=f"{ds.name} {b}")
        if filled:
            untouched_outside(ds, case, got["probs"], ds.prob_sizes, -1.0)


class SampleEntry(PermanentEntry):
    @staticmethod
    def outputs(case, caps):
        import torch
        return dict(asg=((caps["asg"],), torch.int32, -9), lp=((case.B * case.n_sample,), torch.float64, -9.0),
                    perm=((case.B,), torch.float64, -9.0))

    @staticmethod
    def reserve(eng, case, B, R, Cm):
        eng.reserve_sample(B, R, Cm)

    @staticmethod
    def launch(eng, case, b, stream):
        R, Cm = case.bounds
        eng.sample_assoc_dev(case.B, R, Cm, b.nL, b.nM, b.cost, b.coff, case.n_sample, b.out["asg"], b.aoff, b.out["lp"], b.loff,
                             b.out["perm"], seed=b.seed, d_frameKey=b.key, condition=case.condition, stream=stream, reserve=False)

    @staticmethod
    def host(eng, case, frames):
        eng.sample_assoc([f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames], 4)

    @staticmethod
    def check(case, ds, got, filled):
        n = case.n_sample
        want = case.want(ds)
        asg = slices(ds, got["asg"], ds.nM.astype(np.int64) * n, lambda b: (n, int(ds.nM[b])))
        lp = slices(ds, got["lp"], np.full(ds.B, n, np.int64), lambda b: (n,))
        for b, w in enumerate(want):
            if w is None:  # beyond the bounds: perm = 0, assign and logProb are left alone
                assert got["perm"][b] == 0.0, (ds.name, b)
                continue
            assert w.margin >= gl.MIN_MARGIN, (ds.name, b, w.margin)
            assert np.array_equal(asg[b], w.assign), (ds.name, b)
            if w.Z > 0.0:
                assert np.abs(lp[b] - w.logp).max() <= 1e-12, (ds.name, b)
                assert abs(got["perm"][b] - w.Z) <= 1e-12 * w.Z, (ds.name, b)
            else:
                assert np.isnan(lp[b]).all() and got["perm"][b] == 0.0, (ds.name, b)
        if filled:
            untouched_outside(ds, case, got["asg"], ds.nM.astype(np.int64) * n, -9)
            untouched_outside(ds, case, got["lp"], np.full(ds.B, n, np.int64), -9.0)


class BeliefEntry:
    @staticmethod
    def outputs(case, caps):
        import torch
        return dict(probs=((caps["prob"],), torch.float64, -1.0), iters=((case.B,), torch.int32, -77), resid=((case.B,), torch.float64, -1.0))

    @staticmethod
    def setup(eng, case):
        eng.set_belief_lds_limit(case.lds_limit)

    @staticmethod
    def reserve(eng, case, B, R, Cm):
        eng.reserve_belief(B, R, Cm)

    @staticmethod
    def launch(eng, case, b, stream):
        R, Cm = case.bounds
        eng.belief_probs_dev(case.B, R, Cm, b.nL, b.nM, b.cost, b.coff, b.out["probs"], b.poff, b.out["iters"], b.out["resid"],
                             tol=case.tol, max_iter=case.max_iter, stream=stream, reserve=False)

    @staticmethod
    def host(eng, case, frames):
        eng.belief_probs([f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames], tol=0.0, max_iter=2)

    @staticmethod
    def check(case, ds, got, filled):
        want = case.want(ds)
        probs = slices(ds, got["probs"], ds.prob_sizes, lambda b: (int(ds.nM[b]), int(ds.nL[b]) + 1))
        for b, w in enumerate(want):
            if w is None:  # beyond the bounds: iters = -1, its probs are left alone
                assert got["iters"][b] == -1, (ds.name, b)
                continue
            q, wi, wr = w
            assert not np.isnan(probs[b]).any() and np.abs(probs[b] - q).max() <= 1e-12, (ds.name, b)
            assert got["iters"][b] == wi, (ds.name, b, got["iters"][b], wi)
            if wi != gl.lc.INFEASIBLE:
                assert wi == case.max_iter and abs(got["resid"][b] - wr) <= 1e-12, (ds.name, b)
        if filled:
            untouched_outside(ds, case, got["probs"], ds.prob_sizes, -1.0)


class ClusteredEntry:
    @staticmethod
    def outputs(case, caps):
        import torch
        B, Cm = case.B, case.bounds[1]
        return dict(probs=((caps["prob"],), torch.float64, -5.0), lp=((B,), torch.float64, -5.0), info=((B,), torch.int32, -77),
                    maxc=((B,), torch.int32, -77), label=((B, Cm), torch.int32, -77))

    @staticmethod
    def setup(eng, case):
        pass

    @staticmethod
    def reserve(eng, case, B, R, Cm):
        eng.reserve_clustered(B, R, Cm)

    @staticmethod
    def launch(eng, case, b, stream):
        R, Cm = case.bounds
        eng.clustered_probs_dev(case.B, R, Cm, b.nL, b.nM, b.cost, b.coff, b.out["probs"], b.poff, b.out["lp"], b.out["info"],
                                b.out["maxc"], b.out["label"], Cm, condition=case.condition, stream=stream, reserve=False)

    @staticmethod
    def host(eng, case, frames):
        eng.clustered_probs([f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames], condition=True)

    @staticmethod
    def check(case, ds, got, filled):
        want = case.want(ds)
        probs = slices(ds, got["probs"], ds.prob_sizes, lambda b: (int(ds.nM[b]), int(ds.nL[b]) + 1))
        for b, w in enumerate(want):
            if w is None:  # beyond the bounds: info = -1, left alone
                assert got["info"][b] == -1, (ds.name, b)
                if filled:
                    assert got["maxc"][b] == -77 and got["lp"][b] == -5.0, (ds.name, b)
                continue
            p, lp, info, maxc, lab = w
            assert got["info"][b] == info and got["maxc"][b] == maxc, (ds.name, b, got["info"][b], info)
            np.testing.assert_array_equal(got["label"][b][: ds.nM[b]], lab, err_msg=f"{ds.name} {b}")
            assert np.abs(probs[b] - p).max() <= 1e-12, (ds.name, b)
            if info > 0:
                assert abs(got["lp"][b] - lp) <= 1e-12 * info, (ds.name, b)  # (1e-12 per cluster: tests/test_gpu_clustered.py)
            else:
                assert got["lp"][b] == -np.inf and not probs[b].any(), (ds.name, b)
        if filled:
            untouched_outside(ds, case, got["probs"], ds.prob_sizes, -5.0)


class ClusteredSampleEntry(ClusteredEntry):
    @staticmethod
    def outputs(case, caps):
        import torch
        B = case.B
        return dict(asg=((caps["asg"],), torch.int32, -9), lp=((B * case.n_sample,), torch.float64, -9.0),
                    logperm=((B,), torch.float64, -9.0), info=((B,), torch.int32, -9), maxc=((B,), torch.int32, -9))

    @staticmethod
    def reserve(eng, case, B, R, Cm):
        eng.reserve_clustered_sample(B, R, Cm)

    @staticmethod
    def launch(eng, case, b, stream):
        R, Cm = case.bounds
        eng.clustered_sample_assoc_dev(case.B, R, Cm, b.nL, b.nM, b.cost, b.coff, case.n_sample, b.out["asg"], b.aoff, b.out["lp"], b.loff,
                                       b.out["logperm"], b.out["info"], b.out["maxc"], seed=b.seed, d_frameKey=b.key,
                                       condition=case.condition, stream=stream, reserve=False)

    @staticmethod
    def host(eng, case, frames):
        eng.clustered_sample_assoc([f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames], 4, condition=True)

    @staticmethod
    def check(case, ds, got, filled):
        n = case.n_sample
        want = case.want(ds)
        asg = slices(ds, got["asg"], ds.nM.astype(np.int64) * n, lambda b: (n, int(ds.nM[b])))
        lp = slices(ds, got["lp"], np.full(ds.B, n, np.int64), lambda b: (n,))
        for b, w in enumerate(want):
            if w is None:  # beyond the bounds: info = -1, nothing else of it is touched
                assert got["info"][b] == -1, (ds.name, b)
                if filled:
                    assert got["maxc"][b] == -9 and got["logperm"][b] == -9.0, (ds.name, b)
                continue
            assert w.margin >= gl.MIN_MARGIN, (ds.name, b, w.margin)
            assert got["info"][b] == w.info and got["maxc"][b] == w.maxc, (ds.name, b)
            assert np.array_equal(asg[b], w.assign), (ds.name, b)
            if w.info > 0:
                assert np.abs(lp[b] - w.logp).max() <= 1e-12, (ds.name, b)
                assert abs(got["logperm"][b] - w.logperm) <= 1e-12 * max(1.0, abs(w.logperm)), (ds.name, b)  # (tests/test_gpu_cluster_sample.py)
            else:
                assert np.isnan(lp[b]).all() and got["logperm"][b] == -np.inf, (ds.name, b)
        if filled:
            untouched_outside(ds, case, got["asg"], ds.nM.astype(np.int64) * n, -9)
            untouched_outside(ds, case, got["lp"], np.full(ds.B, n, np.int64), -9.0)


class PartialEntry(ClusteredEntry):
    @staticmethod
    def outputs(case, caps):
        import torch
        B, (R, Cm) = case.B, case.bounds
        i32 = lambda *shape: (shape, torch.int32, -77)  # noqa: E731
        return dict(probs=((caps["prob"],), torch.float64, -5.0), sub=((caps["cost"],), torch.float64, -7.0), lp=((B,), torch.float64, -5.0),
                    info=i32(B), maxc=i32(B), nopen=i32(B), label=i32(B, Cm), desc=i32(B, Cm, 4), rows=i32(B, R))

    @staticmethod
    def launch(eng, case, b, stream):
        R, Cm = case.bounds
        o = b.out
        eng.clustered_partial_dev(case.B, R, Cm, b.nL, b.nM, b.cost, b.coff, o["probs"], b.poff, o["nopen"], o["desc"], Cm, o["rows"], R,
                                  o["sub"], max_exact=case.max_exact, d_logPerm=o["lp"], d_info=o["info"], d_maxCluster=o["maxc"],
                                  d_label=o["label"], labelStride=Cm, condition=case.condition, stream=stream, reserve=False)

    @staticmethod
    def check(case, ds, got, filled):
        """tests/test_gpu_hybrid.py, check_handed_out: descriptors, row lists and sub-blocks bit for bit; the answered clusters'
        columns against the restatement."""
        want = case.want(ds)
        probs = slices(ds, got["probs"], ds.prob_sizes, lambda b: (int(ds.nM[b]), int(ds.nL[b]) + 1))
        sub = slices(ds, got["sub"], ds.cost_sizes, lambda b: (-1,))
        for b, w in enumerate(want):
            if w is None:  # beyond the bounds: info -1, nothing open, nothing written
                assert got["info"][b] == -1 and got["nopen"][b] == 0, (ds.name, b)
                continue
            wp, method, opens, info, maxc, lab = w
            assert got["nopen"][b] == len(opens) and got["info"][b] == info and got["maxc"][b] == maxc, (ds.name, b)
            np.testing.assert_array_equal(got["label"][b][: ds.nM[b]], lab, err_msg=f"{ds.name} {b}")
            sub_at = row_at = 0
            op = np.zeros(int(ds.nM[b]), bool)
            for j, o in enumerate(opens):
                assert got["desc"][b, j].tolist() == [o["root"], o["m"], o["nL"], o["R"]], (ds.name, b, j)
                n = o["block"].size
                assert np.array_equal(bits(sub[b][sub_at: sub_at + n]), bits(o["block"])), (ds.name, b, j)
                np.testing.assert_array_equal(got["rows"][b, row_at: row_at + o["nL"]], o["rows"], err_msg=f"{ds.name} {b} {j}")
                sub_at += n
                row_at += o["nL"]
                op[o["cols"]] = True
                assert not probs[b][o["cols"]].any(), (ds.name, b, j)  # the columns of open clusters stay 0.0
            if filled:
                assert (sub[b][sub_at:] == -7.0).all() and (got["rows"][b, row_at:] == -77).all(), (ds.name, b)
                assert (got["desc"][b, len(opens):] == -77).all(), (ds.name, b)
            if info > 0:
                assert np.abs(probs[b][~op] - wp[~op]).max(initial=0.0) <= 1e-12, (ds.name, b)
            else:
                assert not probs[b].any(), (ds.name, b)
        if filled:
            untouched_outside(ds, case, got["probs"], ds.prob_sizes, -5.0)
            untouched_outside(ds, case, got["sub"], ds.cost_sizes, -7.0)


class HybridEntry:
    """The yardstick is the host entry's bits (tests/test_gpu_hybrid_dev.py), from a context of its own: a host-buffer call of the
    capturing context is part of the growth step, not of the reference."""
    _host = {}

    @staticmethod
    def outputs(case, caps):
        import torch
        B = case.B
        i32 = lambda *shape: (shape, torch.int32, -77)  # noqa: E731
        return dict(probs=((caps["prob"],), torch.float64, -5.0), sub=((caps["cost"],), torch.float64, -5.0), lp=((B,), torch.float64, -5.0),
                    method=i32(B), nopen=i32(B), nfr=i32(B), maxc=i32(B))

    @staticmethod
    def setup(eng, case):
        eng.set_clustered_work_cap(case.work_cap())  # (lifted for the growth step)

    @staticmethod
    def reserve(eng, case, B, R, Cm):
        eng.reserve_hybrid_dev(B, R, Cm)

    @staticmethod
    def launch(eng, case, b, stream):
        R, Cm = case.bounds
        o = b.out
        eng.hybrid_frontier_probs_dev(case.B, R, Cm, b.nL, b.nM, b.cost, b.coff, o["sub"], o["probs"], b.poff, o["method"], o["lp"], o["nopen"],
                                      o["nfr"], o["maxc"], condition=True, max_exact=case.max_exact, max_width=case.max_width,
                                      stream=stream, reserve=False)

    @staticmethod
    def grow(eng, case):
        R, Cm = case.bounds
        fr = case.grow_frames()

        def lift_and_reserve():
            eng.set_clustered_work_cap(0)
            eng.reserve_hybrid_dev(case.B, R, Cm)
        return [lift_and_reserve, lambda: eng.hybrid_frontier_probs([f[0] for f in fr], [f[1] for f in fr], [f[2] for f in fr], 0, condition=True,
                                                                    max_exact=case.max_exact, max_big=0, max_width=case.max_width)]

    @classmethod
    def host(cls, case, ds):
        """The host entry on the frames of the set inside the bounds: {frame: (probs, method, nOpen, nFrontier, maxCluster, logPerm)}."""
        key = (case.name, ds.name)
        if key not in cls._host:
            R, Cm = case.bounds
            idx = [b for b in range(ds.B) if ds.inside(b, R, Cm)]
            ref = pk.KBestEngine(0)
            try:
                out, method, nOpen, nBig, maxc, lp, nFr = ref.hybrid_frontier_probs(
                    [ds.frames[b][0] for b in idx], [ds.frames[b][1] for b in idx], [ds.frames[b][2] for b in idx], 0, condition=True,
                    max_exact=case.max_exact, max_big=0, max_width=case.max_width)
            finally:
                ref.close()
            assert not nBig.any()
            cls._host[key] = {b: (out[j], method[j], nOpen[j], nFr[j], maxc[j], lp[j]) for j, b in enumerate(idx)}
        return cls._host[key]

    @classmethod
    def check(cls, case, ds, got, filled):
        want = cls.host(case, ds)
        probs = slices(ds, got["probs"], ds.prob_sizes, lambda b: (int(ds.nM[b]), int(ds.nL[b]) + 1))
        for b in range(ds.B):
            if b not in want:  # beyond the bounds: method -1, nOpen and nFrontier 0, logPerm NaN; slice and maxCluster untouched
                assert (got["method"][b], got["nopen"][b], got["nfr"][b]) == (-1, 0, 0) and np.isnan(got["lp"][b]), (ds.name, b)
                if filled:
                    assert got["maxc"][b] == -77, (ds.name, b)
                continue
            p, method, nOpen, nFr, maxc, lp = want[b]
            assert np.array_equal(bits(probs[b]), bits(p)), (ds.name, b)
            assert (got["method"][b], got["nopen"][b], got["nfr"][b], got["maxc"][b]) == (method, nOpen, nFr, maxc), (ds.name, b)
            assert bits(got["lp"][b: b + 1])[0] == bits(np.array([lp]))[0] or (np.isnan(got["lp"][b]) and np.isnan(lp)), (ds.name, b)
        if ds.infeasible is not None:
            assert got["method"][ds.infeasible] == -2, ds.name
        if ds.name == "L" and case.max_width == 5:
            assert sum(1 for b in want if want[b][1] == -1) >= 1  # (the refusal mix)
        if filled:
            untouched_outside(ds, case, got["probs"], ds.prob_sizes, -5.0)


class HybridSampleEntry(HybridEntry):
    _host = {}

    @staticmethod
    def outputs(case, caps):
        import torch
        B = case.B
        i32 = lambda *shape: (shape, torch.int32, -77)  # noqa: E731
        return dict(asg=i32(caps["asg"]), lp=((B * case.n_sample,), torch.float64, -5.0), sub=((caps["cost"],), torch.float64, -5.0),
                    logperm=((B,), torch.float64, -5.0), method=i32(B), nopen=i32(B), nfr=i32(B), maxc=i32(B))

    @staticmethod
    def reserve(eng, case, B, R, Cm):
        eng.reserve_hybrid_sample_dev(B, R, Cm, case.n_sample)

    @staticmethod
    def launch(eng, case, b, stream):
        R, Cm = case.bounds
        o = b.out
        eng.hybrid_frontier_sample_assoc_dev(case.B, R, Cm, b.nL, b.nM, b.cost, b.coff, o["sub"], case.n_sample, o["asg"], b.aoff, o["lp"],
                                             b.loff, o["method"], o["logperm"], o["nopen"], o["nfr"], o["maxc"], seed=gl.sc.SEED,
                                             d_frameKey=b.key, condition=True, max_exact=case.max_exact, max_width=case.max_width,
                                             stream=stream, reserve=False)

    @staticmethod
    def grow(eng, case):
        R, Cm = case.bounds
        fr = case.grow_frames()

        def lift_and_reserve():
            eng.set_clustered_work_cap(0)
            eng.reserve_hybrid_sample_dev(case.B, R, Cm, case.n_sample)
        return [lift_and_reserve, lambda: eng.hybrid_frontier_sample_assoc([f[0] for f in fr], [f[1] for f in fr], [f[2] for f in fr], 4,
                                                                           condition=True, max_exact=case.max_exact, max_width=case.max_width)]

    @classmethod
    def host(cls, case, ds):
        key = (case.name, ds.name)
        if key not in cls._host:
            R, Cm = case.bounds
            idx = [b for b in range(ds.B) if ds.inside(b, R, Cm)]
            ref = pk.KBestEngine(0)
            try:
                out = ref.hybrid_frontier_sample_assoc([ds.frames[b][0] for b in idx], [ds.frames[b][1] for b in idx],
                                                       [ds.frames[b][2] for b in idx], case.n_sample, seed=gl.sc.SEED, condition=True,
                                                       frame_key=[ds.keys[b] for b in idx], max_exact=case.max_exact, max_width=case.max_width)
            finally:
                ref.close()
            cls._host[key] = {b: tuple(x[j] for x in out) for j, b in enumerate(idx)}  # assign, logProb, logPerm, method, nOpen, nFrontier, maxCluster
        return cls._host[key]

    @classmethod
    def check(cls, case, ds, got, filled):
        n = case.n_sample
        want = cls.host(case, ds)
        same = lambda a, b: bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())  # noqa: E731
        asg = slices(ds, got["asg"], ds.nM.astype(np.int64) * n, lambda b: (n, int(ds.nM[b])))
        lp = slices(ds, got["lp"], np.full(ds.B, n, np.int64), lambda b: (n,))
        for b in range(ds.B):
            if b not in want:  # beyond the bounds: method -1, nOpen and nFrontier 0, logPerm NaN; draws and maxCluster untouched
                assert (got["method"][b], got["nopen"][b], got["nfr"][b]) == (-1, 0, 0) and np.isnan(got["logperm"][b]), (ds.name, b)
                if filled:
                    assert got["maxc"][b] == -77, (ds.name, b)
                continue
            w = want[b]
            assert np.array_equal(asg[b], w[0]), (ds.name, b)
            assert same(lp[b], np.atleast_1d(w[1])) and same(got["logperm"][b: b + 1], np.atleast_1d(w[2])), (ds.name, b)
            assert (got["method"][b], got["nopen"][b], got["nfr"][b], got["maxc"][b]) == (w[3], w[4], w[5], w[6]), (ds.name, b)
        if ds.infeasible is not None:
            assert got["method"][ds.infeasible] == -2, ds.name
        if filled:
            untouched_outside(ds, case, got["asg"], ds.nM.astype(np.int64) * n, -77)
            untouched_outside(ds, case, got["lp"], np.full(ds.B, n, np.int64), -5.0)


class AssocEntry:
    @staticmethod
    def outputs(case, caps):
        import torch
        return dict(probs=((caps["prob"],), torch.float64, -5.0), nf=((case.B,), torch.int32, -77), flags=((case.B,), torch.int32, -77))

    @staticmethod
    def setup(eng, case):
        pass

    @staticmethod
    def reserve(eng, case, B, R, Cm):
        eng.reserve_assoc(B, R, Cm, case.k)

    @staticmethod
    def launch(eng, case, b, stream):
        R, Cm = case.bounds
        eng.set_assoc_tie_flags_dev(b.out["flags"])  # (a host call: where the launch behind it writes the flags)
        eng.assoc_probs_dev(case.B, R, Cm, b.nL, b.nM, b.nRow, b.cost, b.coff, case.k, b.out["probs"], b.poff, b.out["nf"], stream=stream)

    @staticmethod
    def grow(eng, case):
        R, Cm = case.bounds
        fr = case.grow_frames()
        return [lambda: eng.reserve_assoc(case.grow[0] * case.B, R, Cm, case.grow[1] * case.k),
                lambda: eng.weights([f[0] for f in fr], [f[1] for f in fr], [f[2] for f in fr], case.grow[1] * case.k, condition=True)]

    @staticmethod
    def check(case, ds, got, filled):
        want = case.want(ds)
        probs = slices(ds, got["probs"], ds.prob_sizes, lambda b: (int(ds.nM[b]), int(ds.nL[b]) + 1))
        for b, w in enumerate(want):
            if w is None:  # all costs equal: handed back by the walk, answered by the second launch (tests/test_gpu_round4.py)
                assert got["nf"][b] == case.k, (ds.name, b)
                np.testing.assert_allclose(probs[b].sum(axis=1), np.ones(int(ds.nM[b])), rtol=0, atol=1e-12, err_msg=f"{ds.name} {b}")
            elif isinstance(w, str):  # more than 32 rows kept by conditionCosts: d_nf = -2 and zero probabilities (kbest_c.h)
                assert got["nf"][b] == -2 and not probs[b].any(), (ds.name, b)
            elif w[1] == 0:  # no assignment: the checker's 0 / 0 has no value; this project answers such a frame with zeros
                assert got["nf"][b] == 0 and not probs[b].any(), (ds.name, b)
            else:
                assert got["nf"][b] == w[1], (ds.name, b, got["nf"][b], w[1])
                np.testing.assert_allclose(probs[b], w[0], rtol=0, atol=1e-12, err_msg=f"{ds.name} {b}")
            if filled:
                assert got["flags"][b] != -77, (ds.name, b)  # (every frame's flags are written by every launch)
        if filled:
            untouched_outside(ds, case, got["probs"], ds.prob_sizes, -5.0)


class KBestBuffers:
    def __init__(self, case, outputs=None):
        import torch
        self.torch = torch
        dev = torch.device("cuda", 0)
        B, N, M, k = case.Bn, case.N, case.M, case.k
        self.cost = torch.zeros((B, N * M), dtype=torch.float64, device=dev)
        self.out = dict(r4c=torch.empty((B, k, M), dtype=torch.int32, device=dev), c4r=torch.empty((B, k, N), dtype=torch.int32, device=dev),
                        g=torch.empty((B, k), dtype=torch.float64, device=dev), nf=torch.empty(B, dtype=torch.int32, device=dev),
                        flags=torch.empty(B, dtype=torch.int32, device=dev))
        self.fill()

    def load(self, ds):
        self.cost.copy_(self.torch.from_numpy(ds.costs))

    def fill(self):  # (tests/test_gpu_round5.py: -7 and NaN)
        for name, t in self.out.items():
            t.fill_(float("nan") if name == "g" else -7)

    def read(self):
        return {name: t.cpu().numpy() for name, t in self.out.items()}


class KBestEntry:
    Buffers = KBestBuffers

    @staticmethod
    def setup(eng, case):
        pass

    @staticmethod
    def first_reserve(eng, case):
        if case.reference_order:
            eng._check(eng.lib.kbest_reserve_exact(eng.ctx, case.Bn, case.N, case.M, case.k))
        else:
            eng.reserve(case.Bn, case.N, case.k)

    @staticmethod
    def launch(eng, case, b, stream):
        # (the wrapper's own reservation in front of the C entry is a no-op: the work space is large enough)
        o = b.out
        eng.kbest_dev(b.cost, case.Bn, case.N, case.M, case.k, o["r4c"], o["c4r"], o["g"], o["nf"], stream=stream, d_tie_flags=o["flags"],
                      reference_order=case.reference_order)
        E = pk.engine
        route = eng.last_route() & ~E.KBEST_ROUTE_EXTRA
        assert route == {"kbest_general_size": E.KBEST_ROUTE_WIDE, "kbest_small_problem": E.KBEST_ROUTE_SMALL,
                         "kbest_reference_order": E.KBEST_ROUTE_EXACT}[case.name], route

    @staticmethod
    def grow(eng, case):
        B, k = case.grow[0] * case.Bn, case.grow[1] * case.k
        big = np.random.default_rng(3).integers(0, 6, (B, case.N * case.M)).astype(np.float64) if case.integer else \
            np.random.default_rng(3).random((B, case.N * case.M))
        if case.reference_order:
            return [lambda: eng._check(eng.lib.kbest_reserve_exact(eng.ctx, B, case.N, case.M, k)),
                    lambda: eng.kbest(big, case.N, case.M, k, reference_order=True)]
        return [lambda: eng.reserve(B, case.N, k), lambda: eng.kbest(big, case.N, case.M, k)]

    @staticmethod
    def check(case, ds, got, filled):
        wn, wr, wc, wg = case.want(ds)
        assert (got["nf"] == wn).all(), (ds.name, got["nf"], wn)
        for b in range(case.Bn):
            n = int(wn[b])
            assert (bits(got["g"][b, :n]) == bits(wg[b, :n])).all(), (ds.name, b)
            assert (got["r4c"][b, :n] == wr[b, :n]).all(), (ds.name, b)
            if case.reference_order:
                assert (got["c4r"][b, :n] == wc[b, :n]).all(), (ds.name, b)
            else:  # (the padded columns are not mapped: tests/test_gpu_round5.py)
                assert (got["c4r"][b, :n][wc[b, :n] < case.M] == wc[b, :n][wc[b, :n] < case.M]).all(), (ds.name, b)
            if filled:
                assert got["flags"][b] != -7, (ds.name, b)
            if case.reference_order or (n == case.k and len(set(wg[b, :n].tolist())) == n):
                # the reference's own order has nothing to flag; neither has a full table of distinct gains that ran with the extra solution
                assert got["flags"][b] & ~pk.engine.KBEST_TIE_UNCHECKED == 0 or not filled, (ds.name, b, got["flags"][b])


PAD = 64


class ListBuffers:
    """The buffers of a list of clusters of fixed shapes, sentinels between and around everything (tests/test_gpu_frontier.py,
    tests/test_gpu_frontier_sample.py).  The host arrays -- shapes, offsets, keys -- live here: the entry reads them at enqueue time."""

    def __init__(self, case):
        import torch
        self.torch, self.case = torch, case
        dev = torch.device("cuda", 0)
        n, ns = len(case.shapes), max(case.n_sample, 1)
        self.m = np.array([m for _, m in case.shapes], np.int32)
        self.nLk = np.array([l for l, _ in case.shapes], np.int32)
        size = lambda per: PAD + sum(int(x) + PAD for x in per)  # noqa: E731
        offs = lambda per: np.array([PAD + sum(int(x) + PAD for x in per[:j]) for j in range(n)], np.int64)  # noqa: E731
        self.sub_sizes = [(l + m) * m for l, m in case.shapes]
        self.prob_sizes = [m * (l + 1) for l, m in case.shapes]
        self.key_sizes = [l + m for l, m in case.shapes]
        self.asg_sizes = [ns * m for _, m in case.shapes]
        self.lt_sizes = [ns] * n
        self.subOff, self.probOff, self.keyOff = offs(self.sub_sizes), offs(self.prob_sizes), offs(self.key_sizes)
        self.asgOff, self.ltOff = offs(self.asg_sizes), offs(self.lt_sizes)
        # (the captured layout: what a replay answers to, whatever the host arrays say by then)
        self.probOff0, self.asgOff0, self.ltOff0 = self.probOff.copy(), self.asgOff.copy(), self.ltOff.copy()
        self.subOff0, self.keyOff0 = self.subOff.copy(), self.keyOff.copy()
        self.frame_key = np.array(getattr(case, "frame_keys", (0,) * n), np.uint64)
        self.sub = torch.zeros(size(self.sub_sizes), dtype=torch.float64, device=dev)
        self.keys = torch.zeros(size(self.key_sizes), dtype=torch.int32, device=dev)
        full = lambda k, dt, v: torch.full((k,), v, dtype=dt, device=dev)  # noqa: E731
        self.out = dict(probs=full(size(self.prob_sizes), torch.float64, -5.0), asg=full(size(self.asg_sizes), torch.int32, -5),
                        lt=full(size(self.lt_sizes), torch.float64, -5.0), logZ=full(n, torch.float64, -5.0), info=full(n, torch.int32, -77),
                        width=full(n, torch.int32, -77))
        self.fills = dict(probs=-5.0, asg=-5, lt=-5.0, logZ=-5.0, info=-77, width=-77)

    def load(self, ds):
        sub = np.full(self.sub.numel(), -7.0)
        keys = np.full(self.keys.numel(), -9, np.int32)
        for j, blk in enumerate(ds.blocks):
            sub[self.subOff0[j]: self.subOff0[j] + blk.size] = blk
            keys[self.keyOff0[j]: self.keyOff0[j] + ds.keys[j].size] = ds.keys[j]
        self.sub.copy_(self.torch.from_numpy(sub))
        self.keys.copy_(self.torch.from_numpy(keys))

    def fill(self):
        for name, t in self.out.items():
            t.fill_(self.fills[name])

    def read(self):
        return dict({name: t.cpu().numpy() for name, t in self.out.items()}, layout=self)

    def scramble(self):
        """After the capture: the host arrays now describe the same clusters in reverse order (every offset still inside the
        buffers).  A replay must answer in the captured order all the same."""
        for a in (self.m, self.nLk, self.subOff, self.probOff, self.keyOff, self.asgOff, self.ltOff, self.frame_key):
            a[:] = a[::-1].copy()

    def cut(self, flat, off, sizes, fill):
        """The clusters' slices of an output, after checking that nothing around them was written."""
        mask = np.ones(flat.size, bool)
        out = []
        for o, n in zip(off, sizes):
            mask[o: o + n] = False
            out.append(flat[o: o + n])
        assert (flat[mask] == fill).all()
        return out


class ListEntry:
    Buffers = ListBuffers

    @staticmethod
    def setup(eng, case):
        pass

    @staticmethod
    def small16():
        fr = gl.wl.scene_frames(200, *gl.SCENE)[:16]
        return fr, [gl.SCENE[0]] * 16, [gl.SCENE[1]] * 16


class BigClusterEntry(ListEntry):
    @staticmethod
    def first_reserve(eng, case):
        eng.reserve_bigcluster(int(max(m for _, m in case.shapes)), int(max(l + m for l, m in case.shapes)))

    @staticmethod
    def launch(eng, case, b, stream):
        eng.bigcluster_probs_dev(b.m, b.nLk, b.subOff, b.probOff, b.sub, b.out["probs"], b.out["logZ"], b.out["info"], stream=stream,
                                 reserve=False)

    @staticmethod
    def grow(eng, case):
        f = gl.wl.scene_frames(2, 60, 40, 30)[1]  # (a cluster of 17 measurements on 40 rows: tests/test_gpu_bigcluster.py)
        return [lambda: eng.reserve_bigcluster(*case.grow_to), lambda: eng.hybrid_exact_probs([f], [60], [40], 0, condition=True)]

    @staticmethod
    def check(case, ds, got, filled):
        want = case.want(ds)
        lay = got["layout"]
        probs = lay.cut(got["probs"], lay.probOff0, lay.prob_sizes, -5.0) if filled else \
            [got["probs"][o: o + n] for o, n in zip(lay.probOff0, lay.prob_sizes)]
        for j, (wp, wlz, winfo) in enumerate(want):
            assert got["info"][j] == winfo, (ds.name, j)
            assert np.abs(probs[j].reshape(wp.shape) - wp).max() <= 1e-12, (ds.name, j)
            if winfo == 1:
                assert abs(got["logZ"][j] - wlz) <= 1e-12 * abs(wlz), (ds.name, j)  # (tests/test_gpu_bigcluster.py)
            else:
                assert got["logZ"][j] == -np.inf and not probs[j].any(), (ds.name, j)


class FrontierEntry(ListEntry):
    @staticmethod
    def first_reserve(eng, case):
        eng.reserve_frontier(len(case.shapes), int(max(m for _, m in case.shapes)), int(max(l + m for l, m in case.shapes)))

    @staticmethod
    def launch(eng, case, b, stream):
        eng.frontier_probs_dev(b.m, b.nLk, b.subOff, b.probOff, b.sub, b.out["probs"], b.out["logZ"], b.out["info"], b.out["width"],
                               stream=stream, reserve=False)

    @staticmethod
    def grow(eng, case):
        n = case.grow_n * len(case.shapes)
        fr, nL, nM = ListEntry.small16()
        return [lambda: eng.reserve_frontier(n, int(max(m for _, m in case.shapes)), int(max(l + m for l, m in case.shapes))),
                lambda: eng.hybrid_frontier_probs(fr, nL, nM, 0, condition=True, max_exact=4, max_big=0, max_width=16)]

    @staticmethod
    def check(case, ds, got, filled):
        want = case.want(ds)
        lay = got["layout"]
        probs = lay.cut(got["probs"], lay.probOff0, lay.prob_sizes, -5.0) if filled else \
            [got["probs"][o: o + n] for o, n in zip(lay.probOff0, lay.prob_sizes)]
        for j, (wp, wlz, winfo, wW) in enumerate(want):
            assert (got["info"][j], got["width"][j]) == (winfo, wW), (ds.name, j)
            assert np.abs(probs[j].reshape(wp.shape) - wp).max() <= 1e-12, (ds.name, j)
            if winfo == 1:
                assert abs(got["logZ"][j] - wlz) <= 1e-12 * max(1.0, abs(wlz)), (ds.name, j)  # (tests/test_gpu_frontier.py)
            else:
                assert got["logZ"][j] == -np.inf and not probs[j].any(), (ds.name, j)


class FrontierSampleEntry(ListEntry):
    @staticmethod
    def first_reserve(eng, case):
        eng.reserve_frontier_sample(len(case.shapes), int(max(m for _, m in case.shapes)), int(max(l + m for l, m in case.shapes)))

    @staticmethod
    def launch(eng, case, b, stream):
        eng.frontier_sample_dev(b.m, b.nLk, b.subOff, b.sub, b.keys, b.keyOff, case.n_sample, b.out["asg"], b.asgOff, b.out["lt"], b.ltOff,
                                b.out["logZ"], b.out["info"], b.out["width"], seed=gl.sc.SEED, sample_base=0, frame_key=b.frame_key,
                                stream=stream, reserve=False)

    @staticmethod
    def grow(eng, case):
        n = case.grow_n * len(case.shapes)
        fr, nL, nM = ListEntry.small16()
        return [lambda: eng.reserve_frontier_sample(n, int(max(m for _, m in case.shapes)), int(max(l + m for l, m in case.shapes))),
                lambda: eng.hybrid_frontier_sample_assoc(fr, nL, nM, 4, condition=True, max_exact=4, max_width=16)]

    @staticmethod
    def check(case, ds, got, filled):
        want = case.want(ds)
        lay = got["layout"]
        n = case.n_sample
        if filled:
            asg, lt = lay.cut(got["asg"], lay.asgOff0, lay.asg_sizes, -5), lay.cut(got["lt"], lay.ltOff0, lay.lt_sizes, -5.0)
        else:
            asg = [got["asg"][o: o + k] for o, k in zip(lay.asgOff0, lay.asg_sizes)]
            lt = [got["lt"][o: o + k] for o, k in zip(lay.ltOff0, lay.lt_sizes)]
        for j, (wa, wlt, wlz, winfo, wW, margin) in enumerate(want):
            assert margin >= gl.MIN_MARGIN, (ds.name, j, margin)
            assert (got["info"][j], got["width"][j]) == (winfo, wW), (ds.name, j)
            assert np.array_equal(asg[j].reshape(n, -1), wa), (ds.name, j)
            if winfo == 1:
                assert np.abs(lt[j] - wlt).max() <= 1e-12, (ds.name, j)
                assert abs(got["logZ"][j] - wlz) <= 1e-12 * max(1.0, abs(wlz)), (ds.name, j)  # (tests/test_gpu_frontier_sample.py)
            else:
                assert np.isnan(lt[j]).all() and got["logZ"][j] == -np.inf, (ds.name, j)


class TableBuffers:
    def __init__(self, case):
        import torch
        self.torch = torch
        dev = torch.device("cuda", 0)
        n = case.n_sample
        self.m = np.array(case.m, np.int32)
        self.ck, self.fk = np.array(case.cluster_key, np.uint32), np.array(case.frame_key, np.uint64)
        self.asg_sizes, self.lt_sizes = [n * m for m in case.m], [n] * 3
        self.asgOff = np.array([PAD + sum(x + PAD for x in self.asg_sizes[:j]) for j in range(3)], np.int64)
        self.ltOff = np.array([PAD + sum(x + PAD for x in self.lt_sizes[:j]) for j in range(3)], np.int64)
        self.asgOff0, self.ltOff0 = self.asgOff.copy(), self.ltOff.copy()
        self.tab = torch.zeros((3, case.k, case.max_col), dtype=torch.int32, device=dev)
        self.gain = torch.zeros((3, case.k), dtype=torch.float64, device=dev)
        self.nf = torch.zeros(3, dtype=torch.int32, device=dev)
        self.out = dict(asg=torch.full((PAD + sum(x + PAD for x in self.asg_sizes),), -5, dtype=torch.int32, device=dev),
                        lt=torch.full((PAD + sum(x + PAD for x in self.lt_sizes),), -5.0, dtype=torch.float64, device=dev),
                        pick=torch.full((3, n), -5, dtype=torch.int32, device=dev), info=torch.full((3,), -77, dtype=torch.int32, device=dev))
        self.fills = dict(asg=-5, lt=-5.0, pick=-5, info=-77)

    def load(self, ds):
        t = self.torch.from_numpy
        self.tab.copy_(t(ds.tab)); self.gain.copy_(t(ds.gain)); self.nf.copy_(t(ds.nf))

    fill, read, cut = ListBuffers.fill, ListBuffers.read, ListBuffers.cut

    def scramble(self):
        for a in (self.m, self.ck, self.fk, self.asgOff, self.ltOff):
            a[:] = a[::-1].copy()


class TableSampleEntry(ListEntry):
    Buffers = TableBuffers

    @staticmethod
    def first_reserve(eng, case):
        pass  # (no work space: kbest_c.h at kbest_table_sample_f64_dev)

    @staticmethod
    def launch(eng, case, b, stream):
        eng.table_sample_dev(case.k, case.max_col, b.m, b.tab, b.gain, b.nf, case.n_sample, b.out["asg"], b.asgOff, b.out["lt"], b.ltOff,
                             b.out["pick"], b.out["info"], cluster_key=b.ck, frame_key=b.fk, seed=gl.sc.SEED, sample_base=0, stream=stream)

    @staticmethod
    def check(case, ds, got, filled):
        want = case.want(ds)
        lay = got["layout"]
        n = case.n_sample
        if filled:
            asg, lt = lay.cut(got["asg"], lay.asgOff0, lay.asg_sizes, -5), lay.cut(got["lt"], lay.ltOff0, lay.lt_sizes, -5.0)
        else:
            asg = [got["asg"][o: o + k] for o, k in zip(lay.asgOff0, lay.asg_sizes)]
            lt = [got["lt"][o: o + k] for o, k in zip(lay.ltOff0, lay.lt_sizes)]
        for j, (wa, wpick, wlt, margin) in enumerate(want):
            assert margin >= gl.MIN_MARGIN, (ds.name, j, margin)
            assert np.array_equal(got["pick"][j], wpick) and np.array_equal(asg[j].reshape(n, -1), wa), (ds.name, j)
            if ds.nf[j] > 0:  # (tests/test_gpu_table_sample.py, check_problem)
                assert got["info"][j] == 1 and np.abs(lt[j] - wlt).max() <= 1e-12, (ds.name, j)
            else:
                assert got["info"][j] == 0 and np.isnan(lt[j]).all(), (ds.name, j)


ENTRIES = {"permanent_wide": PermanentEntry, "permanent_ragged": PermanentEntry, "sample_wide": SampleEntry, "belief_lds": BeliefEntry,
           "belief_hbm": BeliefEntry, "clustered": ClusteredEntry, "clustered_sample": ClusteredSampleEntry,
           "clustered_partial": PartialEntry, "hybrid_probs_w16": HybridEntry, "hybrid_probs_w5": HybridEntry,
           "hybrid_sample_w16": HybridSampleEntry, "assoc_10_10": AssocEntry, "assoc_20_20": AssocEntry,
           "kbest_general_size": KBestEntry, "kbest_small_problem": KBestEntry, "kbest_reference_order": KBestEntry,
           "bigcluster": BigClusterEntry, "frontier": FrontierEntry, "frontier_sample": FrontierSampleEntry, "table_sample": TableSampleEntry}


# ---- the protocol ---------------------------------------------------------------------------------------------------------------------
def refused_as_captured(call):
    with pytest.raises(pk.KBestError) as err:
        call()
    text = str(err.value)
    assert text.startswith(BAD_ARG_TEXT + ":") and "captured" in text, text


def frame_growth(eng, case, entry):
    """The two calls of the growth step of a frame case: the entry's own reservation and its host-buffer entry."""
    R, Cm = case.bounds
    grow = getattr(case, "grow_to", None)
    big = (case.grow_B * case.B, R, Cm) if grow is None else (case.B,) + tuple(grow)
    return [lambda: entry.reserve(eng, case, *big), lambda: entry.host(eng, case, case.grow_frames())]


def run_protocol(case, entry):
    import torch
    eng = pk.KBestEngine(0)  # a context of the case's own: a captured launch marks its work spaces for life
    try:
        entry.setup(eng, case)
        make = getattr(entry, "Buffers", None) or (lambda c: Buffers(c, entry.outputs))
        main, other = make(case), make(case)
        if hasattr(entry, "first_reserve"):
            entry.first_reserve(eng, case)
        else:
            entry.reserve(eng, case, case.B, *case.bounds)
        s = torch.cuda.Stream(device=torch.device("cuda", 0))
        torch.cuda.synchronize()

        def step(buf, ds, run, fill=True):
            with torch.cuda.stream(s):
                buf.seed = ds.seed
                buf.load(ds)
                if fill:
                    buf.fill()
                run()
            s.synchronize()
            entry.check(case, ds, buf.read(), fill)

        data = case.data
        step(main, data["A"], lambda: entry.launch(eng, case, main, s.cuda_stream))  # the runtime's lazy one-off work: outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):  # one stream, nothing else inside: a chain
            entry.launch(eng, case, main, s.cuda_stream)  # (anything but KBEST_OK raises)
        if hasattr(main, "scramble"):
            main.scramble()  # (host arrays are read at enqueue time: the graph must not look at them again)
        for it, name in enumerate(gl.ORDER):
            step(main, data[name], graph.replay, fill=it != 3)  # (the fourth follows the third with nothing but the input copy in between)
            if it == 1:
                step(other, data["O"], lambda: entry.launch(eng, case, other, s.cuda_stream))
        if getattr(case, "holds_work_space", True):
            assert case.growth_premise(), (case.need_before(), case.need_after())
            for call in (entry.grow(eng, case) if hasattr(entry, "grow") else frame_growth(eng, case, entry)):
                refused_as_captured(call)  # (the test ends here if one is not: a stale graph must never run)
        elif hasattr(entry, "reserve"):  # nothing of the context in the captured launch: the reservation is free to allocate
            entry.reserve(eng, case, case.B, *case.grow_to)
        step(main, data["H1"], graph.replay)
    finally:
        eng.close()


CASES = {c.name: c for c in gl.frame_cases() + gl.hybrid_cases() + gl.assoc_cases() + gl.kbest_cases() + gl.list_cases()}
assert set(CASES) == set(ENTRIES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_entry_captured_and_replayed(name):
    run_protocol(CASES[name], ENTRIES[name])
