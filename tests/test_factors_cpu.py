"""CPU: the factor lists from association probabilities (kbest_factors.hip) before any GPU run -- the conditions of the scenes the
GPU tests stand on, from the numpy restatements alone (quadric_map_lib, quadric_map_sample_lib, factors_lib); the count, scan and
emit passes compiled for the host (tests/cpp/factors_host.cpp: a stand-alone program under AddressSanitizer and UBSan, exact-size
heap buffers, nothing loaded into python) against the restated loops on the generic cases, bit for bit; the library exports the new
symbols, the header states the contract; without a GPU the entries fail loudly."""
import os
import subprocess

import numpy as np
import pytest

import factors_lib as fl
import probabilisticsemslam_amd as pk
import quadric_map_lib as qm
import quadric_map_sample_lib as qs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "probabilisticsemslam_amd", "csrc")


# ---- 1. the restatement and the scenes ---------------------------------------------------------------------------------------------------
def test_vectorised_restatement_is_the_literal_loops():
    """factors_lib.frame_lists (one numpy expression a row set) against frame_lists_literal (system.cpp:279-346 line for line) on
    every generic case but the widest: equal bits, equal order."""
    for name, case in fl.generic_cases().items():
        if name in ("wide", "grid"):
            case = dict(case, frames=case["frames"][:12])
        a, b = fl.restate(case), fl.restate(case, fl.frame_lists_literal)
        for k in a:
            if a[k].dtype == np.float64:
                assert np.array_equal(fl.bits(a[k]), fl.bits(b[k])), (name, k)
            else:
                assert np.array_equal(a[k], b[k]), (name, k)


def scene_lists(re, land_off=0):
    """The lists of a restated frame in compact form at the scene thresholds."""
    nk = len(re["rows"])
    assert re["cprobs"].shape[1] == nk + 1
    return fl.frame_lists(re["cprobs"], re["rows"], fl.SCENE_FACTOR_THRESH, fl.SCENE_NEW_THRESH, fl.BOX_SD)


def test_conditions_of_the_scenes():
    """What tests/test_gpu_factors.py stands on, at the reference's thresholds 0.05 / 0.33: the frames of parity, sparse_batch() and
    chain frames 0 .. 3 give non-empty factor and new-landmark lists, and some measurement has two or more factors; compact and
    dense form of a frame give the same lists; limit holds a frame with nKeep > maxKeep and refused ones; the overlapping windows
    of edge (frames 14 and 15) give some support count >= 2; the far frame has a factor at a landmark beyond 65 535."""
    assert (fl.SCENE_FACTOR_THRESH, fl.SCENE_NEW_THRESH, fl.BOX_SD) == (0.05, 0.33, 3.0)  # constsUtils.h:75-78
    sets = dict(parity=[qm.window_restated("parity", j) for j in range(16)], sparse=[qs.sparse_restated(f) for f in range(4)],
                chain=[qm.chain_restated(f, 0) for f in range(4)])
    double = False
    for name, res in sets.items():
        nf = nn = 0
        for re in res:
            if re["method"] < 0:
                continue
            fm, land, fp, fs, nm, npr, ns = scene_lists(re)
            nf, nn = nf + len(fm), nn + len(nm)
            double = double or (len(fm) and np.bincount(fm).max() >= 2)
            dense = fl.frame_lists(re["probs"], None, fl.SCENE_FACTOR_THRESH, fl.SCENE_NEW_THRESH, fl.BOX_SD)
            for x, y in zip((fm, land, fp, fs, nm, npr, ns), dense):
                assert np.array_equal(x, y), name
            assert np.isfinite(fs).all() and (fp >= 0.05).all() and (npr > 0.33).all()
        print(f"{name}: factors {nf}, new landmarks {nn}")
        assert nf > 0 and nn > 0, name
    assert double
    assert any(re["method"] == 0 for re in sets["parity"])
    # limit at maxMap 300, maxKeep 8, maxCol 4: 8 kept (answered), 9 kept (refused), beyond maxMap, beyond maxCol
    frames = qm.limit_batch()[2]
    assert [len(qm.window_restated("limit", j)["rows"]) for j in (0, 1)] == [8, 9] and frames[2][1] == 301 and len(frames[3][2]) == 5
    assert len(scene_lists(qm.window_restated("limit", 0))[0]) > 0
    # edge: frames 14 and 15 are windows 100 .. 699 and 0 .. 499 of one random map
    frames = qm.edge_batch()[2]
    sup = np.zeros(len(qm.edge_batch()[0]), np.int32)
    for j in (14, 15):
        re = qm.window_restated("edge", j)
        assert re["method"] == 0
        np.add.at(sup, frames[j][0] + scene_lists(re)[1].astype(np.int64), 1)
    assert frames[14][0] == frames[15][0] + 100 and sup.max() >= 2
    far = qm.window_restated("far", 6)
    assert far["method"] == 0 and scene_lists(far)[1].max() > 65535


# ---- 2. the kernels, compiled for the host ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("factors_host")
    (tmp / "hip").mkdir()
    (tmp / "hip" / "hip_runtime.h").write_text("")
    out = str(tmp / "factors_host")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-I", str(tmp), "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                           "-I", os.path.join(ROOT, "tests", "cpp"), "-x", "c++", os.path.join(ROOT, "tests", "cpp", "factors_host.cpp"),
                           "-o", out, "-lpthread"])
    return out


def run_host(exe, tmp_path, case, maxFactor, maxNew):
    src, out = tmp_path / "in.bin", tmp_path / "out.bin"
    fl.write_host_input(src, case, maxFactor, maxNew)
    subprocess.check_call([exe, str(src), str(out)])
    return fl.read_host_output(out, case, maxFactor, maxNew)


CASES = fl.generic_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_generic_cases_on_the_host_under_sanitizers(exe, tmp_path, name):
    """Every generic case at capacity = total: the lists, counts, offsets, totals and support of the restated loops, bit for bit,
    on buffers of exactly that size."""
    case = CASES[name]
    want = fl.restate(case)
    tf, tn = (int(x) for x in want["total"])
    fl.same(run_host(exe, tmp_path, case, tf, tn), want, tf, tn, name)
    if name == "grid":
        assert tf > 1000 and tn > 10 and (want["fProb"] == fl.FT).any() and (want["fMap"] >= case["nSupport"]).any()
        P = np.concatenate([fr["P"][:, -1] for fr in case["frames"]])
        assert (P == fl.NT).any() and not (want["nProb"] == fl.NT).any()  # p == newThresh occurs and is not new
    if name == "keep_all_zero":
        assert tf == sum(fr["P"].shape[0] * (fr["P"].shape[1] - 1) for fr in case["frames"]) and np.isposinf(want["fSigma"]).any()
    if name == "keep_none":
        assert tf == 0 and tn > 0
    if name == "refused":
        assert (want["nFactor"] > 0).tolist() == [True, False, False, True] + [False] * 6 + [True]
    if name == "short_support":
        assert (want["fMap"] >= 3).any()


def test_compact_and_dense_form_give_the_same_list(exe, tmp_path):
    comp, dense = CASES["compact"], CASES["dense"]
    a, b = fl.restate(comp), fl.restate(dense)
    tf, tn = (int(x) for x in a["total"])
    ga, gb = run_host(exe, tmp_path, comp, tf, tn), run_host(exe, tmp_path, dense, tf, tn)
    assert tf > 100 and set(a) == set(b) == set(ga) == set(gb)
    for k in a:
        assert np.array_equal(a[k], b[k]) and np.array_equal(ga[k], gb[k]) and np.array_equal(ga[k], a[k]), k


@pytest.mark.parametrize("name", fl.CAPACITY_CASES)
def test_capacities_on_the_host_under_sanitizers(exe, tmp_path, name):
    """maxFactor in {total, total - 1, 1, 0} and the same for maxNew: an entry beyond the capacity is not written, nothing else
    changes -- the counts, offsets, totals and the support are those of the full call."""
    case = CASES[name]
    want = fl.restate(case)
    tf, tn = (int(x) for x in want["total"])
    assert tf >= 3 and tn >= 3
    for cf, cn in zip(fl.capacities(tf), fl.capacities(tn)):
        fl.same(run_host(exe, tmp_path, case, cf, cn), want, cf, cn, (name, cf, cn))
    fl.same(run_host(exe, tmp_path, case, 0, tn), want, 0, tn, (name, 0, tn))


def test_no_frame_on_the_host(exe, tmp_path):
    """B = 0: the totals 0 and the support zeroed."""
    case = fl.base([], 10, 4, nSupport=5)
    got = run_host(exe, tmp_path, case, 2, 2)
    fl.same(got, fl.restate(case), 2, 2, "B = 0")
    assert got["total"].tolist() == [0, 0] and got["support"].tolist() == [0] * 5


# ---- 3. the library ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pk.lib_path()):
        subprocess.check_call(["make", "-C", CSRC])
    return pk.load_library()


SYMBOLS = ("kbest_reserve_assoc_factors_dev", "kbest_assoc_factors_f64_dev", "kbest_reserve_quadric_map_factors_dev",
           "kbest_quadric_map_factors_batch_f64_dev", "kbest_assoc_factors_batch_f64", "kbest_factors_kernel_usage")


def test_library_exports_the_factor_entries(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pk.lib_path()], text=True)
    from probabilisticsemslam_amd import engine
    header = open(os.path.join(ROOT, "include", "kbest_c.h")).read()
    for sym in SYMBOLS:
        assert sym in engine.C_ABI_SYMBOLS and f" T {sym}\n" in out and hasattr(lib, sym) and f"int {sym}(" in header, sym
        assert getattr(lib, sym).argtypes is not None, sym
    for name in ("reserve_assoc_factors_dev", "assoc_factors_dev", "reserve_quadric_map_factors_dev", "quadric_map_factors_dev",
                 "assoc_factors", "quadric_map_factors"):
        assert callable(getattr(pk.KBestEngine, name)), name
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "kbest_factors.hip" in make.split("SRCS", 1)[1].split("\n", 1)[0] and "kbest_factors.h" in make.split("HDRS", 1)[1].split("\n", 1)[0]


def test_header_states_the_contract():
    """Order, the two comparisons, capacity, which frames emit nothing, and the reference's lines."""
    header = " ".join(open(os.path.join(ROOT, "include", "kbest_c.h")).read().replace(" * ", " ").split())
    for sentence in ("system.cpp:279-346", "slidingWindow.cpp:351-460", "constsUtils.h:57-59",
                     "every (b, m, l) with !(p < factorThresh), in the order b ascending, then m ascending, then l ascending",
                     "every (b, m) with P_b[m][nSlot] > newThresh, strictly, in the order b, then m",
                     "p equal to factorThresh is kept, p equal to newThresh is not new",
                     "an entry whose position is >= maxFactor (>= maxNew) is not written, and nothing else changes",
                     "Capacity 0 with NULL arrays is a legal counting call",
                     "d_method given and d_method[b] < 0; nM < 1, nM > maxCol, nSlot < 0, nSlot > maxSlot, a negative offset",
                     "indices outside [0, nSupport) are not counted", "KBEST_ERR_NOT_RESERVED, nothing launched"):
        assert sentence in header, sentence


def test_defaults_are_the_references(lib):
    import inspect
    for name in ("assoc_factors", "assoc_factors_dev", "quadric_map_factors", "quadric_map_factors_dev"):
        d = {k: v.default for k, v in inspect.signature(getattr(pk.KBestEngine, name)).parameters.items()}
        assert (d["factor_thresh"], d["new_thresh"], d["box_sd"]) == (fl.FACTOR_THRESH, fl.NEW_THRESH, fl.BOX_SD), name


def test_factor_entries_without_gpu_fail_loudly(lib):
    if lib.kbest_device_count() > 0:
        return  # (a GPU is present: tests/test_gpu_factors.py has the rest)
    with pytest.raises(pk.KBestError):
        pk.KBestEngine(0).reserve_assoc_factors_dev(1, 24)
    with pytest.raises(pk.KBestError):
        pk.KBestEngine(0).assoc_factors([np.ones((2, 3))])
