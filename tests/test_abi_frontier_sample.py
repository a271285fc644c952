"""CPU: the library exports the frontier sampler's C entries and the hybridFrontierSampleAssoc shim, include/kbest_c.h declares
them and states the contract, and the Python driver binds them."""
import os
import subprocess

import pytest

import probabilisticsemslam_amd as pk
from probabilisticsemslam_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("kbest_frontier_sample_f64_dev", "kbest_reserve_frontier_sample", "kbest_hybrid_frontier_sample_assoc_batch_f64")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pk.lib_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "probabilisticsemslam_amd", "csrc")])
    return pk.load_library()


def test_library_exports_frontier_sample_entries(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pk.lib_path()], text=True)
    assert "_Z25hybridFrontierSampleAssocRKSt6vectorIdSaIdEEmmmm" in out
    header = open(os.path.join(ROOT, "include", "kbest_c.h")).read()
    for sym in SYMBOLS:
        assert sym in engine.C_ABI_SYMBOLS and f" T {sym}\n" in out and hasattr(lib, sym), sym
        assert f"int {sym}(kbest_ctx *ctx" in header, sym
    assert callable(pk.hybridFrontierSampleAssoc)
    for name in ("hybrid_frontier_sample_assoc", "frontier_sample_dev", "reserve_frontier_sample"):
        assert callable(getattr(pk.KBestEngine, name)), name
    shims = open(os.path.join(ROOT, "include", "kbest_shims.hpp")).read()
    assert "hybridFrontierSampleAssoc(const std::vector<double> &costMatrix, size_t nL, size_t nM, size_t nSample," in shims


def test_header_states_the_contract():
    header = " ".join(open(os.path.join(ROOT, "include", "kbest_c.h")).read().replace(" * ", " ").split())
    assert "(sampleBase + s, 0x80000000 | (q >> 1), frameKey low word, frameKey high word)" in header
    assert "kbest_reserve_frontier_sample reserves exactly what kbest_reserve_frontier does" in header
    assert "are NOT equal for the open clusters, because q is a raw row" in header
    assert "no uniform is ever shared between a small cluster and a frontier cluster of one frame" in header
