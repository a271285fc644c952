"""CPU: the library exports the clustered sampler's C entries and the clusterSampleAssoc shim, include/kbest_c.h declares them and
states the contract, and the Python driver binds them."""
import os
import subprocess

import pytest

import probabilisticsemslam_amd as pk
from probabilisticsemslam_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("kbest_clustered_sample_assoc_batch_f64", "kbest_clustered_sample_assoc_batch_f64_dev", "kbest_reserve_clustered_sample")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pk.lib_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "probabilisticsemslam_amd", "csrc")])
    return pk.load_library()


def test_library_exports_cluster_sample_entries(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pk.lib_path()], text=True)
    assert "_Z18clusterSampleAssocRKSt6vectorIdSaIdEEmmmm" in out
    header = open(os.path.join(ROOT, "include", "kbest_c.h")).read()
    for sym in SYMBOLS:
        assert sym in engine.C_ABI_SYMBOLS and f" T {sym}\n" in out and hasattr(lib, sym), sym
        assert f"int {sym}(kbest_ctx *ctx" in header, sym
    assert callable(pk.clusterSampleAssoc)
    for name in ("clustered_sample_assoc", "clustered_sample_assoc_dev", "reserve_clustered_sample"):
        assert callable(getattr(pk.KBestEngine, name)), name
    shims = open(os.path.join(ROOT, "include", "kbest_shims.hpp")).read()
    assert "clusterSampleAssoc(const std::vector<double> &costMatrix, size_t nL, size_t nM, size_t nSample," in shims


def test_header_states_the_contract():
    header = " ".join(open(os.path.join(ROOT, "include", "kbest_c.h")).read().replace(" * ", " ").split())
    assert "on a frame that kbest_sample_assoc_batch_f64 takes, the decisions are the same function of the same uniforms" in header
    assert "index among the frame's ACTIVE rows" in header
    assert "kbest_reserve_clustered_sample reserves exactly what kbest_reserve_clustered does" in header
