"""The conditions of the inputs of tests/test_gpu_graph_capture.py, from the restatements alone (no GPU): every sampler data set has a
margin of at least 1e-10; the heavy sets list strictly more open clusters than the light one; the light set holds its infeasible frame
and its refused frame; and the growth request of every case at least quadruples the need computed from the formulas of
include/kbest_c.h (and lies beyond what the capture's reservation allocated)."""
import pytest

import graph_capture_lib as gl

FRAME = {c.name: c for c in gl.frame_cases() + gl.assoc_cases()}
HYBRID = {c.name: c for c in gl.hybrid_cases()}
KBEST = {c.name: c for c in gl.kbest_cases()}
LISTS = {c.name: c for c in gl.list_cases()}


@pytest.mark.parametrize("name", list(FRAME))
def test_frame_case_inputs(name):
    c = FRAME[name]
    infeasible, refused = c.light_conditions()
    assert infeasible and refused, name
    for n, m in c.margins().items():
        assert m >= gl.MIN_MARGIN, (name, n, m)
    if c.n_sample:
        assert set(c.margins()) == set(c.data)
    if c.holds_work_space:
        assert c.growth_premise(), (name, c.need_before(), c.need_after())
    R, Cm = c.bounds
    light, heavy = c.data["L"], c.data["A"]
    if not isinstance(c, gl.Assoc):  # (the fused entry's limit is the rows conditionCosts keeps, not the launch bounds)
        assert sum(light.inside(b, R, Cm) for b in range(light.B)) < heavy.B  # fewer frames inside the launch bounds
    assert light.cost_sizes.sum() < heavy.cost_sizes.sum()
    if hasattr(c, "open_clusters"):
        n = c.open_clusters()
        assert all(n[h] > n["L"] for h in ("A", "H1", "H2")), n


@pytest.mark.parametrize("name", list(HYBRID))
def test_hybrid_case_inputs(name):
    c = HYBRID[name]
    infeasible, refused = c.light_conditions()
    assert infeasible and refused, name
    n = c.open_clusters()
    assert all(n[h] > n["L"] > 0 for h in ("A", "H1", "H2")), n
    assert c.light_refused_at(5) and not c.light_refused_at(16)  # refused in the second parametrisation only
    assert c.data["L"].infeasible not in c.light_refused_at(5)  # (the infeasible frame stays infeasible there)
    assert c.growth_premise(), (c.need_before(), c.need_after())


@pytest.mark.parametrize("name", list(KBEST))
def test_kbest_case_inputs(name):
    c = KBEST[name]
    infeasible, few = c.light_conditions()
    assert infeasible and few, name
    assert c.growth_premise(), (name, c.need_before(), c.need_after())


@pytest.mark.parametrize("name", list(LISTS))
def test_list_case_inputs(name):
    c = LISTS[name]
    for n, m in c.margins().items():
        assert m >= gl.MIN_MARGIN, (name, n, m)
    if c.n_sample:
        assert set(c.margins()) == set(c.data)
    if name == "table_sample":  # no work space: nothing grows; the light tables are short, one is empty
        nf = {n: s.nf.tolist() for n, s in c.data.items()}
        assert nf["L"][1] == 0 and sum(nf["L"]) < min(sum(nf[h]) for h in ("A", "H1", "H2"))
        return
    assert c.is_infeasible(c.want(c.data["L"])[c.dead]), name
    assert c.growth_premise(), (name, c.need_before(), c.need_after())
    if hasattr(c, "widths"):  # the light set's frontiers are narrower: fewer states in every layer
        w = c.widths()
        assert all(sum(w[h]) > sum(w["L"]) for h in ("A", "H1", "H2")), w
