"""The reference of the engine-graph tests, checked without a GPU (tests/_engine_ref.py): the grid twins are exact in
float32, the mirrors state the operations (autograd against central differences), and the table is complete."""
import pytest
import torch

import _engine_ref as R

GRID = [n for n, g in R.GRAPHS.items() if g.grid]
WITH_GRADS = [n for n, g in R.GRAPHS.items() if g.outs]


@pytest.mark.parametrize("name", GRID)
def test_grid_twin_is_exact(name):
    """every forward value and gradient of the mirror on `grid` is an integer, and the same mirror on |inputs|, |weights|
    (the sum of the absolute terms of every sum in it) stays below 2^24 -- below 2^22 where a Winograd variant runs,
    whose transforms work in multiples of 1/4: no float32 evaluation order can round, so the GPU owes the bits"""
    ref = R.reference(name, "grid")
    for label, v in R.tensors_of(ref):
        assert torch.equal(v, v.round()), label
        assert torch.equal(v.float().double(), v), label
    room = R.grid_headroom(name, wino=name.startswith("chain"))
    print(f"{name}: largest absolute sum {room:.0f} ({room / 2 ** 24:.3f} of 2^24)")
    assert room < 2 ** 24


@pytest.mark.parametrize("name", WITH_GRADS)
def test_mirror_against_finite_differences(name):
    """the mirror's autograd gradients against central differences of the mirror in float64, 8 seeded coordinates per
    leaf: relative 1e-6 of the gradient's max norm (anything near it means a wrong mirror, not noise)"""
    worst = R.fd_check(R.GRAPHS[name])
    print(f"{name}: worst |autograd - central difference| / |gradient|max = {worst:.2e}")
    assert worst <= R.FD_TOL


def test_table_is_total():
    """every branch has a graph; a graph without a grid twin says why; stops and pre-bound tensors are leaves"""
    have = {g.branch for g in R.GRAPHS.values()}
    missing = [b for b in R.BRANCHES if b not in have and b not in R.NOT_IN_TABLE]
    assert not missing, missing
    assert not (set(R.NOT_IN_TABLE) & have)
    for g in R.GRAPHS.values():
        assert g.grid or g.note, g.name
        assert set(g.stops) <= set(R.leaves(g)) and set(g.prebound) <= set(R.leaves(g)), g.name
        outs = R.reference(g.name, "real").outs
        assert set(g.outs) | set(g.free) == set(outs), g.name
    # every branch made of exact operations has a graph with a grid twin
    for b in ("chain", "ride", "ride_mismatch", "ride_preempted", "ride_leftover", "ride_twice", "ride_slice", "fanout",
              "group_shared", "group_mixed_accum", "group_partial_want", "group_missing", "bias_paths", "shared_weight",
              "thin", "aliased_views"):
        assert any(g.grid for g in R.GRAPHS.values() if g.branch == b), b


def test_limit_has_every_term():
    """the real limit of a GELU graph: ref32's error, the roundoff of the result and a non-zero function floor"""
    lim = R.limits("ride_gelu")
    for label, (limit, e32, floor) in lim.items():
        assert floor >= 0 and e32 > 0 and limit > R.FACTOR * e32 + floor, label
    # the last bias gradient is the sum of the upstream gradient: no function in front of it.  Everything else has one
    assert lim["d.ru.conv.4.bias"][2] == 0.0
    assert all(v[2] > 0 for k, v in lim.items() if k != "d.ru.conv.4.bias")


@pytest.mark.parametrize("name", [n for n, g in R.GRAPHS.items() if g.branch == "entropy_tail"])
def test_entropy_graphs_round_away_from_ties(name):
    """round() is a discontinuity: no value the entropy graphs round lies within ROUND_MARGIN of a half-integer, and
    float32 and float64 take the same decisions, so the float32 error of the operand (1e-5 at the most here) cannot flip
    one on any side; the Gaussian graphs' scales stay above the 0.11 bound, where lower_bound's backward is the derivative"""
    m64, v64, sc = R.rounding_margin(name)
    m32, v32, _ = R.rounding_margin(name, R.F32)
    print(f"{name}: nearest half-integer at {m64:.2e}")
    assert m64 > R.ROUND_MARGIN and m32 > R.ROUND_MARGIN
    assert torch.equal(torch.round(v64), torch.round(v32).double())
    assert (v64 - v32.double()).abs().max().item() < 0.1 * R.ROUND_MARGIN
    if sc is not None:
        assert sc.min().item() > 0.2
