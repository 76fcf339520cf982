"""What tests/test_gpu_winattn_numerics.py relies on, checked without a GPU: the plain-torch attention core of
tests/_winattn_ref.py restates the oracle's WinBasedAttention, the ``hot`` inputs give peaked softmax rows, the
``leak`` inputs put the -100 of the shift mask in competition with the un-masked logits (none / about half / all of a
row's mass on masked keys at L = 60 / 100 / 140), and the float32 evaluation the GPU limits are formed from is itself
close to float64.  Prints the shares and the float32 errors (pytest -s).  The routing entry is host code, so the
kernel family every case is meant to reach is asserted here too."""
import pytest
import torch
import torch.nn.functional as F

import _winattn_ref as R
from oracle import wacnn_oracle as O
from oracle import weights as Wt

HOT_SHARE_MIN = 0.70
LEAK_LOW_MAX, LEAK_HIGH_MIN, LEAK_MID_SHARE_MIN = 1e-6, 0.99, 0.50
ALL_CASES = R.MATRIX + [R.LDS_CASE] + R.REDUCTION


@pytest.mark.parametrize("ws,shift,H,W", [(4, 0, 8, 12), (4, 3, 12, 8), (8, 0, 16, 8), (8, 5, 8, 24)])
def test_core_restates_the_oracle(ws, shift, H, W):
    heads, C, N = 2, 16, 2
    p = f"ref.ws{ws}.s{shift}"
    sd = {p + ".attn.qkv.weight": Wt._u(p + "qw", (3 * C, C), -0.25, 0.25).double(),
          p + ".attn.qkv.bias": Wt._u(p + "qb", (3 * C,), -0.05, 0.05).double(),
          p + ".attn.proj.weight": Wt._u(p + "pw", (C, C), -0.25, 0.25).double(),
          p + ".attn.proj.bias": Wt._u(p + "pb", (C,), -0.05, 0.05).double(),
          p + ".attn.relative_position_bias_table": Wt._u(p + "t", ((2 * ws - 1) ** 2, heads), -0.5, 0.5).double()}
    x = Wt._u(p + "x", (N, C, H, W), -1.0, 1.0).double()
    qkv = F.conv2d(x, sd[p + ".attn.qkv.weight"][:, :, None, None], sd[p + ".attn.qkv.bias"])
    o = R.core(qkv, sd[p + ".attn.relative_position_bias_table"], heads, ws, shift)
    y = x + F.conv2d(o, sd[p + ".attn.proj.weight"][:, :, None, None], sd[p + ".attn.proj.bias"])
    ref = O.win_based_attention(x, sd, p, heads, ws, shift)
    err = (y - ref).abs().max().item()
    print(f"core vs oracle ws {ws} shift {shift}: {err:.3e}")
    assert err <= 1e-12


def test_region_code_separates_the_mask_labels():
    """inside every window two tokens are masked from each other exactly when their region codes differ"""
    for H, W, ws, shift in ((8, 16, 8, 3), (8, 8, 4, 1), (10, 5, 5, 2), (7, 14, 7, 6), (4, 6, 2, 1)):
        code = torch.roll(R.region_code(H, W, shift), shifts=(-shift, -shift), dims=(0, 1))
        cw = code.view(H // ws, ws, W // ws, ws).permute(0, 2, 1, 3).reshape(-1, ws * ws)
        differ = cw.unsqueeze(1) != cw.unsqueeze(2)
        assert torch.equal(differ, O.shift_mask(H, W, ws, shift) != 0)


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_hot_rows_are_peaked(case):
    p, _ = R.probabilities(case, "hot")
    share = (p.max(-1).values > 0.5).double().mean().item()
    print(f"hot {case.name}: rows with a probability above 0.5: {share:.3f}")
    assert share >= HOT_SHARE_MIN, (case.name, share)


@pytest.mark.parametrize("case", [c for c in ALL_CASES if c.shift > 0], ids=lambda c: c.name)
def test_leak_puts_the_mask_constant_in_play(case):
    res = {}
    for L in R.LEAKS:
        p, masked = R.probabilities(case, f"leak{L}")
        mass = (p * masked[:, None].double()).sum(-1)                  # [windows, heads, T]
        rows = masked.any(-1)[:, None].expand_as(mass)
        res[L] = mass[rows]
    assert res[100].numel() > 0
    mid = ((res[100] >= 0.01) & (res[100] <= 0.99)).double().mean().item()
    print(f"leak {case.name}: rows with masked keys {res[100].numel()}, masked mass L=60 max {res[60].max().item():.3e}, "
          f"L=140 min {res[140].min().item():.6f}, L=100 share in [0.01, 0.99] {mid:.3f}")
    if "leak60" in R.input_sets(case):
        assert res[60].max().item() < LEAK_LOW_MAX
        assert res[140].min().item() > LEAK_HIGH_MIN
    assert mid >= LEAK_MID_SHARE_MIN, (case.name, mid)


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_float32_oracle_error(case):
    """the yardstick itself: finite, and small against the tensor it measures"""
    for kind in R.input_sets(case):
        ref = R.reference(case.name, kind)
        own = R.oracle_error(ref)
        print(f"{case.name} {kind}: float32 oracle error / limit / ref max  "
              + "  ".join(f"{t} {own[t]:.2e}/{ref.lim[t]:.2e}/{ref.x64[t].abs().max().item():.2e}" for t in R.TENSORS))
        for t in R.TENSORS:
            scale = max(ref.x64[t].abs().max().item(), 1e-30)
            assert own[t] == own[t] and own[t] <= 1e-3 * scale, (case.name, kind, t, own[t], scale)


def test_every_case_reaches_the_family_it_is_meant_for():
    """icm_debug_winattn_route makes no HIP call: the route column of the case list, the test hook and the refusals"""
    from icm_amd import _lib
    lib = _lib.lib()
    try:
        for case in ALL_CASES:
            lib.icm_debug_force_winattn_valu(case.force)
            got = tuple(lib.icm_debug_winattn_route(*R.geometry(case), b) for b in (0, 1))
            assert got == case.route, (case.name, got)
            if case.force:
                continue
            lib.icm_debug_force_winattn_valu(1)      # the hook sends everything to the VALU kernels, or refuses
            forced = tuple(lib.icm_debug_winattn_route(*R.geometry(case), b) for b in (0, 1))
            assert all(r in (R.ROUTE_VALU, -R.ERR_UNSUPPORTED) for r in forced), (case.name, forced)
    finally:
        lib.icm_debug_force_winattn_valu(0)
    seen = {(r, c.hd) for c in R.MATRIX for r in c.route}
    assert {(R.ROUTE_MFMA, h) for h in (8, 16, 24, 32, 48)} <= seen
    assert {(R.ROUTE_MFMA16, h) for h in (8, 16, 24, 32, 40)} <= seen
    assert {(c.ws, c.hd) for c in R.MATRIX if c.route == R.V} >= {
        (8, 10), (8, 40), (8, 8), (8, 16), (8, 24), (8, 32), (4, 10), (4, 48), (4, 8), (4, 16), (4, 24), (4, 32), (4, 40),
        (1, 8), (2, 8), (3, 8), (5, 8), (6, 8), (7, 8), (5, 10), (7, 16), (2, 48)}
    for geo, code in (((1, 8, 4, 4, 1, 4, 4), R.ERR_ARG), ((1, 8, 6, 4, 1, 4, 0), R.ERR_ARG),
                      ((1, 10, 4, 4, 3, 4, 0), R.ERR_ARG), ((1, 8, 9, 9, 1, 9, 0), R.ERR_UNSUPPORTED),
                      ((1, 12, 4, 4, 1, 4, 0), R.ERR_UNSUPPORTED)):
        assert [lib.icm_debug_winattn_route(*geo, b) for b in (0, 1)] == [-code, -code], geo


def test_recorded_routes_replay():
    """tests/golden/winattn_routes.npz (tests/golden/make_winattn_routes.py): every recorded row gets the family, the
    refusal code and the backward workspace size it got when the fixture was written"""
    import os
    import numpy as np
    from icm_amd import _lib
    lib = _lib.lib()
    rec = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "winattn_routes.npz"))
    args, route, wsf = rec["args"], rec["route"], rec["wsf"]
    assert len(args) >= 3000 and len(args) == len(route) == len(wsf)
    bad = []
    try:
        for row, want_r, want_w in zip(args.tolist(), route.tolist(), wsf.tolist()):
            force, geo = row[0], row[1:]
            lib.icm_debug_force_winattn_valu(force)
            got_r = [lib.icm_debug_winattn_route(*geo, b) for b in (0, 1)]
            got_w = lib.icm_winattn_bwd_workspace_floats(*geo[:6])
            if got_r != want_r or got_w != want_w:
                bad.append((row, got_r, want_r, got_w, want_w))
    finally:
        lib.icm_debug_force_winattn_valu(0)
    assert not bad, (len(bad), bad[:5])
