"""CPU: the weight-gradient reference of tests/_wgrad_ref.py against torch's own weight gradients, and every case of its
tables against the branch it is named for -- the planner (icm_debug_wgrad_plan, icm_wgrad_workspace_floats*: host code
of the cross-compiled library, as in tests/test_host_logic.py) is asked, the host-path predicates are evaluated, and
every `grid` case is shown to be unable to round.  Fails when a shape stops reaching its branch: the shape is then
changed, not the assertion."""
import math

import pytest
import torch
import torch.nn.functional as F

import _wgrad_ref as R

F64 = torch.float64
KSP = sorted({(g.KH, g.KW, g.stride, g.pad) for g in R.ALL_GEOMS + R.WINO_GEOMS + R.VEC_RAGGED + [R.INT32_G]})


def small_geom(k, s, p):
    """a small geometry of this kernel / stride / pad: odd sizes, and for stride 2 a big grid whose last row only some
    taps reach"""
    KH, KW = k
    OH, OW = 5, 6
    HW = None
    if s == 2:
        h, w = (OH - 1) * s + KH - 2 * p, (OW - 1) * s + KW - 2 * p
        HW = (h + 1, w + 1) if (h + 1 + 2 * p - KH) // s + 1 == OH and (w + 1 + 2 * p - KW) // s + 1 == OW else None
    return R.geom(2, OH, OW, k, s, p, ch=(5, 3), HW=HW)


def close(a, b, what):
    err = (a - b).abs().max().item()
    scale = max(b.abs().max().item(), 1e-300)
    assert err <= 1e-12 * scale, f"{what}: {err:.3e} of {scale:.3e}"


@pytest.mark.parametrize("KH,KW,s,p", KSP)
def test_wgrad64_is_torchs_weight_gradient(KH, KW, s, p):
    """conv orientation: torch.nn.grad.conv2d_weight; transposed: autograd of F.conv_transpose2d with gs = x, gb = dY"""
    g = small_geom((KH, KW), s, p)
    gs = torch.rand((g.N, g.Ca, g.OH, g.OW), dtype=F64) * 2 - 1
    gb = torch.rand((g.N, g.Cb, g.H, g.W), dtype=F64) * 2 - 1
    dw, db = R.wgrad64(gs, gb, g)
    want = torch.nn.grad.conv2d_weight(gb, (g.Ca, g.Cb, KH, KW), gs, stride=s, padding=p)
    close(dw.reshape(g.Ca, g.Cb, KH, KW), want, "conv")
    close(db, gs.sum((0, 2, 3)), "dbias")
    w = torch.zeros((g.Ca, g.Cb, KH, KW), dtype=F64, requires_grad=True)
    oph, opw = g.H - ((g.OH - 1) * s - 2 * p + KH), g.W - ((g.OW - 1) * s - 2 * p + KW)
    assert 0 <= oph < s and 0 <= opw < s
    y = F.conv_transpose2d(gs, w, stride=s, padding=p, output_padding=(oph, opw))
    assert y.shape == gb.shape
    (wt,) = torch.autograd.grad(y, w, gb)
    close(dw.reshape(g.Ca, g.Cb, KH, KW), wt, "transposed conv")


def test_activations_and_zero_fill():
    x = torch.linspace(-6, 6, 101, dtype=F64)
    assert (R.act64(x, R.GELU) - F.gelu(x)).abs().max() < 1e-15
    assert torch.equal(R.act64(x, R.SQUARE), x * x) and torch.equal(R.act64(x, R.NONE), x)
    # the activation applies to the operands, the zero fill to what lies outside the image
    g = small_geom((3, 3), 1, 1)
    gs, gb = R.make_input(g, "real", "gs"), R.make_input(g, "real", "gb")
    a, _ = R.wgrad64(gs, gb, g, R.GELU, R.SQUARE)
    b, _ = R.wgrad64(F.gelu(gs.double()), gb.double() ** 2, g)
    close(a, b, "activations")
    ones = torch.ones_like(gs)
    taps = R.gather_taps(torch.ones_like(gb).double(), g)
    assert taps.shape == (9, g.Cb, g.N * g.OH * g.OW)
    assert taps[4].min() == 1 and taps[0].reshape(g.Cb, g.N, g.OH, g.OW)[:, :, 0, :].max() == 0
    assert R.wgrad64(ones, torch.ones_like(gb), g)[0][0, 0, 4] == g.N * g.OH * g.OW


def test_inputs():
    g = R.ONE_TRIP[1]
    for name in ("gs", "gb", "dw", "dbias"):
        v = R.make_input(g, "grid", name)
        assert torch.equal(v, v.round()) and v.min() == -2 and v.max() == 2
        assert not torch.equal(v, R.make_input(g, "grid", name, 1))
        r = R.make_input(g, "real", name)
        assert r.min() >= -1 and r.max() < 1 and r.dtype == torch.float32
    assert len(set(R.make_input(g, "grid", "gs").reshape(-1).tolist())) == 5


def test_float32_restatement_order():
    idx = R.split_order(10, 4, 2)          # chunks [0 1 2] [3 4 5] [6 7] [8 9]: split 0 takes chunks 0, 2; split 1 chunks 1, 3
    assert idx[:, 0].tolist() == [0, 1, 2, 6, 7] and idx[:, 1].tolist() == [3, 4, 5, 8, 9]
    g = R.ONE_TRIP[4]
    p = R.plan(g)
    gs, gb = R.make_input(g, "real", "gs"), R.make_input(g, "real", "gb")
    w32, b32 = R.wgrad32_ordered(gs, gb, g, R.NONE, R.NONE, p.ntiles, p.nsplit)
    w64, b64 = R.wgrad64(gs, gb, g)
    lim, e32 = R.limit(w32, w64)
    assert 0 < e32 < 64 * R.U * w64.abs().max() * math.sqrt(g.N * g.OH * g.OW) and lim >= R.FACTOR * e32
    # on grid inputs the float32 restatement is exact in any order
    gs, gb = R.make_input(g, "grid", "gs"), R.make_input(g, "grid", "gb")
    w32, b32 = R.wgrad32_ordered(gs, gb, g, R.SQUARE, R.NONE, 7, 3)
    w64, b64 = R.wgrad64(gs, gb, g, R.SQUARE, R.NONE)
    assert torch.equal(w32.double(), w64) and torch.equal(b32.double(), b64)
    assert R.FACTOR == 4


# ================================================================================================ the cases reach their branches
def ok_plan(g, **kw):
    p = R.plan(g, **kw)
    assert p.rc == 0, (R.gname(g), kw, p.rc)
    return p


def test_one_trip_and_tiny():
    for g in R.ONE_TRIP:
        p = ok_plan(g)
        assert p.nsplit == p.ntiles and R.trips(p) == (1, 1)
        assert g.OW % p.TW and g.OH % p.TH, "ragged tiles in x and y"
        assert g.Ca % 32 and g.Cb % 32, "channel tails"
    for g, ti in zip(R.TINY, R.TINY_TI):
        p = ok_plan(g)
        assert p.TI == ti and g.N % ti, "a batch tail inside the tile"
    assert ok_plan(R.TINY[2]).npx == 32


def test_multi_trip_reaches_reuse_and_ragged_trips():
    """per kernel size: every family the planner admits has a forced variant whose workgroups run >= 3 trips (both LDS
    buffers reused) with a ragged last trip (niter differing between workgroups)"""
    for k in (1, 3, 5):
        fams, ragged = set(), set()
        for g in [g for g in R.MULTI_TRIP if g.KH == k]:
            for v in range(R.NVARIANTS):
                p = R.plan(g, variant=v)
                if p.rc:
                    continue
                fams.add(p.family)
                lo, hi = R.trips(p)
                assert hi >= 3, (R.gname(g), v)
                if p.ntiles % p.nsplit:
                    assert lo == hi - 1
                    ragged.add(p.family)
        assert ragged == fams, (k, fams, ragged)
    # tile sizes of 16, 32 and 64 pixels are all forced somewhere
    sizes = {R.plan(g, variant=v).npx for g in R.ONE_TRIP + R.MULTI_TRIP for v in range(R.NVARIANTS) if R.plan(g, variant=v).rc == 0}
    assert {16, 32, 64} <= sizes
    # the largest shape: exactly three trips of the 25-tap kernel, which is also the automatic choice there
    p = ok_plan(R.MULTI_TRIP[3], variant=10)
    assert R.trips(p) == (3, 3) and ok_plan(R.MULTI_TRIP[3]).variant == 10
    p = ok_plan(R.MULTI_TRIP_VEC)
    assert R.trips(p)[1] >= 3 and R.MULTI_TRIP_VEC.OW % 4 == 0


def test_variant_admission():
    """which rows the planner admits per kernel size, and that a refused row is ICM_ERR_UNSUPPORTED"""
    rows = R.variant_table(R.ONE_TRIP + R.MULTI_TRIP)
    assert all(rc in (R.OK, R.ERR_UNSUPPORTED) for _, _, rc in rows)
    adm = lambda g: {v for gg, v, rc in rows if gg == g and rc == 0}
    assert adm(R.ONE_TRIP[0]) == adm(R.MULTI_TRIP[0]) == set(range(8)) | {11, 12, 13, 14}
    assert adm(R.ONE_TRIP[1]) == adm(R.MULTI_TRIP[1]) == set(range(10))
    assert adm(R.ONE_TRIP[4]) == adm(R.MULTI_TRIP[3]) == {0, 1, 3, 6, 7, 10}
    for v in (3, 6, 7):
        assert R.plan(R.ONE_TRIP[4], variant=v).npx == 16
    for g, v, rc in rows:
        if rc == 0:
            p = R.plan(g, variant=v)
            assert p.variant == v and p.family == R.FAMILY[v]
    # every family is launched
    assert {R.FAMILY[v] for _, v, rc in rows if rc == 0} == set(R.FAMILY)


def test_blocks_convT_odd_kernels_deep_reduce():
    for g in R.BLOCKS:
        for v in (0,) + ((-1,) if g.Ca == 200 else ()):
            ba, bb = R.BLOCK[ok_plan(g, variant=v).variant]
            assert g.Ca > ba and g.Ca % ba and g.Cb > bb and g.Cb % bb, "several blocks, ragged last block, both directions"
    # nsplit < ntiles with one problem: every (200, 196) shape on the automatic choice; at (100, 70) the 5x5, and the 1x1
    # under the 64 x 32 blocks of variant 0.  The 24-tile 3x3 at (100, 70) keeps one trip per workgroup: it is there for
    # its blocks alone
    short = lambda g, v: ok_plan(g, variant=v).nsplit < ok_plan(g, variant=v).ntiles
    assert [short(g, -1) for g in R.BLOCKS] == [True, True, True, False, False, True]
    assert [short(g, 0) for g in R.BLOCKS] == [True, True, True, False, True, True]
    p = ok_plan(R.BLOCKS[2], variant=0)
    assert p.tpg == 13 and R.BLOCKS[2].Cb > R.BLOCK[0][1], "two tap groups, several b-blocks"
    for g in R.CONVT:
        assert ok_plan(g).rc == 0 and g.Ca < g.Cb and g.stride == 2
    assert R.CONVT[1].H % 2 == 1 and R.CONVT[1].W % 2 == 1
    taps = []
    for g in R.ODD_KERNELS:
        p = ok_plan(g)
        taps.append(g.KH * g.KW)
        assert p.family == "general"
    assert taps == [4, 16, 3, 15]
    assert ok_plan(R.ODD_KERNELS[1], variant=0).tpg == 8 and ok_plan(R.ODD_KERNELS[3], variant=0).tpg == 8, "the halves rule"
    for g, v in zip(R.DEEP_REDUCE, R.DEEP_VARIANT):
        p = ok_plan(g)
        assert p.nsplit == 256 and (v is None or p.variant == v)
    lay = R.layout(R.DEEP_REDUCE[0], 1)
    assert R.host_paths(R.DEEP_REDUCE[0], ok_plan(R.DEEP_REDUCE[0]), lay)["reduce"] == "float4" and 256 > 7 * 16
    assert R.host_paths(R.DEEP_REDUCE[1], ok_plan(R.DEEP_REDUCE[1]), R.layout(R.DEEP_REDUCE[1], 1))["reduce"] == "taps"
    for g, code in R.REFUSED_KERNELS:
        assert R.plan(g).rc == code and R.workspace_floats(g) == -1


def test_activations_leave_the_dma_families():
    for g in R.ONE_TRIP_CROSS + R.DEEP_REDUCE:
        assert ok_plan(g).family in R.DMA_FAMILIES or g in R.ONE_TRIP_CROSS[1:]
        for a_s, a_b in ((R.GELU, R.NONE), (R.NONE, R.SQUARE), (R.SQUARE, R.GELU)):
            assert ok_plan(g, act_s=a_s, act_b=a_b).family not in R.DMA_FAMILIES
            for v in (8, 9, 10, 11, 12, 13, 14):
                assert R.plan(g, act_s=a_s, act_b=a_b, variant=v).rc == R.ERR_UNSUPPORTED
    for c in R.cross_cases():
        p = ok_plan(c["g"], act_s=c["act_s"], act_b=c["act_b"], variant=c["variant"])
        assert c["variant"] < 0 or p.variant == c["variant"]


def test_cross_forces_every_admitted_family():
    """the argument cross: for every (geometry, activations) each family the planner admits is launched, by the
    automatic choice or by a forced row, and no forced case repeats the plan of its `auto` sibling"""
    cross = R.cross_cases()
    for g in R.ONE_TRIP_CROSS:
        for a_s in (R.NONE, R.GELU, R.SQUARE):
            for a_b in (R.NONE, R.GELU, R.SQUARE):
                auto = ok_plan(g, act_s=a_s, act_b=a_b)
                forced = R.forced_variants(g, a_s, a_b)
                plans = [ok_plan(g, act_s=a_s, act_b=a_b, variant=v) for v in forced]
                assert all(p.variant == v != auto.variant and p != auto for p, v in zip(plans, forced))
                assert {auto.family} | {p.family for p in plans} == R.admitted_families(g, a_s, a_b), (R.gname(g), a_s, a_b)
                got = {c["variant"] for c in cross if c["g"] == g and (c["act_s"], c["act_b"]) == (a_s, a_b)}
                assert got >= set(forced) | {-1}
        # every other argument of the cross is applied to every one of these rows
        rows = set(R.forced_variants(g)) | {-1}
        assert len(rows) >= 5 and R.admitted_families(g) >= {"general", "t33", "t33_tapw"}
        plain = [c for c in cross if c["g"] == g and (c["act_s"], c["act_b"]) == (R.NONE, R.NONE)]
        for pick in (lambda c: not c["dbias"], lambda c: c["accum_bias"] and c["dbias"], lambda c: c["accum"],
                     lambda c: c["dw_ld"] == g.Cb + 3, lambda c: c["dw_ld"] == g.Cb + 8, lambda c: c["dw_ld"] == g.Cb,
                     lambda c: c["gs_stride"] == "slice", lambda c: c["gs_stride"] == "odd", lambda c: c["gb_stride"] == "slice",
                     lambda c: c["gb_stride"] == "odd", lambda c: c["ws_mode"] == "unchecked", lambda c: c["ws_mode"] == "larger",
                     lambda c: c["inputs"] == "real") + tuple((lambda c, m=m: c["misalign"] == m) for m in ("gs", "gb", "dw", "ws")):
            assert {c["variant"] for c in plain if pick(c)} == rows
    assert len({c["id"] for c in cross}) == len(cross)
    # the multi-trip rows that also run on `real` inputs name every admitted family
    for g in R.MULTI_TRIP[:4]:
        assert {R.FAMILY[v] for v in R.real_variant_rows(g)} == R.admitted_families(g)


def test_vec_cases_land_on_their_side():
    taken = {}
    for c, exp in R.vec_cases():
        g = c["g"]
        p = ok_plan(g, act_s=c["act_s"], act_b=c["act_b"], variant=c["variant"])
        lay = R.layout(g, 1, c["gs_stride"], c["gb_stride"], c["dw_ld"], c["misalign"], c["ws_mode"])
        got = R.host_paths(g, p, lay, c["act_s"], c["act_b"])
        for k, v in exp.items():
            assert got[k] == v, (c["id"], k, got)
        for k, v in got.items():
            taken.setdefault((k, v), []).append(c["id"])
    for key in (("gs_vec4", True), ("gs_vec4", False), ("pg", "vec4"), ("pg", "dma"), ("pg", "planes"), ("dma16", True),
                ("dma16", False), ("reduce", "float4"), ("reduce", "taps")):
        assert key in taken, key
    # a ragged last float4 column: OW is a multiple of 4 and no multiple of the tile width
    for g in R.VEC_RAGGED:
        p = ok_plan(g, variant=3)
        assert g.OW % 4 == 0 and g.OW % p.TW
    # the cross reaches the scalar loader and the odd-stride forms as well
    for c in R.cross_cases():
        g = c["g"]
        p = ok_plan(g, act_s=c["act_s"], act_b=c["act_b"], variant=c["variant"])
        lay = R.layout(g, 1, c["gs_stride"], c["gb_stride"], c["dw_ld"], c["misalign"], c["ws_mode"])
        got = R.host_paths(g, p, lay, c["act_s"], c["act_b"])
        if g.KH == 1 and c["dw_ld"] == g.Cb + 3:
            assert got["reduce"] == "taps"
        if g.KH == 1 and c["dw_ld"] in (0, g.Cb + 8) and c["misalign"] not in ("dw", "ws"):
            assert got["reduce"] == "float4"


def test_group_plans():
    for g in R.GROUP_GEOMS:
        splits = [ok_plan(g, n=n).nsplit for n in R.GROUP_NS]
        assert splits[-1] < splits[0], "the planner gives a group of 32 fewer splits than a single launch"
        assert R.workspace_floats(g, n=32) < R.workspace_floats(g, n=1)
    for g in R.GROUP_GEOMS[2:]:
        p = ok_plan(g, n=32)
        assert p.nsplit == 8 and 9 <= R.trips(p)[1] <= 12
    ms = R.group_members(R.GROUP_GEOMS[0], 32, "grid")
    assert {m["accum"] for m in ms} == {0, 1} and {m["dbias"] for m in ms} == {True, False} and len({m["dw_ld"] for m in ms}) == 4


def test_winograd_plans():
    want = {3: (124, 1116), 4: (18, 36)}
    for i, g in enumerate(R.WINO_GEOMS):
        nsplit, nchunks = R.wino_splits(g)
        assert 1 <= nsplit <= nchunks
        if i in want:
            assert (nsplit, nchunks) == want[i]
    assert R.wino_splits(R.WINO_GEOMS[3])[1] // R.wino_splits(R.WINO_GEOMS[3])[0] == 9
    assert R.wino_splits(R.WINO_GEOMS[4], 32)[0] == 2
    g = R.WINO_GEOMS[4]
    assert g.Ca % 64 and g.Cb % 64 and g.Ca > 64 and g.Cb > 64
    # 65 536 tiles are refused by the workspace query (the launch is never made); 64 512 are accepted
    assert R.workspace_floats(R.geom(16, 128, 128, 3, 1, 1), algo=R.WINOGRAD) == -1
    assert R.workspace_floats(R.geom(16, 128, 126, 3, 1, 1), algo=R.WINOGRAD) > 0
    for g, kw in ((R.ONE_TRIP[3], {}), (R.ONE_TRIP[5], {}), (R.ONE_TRIP[2], {}), (R.ONE_TRIP[1], dict(act_s=R.GELU))):
        assert R.workspace_floats(g, algo=R.WINOGRAD, **kw) == -1


def test_int32_guard():
    g = R.INT32_G
    assert R.int32_guard_refuses(g, R.INT32_REFUSED_BS) and not R.int32_guard_refuses(g, R.INT32_LARGEST_BS)
    assert R.int32_guard_refuses(g, R.INT32_LARGEST_BS + 1)
    assert R.INT32_LARGEST_BS >= g.Cb * g.H * g.W and ok_plan(g).rc == 0


# ================================================================================================ grid cases cannot round
def grid_cases():
    out = [c for c in R.geometry_cases() + R.cross_cases() + R.wino_cases() + [c for c, _ in R.vec_cases()] if c["inputs"] == "grid"]
    out += [R.case("v", g, variant=v) for g, v, rc in R.variant_table(R.ONE_TRIP + R.MULTI_TRIP) if rc == 0]
    for g in R.GROUP_GEOMS:
        out += R.group_members(g, 3, "grid")
    out += R.group_members(R.WINO_GEOMS[4], 2, "grid", algo=R.WINOGRAD) + [R.case("int32", R.INT32_G)]
    return out


def test_grid_cases_cannot_round():
    """sum |terms| + |prefill| < 2^24 for every distinct (geometry, activations, algo) of the grid cases, and for
    Winograd 16 x the same sum over the transformed operands"""
    seen = {}
    for c in grid_cases():
        assert R.GELU not in (c["act_s"], c["act_b"]), c["id"]
        key = (c["g"], c["act_s"], c["act_b"], c["algo"])
        seen[key] = max(seen.get(key, 0), c["accum"] | c["accum_bias"])
    assert len(seen) > 40
    worst = 0
    for (g, a_s, a_b, algo), accum in seen.items():
        m = R.grid_headroom(g, a_s, a_b, accum, algo)
        assert m < 2 ** 24, (R.gname(g), a_s, a_b, algo, m)
        worst = max(worst, m)
    print("largest grid partial sum bound: %d of %d" % (worst, 2 ** 24))
    # members of a group draw their own data: same distribution, checked for the largest group geometry
    for i in range(1, 3):
        assert R.grid_headroom(R.GROUP_GEOMS[3], R.NONE, R.NONE, 1, member=i) < 2 ** 24
