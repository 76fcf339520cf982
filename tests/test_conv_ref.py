"""CPU: the float64 reference, the limit rule and the case tables of the convolution numerics suite
(tests/_conv_ref.py), and -- asked of the library's own planner, which is host code -- that every case of
tests/test_gpu_conv_numerics.py reaches the regime it is named for.  No GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

import _conv_ref as R
import _pointwise_ref as PR

F64 = torch.float64
KERNELS = sorted({(g.KH, g.KW, g.stride, g.pad) for g in R.ONE_TRIP + R.TRANSPOSED_S2 + R.TINY})


def rnd(*shape):
    return torch.rand(*shape, dtype=F64, generator=torch.Generator().manual_seed(sum(shape))) * 2 - 1


def scatter_torch(x, w_oi, g):
    """F.conv_transpose2d without its crop, then the window [pad, pad + OH) x [pad, pad + OW) with zero fill"""
    full = F.conv_transpose2d(x, w_oi.permute(1, 0, 2, 3).contiguous(), stride=g.stride)
    full = F.pad(full, (0, g.pad + g.OW, 0, g.pad + g.OH))
    return full[:, :, g.pad:g.pad + g.OH, g.pad:g.pad + g.OW]


# ================================================================================================ the reference
@pytest.mark.parametrize("KH,KW,s,p", KERNELS, ids=["%dx%ds%dp%d" % k for k in KERNELS])
def test_conv64_is_torchs_convolution_and_input_gradient(KH, KW, s, p):
    """gather = F.conv2d and the autograd input gradient of F.conv_transpose2d; scatter = F.conv_transpose2d and the
    autograd input gradient of F.conv2d; to 1e-12, odd and even output sizes"""
    for OH, OW in ((7, 9), (6, 4), (1, 5)):
        if (OH - 1) * s + KH - 2 * p < 1:
            continue                                  # no input grid gives a single output row under this padding
        g = R.geom(2, OH, OW, (KH, KW), s, p, ch=(5, 3))
        c = R.case("t", g, bias=False)
        x, w = rnd(2, 5, g.H, g.W), rnd(3, 5, KH, KW)
        acc, ab = R.contract64(x, w, c)
        want = F.conv2d(x, w, stride=s, padding=p)
        assert (acc - want).abs().max() < 1e-12 and (ab - F.conv2d(x.abs(), w.abs(), stride=s, padding=p)).abs().max() < 1e-12
        # its input gradient is the scatter form with the same weights, roles exchanged
        gt = R.Geom(2, 3, 5, OH, OW, g.H, g.W, KH, KW, s, p, 1)
        dy = rnd(2, 3, OH, OW)
        xr = x.clone().requires_grad_(True)
        (F.conv2d(xr, w, stride=s, padding=p) * dy).sum().backward()
        got, _ = R.contract64(dy, w.permute(1, 0, 2, 3), R.case("t", gt, bias=False))
        assert (got - xr.grad).abs().max() < 1e-12
        assert (got - scatter_torch(dy, w.permute(1, 0, 2, 3), gt)).abs().max() < 1e-12
        # the gather form is the input gradient of the transposed convolution
        dyr = dy.clone().requires_grad_(True)
        (scatter_torch(dyr, w.permute(1, 0, 2, 3), gt) * x).sum().backward()
        assert (acc - dyr.grad).abs().max() < 1e-12
    for g in [q for q in R.TRANSPOSED_S2 + R.ONE_TRIP if q.transposed and (q.KH, q.KW, q.stride, q.pad) == (KH, KW, s, p)]:
        x, w = rnd(g.N, g.Cin, g.H, g.W), rnd(g.Cout, g.Cin, KH, KW)
        got, _ = R.contract64(x, w, R.case("t", g, bias=False))
        assert (got - scatter_torch(x, w, g)).abs().max() < 1e-12, R.gname(g)


def test_operand_activation_channel_map_and_shuffle():
    g = R.geom(2, 5, 6, 3, 1, 1, ch=(40, 8))
    c = R.case("t", g, seg=(12, 4), pro_act=R.SQUARE)
    assert R.phys_channels(c) == 40 + 3 * 4 and R.channel_planes(c).tolist()[11:14] == [11, 16, 17]
    x, w = rnd(2, 52, 5, 6), rnd(8, 40, 3, 3)
    acc, _ = R.contract64(x, w, c)
    keep = [p for p in range(52) if p % 16 < 12]
    assert (acc - F.conv2d(x[:, keep] ** 2, w, padding=1)).abs().max() < 1e-12
    cg = R.case("t", g, pro_act=R.GELU, inputs="real")
    assert (R.contract64(x[:, :40], w, cg)[0] - F.conv2d(F.gelu(x[:, :40]), w, padding=1)).abs().max() < 1e-12
    v = rnd(2, 8, 3, 5)
    assert torch.equal(R.shuffle2(v), F.pixel_shuffle(v, 2))
    assert (PR.gelu(v) - F.gelu(v)).abs().max() < 1e-15


@pytest.mark.parametrize("epi", R.EPI_ALL, ids=R.EPI_NAMES)
def test_epilogue_kinds(epi):
    g = R.geom(2, 4, 5, 3, 1, 1, ch=(8, 8))
    sq = epi in (R.E_GDN, R.E_IGDN)
    for ps in (0, 2):
        for accum in (0, 1):
            for y2 in ("none", "sep") + (("same",) if R.may_gelu(epi) else ()):
                c = R.case("t", g, epi=epi, pro_act=R.SQUARE if sq else R.NONE, inputs="real", ps=ps, accum=accum, y2=y2)
                t = R.make_inputs(c)
                o, acc, _ = R.conv64(c, t)
                v = acc + t["bias"].double().view(1, -1, 1, 1)
                v = F.pixel_shuffle(v, 2) if ps else v
                res, aux, aux2, pre = (t[k].double() for k in ("res", "aux", "aux2", "prefill"))
                side = None
                if epi == R.E_RES:
                    v = v + res
                if epi == R.E_RES_GELU:
                    v = v + F.gelu(res)
                if sq:
                    side, v = v, aux * (v ** -0.5 if epi == R.E_GDN else v ** 0.5)
                    assert side.min() >= 1
                if epi == R.E_MUL_DGELU:
                    v = v * torch.autograd.functional.jacobian(lambda a: F.gelu(a).sum(), aux)
                if epi == R.E_RES_MUL_DGELU:
                    v = (v + res) * torch.autograd.functional.jacobian(lambda a: F.gelu(a).sum(), aux)
                if epi == R.E_AXPY2:
                    v = aux2 + 2 * aux * v
                if epi == R.E_LRP:
                    side = torch.tanh(v)
                    v = aux + 0.5 * side
                if accum:
                    v = v + pre
                if y2 == "none" or not (R.side_kind(epi) or R.may_gelu(epi)):
                    want, want2 = v, None
                elif R.side_kind(epi):
                    want, want2 = v, side
                elif y2 == "same":
                    want, want2 = F.gelu(v), None
                else:
                    want, want2 = v, F.gelu(v)
                assert (o.y - want).abs().max() < 1e-12
                assert (o.y2 is None) == (want2 is None) and (want2 is None or (o.y2 - want2).abs().max() < 1e-12)


def test_inputs():
    c = R.case("t", R.G3)
    t = R.make_inputs(c)
    for k, v in t.items():
        assert v.dtype == torch.float32 and set(v.unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}, k
    assert len(t["x"].unique()) == 5 and not torch.equal(t["res"], t["aux"])
    tg = R.make_inputs(R.case("t", R.G3, epi=R.E_GDN, pro_act=R.SQUARE))
    assert tg["w"].min() == 0 and tg["bias"].min() == 1 and tg["bias"].max() == 2
    tr = R.make_inputs(R.case("t", R.G3, inputs="real"))
    assert -1 <= tr["x"].min() < -0.99 and 0.99 < tr["x"].max() < 1
    assert not torch.equal(R.make_inputs(R.case("t", R.G3, member=1))["x"], t["x"])
    trg = R.make_inputs(R.case("t", R.G3, inputs="real", epi=R.E_IGDN, pro_act=R.SQUARE))
    assert trg["w"].min() >= 0 and trg["bias"].min() >= 1


def test_float32_restatement_orders():
    """the three chain layouts differ from each other in float32 and all equal the exact result on `grid`"""
    g = R.multi_trip_geom(3)
    cr, cg = R.case("t", g, inputs="real"), R.case("t", g)
    tr, tg = R.make_inputs(cr), R.make_inputs(cg)
    exact = R.conv64(cg)[1]
    outs = []
    for order in (("serial",), ("ks", 2, 5), ("ks", 4, 5), ("ks8",)):
        assert torch.equal(R.acc32_direct(tg["x"], tg["w"], cg, order).double(), exact)
        outs.append(R.acc32_direct(tr["x"], tr["w"], cr, order))
    for i in range(len(outs)):
        for j in range(i):
            assert not torch.equal(outs[i], outs[j])
    w = R.case("t", R.G3, algo=R.WINOGRAD)
    assert torch.equal(R.acc32_wino(R.make_inputs(w)["x"], R.make_inputs(w)["w"], w).double(), R.conv64(w)[1])
    wt = R.case("t", R.WINO_GEOMS[7], algo=R.WINOGRAD)
    assert wt["g"].transposed
    assert torch.equal(R.acc32_wino(R.make_inputs(wt)["x"], R.make_inputs(wt)["w"], wt).double(), R.conv64(wt)[1])


TEETH = [("staged", R.case("t", R.G3, cfg=9)), ("ks-row", R.case("t", R.G3, cfg=12)), ("ks8", R.case("t", R.G3, cfg=R.CFG_KS8_64)),
         ("pointwise", R.case("t", R.geom(3, 11, 13, 1, 1, 0), f1x1=1)), ("winograd", R.case("t", R.G3, algo=R.WINOGRAD)),
         ("transposed", R.case("t", R.G5T))]


@pytest.mark.parametrize("fam,c", TEETH, ids=[t[0] for t in TEETH])
def test_limit_has_teeth(fam, c):
    """a tap dropped from one output tile, a channel dropped from the last K group, one pixel taking its neighbour's
    value: each exceeds the `real` limit and breaks the `grid` equality; the restatement itself passes both"""
    p = R.plan(c)
    assert p.rc == R.OK and R.FAMILY_NAMES[p.family] == {"ks-row": "staged", "winograd": "wino44", "transposed": "staged"}.get(fam, fam)
    real = dict(c, inputs="real")
    o64, acc64, _ = R.conv64(real)
    lim = R.limits(real, R.acc32(real, p))
    assert (R.epilogue(R.acc32(real, p), real, R.make_inputs(real), R.FN32).y.double() - o64.y).abs().max().item() <= lim.y
    exact = R.conv64(c)[1]
    assert torch.equal(R.acc32(c, p).double(), exact)
    for fault in ("tap", "channel", "pixel"):
        bad = R.acc32(real, p, fault)
        y = R.epilogue(bad, real, R.make_inputs(real), R.FN32).y
        err = (y.double() - o64.y).abs().max().item()
        assert err > lim.y, (fam, fault, err, lim.y)
        assert not torch.equal(R.acc32(c, p, fault).double(), exact), (fam, fault)


# ================================================================================================ the tables
def all_grid_cases():
    import test_gpu_conv_numerics as T
    return T.all_cases()


def test_grid_cases_cannot_round():
    """grid_headroom of every distinct grid contraction of the GPU file: below 2^24"""
    seen, worst = set(), (0, None)
    for c in all_grid_cases():
        k = R.ckey(c) + (c["accum"], c["epi"] == R.E_AXPY2, c["algo"])
        if c["inputs"] != "grid" or k in seen:
            continue
        seen.add(k)
        h = R.grid_headroom(c)
        worst = max(worst, (h, c["id"]), key=lambda v: v[0])
        assert h < 2 ** 24, (c["id"], h)
    assert len(seen) > 60
    print("\nlargest grid headroom: %g of %g (%s)" % (worst[0], 2.0 ** 24, worst[1]))
    assert worst[0] < 2 ** 21                     # DESIGN quotes the figure: 3 bits to spare at the least


def test_every_case_is_valid_for_the_planner():
    """every launch case plans with ICM_OK under its forced configuration (refusal cases are listed apart)"""
    for c in all_grid_cases():
        for p in R.class_plans(c):
            assert p.rc == R.OK, (c["id"], p)


# ================================================================================================ reach
def test_one_trip_tiny_and_classes():
    for g in R.ONE_TRIP:
        for k, p in enumerate(R.class_plans(R.case("t", g))):
            assert p.rc == R.OK and (p.nblk == 0 or g.KH * g.KW > 9 or R.trips(R.case("t", g), p) == 1), (R.gname(g), k, p)
    assert R.plan(R.case("t", R.REFUSED_KERNEL)).rc == R.ERR_UNSUPPORTED
    assert all(R.plan(R.case("t", R.TINY_REFUSED, cfg=cfg)).rc == R.ERR_UNSUPPORTED for cfg in [R.CFG_AUTO] + R.forced_configs())
    assert R.plan(R.case("t", R.TINY_REFUSED._replace(N=1))).rc == R.ERR_UNSUPPORTED     # the tile, not the batch
    assert R.plan(R.case("t", R.geom(33, 1, 2, 5, 1, 2))).rc == R.OK
    assert R.plan(R.case("t", R.ONE_TRIP[-1])).rc == R.OK and R.ONE_TRIP[-1].KH * R.ONE_TRIP[-1].KW == 32
    # several images per tile, a batch tail inside a tile
    for g in R.TINY:
        p = R.plan(R.case("t", g))
        assert p.rc == R.OK and p.family == R.STAGED and p.lgTI >= 1 and g.N % (1 << p.lgTI), (R.gname(g), p)
    # transposed stride 2: four classes with their own tap counts; OH = 1 leaves the cy = 1 classes empty
    for g in R.TRANSPOSED_S2:
        cls = R.build_classes(g)
        ps = R.class_plans(R.case("t", g))
        assert len(cls) == 4 == ps[0].classes and sum(len(c.taps) for c in cls) == g.KH * g.KW
        for cl, p in zip(cls, ps):
            oh, ow = R.class_grid(g, cl)
            assert (p.nblk == 0) == (oh * ow == 0)
        assert (g.OH == 1) == (ps[2].nblk == 0 and ps[3].nblk == 0) and ps[0].nblk > 0
        offs = [p.off for p in ps if p.nblk]
        assert offs == sorted(set(offs))
    assert {g.OH % 2 for g in R.TRANSPOSED_S2} == {0, 1}


def test_multi_trip_and_blocks():
    for k in (1, 3, 5):
        g = R.multi_trip_geom(k)
        p = R.plan(R.case("t", g))
        n8 = R.cdiv(g.Cin, 8)
        assert p.family == R.STAGED and R.cdiv(n8, p.ckm) >= 3 and n8 % p.ckm and g.Cin % 8 and g.H * g.W <= 64
    for g in R.BLOCKS:
        assert R.cdiv(g.Cout, 32) == 7
        for cfg in [R.CFG_AUTO] + list(range(R.NROWS)):
            for k, p in enumerate(R.class_plans(R.case("t", g, cfg=cfg))):
                if p.rc or p.family != R.STAGED:
                    continue
                wco, wpx, tco, tpx, ks = R.ROWS[p.row]
                assert p.ncb == R.cdiv(7, wco * tco) and (7 % (wco * tco) or wco * tco == 1 or wco * tco == 7)
                if cfg == R.CFG_AUTO:
                    TW, TH = 1 << p.lgTW, 1 << p.lgTH
                    oh, ow = R.class_grid(g, R.build_classes(g)[k])
                    assert ow % TW and (oh % TH or TH == 1), "ragged tiles in x and y"


def test_forced_rows():
    """every staged row and both K-split blocks are reached under force; a refusal is the refusal of class 0 (nothing
    launched before it); a forced configuration does not repeat its automatic sibling's plan"""
    rows, ks8 = set(), set()
    for g, cfg, rc in R.forced_row_table():
        c = R.case("t", g, cfg=cfg)
        ps = R.class_plans(c)
        assert rc == ps[0].rc and rc in (R.OK, R.ERR_UNSUPPORTED)
        if rc:
            continue
        if cfg < R.NROWS:
            assert all(p.family == R.STAGED and p.row == cfg for p in ps if p.nblk)
            rows.add(cfg)
        elif ps[0].family == R.KS8:
            assert R.ks8_admits(c) and ps[0].row == (2 if cfg == R.CFG_KS8_64 else 1)
            ks8.add(cfg)
        else:
            assert not R.ks8_admits(c) or len(R.build_classes(g)[0].taps) <= 1
    assert rows == set(range(R.NROWS)) and ks8 == {R.CFG_KS8_64, R.CFG_KS8_128}
    for g in R.forced_row_geoms():
        assert any(rc == R.OK and cfg in (10, 11, 12) for gg, cfg, rc in R.forced_row_table() if gg == g)
    for c in R.cross_cases():
        if c["cfg"] != R.CFG_AUTO and c["pro_act"] == R.NONE and c["epi"] == R.E_NONE and not c["seg"]:
            a, f = R.plan(dict(c, cfg=R.CFG_AUTO)), R.plan(c)
            assert (a.family, a.row) != (f.family, f.row), c["id"]


def test_automatic_k_split_choice():
    c = R.KS8_AUTO
    p = R.plan(c)
    assert c["cfg"] == R.CFG_AUTO and p.family == R.KS8 and p.row == 2 and 160 <= p.nblk * R.KS8_AUTO_N <= 256 and R.ks8_admits(c)
    # each argument condition of plan_ks8 sends the launch back to the staged kernel
    for kw in (dict(pro_act=R.SQUARE), dict(epi=R.E_AXPY2), dict(seg=(112, 8))):
        assert R.plan(dict(c, **kw)).family == R.STAGED and not R.ks8_admits(dict(c, **kw))


def test_cross_families_and_kinds():
    fams = {}
    for c in R.cross_cases():
        ps = [p for p in R.class_plans(c) if p.nblk]
        assert all(p.rc == R.OK for p in ps), c["id"]
        fam = {p.family for p in ps}
        assert len(fam) == 1
        fam = fam.pop()
        fams.setdefault(c["id"].split("-")[0], set()).add(fam)
        if fam == R.KS8:
            assert c["epi"] in R.EPI_KS8 and c["pro_act"] == R.NONE and not c["seg"], c["id"]
        if c["cfg"] in (R.CFG_KS8_64, R.CFG_KS8_128) and not R.ks8_admits(c):
            assert fam == R.STAGED, c["id"]            # a kind outside EpiKs8 leaves the family
        if c["f1x1"] == 1:
            assert (fam == R.P1) == R.pointwise_eligible(c), c["id"]
            if c["ps"] or c["seg"]:
                assert fam == R.STAGED
    assert fams["1x1"] == {R.STAGED, R.P1} and fams["3x3"] == {R.STAGED, R.KS8} and fams["T5x5s2"] == {R.STAGED, R.KS8}
    # every kind x operand activation is in the cross for every family that is compiled for it
    for tag, fam, kinds in (("1x1-p1", R.P1, R.EPI_ALL), ("3x3-ks8", R.KS8, R.EPI_KS8), ("3x3-auto", R.STAGED, R.EPI_ALL)):
        got = {(c["epi"], c["pro_act"]) for c in R.cross_cases() if c["id"].startswith(tag) and R.plan(c).family == fam}
        for e in kinds:
            acts = (R.SQUARE,) if e in (R.E_GDN, R.E_IGDN) else ((R.NONE,) if fam == R.KS8 else (R.NONE, R.GELU, R.SQUARE))
            assert {(e, a) for a in acts} <= got, (tag, R.EPI_NAMES[e])


def test_staging_forms_land_on_their_side():
    for c, form, knocked in R.staging_cases():
        p = R.plan(c)
        assert p.rc == R.OK and p.family == R.STAGED and p.row == c["cfg"], c["id"]
        got = "vec4" if p.vec4 else ("dma" if p.dma else "planes")
        want, why = R.staging_form(c, p)
        assert got == want == form, (c["id"], got, want, why)
        if knocked:                                      # knocked out by exactly this condition (or this pair)
            assert why == ([knocked] if isinstance(knocked, str) else list(knocked)), (c["id"], why)
    assert {f for _, f, _ in R.staging_cases()} == {"vec4", "dma", "planes"}
    # the predicates agree with the planner on every other case too
    for c in R.cross_cases():
        for k, p in enumerate(R.class_plans(c)):
            if p.nblk and p.family == R.STAGED:
                assert ("vec4" if p.vec4 else ("dma" if p.dma else "planes")) == R.staging_form(c, p, k)[0], (c["id"], k)


def test_pointwise_rows():
    """which rows of kCfgs1x1 any geometry reaches: the planner swept over 1 - 24 co tiles, pixel counts to 2^20 and 1 / 2 /
    12 members.  Row 7 <2,1> is reached by none: with equal efficiency it never has more waves than row 5 <1,2>, and a
    tie goes to the earlier row.  It runs only under ICM_1X1_CFG (the child-process test of the GPU file)."""
    first = R.pointwise_sweep()
    assert set(first) == set(range(8)) - set(R.POINTWISE_UNREACHABLE) == set(R.pointwise_row_cases())
    for row, (n, g) in R.pointwise_row_cases().items():
        c = R.case("t", g, f1x1=1)
        p = R.plan(c, n)
        assert p.family == R.P1 and p.row == row == R.pointwise_row(g, n)[0], (row, n, g, p)
        tco, tpx = R.ROWS_1X1[row]
        assert g.Cout % 32 and (g.N * g.H * g.W) % (32 * tpx), "co tail, ragged last strip"
        if row not in (5, 6):                         # the smaller launches of a row's co-tile count go elsewhere
            small = g._replace(H=max(1, g.H // 2), OH=max(1, g.H // 2))
            assert R.plan(R.case("t", small, f1x1=1), n).row != row
    for g in R.POINTWISE_CHUNKS:
        assert R.plan(R.case("t", g, f1x1=1)).family == R.P1
    assert [g.Cin // 8 for g in R.POINTWISE_CHUNKS] == [1, 3, 40]
    # the automatic threshold, both sides
    big = R.pointwise_row_cases()[3][1]
    assert R.pointwise_auto(big, 12) and R.plan(R.case("t", big), 12).family == R.P1
    assert not R.pointwise_auto(R.G1._replace(Cin=40)) and R.plan(R.case("t", R.G1)).family == R.STAGED
    # the module-level shapes of tests/test_gpu_ops.py: what their comments must say
    from test_gpu_ops import P1_CASES
    rows = {name: R.plan(R.case("t", R.Geom(N, Cin, Cout, H, Wd, H, Wd, 1, 1, 1, 0, 0), f1x1=1)).row
            for name, N, Cin, H, Wd, Cout in P1_CASES}
    assert set(rows.values()) == {5, 6}, rows


def test_winograd_plans():
    seen = set()
    for c, n in [(c, 1) for c in R.wino_cases()] + [(c, R.WINO_W8_N) for c in R.W8_CASES]:
        p = R.plan(c, n)
        assert p.rc == R.OK and R.wino_supported(c), c["id"]
        fam, tco, px_fast, ncb, nblk = R.wino_plan_expect(c, n)
        assert (p.family, p.row, p.dma, p.ncb, p.nblk) == (fam, tco, px_fast, ncb, nblk), (c["id"], p)
        assert p.vec4 == int(c["xv"])
        seen.add((p.family, p.row, p.dma, R.wino_transform_vec(c["g"]) if c["xv"] else None))
    for c in R.W8_CASES:
        if "N25" in c["id"]:                          # two images per tile and a batch tail, on the eight-wave kernel
            p = R.plan(c)
            assert p.family == R.WINO8 and p.lgTI == 1 and c["g"].N % 2 == 1 and p.row == int(c["id"][9])
    got = {(c["epi"], c["accum"], c["bias"], c["y2"]) for c in R.W8_CASES if "N25" in c["id"]}
    assert len(got) == len(R.W8_VARIANTS) and {k for c in R.W8_CASES for k in c["strides"]} == {"x", "y", "res", "aux", "y2"}
    fams = {(f, t) for f, t, _, _ in seen}
    assert {(R.WINO44, 1), (R.WINO44, 2), (R.WINO8, 2), (R.WINO8, 3), (R.WINO8, 4)} <= fams, fams
    assert {d for _, _, d, _ in seen} == {0, 1} and {v for _, _, _, v in seen} == {None, False, True}
    assert R.WINO_PXFAST_G.Cin == 224 and R.plan(R.case("t", R.WINO_PXFAST_G, algo=R.WINOGRAD)).dma == 1
    for g in (R.G3S2, R.ONE_TRIP[4], R.geom(3, 11, 13, 5, 1, 2)):
        assert R.plan(R.case("t", g, algo=R.WINOGRAD)).rc == R.ERR_UNSUPPORTED
    for e in set(R.EPI_ALL) - set(R.EPI_WINO):
        c = R.case("t", R.G3, algo=R.WINOGRAD, epi=e, pro_act=R.SQUARE if e in (R.E_GDN, R.E_IGDN) else R.NONE)
        assert R.plan(c).rc == R.ERR_UNSUPPORTED and not R.wino_supported(c)


def test_group_limits_and_int32_guard():
    c = R.case("t", R.G3)
    assert R.plan(c, 12).rc == R.OK and R.plan(c, 13).rc == R.ERR_ARG and R.plan(c, 0).rc == R.ERR_ARG
    g = R.INT32_G
    assert R.int32_guard_refuses(g, R.INT32_REFUSED_BS) and not R.int32_guard_refuses(g, R.INT32_LARGEST_BS)
    assert R.int32_guard_refuses(g, R.INT32_LARGEST_BS + 1)
    a = R.conv_args(c=R.case("t", g))
    a.x_bs = R.INT32_REFUSED_BS
    assert R.plan_args(a).rc == R.ERR_UNSUPPORTED
    a.x_bs = R.INT32_LARGEST_BS + 1
    assert R.plan_args(a).rc == R.ERR_UNSUPPORTED
    a.x_bs = R.INT32_LARGEST_BS
    assert R.plan_args(a).rc == R.OK


def test_refusal_table_codes():
    """validate() and check_group() are host code: every row of the GPU file's refusal table (the named views apart) gets
    its code from the planner too, so no row of it can reach a launch"""
    import types
    import test_gpu_conv_numerics as T
    assert len(T.REFUSALS) >= 80
    seen = set()
    for rid, g, kw, nm, tweak, view, code in T.REFUSALS:
        ms = [types.SimpleNamespace(args=R.conv_args(R.case(rid, g, member=i, **kw))) for i in range(nm)]
        if view:
            assert R.plan_array([m.args for m in ms], nm) == R.OK and ms[0].args.transposed == (view in ("icm_conv2d_fwd", "icm_convT2d_dgrad"))
            continue
        if tweak:
            tweak(ms)
        assert R.plan_array([m.args for m in ms], nm) == code, rid
        if rid.startswith("member-differs-in-"):      # every member valid alone: the code is check_group's comparison
            field = rid[len("member-differs-in-"):]
            assert nm == 2 and all(R.plan_array([m.args], 1) == R.OK for m in ms), rid
            assert getattr(ms[0].args, field) != getattr(ms[1].args, field), rid
            for f, _ in ms[0].args._fields_:            # ... and of this field alone
                assert f == field or f in ("x", "wp", "y") or getattr(ms[0].args, f) == getattr(ms[1].args, f), (rid, f)
            seen.add(field)
    assert seen == {f for f, _ in ms[0].args._fields_} - {"x", "wp", "y"}, "every field check_group compares"
