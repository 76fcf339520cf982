"""The pointwise, LayerNorm, reduction, optimiser and layout kernels (csrc/pointwise.hip) through the C ABI against
float64, on every host-side branch: split counts and finish kernels, the fused and the split LayerNorm parameter pass,
persistent and grid-stride loops past their first trip, scalar and float4 load paths, null optional pointers, every
accum flag.

Operands with a batch stride are channel slices of their own wider NaN-filled buffers; flat operands sit between NaN
guards; an output written with accum = 0 starts as NaN and must come back finite; workspaces start as NaN.  Every limit
is tests/_pointwise_ref.py's (its docstring states the rule; none is taken from a kernel's output), and
tests/test_pointwise_ref.py asserts without a GPU that each case reaches the branch it is named for.  Every reduction
is called twice and must return the same bits.  Each check prints the measured figure next to its limit (pytest -s);
DESIGN.md "Pointwise-kernel numerics" holds one such run."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import _pointwise_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
F64 = torch.float64
ERR_ARG, ERR_UNSUPPORTED = 1, 3
WS_FLOATS = 8192                # ICM_REDUCE_WS_FLOATS


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def lib():
    from icm_amd import _lib
    return _lib


def call(name, *args):
    L = lib()
    L.check(getattr(L.lib(), name)(*args, L.stream()), name)


class Slice:
    """a [N, C, HW] channel slice, ``off`` channels into its own buffer of C + extra channels filled with NaN"""

    def __init__(self, shape, extra, off, value=None):
        N, Cc, HW = shape
        assert 0 <= off <= extra
        self.buf = torch.full((N, Cc + extra, HW), NAN, dtype=torch.float32, device=dev())
        self.off, self.C = off, Cc
        self.view = self.buf[:, off:off + Cc]
        if value is not None:
            self.view.copy_(value.reshape(shape))
        self.ptr, self.bs = self.view.data_ptr(), self.buf.stride(0)

    def cpu(self):
        return self.view.cpu()

    def guards_ok(self):
        b = self.buf.cpu()
        return bool(torch.isnan(b[:, :self.off]).all() and torch.isnan(b[:, self.off + self.C:]).all())


class Flat:
    """n floats between NaN guards; lead = 4 keeps the pointer 16-byte aligned, lead = 1 is base.data_ptr() + 4"""

    def __init__(self, n, value=None, lead=4, dtype=torch.float32):
        self.n, self.lead = int(n), lead
        self.buf = torch.full((self.n + lead + 4,), NAN, dtype=dtype, device=dev())
        self.view = self.buf[lead:lead + self.n]
        if value is not None:
            self.view.copy_(value.reshape(-1))
        self.ptr, self.bs = self.view.data_ptr(), 0
        assert self.ptr == self.buf.data_ptr() + 4 * lead and self.buf.data_ptr() % 16 == 0

    def cpu(self):
        return self.view.cpu()

    def guards_ok(self):
        b = self.buf.cpu()
        return bool(torch.isnan(b[:self.lead]).all() and torch.isnan(b[self.lead + self.n:]).all())


class Null:
    ptr, bs = 0, 0

    @staticmethod
    def guards_ok():
        return True


def same_bits(a, b):
    a, b = a.cpu().contiguous().reshape(-1), b.cpu().contiguous().reshape(-1)
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def guards(what, *bufs):
    for i, b in enumerate(bufs):
        assert b.guards_ok(), f"{what}: operand {i} was written outside its extent"


def finite(what, *outs):
    for o in outs:
        assert torch.isfinite(o.cpu()).all(), f"{what}: an output kept (or read) its NaN prefill"


def check_bound(what, got, ref64, lim):
    """|got - ref64| <= lim element by element, printing the worst ratio"""
    got = got.cpu().double().reshape(ref64.shape)
    err = (got - ref64).abs()
    ratio = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err / lim)
    w = int(ratio.argmax())
    e, l = err.reshape(-1)[w].item(), lim.reshape(-1)[w].item()
    print(f"{what}: gpu {e:.3e}, limit {l:.3e} ({e / l:.2f} of it)")
    assert bool((err <= lim).all()), f"{what}: {e:.3e} > limit {l:.3e}"


def ulps(x64, n):
    return n * R.ULP * x64.abs()


NS = pytest.mark.parametrize("n", R.ELEMENT_NS, ids=lambda n: "n%d%s" % (n, "-second-grid-trip" if n == R.LONG_N else ""))


# ================================================================================================ channel sum
@pytest.mark.parametrize("accum", [0, 1], ids=["accum0", "accum1"])
@pytest.mark.parametrize("case", R.CHANNEL_SUM_CASES, ids=lambda c: c["id"])
def test_channel_sum(case, accum):
    N, Cc, HW = case["N"], case["C"], case["HW"]
    xv = R.u("cs.x", (N, Cc, HW), -1.0, 2.0)
    prev = R.u("cs.prev", (Cc,), -50.0, 50.0)
    layout = case["layout"]
    if layout == "slice":
        x = Slice((N, Cc, HW), 3, 1, xv)
        ptr, bs = x.ptr, x.bs
        assert bs % 4 == 0 and ptr % 16 == 0
    elif layout == "oddstride":
        x = Slice((N, 1, Cc * HW + 2), 0, 0)             # [N, C*HW + 2]: two NaN floats behind every sample
        x.buf[:, 0, :Cc * HW] = xv.reshape(N, -1).to(dev())
        ptr, bs = x.ptr, Cc * HW + 2
    else:
        x = Flat(N * Cc * HW, xv, lead=1 if layout == "misaligned" else 4)
        ptr, bs = x.ptr, Cc * HW
        assert (ptr % 16 == 0) == (layout != "misaligned")
    wsf = R.channel_sum_ws_floats(case)
    g = R.channel_sum_geometry(N, Cc, HW, wsf, case["vec"])
    assert g["S"] == case["S"]
    outs = []
    for _ in range(2):
        out = Flat(Cc, prev if accum else None)
        ws = Null if wsf is None else Flat(wsf)
        call("icm_channel_sum", ptr, bs, N, Cc, HW, out.ptr, accum, ws.ptr, 0 if wsf is None else wsf)
        guards(case["id"], out, ws)
        outs.append(out.cpu())
    assert same_bits(outs[0], outs[1]), "channel_sum: two runs differ"
    x64 = xv.double()
    ref = R.channel_sum(x64) + (prev.double() if accum else 0)
    terms = x64.abs().sum((0, 2)) + (prev.double().abs() if accum else 0)
    finite(case["id"], out)
    R.check_sum(f"channel_sum {case['id']} accum={accum}", outs[0], ref, g["k"], terms)


# ================================================================================================ LayerNorm
def ln_forward(N, Cc, HW, stats_modes=(True, False)):
    c = R.layernorm_case(N, Cc, HW)
    shape = (N, Cc, HW)
    x64, g64, b64 = c["x"].double(), c["gamma"].double(), c["beta"].double()
    lim_mean, lim_rstd, floor_y = R.layernorm_fwd_limits(x64, g64, b64, c["y64"], c["mean64"], c["rstd64"])
    y32 = c["y32"]
    x = Slice(shape, 2, 1, c["x"])
    gam, bet = Flat(Cc, c["gamma"]), Flat(Cc, c["beta"])
    for stats in stats_modes:
        what = f"layernorm fwd C={Cc} N={N} HW={HW} stats={int(stats)}"
        y = Slice(shape, 3, 2)
        assert y.bs != x.bs
        mean, rstd = (Flat(N * HW), Flat(N * HW)) if stats else (Null, Null)
        call("icm_layernorm_fwd", x.ptr, x.bs, gam.ptr, bet.ptr, y.ptr, y.bs, mean.ptr, rstd.ptr, N, Cc, HW, R.LN_EPS)
        guards(what, x, y, mean, rstd, gam, bet)
        assert same_bits(x.cpu(), c["x"]), what + ": x changed"
        finite(what, y)
        if stats:
            check_bound(what + " mean", mean.cpu(), c["mean64"], lim_mean)
            check_bound(what + " rstd", rstd.cpu(), c["rstd64"], lim_rstd)
        R.check_elementwise(what + " y", y.cpu(), y32, c["y64"], floor_y)


@pytest.mark.parametrize("stats", [True, False], ids=["mean-rstd-set", "mean-rstd-null"])
@pytest.mark.parametrize("N,HW", R.LN_NHW, ids=["N1-HW1", "N1-HW63", "N1-HW64", "N1-HW65", "N2-HW65-tile-spans-batch"])
@pytest.mark.parametrize("Cc", R.LN_CS, ids=lambda c: ("cached-C%d" if c in R.LN_CACHED else "generic-C%d") % c)
def test_layernorm_fwd(Cc, N, HW, stats):
    ln_forward(N, Cc, HW, stats_modes=(stats,))


@pytest.mark.parametrize("N,Cc,HW", R.LN_LONG, ids=["generic-C5", "cached-C48"])
def test_layernorm_fwd_persistent_loop(N, Cc, HW):
    assert R.ln_fwd_geometry(N, Cc, HW)["tiles_per_wg"] == 2
    ln_forward(N, Cc, HW, stats_modes=(True,))


# (outputs, accum_dx, accum_params, dx_extra) -- every combination the requested outputs take part in
LN_COMBOS = ([("dx", a, 0, e) for a in (0, 1) for e in (0, 1)] + [("params", 0, a, 0) for a in (0, 1)]
             + [("both", ad, ap, e) for ad in (0, 1) for ap in (0, 1) for e in (0, 1)])
LN_FEW = [("both", 0, 0, 0), ("both", 1, 1, 1), ("params", 0, 1, 0)]


def ln_backward(N, Cc, HW, ws_floats, combos):
    c = R.layernorm_case(N, Cc, HW)
    shape = (N, Cc, HW)
    need_extras = any(ad or e for _, ad, _, e in combos)
    extra_v, prev_v = R.layernorm_extras(N, Cc, HW) if need_extras else (None, None)
    m32, r32 = c["mean32"], c["rstd32"]                   # the statistics backward is given: the reference's, rounded
    x64, dy64, g64 = c["x"].double(), c["dy"].double(), c["gamma"].double()
    dx64, dg64, db64 = R.layernorm_bwd(x64, dy64, g64, m32.double(), r32.double())
    dx32, dg32, db32 = R.layernorm_bwd(c["x"], c["dy"], c["gamma"], m32, r32)
    xh64 = (x64 - m32.double()[:, None]) * r32.double()[:, None]
    terms_g, terms_b = (dy64 * xh64).abs().sum((0, 2)), dy64.abs().sum((0, 2))
    del xh64
    x, dy = Slice(shape, 1, 0, c["x"]), Slice(shape, 2, 2, c["dy"])
    gam, mean, rstd = Flat(Cc, c["gamma"]), Flat(N * HW, m32), Flat(N * HW, r32)
    extra = Slice(shape, 4, 3, extra_v) if need_extras else None
    for outs, accum_dx, accum_p, use_extra in combos:
        want_dx, want_p = outs in ("dx", "both"), outs in ("params", "both")
        g = R.ln_bwd_geometry(N, Cc, HW, want_dx, want_p, ws_floats)
        what = (f"layernorm bwd C={Cc} N*HW={N * HW} ws={ws_floats} {outs} accum_dx={accum_dx} accum_params={accum_p} "
                f"extra={use_extra} [{'fused' if g['fused'] else 'split'} S={g['S']} {g['finish']}]")
        runs = []
        for _ in range(2):
            dx = Slice(shape, 3, 1, prev_v if accum_dx else None) if want_dx else Null
            dgam = Flat(Cc, c["gprev"] if accum_p else None) if want_p else Null
            dbet = Flat(Cc, c["bprev"] if accum_p else None)        # dgamma null, dbeta set: no parameter pass at all
            ws = Null if ws_floats is None else Flat(ws_floats)
            ex = extra if use_extra else Null
            call("icm_layernorm_bwd", x.ptr, x.bs, dy.ptr, dy.bs, gam.ptr, mean.ptr, rstd.ptr, dx.ptr, dx.bs, dgam.ptr,
                 dbet.ptr, N, Cc, HW, accum_dx, accum_p, ex.ptr, ex.bs, ws.ptr, 0 if ws_floats is None else ws_floats)
            guards(what, dx, dgam, dbet, ws, x, dy)
            runs.append((dx.cpu() if want_dx else None, dgam.cpu() if want_p else None, dbet.cpu()))
        if want_dx:
            assert same_bits(runs[0][0], runs[1][0]), what + ": dx differs between two runs"
            r64, r32_ = dx64, dx32
            if use_extra:
                r64, r32_ = r64 + extra_v.double(), r32_ + extra_v
            if accum_dx:
                r64, r32_ = r64 + prev_v.double(), r32_ + prev_v
            floor = R.layernorm_bwd_floor(x64, dy64, g64, m32.double(), r32.double(),
                                          extra_v.double() if use_extra else None, prev_v.double() if accum_dx else None)
            finite(what, runs[0][0])
            R.check_elementwise(what + " dx", runs[0][0], r32_, r64, floor)
        if want_p:
            assert same_bits(runs[0][1], runs[1][1]) and same_bits(runs[0][2], runs[1][2]), \
                what + ": parameter gradients differ between two runs"
            pg, pb = (c["gprev"].double(), c["bprev"].double()) if accum_p else (0, 0)
            finite(what, runs[0][1], runs[0][2])
            R.check_sum(what + " dgamma", runs[0][1], dg64 + pg, g["k"], terms_g + (pg.abs() if accum_p else 0))
            R.check_sum(what + " dbeta", runs[0][2], db64 + pb, g["k"], terms_b + (pb.abs() if accum_p else 0))
        else:
            assert same_bits(runs[0][2], c["bprev"]) if accum_p else torch.isnan(runs[0][2]).all(), \
                what + ": dbeta written although dgamma is null"


LN_OUTPUTS = {"dx-only-dgamma-null": "dx", "params-only-dx-null": "params", "dx-and-params": "both"}


@pytest.mark.parametrize("outputs", list(LN_OUTPUTS))
@pytest.mark.parametrize("ws_kind", R.LN_WS_KINDS, ids=["ws-" + k for k in R.LN_WS_KINDS])
@pytest.mark.parametrize("Cc", R.LN_CS, ids=lambda c: ("cached-C%d" if c in R.LN_CACHED else "generic-C%d") % c)
def test_layernorm_bwd(Cc, ws_kind, outputs):
    """every accum_dx x accum_params x dx_extra combination the requested outputs take part in"""
    N, HW = R.LN_BWD_SHAPE
    ln_backward(N, Cc, HW, R.ln_ws_floats(ws_kind, Cc), [c for c in LN_COMBOS if c[0] == LN_OUTPUTS[outputs]])


@pytest.mark.parametrize("case", R.LN_BWD_BRANCH_CASES, ids=lambda c: c["id"])
def test_layernorm_bwd_branches(case):
    N, Cc, HW = case["N"], case["C"], case["HW"]
    wsf = R.ln_ws_floats(case["ws"], Cc)
    g = R.ln_bwd_geometry(N, Cc, HW, True, True, wsf)
    for key, want in case["expect"].items():
        assert g[key] == want
    ln_backward(N, Cc, HW, wsf, LN_FEW if N * HW < 100000 else LN_FEW[::2])


# ================================================================================================ elementwise
@NS
def test_nonneg_fwd_bwd(n):
    p, gv, prev = R.nonneg_inputs("nn.p", n), R.u("nn.g", (n,), -1.0, 1.0), R.u("nn.prev", (n,), -1e-3, 1e-3)
    bound, ped = R.NONNEG_BOUND, R.NONNEG_PED
    pd, gd = Flat(n, p), Flat(n, gv)
    out = Flat(n)
    call("icm_nonneg_fwd", pd.ptr, out.ptr, n, bound, ped)
    guards("nonneg_fwd", pd, out)
    p64 = p.double()
    v2 = torch.clamp_min(p64, bound) ** 2
    finite("nonneg_fwd", out)
    R.check_elementwise(f"nonneg_fwd n={n}", out.cpu(), R.nonneg_fwd(p, bound, ped), R.nonneg_fwd(p64, bound, ped),
                        ulps(v2, 1))
    for accum in (0, 1):
        dp = Flat(n, prev if accum else None)
        call("icm_nonneg_bwd", pd.ptr, gd.ptr, dp.ptr, n, bound, accum)
        guards("nonneg_bwd", pd, gd, dp)
        finite("nonneg_bwd", dp)
        r64 = R.nonneg_bwd(p64, gv.double(), bound, prev.double() if accum else None)
        r32 = R.nonneg_bwd(p, gv, bound, prev if accum else None)
        gg = (gv.double() * 2 * torch.clamp_min(p64, bound)).abs()
        R.check_elementwise(f"nonneg_bwd n={n} accum={accum}", dp.cpu(), r32, r64,
                            ulps(gg, 2) + (ulps(gg + prev.double().abs(), 1) if accum else 0))
        # the gate itself, exactly: below the bound only a negative gradient passes
        closed = (p < bound) & (gv >= 0)
        want = prev if accum else torch.zeros(n)
        assert torch.equal(dp.cpu()[closed], want[closed]), "nonneg_bwd: a gradient passed below the bound"


@pytest.mark.parametrize("inverse", [0, 1], ids=["gdn", "igdn"])
@NS
def test_gdn_bwd_pre(n, inverse):
    gv, xv = R.u("gdn.g", (n,), -1.0, 1.0), R.u("gdn.x", (n,), -3.0, 3.0)
    nrm = R.log_uniform("gdn.nrm", n, -6.0, 3.0)
    gd, xd, nd = Flat(n, gv), Flat(n, xv), Flat(n, nrm)
    dn, t1 = Flat(n), Flat(n)
    call("icm_gdn_bwd_pre", gd.ptr, xd.ptr, nd.ptr, dn.ptr, t1.ptr, n, inverse)
    guards("gdn_bwd_pre", gd, xd, nd, dn, t1)
    finite("gdn_bwd_pre", dn, t1)
    dn64, t64 = R.gdn_bwd_pre(gv.double(), xv.double(), nrm.double(), inverse)
    dn32, t32 = R.gdn_bwd_pre(gv, xv, nrm, inverse)
    # v_rsq_f32 (or the square root) 2 ulp, then a product; dn has a quotient and two more products
    R.check_elementwise(f"gdn_bwd_pre inverse={inverse} n={n} t1", t1.cpu(), t32, t64, ulps(t64, 3))
    R.check_elementwise(f"gdn_bwd_pre inverse={inverse} n={n} dn", dn.cpu(), dn32, dn64, ulps(dn64, 5))


@NS
def test_gelu_fwd(n):
    xv = R.gelu_inputs("gelu.x", n)
    xd, y = Flat(n, xv), Flat(n)
    call("icm_gelu_fwd", xd.ptr, y.ptr, n)
    guards("gelu_fwd", xd, y)
    finite("gelu_fwd", y)
    r64 = R.gelu(xv.double())
    R.check_elementwise(f"gelu_fwd n={n}", y.cpu(), R.gelu(xv), r64, R.gelu_floor(xv.double()) + ulps(r64, 2))


@NS
def test_gate_fwd(n):
    a, b, xv = R.gelu_inputs("gate.a", n), R.sigmoid_inputs("gate.b", n), R.u("gate.x", (n,), -2.0, 2.0)
    ad, bd, xd, out = Flat(n, a), Flat(n, b), Flat(n, xv), Flat(n)
    call("icm_gate_fwd", ad.ptr, bd.ptr, xd.ptr, out.ptr, n)
    guards("gate_fwd", ad, bd, xd, out)
    finite("gate_fwd", out)
    a64, b64 = a.double(), b.double()
    s64, ge64 = R.sigmoid(b64), R.gelu(a64)
    floor = R.gelu_floor(a64) * s64 + ulps(ge64 * s64, 5) + ulps((ge64 * s64).abs() + xv.double().abs(), 1)
    R.check_elementwise(f"gate_fwd n={n}", out.cpu(), R.gate_fwd(a, b, xv), R.gate_fwd(a64, b64, xv.double()), floor)


@pytest.mark.parametrize("accum_da,accum_dx", [(0, 0), (0, 1), (1, 0), (1, 1)])
@NS
def test_gate_bwd(n, accum_da, accum_dx):
    gv, a, b = R.u("gateb.g", (n,), -1.0, 1.0), R.gelu_inputs("gateb.a", n), R.sigmoid_inputs("gateb.b", n)
    pa, px = R.u("gateb.pa", (n,), -1.0, 1.0), R.u("gateb.px", (n,), -1.0, 1.0)
    gd, ad, bd = Flat(n, gv), Flat(n, a), Flat(n, b)
    da, db, dx = Flat(n, pa if accum_da else None), Flat(n), Flat(n, px if accum_dx else None)
    call("icm_gate_bwd", gd.ptr, ad.ptr, bd.ptr, da.ptr, db.ptr, dx.ptr, n, accum_da, accum_dx)
    guards("gate_bwd", gd, ad, bd, da, db, dx)
    finite("gate_bwd", da, db, dx)
    r64 = R.gate_bwd(gv.double(), a.double(), b.double(), pa.double() if accum_da else None,
                     px.double() if accum_dx else None)
    r32 = R.gate_bwd(gv, a, b, pa if accum_da else None, px if accum_dx else None)
    f_da, f_db = R.gate_bwd_floors(gv.double(), a.double(), b.double(), pa.double() if accum_da else None)
    what = f"gate_bwd n={n} accum_da={accum_da} accum_dx={accum_dx}"
    R.check_elementwise(what + " da", da.cpu(), r32[0], r64[0], f_da)
    R.check_elementwise(what + " db", db.cpu(), r32[1], r64[1], f_db)
    assert same_bits(dx.cpu(), gv + px if accum_dx else gv), what + ": dx is one float32 add"


@pytest.mark.parametrize("accum", [0, 1], ids=["accum0", "accum1"])
@pytest.mark.parametrize("with_dgelu", [0, 1], ids=["plain", "times-dgelu"])
@NS
def test_add_grad(n, with_dgelu, accum):
    src, pre, prev = R.u("ag.s", (n,), -1.0, 1.0), R.gelu_inputs("ag.p", n), R.u("ag.d", (n,), -1.0, 1.0)
    sd, pd = Flat(n, src), (Flat(n, pre) if with_dgelu else Null)
    dst = Flat(n, prev if accum else None)
    call("icm_add_grad", sd.ptr, pd.ptr, dst.ptr, n, accum)
    guards("add_grad", sd, pd, dst)
    finite("add_grad", dst)
    what = f"add_grad n={n} dgelu={with_dgelu} accum={accum}"
    if not with_dgelu:
        assert same_bits(dst.cpu(), src + prev if accum else src), what + ": a copy / one float32 add"
        return
    r64 = R.add_grad(src.double(), pre.double(), prev.double() if accum else None)
    r32 = R.add_grad(src, pre, prev if accum else None)
    floor = src.double().abs() * R.dgelu_floor(pre.double()) + ulps(r64, 1) + (ulps(prev.double(), 1) if accum else 0)
    R.check_elementwise(what, dst.cpu(), r32, r64, floor)


STRIDED_SHAPES = ((1, 1, 1), (3, 5, 17), (2, 2, 64), (5, 5, 41), (1, 7, 299605))
STRIDED_IDS = ["n1", "n255", "n256", "n1025", "second-grid-trip"]
assert [a * b * c for a, b, c in STRIDED_SHAPES][:4] == list(R.ELEMENT_NS[:4]) and 7 * 299605 > R.GRID_CAP * 1024


@pytest.mark.parametrize("shape", STRIDED_SHAPES, ids=STRIDED_IDS)
def test_lrp_bwd_three_strides(shape):
    N, Cc, HW = shape
    gv, tv = R.u("lrp.g", shape, -1.0, 1.0), torch.tanh(R.u("lrp.t", shape, -4.0, 4.0))
    g, t, d = Slice(shape, 1, 1, gv), Slice(shape, 2, 0, tv), Slice(shape, 3, 2)
    assert len({g.bs, t.bs, d.bs}) == 3
    call("icm_lrp_bwd", g.ptr, g.bs, t.ptr, t.bs, d.ptr, d.bs, N, Cc, HW)
    guards("lrp_bwd", g, t, d)
    finite("lrp_bwd", d)
    floor = ulps(0.5 * gv.double().abs() * (1 + tv.double() ** 2), 2)
    R.check_elementwise(f"lrp_bwd {shape}", d.cpu(), R.lrp_bwd(gv, tv), R.lrp_bwd(gv.double(), tv.double()), floor)


@pytest.mark.parametrize("shortcut", [0, 1], ids=["shortcut-null", "shortcut-set"])
@pytest.mark.parametrize("shape", STRIDED_SHAPES, ids=STRIDED_IDS)
def test_residual_scale(shape, shortcut):
    N, per = shape[0], shape[1] * shape[2]
    sc, br = R.u("rs.s", (N, per), -1.0, 1.0), R.u("rs.b", (N, per), -1.0, 1.0)
    scale = R.u("rs.k", (N,), 0.0, 2.0)
    scale[0] = 0.0                                               # a dropped path
    sd, bd, kd, out = (Flat(N * per, sc) if shortcut else Null), Flat(N * per, br), Flat(N, scale), Flat(N * per)
    call("icm_residual_scale", sd.ptr, bd.ptr, kd.ptr, out.ptr, N, per)
    guards("residual_scale", sd, bd, kd, out)
    finite("residual_scale", out)
    r64 = R.residual_scale(sc.double() if shortcut else None, br.double(), scale.double())
    r32 = R.residual_scale(sc if shortcut else None, br, scale)
    floor = ulps((scale.double()[:, None] * br.double()).abs() + (sc.double().abs() if shortcut else 0), 1)
    R.check_elementwise(f"residual_scale {shape} shortcut={shortcut}", out.cpu(), r32, r64, floor)
    if not shortcut:
        assert same_bits(out.cpu().reshape(N, per)[0].abs(), torch.zeros(per))


@NS
def test_fill_and_clamp(n):
    p = Flat(n)
    call("icm_fill", p.ptr, n, 0.3)
    guards("fill", p)
    assert same_bits(p.cpu(), torch.full((n,), 0.3))
    v = R.u("clamp.x", (n,), -3.0, 3.0)
    v[0] = -0.5
    q = Flat(n, v)
    call("icm_clamp", q.ptr, n, -0.5, 1.25)
    guards("clamp", q)
    assert same_bits(q.cpu(), torch.clamp(v, -0.5, 1.25))
    call("icm_clamp", q.ptr, n, 0.75, 0.75)                       # lo == hi is allowed
    assert same_bits(q.cpu(), torch.full((n,), 0.75))


@pytest.mark.parametrize("shape", STRIDED_SHAPES[:4], ids=STRIDED_IDS[:4])
def test_ste_round_offset(shape):
    N, Cc, HW = shape
    z, q = R.u("ste.z", shape, -9.0, 9.0), R.u("ste.q", (Cc, 1, 3), -2.0, 2.0)
    ties = torch.tensor([0.5, -0.5, 1.5, 2.5])[:HW]
    z[0, 0, :ties.numel()] = q[0, 0, 1] + ties
    zd, qd, out = Flat(N * Cc * HW, z), Flat(Cc * 3, q), Flat(N * Cc * HW)
    call("icm_ste_round_offset", zd.ptr, qd.ptr, out.ptr, N, Cc, HW)
    guards("ste_round_offset", zd, qd, out)
    assert same_bits(out.cpu(), R.ste_round_offset(z, q))


# ================================================================================================ layout
@pytest.mark.parametrize("accum", [0, 1], ids=["accum0", "accum1"])
@pytest.mark.parametrize("shape", STRIDED_SHAPES, ids=STRIDED_IDS)
def test_copy_strided(shape, accum):
    N, Cc, HW = shape
    sv, prev = R.u("cp.s", shape, -1.0, 1.0), R.u("cp.d", shape, -1.0, 1.0)
    s, d = Slice(shape, 2, 1, sv), Slice(shape, 3, 3, prev if accum else None)
    call("icm_copy_strided", s.ptr, s.bs, d.ptr, d.bs, N, Cc, HW, accum)
    guards("copy_strided", s, d)
    assert same_bits(d.cpu(), sv + prev if accum else sv) and same_bits(s.cpu(), sv)


@pytest.mark.parametrize("accum", [0, 1], ids=["accum0", "accum1"])
@pytest.mark.parametrize("A,B,K", R.PERMUTE_FLIP_CASES)
def test_permute_flip(A, B, K, accum):
    w, prev = R.u("pf.w", (A, B, K), -1.0, 1.0), R.u("pf.d", (B, A, K), -1.0, 1.0)
    s, d = Flat(A * B * K, w), Flat(A * B * K, prev if accum else None)
    call("icm_permute_flip", s.ptr, d.ptr, A, B, K, accum)
    guards("permute_flip", s, d)
    want = R.permute_flip(w)
    assert same_bits(d.cpu(), want + prev if accum else want)


@pytest.mark.parametrize("mode", ["forward", "inverse", "inverse-accum"])
def test_space_to_depth2(mode):
    N, Cc, H, W = 2, 3, 6, 10
    n = N * Cc * H * W
    if mode == "forward":
        xv = R.u("sd.x", (N, Cc, H, W), -1.0, 1.0)
        s, d = Flat(n, xv), Flat(n)
        call("icm_space_to_depth2", s.ptr, d.ptr, N, Cc, H, W, 0, 0)
        want = R.space_to_depth2(xv)
    else:
        accum = int(mode == "inverse-accum")
        gv, prev = R.u("sd.g", (N, 4 * Cc, H // 2, W // 2), -1.0, 1.0), R.u("sd.p", (N, Cc, H, W), -1.0, 1.0)
        s, d = Flat(n, gv), Flat(n, prev if accum else None)
        call("icm_space_to_depth2", s.ptr, d.ptr, N, Cc, H, W, 1, accum)
        want = R.depth_to_space2(gv)
        want = want + prev if accum else want
    guards("space_to_depth2", s, d)
    assert same_bits(d.cpu(), want)


def test_pixel_unshuffle2():
    N, Cc, H, W = 2, 3, 5, 7                                     # of the output [N, 4C, H, W]
    xv = R.u("pu.x", (N, Cc, 2 * H, 2 * W), -1.0, 1.0)
    s, d = Flat(xv.numel(), xv), Flat(xv.numel())
    call("icm_pixel_unshuffle2", s.ptr, d.ptr, N, Cc, H, W)
    guards("pixel_unshuffle2", s, d)
    assert same_bits(d.cpu(), R.pixel_unshuffle2(xv))


@pytest.mark.parametrize("top,left,OH,OW", R.PAD_CASES)
def test_pad2d(top, left, OH, OW):
    N, Cc, H, W = R.PAD_SHAPE
    xv = R.u("pad.x", R.PAD_SHAPE, -1.0, 1.0)
    s, d = Flat(xv.numel(), xv), Flat(N * Cc * OH * OW)
    call("icm_pad2d", s.ptr, N, Cc, H, W, d.ptr, OH, OW, top, left, 0.25)
    guards("pad2d", s, d)
    assert same_bits(d.cpu(), R.pad2d(xv, top, left, OH, OW, 0.25))


@pytest.mark.parametrize("K,S,pad", R.COL_CASES)
def test_im2col(K, S, pad):
    N, Cc, H, W = R.COL_SHAPE
    xv = R.u("col.x", R.COL_SHAPE, -1.0, 1.0)
    want = R.im2col(xv, K, S, pad)
    s, d = Flat(xv.numel(), xv), Flat(want.numel())
    call("icm_im2col", s.ptr, d.ptr, N, Cc, H, W, K, S, pad)
    guards("im2col", s, d)
    assert same_bits(d.cpu(), want)


def col2im_case(shape, K, S, pad, with_bias, accum):
    N, Cc, H, W = shape
    OH, OW = (H + 2 * pad - K) // S + 1, (W + 2 * pad - K) // S + 1
    cols = R.u("c2i.c", (N, Cc * K * K, OH, OW), -1.0, 1.0)
    bias, prev = R.u("c2i.b", (Cc,), -1.0, 1.0), R.u("c2i.p", shape, -1.0, 1.0)
    s, b = Flat(cols.numel(), cols), (Flat(Cc, bias) if with_bias else Null)
    d = Flat(N * Cc * H * W, prev if accum else None)
    call("icm_col2im", s.ptr, b.ptr, d.ptr, N, Cc, H, W, K, S, pad, accum)
    guards("col2im", s, b, d)
    finite("col2im", d)
    c64 = cols.double()
    ref = R.col2im(c64, H, W, K, S, pad, bias.double() if with_bias else None, prev.double() if accum else None)
    terms = R.col2im(c64.abs(), H, W, K, S, pad, bias.double().abs() if with_bias else None,
                     prev.double().abs() if accum else None)
    # at most K*K taps, the bias and the accumulated value on one serial chain
    R.check_sum(f"col2im {shape} K={K} S={S} pad={pad} bias={with_bias} accum={accum}", d.cpu().reshape(shape), ref,
                K * K + 2, terms)


@pytest.mark.parametrize("accum", [0, 1], ids=["accum0", "accum1"])
@pytest.mark.parametrize("with_bias", [0, 1])
@pytest.mark.parametrize("K,S,pad", R.COL_CASES)
def test_col2im(K, S, pad, with_bias, accum):
    col2im_case(R.COL_SHAPE, K, S, pad, with_bias, accum)


def test_col2im_second_grid_trip():
    shape = (1, 5, 527, 199)
    assert int(np.prod(shape)) == R.LONG_N1
    col2im_case(shape, 3, 1, 1, 1, 0)


@pytest.mark.parametrize("ns,nh,nw", R.ZIGZAG_CASES)
def test_zigzag(ns, nh, nw):
    B, Cc, H, W = 2, ns * 2, nh * 3, nw * 5
    xv = R.u("zz.x", (B, Cc, H, W), -1.0, 1.0)
    want = R.zigzag_splits(xv, ns, nh, nw)
    x, z = Slice((B, Cc, H * W), 3, 2, xv), Flat(xv.numel())
    call("icm_zigzag_splits", x.ptr, x.bs, z.ptr, B, Cc, H, W, ns, nh, nw)
    guards("zigzag_splits", x, z)
    assert same_bits(z.cpu(), want)
    back = Slice((B, Cc, H * W), 2, 1)
    call("icm_zigzag_reverse", z.ptr, back.ptr, back.bs, B, Cc, H, W, ns, nh, nw)
    guards("zigzag_reverse", back, z)
    assert same_bits(back.cpu(), R.zigzag_reverse(want, ns, nh, nw)) and same_bits(back.cpu(), xv)


@pytest.mark.parametrize("ln", [1, 257])
@pytest.mark.parametrize("n", [1, 64])
def test_gather_vectors(n, ln):
    vecs = R.u("gv.v", (n, ln), -1.0, 1.0)
    srcs = [Flat(ln, vecs[i]) for i in range(n)]
    arr = (C.c_void_p * n)(*[s.ptr for s in srcs])
    dst = Flat(n * ln)
    call("icm_gather_vectors", arr, n, ln, dst.ptr)
    guards("gather_vectors", dst, *srcs)
    assert same_bits(dst.cpu(), vecs)


# ================================================================================================ R-D loss
@functools.lru_cache(maxsize=None)
def rd_image(nx):
    x = R.u("rd.x", (nx,), 0.0, 1.0)
    return x, (x + R.u("rd.e", (nx,), -0.1, 0.1))


@functools.lru_cache(maxsize=None)
def rd_lik(name, n):
    return R.likelihoods(name, n)


RD_CASES = [(nx, ny, nz) for nx in R.RD_NX for ny in R.rd_ny(nx) for nz in R.RD_NZ]


@pytest.mark.parametrize("nx,ny,nz", RD_CASES)
def test_rd_loss(nx, ny, nz):
    xv, xh = rd_image(nx)
    ly, lz = rd_lik("rd.ly", ny), rd_lik("rd.lz", nz)
    npix, lmbda = max(1, nx // 3), R.f32(0.0067)
    g = R.rd_geometry(nx, ny, nz)
    xd, hd, yd, zd = Flat(nx, xv), Flat(nx, xh), Flat(ny, ly), Flat(nz, lz)
    outs = []
    for _ in range(2):
        out, ws = Flat(5), Flat(WS_FLOATS)
        call("icm_rd_loss_fwd", xd.ptr, hd.ptr, nx, yd.ptr, ny, zd.ptr, nz, npix, lmbda, out.ptr, ws.ptr)
        guards("rd_loss_fwd", out, ws, xd, hd, yd, zd)
        outs.append(out.cpu())
    assert same_bits(outs[0], outs[1]), "rd_loss_fwd: two runs differ"
    finite("rd_loss_fwd", out)
    x64, h64, y64, z64 = xv.double(), xh.double(), ly.double(), lz.double()
    ref = R.rd_loss_fwd(x64, h64, y64, z64, npix, lmbda)
    se, ay, az = ((h64 - x64) ** 2).sum().item(), y64.log().abs().sum().item(), z64.log().abs().sum().item()
    den = math.log(2.0) * npix
    kx, ky, kz = g["k"][nx], g["k"][ny], g["k"][nz]
    what = f"rd_loss_fwd nx={nx} ny={ny} nz={nz}"
    got = outs[0].double()
    # bpp: two sums, the constant's product, two quotients and a sum; mse: a quotient; loss: two products and a sum
    lim_bpp = R.sum_limit(max(ky, kz) + 4, (ay + az) / den)
    lim_mse = R.sum_limit(kx + 1, se / nx)
    for i, name, k, terms in ((0, "bpp", max(ky, kz) + 4, (ay + az) / den), (1, "mse", kx + 1, se / nx),
                              (3, "sum log lik_y", ky, ay), (4, "sum log lik_z", kz, az)):
        R.check_sum(f"{what} {name}", got[i:i + 1], ref[i:i + 1], k, terms)
    lim_loss = lmbda * 255.0 ** 2 * lim_mse * (1 + 3 * R.ULP) + 3 * R.ULP * ref[2].abs().item() + lim_bpp
    check_bound(f"{what} loss", got[2:3], ref[2:3], torch.tensor([lim_loss], dtype=F64))
    for gscale in (1.0, 0.125):
        dxh, dly, dlz = Flat(nx), Flat(ny), Flat(nz)
        call("icm_rd_loss_bwd", xd.ptr, hd.ptr, nx, yd.ptr, ny, zd.ptr, nz, npix, lmbda, gscale, dxh.ptr, dly.ptr, dlz.ptr)
        guards("rd_loss_bwd", dxh, dly, dlz)
        finite("rd_loss_bwd", dxh, dly, dlz)
        r64 = R.rd_loss_bwd(x64, h64, y64, z64, npix, lmbda, gscale)
        r32 = R.rd_loss_bwd(xv, xh, ly, lz, npix, lmbda, gscale)
        # the two coefficients are formed in float32: five roundings, then a difference and a product / a quotient
        for name, o, a, b in zip(("dx_hat", "dlik_y", "dlik_z"), (dxh, dly, dlz), r32, r64):
            R.check_elementwise(f"rd_loss_bwd nx={nx} ny={ny} nz={nz} gscale={gscale} {name}", o.cpu(), a, b, ulps(b, 4))


def test_rd_loss_as_mean_squared_error():
    """the utils.py use: no likelihoods (one element equal to 1 each), lambda 0: only out[1], the mse, is read; the rate
    terms and the loss are exactly 0"""
    nx = 2047
    xv, xh = rd_image(nx)
    one = torch.ones(1)
    xd, hd, yd, zd, out, ws = Flat(nx, xv), Flat(nx, xh), Flat(1, one), Flat(1, one), Flat(5), Flat(WS_FLOATS)
    call("icm_rd_loss_fwd", xd.ptr, hd.ptr, nx, yd.ptr, 1, zd.ptr, 1, nx, 0.0, out.ptr, ws.ptr)
    guards("rd_loss_fwd", out, ws)
    o = out.cpu()
    assert o[0] == 0 and o[2] == 0 and o[3] == 0 and o[4] == 0
    g = R.rd_geometry(nx, 1, 1)
    se = ((xh.double() - xv.double()) ** 2).sum()
    R.check_sum("rd_loss_fwd as mse", o[1:2], (se / nx).reshape(1), g["k"][nx] + 1, (se / nx).item())


# ================================================================================================ optimiser
@pytest.mark.parametrize("aligned", [1, 0], ids=["aligned", "misaligned-by-4-bytes"])
@pytest.mark.parametrize("n", R.SQNORM_NS)
def test_grad_sqnorm(n, aligned):
    gv = R.u("sq.g", (n,), -3.0, 3.0)
    g = Flat(n, gv, lead=4 if aligned else 1)
    assert (g.ptr % 16 == 0) == bool(aligned)
    geo = R.sqnorm_geometry(n, bool(aligned))
    outs = []
    for _ in range(2):
        out, ws = Flat(1), Flat(WS_FLOATS)
        call("icm_grad_sqnorm", g.ptr, n, out.ptr, ws.ptr)
        guards("grad_sqnorm", g, out, ws)
        outs.append(out.cpu())
    assert same_bits(outs[0], outs[1]), "grad_sqnorm: two runs differ"
    ref = R.sqnorm(gv.double())
    R.check_sum(f"grad_sqnorm n={n} aligned={aligned}", outs[0], ref.reshape(1), geo["k"], ref.item())


@pytest.mark.parametrize("gscale", [1.0, 0.125])
@pytest.mark.parametrize("clip", ["sqnorm-null", "clip-active", "clip-inactive"])
@pytest.mark.parametrize("n", R.ADAM_NS)
def test_adam_step_and_adam_step_hyper(n, clip, gscale):
    lr, b1, b2, eps, steps = 1e-3, 0.9, 0.999, 1e-8, 3
    p0, gv = R.u("adam.p", (n,), -1.0, 1.0), R.u("adam.g", (n,), -30.0, 30.0)
    m0, v0 = R.u("adam.m", (n,), -0.1, 0.1), R.u("adam.v", (n,), 0.0, 0.01)
    sq = None if clip == "sqnorm-null" else R.f32(R.sqnorm(gv.double()).item())
    max_norm = 1.0 if clip == "clip-active" else 1e9
    coef = R.clip_coef(sq, max_norm, gscale)
    if clip == "clip-active":
        assert math.sqrt(sq) * gscale > 2.0 * max_norm and coef < 0.5 * gscale
    if clip == "clip-inactive":
        assert coef == gscale
    gd = Flat(n, gv)
    sqd = Null if sq is None else Flat(1, torch.tensor([sq]))
    a = [Flat(n, t) for t in (p0, m0, v0)]
    h = [Flat(n, t) for t in (p0, m0, v0)]
    for t in range(1, steps + 1):
        call("icm_adam_step", a[0].ptr, gd.ptr, a[1].ptr, a[2].ptr, n, lr, b1, b2, eps, t, sqd.ptr, max_norm, gscale)
        hyper = Flat(2, torch.from_numpy(R.adam_hyper(lr, b1, b2, t)))
        call("icm_adam_step_hyper", h[0].ptr, gd.ptr, h[1].ptr, h[2].ptr, n, b1, b2, eps, hyper.ptr, sqd.ptr, max_norm,
             gscale)
        torch.cuda.synchronize()
    guards("adam", gd, sqd, *a, *h)
    what = f"adam n={n} {clip} gscale={gscale}"
    for x, y, name in zip(a, h, "pmv"):
        assert same_bits(x.cpu(), y.cpu()), f"{what}: {name} of adam_step_hyper differs from adam_step"
    assert same_bits(gd.cpu(), gv)
    r64 = R.adam_steps(p0.double(), gv.double(), m0.double(), v0.double(), steps, lr, b1, b2, eps, coef)
    r32 = R.adam_steps(p0, gv, m0, v0, steps, lr, b1, b2, eps, coef)
    floors = R.adam_floors(p0.double(), gv.double(), m0.double(), r64[2], coef, steps, *r64[3:])
    for i, name in enumerate("pmv"):
        finite(what, a[i])
        R.check_elementwise(f"{what} {name}", a[i].cpu(), r32[i], r64[i], floors[i])


# ================================================================================================ determinism
def _case(table, id):
    return next(c for c in table if c["id"] == id)


def _ln_twice(id):
    c = _case(R.LN_BWD_BRANCH_CASES, id)
    ln_backward(c["N"], c["C"], c["HW"], R.ln_ws_floats(c["ws"], c["C"]), [("both", 0, 0, 0)])


TWICE = {          # each of these helpers calls its entry twice with fresh NaN workspaces and compares the bits
    "channel_sum-S32": lambda: test_channel_sum(_case(R.CHANNEL_SUM_CASES, "S32-wave-finish"), 0),
    "layernorm_bwd-params-fused": lambda: _ln_twice("fused-4-tiles-per-workgroup-C96"),
    "layernorm_bwd-params-split": lambda: _ln_twice("split-S6-wave-K2-C384"),
    "rd_loss_fwd": lambda: test_rd_loss(24576, 10240, 384),
    "grad_sqnorm": lambda: test_grad_sqnorm(100003, 1),
}


@pytest.mark.parametrize("entry", list(TWICE))
def test_two_calls_return_the_same_bits(entry):
    """"every rank must derive bit-identical sums from bit-identical inputs" (the header of pointwise.hip)"""
    TWICE[entry]()


# ================================================================================================ argument contract
def contract_calls(b, s):
    """(id, entry, arguments without the stream, expected code); b = a valid 4096-float device buffer, s = the address
    of its second half.  Every size here fits b, so a guard that failed to fire would still launch in bounds."""
    P, Q = b.ptr, s
    arr = (C.c_void_p * 65)(*([P] * 65))
    return [
        ("channel_sum-x-null", "icm_channel_sum", (0, 8, 1, 2, 4, Q, 0, 0, 0), ERR_ARG),
        ("channel_sum-out-null", "icm_channel_sum", (P, 8, 1, 2, 4, 0, 0, 0, 0), ERR_ARG),
        ("channel_sum-HW-0", "icm_channel_sum", (P, 8, 1, 2, 0, Q, 0, 0, 0), ERR_ARG),
        ("nonneg_fwd-n-0", "icm_nonneg_fwd", (P, Q, 0, 0.1, 0.0), ERR_ARG),
        ("nonneg_bwd-dp-null", "icm_nonneg_bwd", (P, P, 0, 4, 0.1, 0), ERR_ARG),
        ("gdn_bwd_pre-nrm-null", "icm_gdn_bwd_pre", (P, P, 0, Q, Q, 4, 0), ERR_ARG),
        ("gelu_fwd-n-negative", "icm_gelu_fwd", (P, Q, -1), ERR_ARG),
        ("gate_fwd-x-null", "icm_gate_fwd", (P, P, 0, Q, 4), ERR_ARG),
        ("gate_bwd-db-null", "icm_gate_bwd", (P, P, P, Q, 0, Q, 4, 0, 0), ERR_ARG),
        ("add_grad-src-null", "icm_add_grad", (0, 0, Q, 4, 0), ERR_ARG),
        ("ste_round_offset-quantiles-null", "icm_ste_round_offset", (P, 0, Q, 1, 1, 4), ERR_ARG),
        ("copy_strided-C-0", "icm_copy_strided", (P, 8, Q, 8, 1, 0, 4, 0), ERR_ARG),
        ("permute_flip-src-is-dst", "icm_permute_flip", (P, P, 2, 3, 4, 0), ERR_ARG),
        ("permute_flip-K-0", "icm_permute_flip", (P, Q, 2, 3, 0, 0), ERR_ARG),
        ("gather_vectors-n-0", "icm_gather_vectors", (arr, 0, 4, Q), ERR_ARG),
        ("gather_vectors-n-65", "icm_gather_vectors", (arr, 65, 4, Q), ERR_ARG),
        ("gather_vectors-len-0", "icm_gather_vectors", (arr, 2, 0, Q), ERR_ARG),
        ("lrp_bwd-t-null", "icm_lrp_bwd", (P, 8, 0, 8, Q, 8, 1, 2, 4), ERR_ARG),
        ("pixel_unshuffle2-W-0", "icm_pixel_unshuffle2", (P, Q, 1, 1, 2, 0), ERR_ARG),
        ("layernorm_fwd-gamma-null", "icm_layernorm_fwd", (P, 8, 0, P, Q, 8, 0, 0, 1, 2, 4, 1e-5), ERR_ARG),
        ("layernorm_fwd-N-0", "icm_layernorm_fwd", (P, 8, P, P, Q, 8, 0, 0, 0, 2, 4, 1e-5), ERR_ARG),
        ("layernorm_bwd-mean-null", "icm_layernorm_bwd", (P, 8, P, 8, P, 0, P, Q, 8, 0, 0, 1, 2, 4, 0, 0, 0, 0, 0, 0), ERR_ARG),
        ("layernorm_bwd-HW-0", "icm_layernorm_bwd", (P, 8, P, 8, P, P, P, Q, 8, 0, 0, 1, 2, 0, 0, 0, 0, 0, 0, 0), ERR_ARG),
        ("space_to_depth2-odd-H", "icm_space_to_depth2", (P, Q, 1, 2, 3, 4, 0, 0), ERR_ARG),
        ("space_to_depth2-odd-W", "icm_space_to_depth2", (P, Q, 1, 2, 4, 3, 1, 0), ERR_ARG),
        ("residual_scale-scale-null", "icm_residual_scale", (0, P, 0, Q, 1, 4), ERR_ARG),
        ("residual_scale-per-0", "icm_residual_scale", (0, P, P, Q, 1, 0), ERR_ARG),
        ("im2col-OH-not-positive", "icm_im2col", (P, Q, 1, 1, 2, 8, 5, 1, 0), ERR_ARG),
        ("im2col-negative-pad", "icm_im2col", (P, Q, 1, 1, 8, 8, 3, 1, -1), ERR_ARG),
        ("col2im-stride-0", "icm_col2im", (P, 0, Q, 1, 1, 8, 8, 3, 0, 1, 0), ERR_ARG),
        ("col2im-OW-not-positive", "icm_col2im", (P, 0, Q, 1, 1, 8, 2, 5, 1, 0, 0), ERR_ARG),
        ("fill-p-null", "icm_fill", (0, 4, 1.0), ERR_ARG),
        ("clamp-lo-above-hi", "icm_clamp", (P, 4, 1.0, 0.5), ERR_ARG),
        ("clamp-nan-bound", "icm_clamp", (P, 4, NAN, 0.5), ERR_ARG),
        ("pad2d-OH-0", "icm_pad2d", (P, 1, 1, 4, 4, Q, 0, 4, 0, 0, 0.0), ERR_ARG),
        ("zigzag_splits-C-not-divisible", "icm_zigzag_splits", (P, 80, Q, 1, 5, 4, 4, 2, 2, 2), ERR_ARG),
        ("zigzag_reverse-H-not-divisible", "icm_zigzag_reverse", (P, Q, 60, 1, 4, 3, 4, 2, 2, 2), ERR_ARG),
        ("zigzag_splits-more-than-64-blocks", "icm_zigzag_splits", (P, 1300, Q, 1, 65, 4, 5, 65, 1, 1), ERR_UNSUPPORTED),
        ("zigzag_reverse-more-than-64-blocks", "icm_zigzag_reverse", (P, Q, 1300, 1, 65, 4, 5, 65, 1, 1), ERR_UNSUPPORTED),
        ("rd_loss_fwd-ws-null", "icm_rd_loss_fwd", (P, P, 4, P, 4, P, 4, 4, 0.01, Q, 0), ERR_ARG),
        ("rd_loss_fwd-num_pixels-0", "icm_rd_loss_fwd", (P, P, 4, P, 4, P, 4, 0, 0.01, Q, Q + 64), ERR_ARG),
        ("rd_loss_bwd-dlik_z-null", "icm_rd_loss_bwd", (P, P, 4, P, 4, P, 4, 4, 0.01, 1.0, Q, Q + 64, 0), ERR_ARG),
        ("grad_sqnorm-n-0", "icm_grad_sqnorm", (P, 0, Q, Q + 64), ERR_ARG),
        ("adam_step-step-0", "icm_adam_step", (Q, P, Q + 64, Q + 128, 4, 1e-3, 0.9, 0.999, 1e-8, 0, 0, 1.0, 1.0), ERR_ARG),
        ("adam_step-m-null", "icm_adam_step", (Q, P, 0, Q + 128, 4, 1e-3, 0.9, 0.999, 1e-8, 1, 0, 1.0, 1.0), ERR_ARG),
        ("adam_step_hyper-hyper-null", "icm_adam_step_hyper", (Q, P, Q + 64, Q + 128, 4, 0.9, 0.999, 1e-8, 0, 0, 1.0, 1.0), ERR_ARG),
    ]


CONTRACT_IDS = [c[0] for c in contract_calls(Null, 0)]


@pytest.mark.parametrize("which", range(len(CONTRACT_IDS)), ids=CONTRACT_IDS)
def test_argument_contract(which):
    L = lib()
    b = Flat(4096, torch.ones(4096))
    name, entry, args, want = contract_calls(b, b.ptr + 4 * 2048)[which]
    rc = getattr(L.lib(), entry)(*args, L.stream())
    assert rc == want, f"{name}: returned {rc}, expected {want}"
    torch.cuda.synchronize()
    assert same_bits(b.cpu(), torch.ones(4096)) and b.guards_ok(), f"{name}: the refused call wrote memory"
