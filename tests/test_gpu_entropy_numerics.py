"""The entropy-model kernels (csrc/entropy.hip) through the C ABI against float64, where the rate is decided: in the
tails, in bits.  Every operand can be a channel slice of its own wider buffer, optional pointers are passed null and
set, and the bottleneck runs at L = N*HW on both sides of its 256-lane trip.

Every limit is tests/_entropy_ref.py's: FACTOR (4) times the error of the float32 oracle against the float64 oracle on
the same inputs, plus a floor; none is taken from a kernel's output.  tests/test_entropy_ref.py asserts, without a GPU,
that the inputs populate every band and keep the excluded ``grey`` elements under 5 %.  Each check prints the measured
figure next to its limit (pytest -s); DESIGN.md "Entropy-kernel numerics" holds one such run."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import _entropy_ref as R
from oracle import wacnn_oracle as O

pytestmark = pytest.mark.gpu

NAN = float("nan")
SCALE_BOUND, LIK_BOUND = 0.11, 1e-9
BOUND32 = torch.tensor(LIK_BOUND, dtype=torch.float32)
EB = R.EB


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def lib():
    from icm_amd import _lib
    return _lib


class Slice:
    """a [N,C,...] channel slice, ``off`` channels into its own buffer of C + extra channels filled with NaN"""

    def __init__(self, shape, extra, off, value=None, fill=NAN, dtype=torch.float32):
        N, Cc = shape[:2]
        assert 0 <= off <= extra
        self.buf = torch.full((N, Cc + extra) + tuple(shape[2:]), fill, dtype=dtype, device=dev())
        self.off, self.C = off, Cc
        self.view = self.buf[:, off:off + Cc]
        if value is not None:
            self.view.copy_(value)
        self.ptr, self.bs = self.view.data_ptr(), self.buf.stride(0)

    def cpu(self):
        return self.view.cpu()

    def outside_untouched(self):
        b = self.buf.cpu()
        return bool(torch.isnan(b[:, :self.off]).all() and torch.isnan(b[:, self.off + self.C:]).all())


class Null:
    ptr, bs = 0, 0


def same_bits(a, b):
    return torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


def check_bands(what, lik, lik32, r):
    """live elements: per band, max |log2 lik - log2 r| within FACTOR * the float32 oracle's + 1e-6 bits; floor: the bound"""
    lik = lik.cpu()
    got, own, lim = R.band_bits(lik, r), R.band_bits(lik32, r), R.band_limits(lik32, r)
    for b, g, o, l in zip(R.BAND_NAMES, got, own, lim):
        print(f"{what} {b}: gpu {g:.3e} bits, float32 oracle {o:.3e}, limit {l:.3e}")
    for b, g, l in zip(R.BAND_NAMES, got, lim):
        assert math.isfinite(g) and g <= l, f"{what} band {b}: {g:.3e} bits > limit {l:.3e}"
    floor = R.classify(r)[1]
    assert (lik[floor] == BOUND32).all(), f"{what}: a floor element is not the bound"
    assert torch.isfinite(lik).all() and (lik >= BOUND32).all(), what


def check_grad(what, got, g32, g64, r, keep):
    """element-wise, on ``keep``: |got - g64| within the per-group limit of R.grad_tolerance"""
    got = got.cpu().double()
    tol = R.grad_tolerance(g32, g64, r, keep)
    err = (got - g64).abs()
    own = (g32.double() - g64).abs()
    for name, m in zip(R.BAND_NAMES + ("floor",), R.groups(r)):
        m = m & keep
        if m.any():
            print(f"{what} {name}: gpu {err[m].max().item():.3e}, float32 oracle {own[m].max().item():.3e}, "
                  f"limit {tol[m].max().item():.3e}, ref max {g64[m].abs().max().item():.3e}")
    bad = keep & ~(err <= tol)       # NaN counts as bad
    assert not bad.any(), (f"{what}: {int(bad.sum())} elements over the limit, worst {err[bad].max().item():.3e} "
                           f"against {tol[bad].min().item():.3e}")


# ------------------------------------------------------------------------------------------------ Gaussian
@functools.lru_cache(maxsize=None)
def gc_forward_ref(shape, mode):
    inp = R.gaussian_inputs(shape)
    return R.gaussian_raw(inp, mode), R.gaussian_oracle(inp, mode, torch.float32)


@functools.lru_cache(maxsize=None)
def gc_backward_ref(mode, seed):
    inp = R.gaussian_inputs()
    r = R.gaussian_raw(inp, mode)
    dlik = R.seed(r, seed, "gcn." + mode)
    return r, dlik, R.gaussian_oracle(inp, mode, torch.float64, dlik)[1], R.gaussian_oracle(inp, mode, torch.float32, dlik)[1]


def gc_fwd(y, mu, sc, nz, lik, yh, yh2, shape):
    L = lib()
    N, Cc, H, W = shape
    L.check(L.lib().icm_gc_likelihood_ste_fwd(y.ptr, y.bs, mu.ptr, mu.bs, sc.ptr, sc.bs, nz.ptr, nz.bs, lik.ptr, lik.bs,
                                              yh.ptr, yh.bs, yh2.ptr, yh2.bs, N, Cc, H * W, SCALE_BOUND, LIK_BOUND,
                                              L.stream()), "gc_fwd")


@pytest.mark.parametrize("mode", R.MODES)
def test_gaussian_forward_strided(mode):
    shape = R.GC_SHAPE
    inp = R.gaussian_inputs(shape)
    r, lik32 = gc_forward_ref(shape, mode)
    yh_ref = R.gaussian_yhat(inp)
    # seven operands, seven batch strides
    y, mu, sc = Slice(shape, 1, 0, inp["y"]), Slice(shape, 2, 1, inp["mu"]), Slice(shape, 3, 3, inp["scale"])
    nz = Slice(shape, 4, 2, inp["noise"]) if mode == "train" else Null
    for want_yh, want_yh2 in ((True, True), (False, True), (True, False), (False, False)):
        lik = Slice(shape, 5, 0)
        yh = Slice(shape, 6, 4) if want_yh else Null
        yh2 = Slice(shape, 7, 7) if want_yh2 else Null
        if mode == "train" and want_yh and want_yh2:
            assert len({s.bs for s in (y, mu, sc, nz, lik, yh, yh2)}) == 7
        gc_fwd(y, mu, sc, nz, lik, yh, yh2, shape)
        what = f"gaussian fwd {mode} yh={int(want_yh)} yh2={int(want_yh2)}"
        for s in (y, mu, sc, lik) + ((nz,) if mode == "train" else ()) + ((yh,) if want_yh else ()) + ((yh2,) if want_yh2 else ()):
            assert s.outside_untouched(), what
        for s, v in ((y, inp["y"]), (mu, inp["mu"]), (sc, inp["scale"])):
            assert same_bits(s.cpu(), v), what + ": an input changed"
        if want_yh:
            assert same_bits(yh.cpu(), yh_ref), what + " yh"
        if want_yh2:
            assert same_bits(yh2.cpu(), yh_ref), what + " yh2"
        check_bands(what, lik.cpu(), lik32, r)


def test_gaussian_forward_long_grid():
    shape = R.GC_LONG_SHAPE
    assert int(np.prod(shape)) > 2048 * 256
    inp = R.gaussian_inputs(shape)
    r, lik32 = gc_forward_ref(shape, "eval")
    d = dev()
    t = {k: v.to(d) for k, v in inp.items()}
    lik = torch.full(shape, NAN, dtype=torch.float32, device=d)
    yh = torch.full(shape, NAN, dtype=torch.float32, device=d)
    L = lib()
    N, Cc, H, W = shape
    per = Cc * H * W
    L.check(L.lib().icm_gc_likelihood_ste_fwd(t["y"].data_ptr(), per, t["mu"].data_ptr(), per, t["scale"].data_ptr(), per,
                                              0, 0, lik.data_ptr(), per, yh.data_ptr(), per, 0, 0, N, Cc, H * W,
                                              SCALE_BOUND, LIK_BOUND, L.stream()), "gc_fwd")
    assert same_bits(yh, R.gaussian_yhat(inp))
    check_bands("gaussian fwd long eval", lik, lik32, r)


@pytest.mark.parametrize("seed", R.SEEDS)
@pytest.mark.parametrize("mode", R.MODES)
def test_gaussian_backward(mode, seed):
    shape = R.GC_SHAPE
    N, Cc, H, W = shape
    inp = R.gaussian_inputs(shape)
    r, dlik, g64, g32 = gc_backward_ref(mode, seed)
    live, floor, grey = R.classify(r)
    below, above, sgrey = R.scale_classes(inp["scale"])
    dyh_v = R.U("gcn.dyh", shape, -1.0, 1.0)
    prev_v = R.U("gcn.prev", shape, -2.0, 2.0)
    L = lib()
    y, mu, sc = Slice(shape, 1, 1, inp["y"]), Slice(shape, 2, 0, inp["mu"]), Slice(shape, 3, 2, inp["scale"])
    nz = Slice(shape, 4, 3, inp["noise"]) if mode == "train" else Null
    dl = Slice(shape, 5, 1, dlik)
    for use_dyh in (False, True):
        for accum in (0, 1):
            what = f"gaussian bwd {mode} {seed} dyh={int(use_dyh)} accum={accum}"
            dyh = Slice(shape, 6, 6, dyh_v) if use_dyh else Null
            dy = Slice(shape, 7, 3, prev_v if accum else None)          # NaN inside too when not accumulating
            dmu, dsc = Slice(shape, 8, 4), Slice(shape, 9, 0)
            L.check(L.lib().icm_gc_likelihood_ste_bwd(y.ptr, y.bs, mu.ptr, mu.bs, sc.ptr, sc.bs, nz.ptr, nz.bs, dl.ptr,
                                                      dl.bs, dyh.ptr, dyh.bs, dy.ptr, dy.bs, dmu.ptr, dmu.bs, dsc.ptr,
                                                      dsc.bs, N, Cc, H * W, SCALE_BOUND, LIK_BOUND, accum, L.stream()),
                    "gc_bwd")
            for s in (dy, dmu, dsc):
                assert s.outside_untouched(), what
            got_dy, got_dmu, got_dsc = dy.cpu(), dmu.cpu(), dsc.cpu()
            # what dyh and the accumulated value add, in the kernel's order and in float64
            add32 = torch.zeros(shape)
            add64 = torch.zeros(shape, dtype=torch.float64)
            dy32 = g32[0]
            if use_dyh:
                dy32, add32, add64 = dy32 + dyh_v, add32 + dyh_v, add64 + dyh_v.double()
            if accum:
                dy32, add32, add64 = dy32 + prev_v, add32 + prev_v, add64 + prev_v.double()
            check_grad(what + " dy", got_dy, dy32, g64[0] + add64, r, ~grey)
            check_grad(what + " dmu", got_dmu, g32[1], g64[1], r, ~grey)
            check_grad(what + " dscale", got_dsc, g32[2], g64[2], r, ~grey & ~sgrey)
            # gating
            off = floor & (dlik >= 0)
            assert off.any() or seed == "bits"
            assert (got_dmu[off] == 0).all() and (got_dsc[off] == 0).all(), what + ": gradient through the floor"
            assert torch.equal(got_dy[off], add32[off]), what + ": dy through the floor"
            quiet = below & ~grey & (g64[2] == 0)
            assert quiet.any() and (g64[2][below] <= 0).all()
            assert (got_dsc[quiet] == 0).all(), what + ": dscale below the scale bound"
            if mode == "eval":
                assert (got_dmu == 0).all(), what + ": dmu in eval mode"
                assert same_bits(got_dy, add32), what + ": dy in eval mode"


# ------------------------------------------------------------------------------------------------ bottleneck
def eb_device(sd):
    """(EbParams, the device tensors it points into)"""
    L = lib()
    P = {k: v.to(dev()).contiguous() for k, v in sd.items()}
    s = L.EbParams()
    for i in range(5):
        s.matrix[i], s.bias[i] = P[f"{EB}._matrix{i}"].data_ptr(), P[f"{EB}._bias{i}"].data_ptr()
    for i in range(4):
        s.factor[i] = P[f"{EB}._factor{i}"].data_ptr()
    s.quantiles = P[f"{EB}.quantiles"].data_ptr()
    return s, P


def eb_grad_buffers(P, with_median):
    """(EbGrads, {name: NaN-filled device tensor})"""
    L = lib()
    G = {n: torch.full_like(P[f"{EB}.{n}"], NAN) for n in R.EB_NAMES}
    g = L.EbGrads()
    for i in range(5):
        g.matrix[i], g.bias[i] = G[f"_matrix{i}"].data_ptr(), G[f"_bias{i}"].data_ptr()
    for i in range(4):
        g.factor[i] = G[f"_factor{i}"].data_ptr()
    if with_median:
        G["dmedian"] = torch.full((P[f"{EB}.quantiles"].shape[0],), NAN, dtype=torch.float32, device=dev())
        g.dmedian = G["dmedian"].data_ptr()
    else:
        g.dmedian = None
    return g, G


@functools.lru_cache(maxsize=None)
def eb_forward_ref(shape, mode):
    inp, sd = R.eb_inputs(shape), R.eb_params(shape[1])
    return R.eb_raw(inp, sd, mode), R.eb_oracle(inp, sd, mode, torch.float32)


@functools.lru_cache(maxsize=None)
def eb_backward_ref(shape, mode, seed):
    inp, sd = R.eb_inputs(shape), R.eb_params(shape[1])
    r = R.eb_raw(inp, sd, mode)
    dlik = R.seed(r, seed, f"ebn.{shape}.{mode}", zero_grey=True)
    return r, dlik, R.eb_oracle(inp, sd, mode, torch.float64, dlik)[1], R.eb_oracle(inp, sd, mode, torch.float32, dlik)[1]


EB_IDS = [f"L{n * hw}" for n, _, hw in R.EB_SHAPES]


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", R.EB_SHAPES, ids=EB_IDS)
def test_bottleneck_forward(shape, mode):
    N, Cc, HW = shape
    inp, sd = R.eb_inputs(shape), R.eb_params(Cc)
    r, lik32 = eb_forward_ref(shape, mode)
    L = lib()
    d = dev()
    prm, P = eb_device(sd)
    z = inp["z"].to(d)
    nz = inp["noise"].to(d) if mode == "train" else None
    what = f"bottleneck fwd {mode} L={N * HW}"
    for want_zt in (True, False):
        lik = torch.full(shape, NAN, dtype=torch.float32, device=d)
        zt = torch.full(shape, NAN, dtype=torch.float32, device=d) if want_zt else None
        L.check(L.lib().icm_eb_likelihood_fwd(z.data_ptr(), L.ptr(nz), C.byref(prm), lik.data_ptr(), L.ptr(zt), N, Cc, HW,
                                              LIK_BOUND, L.stream()), "eb_fwd")
        check_bands(what + f" zt={int(want_zt)}", lik, lik32, r)
        if want_zt:
            assert same_bits(zt, R.eb_value(inp, sd, mode)), what + " zt"
    assert same_bits(z, inp["z"])


@pytest.mark.parametrize("seed", R.SEEDS)
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", R.EB_SHAPES, ids=EB_IDS)
def test_bottleneck_backward(shape, mode, seed):
    N, Cc, HW = shape
    inp, sd = R.eb_inputs(shape), R.eb_params(Cc)
    r, dlik, g64, g32 = eb_backward_ref(shape, mode, seed)
    grey = R.classify(r)[2]
    assert (dlik[grey] == 0).all()
    L = lib()
    d = dev()
    prm, P = eb_device(sd)
    z, dl = inp["z"].to(d), dlik.to(d)
    nz = inp["noise"].to(d) if mode == "train" else None
    prev = R.U("ebn.prev", shape, -2.0, 2.0)
    what = f"bottleneck bwd {mode} {seed} L={N * HW}"

    def run(accum):
        dz = prev.to(d) if accum else torch.full(shape, NAN, dtype=torch.float32, device=d)
        g, G = eb_grad_buffers(P, with_median=(mode == "eval"))
        L.check(L.lib().icm_eb_likelihood_bwd(z.data_ptr(), L.ptr(nz), C.byref(prm), dl.data_ptr(), dz.data_ptr(),
                                              C.byref(g), N, Cc, HW, LIK_BOUND, accum, L.stream()), "eb_bwd")
        return dz.cpu(), {k: v.cpu() for k, v in G.items()}

    outs = {accum: run(accum) for accum in (0, 1)}
    again = run(0)
    assert same_bits(outs[0][0], again[0]), what + ": dz differs between two runs"
    for accum in (0, 1):
        dz, G = outs[accum]
        for n in G:
            assert same_bits(G[n], again[1][n]), f"{what}: grad {n} differs between two runs"
        for n in R.EB_NAMES:
            check_tensor(f"{what} accum={accum} grad {n}", G[n], g32[n], g64[n])
        if mode == "eval":
            check_tensor(f"{what} accum={accum} dmedian", G["dmedian"], g32["quantiles"][:, 0, 1], g64["quantiles"][:, 0, 1])
            want = prev if accum else torch.zeros(shape)
            assert same_bits(dz, want), f"{what} accum={accum}: dz in eval mode"
        else:
            add = prev if accum else torch.zeros(shape)
            check_grad(f"{what} accum={accum} dz", dz, g32["z"] + add, g64["z"] + add.double(), r, ~grey)


def check_tensor(what, got, g32, g64):
    """a gradient summed over L: relative to the float64 reference's largest magnitude"""
    got = got.cpu().double().reshape(g64.shape)
    if g64.abs().max().item() == 0:
        assert (got == 0).all(), what + ": reference is identically zero"
        return
    tol = R.tensor_tolerance(g32, g64)
    err = (got - g64).abs().max().item()
    ref = g64.abs().max().item()
    print(f"{what}: gpu {err / ref:.3e} of the largest magnitude, float32 oracle "
          f"{(g32.double() - g64).abs().max().item() / ref:.3e}, limit {tol / ref:.3e}")
    assert math.isfinite(err) and err <= tol, f"{what}: {err:.3e} > limit {tol:.3e} (ref max {ref:.3e})"


@pytest.mark.parametrize("Cc", [1, 24, 192, 200])
def test_aux_loss(Cc):
    sd = R.eb_params(Cc)
    (l64, q64), (l32, q32) = R.eb_aux(sd, torch.float64), R.eb_aux(sd, torch.float32)
    L = lib()
    d = dev()
    prm, P = eb_device(sd)
    loss = torch.full((1,), NAN, dtype=torch.float32, device=d)
    dq = torch.full((Cc, 1, 3), NAN, dtype=torch.float32, device=d)
    L.check(L.lib().icm_eb_aux_loss(C.byref(prm), loss.data_ptr(), dq.data_ptr(), Cc, math.log(2 / 1e-9 - 1), L.stream()),
            "eb_aux")
    check_tensor(f"aux C={Cc} loss", loss, l32.reshape(1), l64.reshape(1))
    check_tensor(f"aux C={Cc} dquantiles", dq, q32, q64)


# ------------------------------------------------------------------------------------------------ tables
def test_eb_table_bounds():
    f = np.float32
    nx = lambda a, b: float(np.nextafter(f(a), f(b)))
    rows = [                                    # (q0, median, q2)
        (-2.75, 0.25, 4.25),                    # differences exactly 3 and 4
        (nx(-2.75, -9), 0.25, nx(4.25, 9)),     # one ulp above an integer -> 4 and 5
        (nx(-2.75, 0), 0.25, nx(4.25, 0)),      # one ulp below -> 3 and 4
        (2.25, 0.25, -1.25),                    # negative differences clamp to 0
        (0.25, 0.25, 0.25),                     # zero
        (-10.3, -7.3, 1.9),
        (-0.001, 0.0, 1e-6),
        (-131.5, 0.5, 168.25),
    ]
    q = torch.tensor(rows, dtype=torch.float32).reshape(-1, 1, 3)
    Cc = q.shape[0]
    sd = dict(R.eb_params(Cc))
    sd[f"{EB}.quantiles"] = q
    offset, _, _, pmf_length, _ = O.eb_update_tables(sd)
    want_min = -offset
    want_max = pmf_length - 1 - want_min
    assert want_min.tolist()[:5] == [3, 4, 3, 0, 0] and want_max.tolist()[:5] == [4, 5, 4, 0, 0]
    L = lib()
    d = dev()
    qd = q.to(d)
    mi = torch.full((Cc,), -7, dtype=torch.int32, device=d)
    ma = torch.full((Cc,), -7, dtype=torch.int32, device=d)
    L.check(L.lib().icm_eb_table_bounds(qd.data_ptr(), Cc, mi.data_ptr(), ma.data_ptr(), L.stream()), "eb_table_bounds")
    assert torch.equal(mi.cpu(), want_min.int()) and torch.equal(ma.cpu(), want_max.int())


def test_eb_pmf_table():
    Cc, max_length = 5, 300
    sd = dict(R.eb_params(Cc, "ebt", 1.0))       # tails that stay inside float32's range 150 from the median
    q = sd[f"{EB}.quantiles"].clone()
    m0, m4 = q[0, 0, 1].item(), q[4, 0, 1].item()
    q[0, 0] = torch.tensor([m0 - 149.6, m0, m0 + 148.7])       # 150 + 149 + 1 = 300 samples
    q[4, 0] = torch.tensor([m4 - 39.5, m4, m4 + 2.5])
    sd[f"{EB}.quantiles"] = q
    off32, pmf32, tail32, _, ml = O.eb_update_tables(sd)
    off64, pmf64, tail64, _, ml64 = O.eb_update_tables(R.cast(sd, torch.float64))
    assert ml == ml64 == max_length and torch.equal(off32, off64)
    assert tail64.min().item() > 1e-30
    L = lib()
    d = dev()
    prm, P = eb_device(sd)
    minima = (-off32).int().to(d)
    pmf = torch.full((Cc, max_length), NAN, dtype=torch.float32, device=d)
    tail = torch.full((Cc,), NAN, dtype=torch.float32, device=d)
    L.check(L.lib().icm_eb_pmf_table(C.byref(prm), minima.data_ptr(), Cc, max_length, pmf.data_ptr(), tail.data_ptr(),
                                     L.stream()), "eb_pmf_table")
    pmf, tail = pmf.cpu(), tail.cpu()
    assert all(m.any() for m in R.bands(pmf64))
    got, own, lim = R.band_bits(pmf, pmf64), R.band_bits(pmf32, pmf64), R.band_limits(pmf32, pmf64)
    for b, g, o, l in zip(R.BAND_NAMES, got, own, lim):
        print(f"eb pmf table {b}: gpu {g:.3e} bits, float32 oracle {o:.3e}, limit {l:.3e}")
        assert math.isfinite(g) and g <= l, f"eb pmf table {b}: {g:.3e} > {l:.3e}"
    assert torch.isfinite(pmf).all() and (pmf >= 0).all()
    t64 = tail64.reshape(-1)
    rel = ((tail.double() - t64).abs() / t64).max().item()
    own = ((tail32.reshape(-1).double() - t64).abs() / t64).max().item()
    print(f"eb pmf table tail mass: gpu rel {rel:.3e}, float32 oracle {own:.3e}")
    assert math.isfinite(rel) and rel <= R.FACTOR * own + R.REL_FLOOR


@pytest.mark.parametrize("which", ["table64", "ns3"])
def test_gc_tables(which):
    table = O.scale_table() if which == "table64" else torch.tensor([0.5, 7.3, 20.9])
    ns = table.numel()
    mult = R.gc_multiplier()
    off, pmf_o, tail_o, _, ml = O.gc_update_tables(table)
    if which == "ns3":
        assert ml == 257
    L = lib()
    d = dev()
    td = table.to(d)
    centers = torch.full((ns,), -7, dtype=torch.int32, device=d)
    L.check(L.lib().icm_gc_table_centers(td.data_ptr(), ns, mult, centers.data_ptr(), L.stream()), "gc_table_centers")
    assert torch.equal(centers.cpu(), (-off).int())
    pmf = torch.full((ns, ml), NAN, dtype=torch.float32, device=d)
    tail = torch.full((ns,), NAN, dtype=torch.float32, device=d)
    L.check(L.lib().icm_gc_pmf_table(td.data_ptr(), centers.data_ptr(), ns, ml, pmf.data_ptr(), tail.data_ptr(), L.stream()),
            "gc_pmf_table")
    pmf, tail = pmf.cpu(), tail.cpu()
    pmf64, tail64 = R.gc_pmf(table, -off, ml, torch.float64)
    pmf32, tail32 = R.gc_pmf(table, -off, ml, torch.float32)
    assert torch.equal(pmf32, pmf_o) and torch.equal(tail32, tail_o.reshape(-1))     # R.gc_pmf restates the oracle
    got, own, lim = R.band_bits(pmf, pmf64), R.band_bits(pmf32, pmf64), R.band_limits(pmf32, pmf64)
    for b, g, o, l in zip(R.BAND_NAMES, got, own, lim):
        print(f"gc pmf table {which} {b}: gpu {g:.3e} bits, float32 oracle {o:.3e}, limit {l:.3e}")
        assert math.isfinite(g) and g <= l, f"gc pmf table {which} {b}: {g:.3e} > {l:.3e}"
    assert torch.isfinite(pmf).all()
    # relative error where float32 holds the tail mass as a normal number; the narrow scales' tails lie below that
    ok = tail64 >= 1e-30
    assert ok.any() and (tail >= 0).all() and (tail[~ok] <= 1e-29).all()
    rel = ((tail.double() - tail64).abs() / tail64)[ok].max().item()
    own = ((tail32.double() - tail64).abs() / tail64)[ok].max().item()
    print(f"gc pmf table {which} tail mass: gpu rel {rel:.3e}, float32 oracle {own:.3e}")
    assert math.isfinite(rel) and rel <= R.FACTOR * own + R.REL_FLOOR


# ------------------------------------------------------------------------------------------------ symbols
TIES = (0.5, -0.5, 1.5, -1.5, 2.5, -2.5)


def quantize_case(layout):
    """x [N,C,H,W], the means tensor the kernel reads, its (bs, cs, ps) strides and the broadcast means (or None).
    Means are multiples of 1/64 so that the ties x - mean = +-0.5, +-1.5, +-2.5 are exact."""
    shape = (2, 6, 5, 7)
    N, Cc, H, W = shape
    HW = H * W
    x = R.U("qz.x", shape, -9.0, 9.0)
    if layout == "null":
        m = None
    elif layout == "medians":
        m = torch.round(R.U("qz.q", (Cc, 1, 3), -2.0, 2.0) * 64) / 64 + torch.tensor([-10.0, 0.0, 10.0])
    else:
        m = torch.round(R.U("qz.m", shape, -3.0, 3.0) * 64) / 64
    full = None if m is None else (m[:, 0, 1].reshape(1, Cc, 1, 1).expand(shape) if layout == "medians" else m)
    xt = x.reshape(N, Cc, HW)
    base = torch.zeros(shape) if full is None else full
    xt[:, :, :len(TIES)] = base.reshape(N, Cc, HW)[:, :, :len(TIES)] + torch.tensor(TIES)
    assert torch.equal((x - base).reshape(N, Cc, HW)[0, 0, :len(TIES)], torch.tensor(TIES))
    return shape, x, m, full


@pytest.mark.parametrize("layout", ["null", "medians", "strided"])
def test_quantize_dequantize_layouts(layout):
    shape, x, m, full = quantize_case(layout)
    N, Cc, H, W = shape
    HW = H * W
    L = lib()
    d = dev()
    xs = Slice(shape, 3, 2, x)
    if layout == "null":
        mp, strides = 0, (0, 0, 0)
    elif layout == "medians":
        md = m.to(d)
        mp, strides = md.data_ptr() + 4, (0, 3, 0)           # quantiles[c, 0, 1] straight out of the [C, 1, 3] tensor
    else:
        ms = Slice(shape, 5, 1, m)
        mp, strides = ms.ptr, (ms.bs, HW, 1)
    base = torch.zeros(shape) if full is None else full
    q = torch.round(x - base)
    want_sym = torch.from_numpy(np.rint((x - base).numpy()).astype(np.int32))
    assert torch.equal(want_sym, q.int())
    assert want_sym.reshape(N, Cc, HW)[0, 0, :6].tolist() == [0, 0, 2, -2, 2, -2]      # ties go to even
    want_deq = q + base
    for want_s, want_d in ((True, False), (False, True), (True, True)):
        sym = torch.full(shape, -77, dtype=torch.int32, device=d) if want_s else None
        deq = torch.full(shape, NAN, dtype=torch.float32, device=d) if want_d else None
        L.check(L.lib().icm_quantize(xs.ptr, xs.bs, mp, *strides, 0 if sym is None else sym.data_ptr(), L.ptr(deq), N, Cc,
                                     HW, L.stream()), "quantize")
        if want_s:
            assert torch.equal(sym.cpu(), want_sym), layout
        if want_d:
            assert same_bits(deq, want_deq), layout
    assert xs.outside_untouched() and same_bits(xs.cpu(), x)
    # dequantise into a wider buffer
    out = Slice(shape, 4, 3)
    assert out.bs > Cc * HW
    symd = want_sym.to(d)
    L.check(L.lib().icm_dequantize(symd.data_ptr(), mp, *strides, out.ptr, out.bs, N, Cc, HW, L.stream()), "dequantize")
    assert out.outside_untouched()
    assert same_bits(out.cpu(), want_sym.float() + base)


def test_gc_build_indexes_strided():
    shape = (2, 6, 5, 7)
    N, Cc, H, W = shape
    n = int(np.prod(shape))
    table = O.scale_table()
    sc = (table[torch.arange(n) % 64] * R.U("bi.f", (n,), 0.7, 1.4)).reshape(shape)
    flat = sc.view(-1)
    flat[:64] = table                                    # exactly on every table entry
    flat[64:70] = torch.tensor([0.11, R.SCALE_BELOW, R.SCALE_ABOVE, 0.0, -1.0, 300.0])
    want = O.gc_build_indexes(sc, table)
    L = lib()
    d = dev()
    s = Slice(shape, 2, 1, sc)
    idx = torch.full(shape, -7, dtype=torch.int32, device=d)
    td = table.to(d)
    L.check(L.lib().icm_gc_build_indexes(s.ptr, s.bs, td.data_ptr(), 64, SCALE_BOUND, idx.data_ptr(), N, Cc, H * W,
                                         L.stream()), "gc_build_indexes")
    assert torch.equal(idx.cpu(), want)
