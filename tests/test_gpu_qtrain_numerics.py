"""The kernels of variable-rate training through the C ABI against float64: the stepped likelihood + STE pair
(csrc/qstep.hip: icm_gc_likelihood_ste_qs_fwd / _bwd, a quantiser step per image read from device memory) and the
per-image weighted R-D loss (csrc/pointwise.hip: icm_rd_loss_w_fwd / _bwd).

Likelihoods are compared in bits and gradients element-wise, by the rule and constants of tests/_entropy_ref.py: every
limit is FACTOR times the error of the float32 restatement of tests/_qtrain_ref.py against its float64 run on the same
inputs, plus that file's floor; none is taken from a kernel's output.  y_hat is compared bit for bit, with
tests/_qstep_ref.py's numpy arithmetic and with what the codec's own kernels (icm_gc_code_q, icm_dequantize_q) return on
the same inputs.  The sums of the weighted loss follow tests/_pointwise_ref.py's rule (gamma(k) of the longest chain of
additions).  tests/test_qtrain_ref.py asserts, without a GPU, that the inputs populate every class.  pytest -s prints
each measured figure next to its limit."""
import functools
import math

import numpy as np
import pytest
import torch

import _entropy_ref as R
import _pointwise_ref as P
import _qstep_ref as Q
import _qtrain_ref as T
from oracle import wacnn_oracle as O
from test_gpu_entropy_numerics import (LIK_BOUND, NAN, SCALE_BOUND, Null, Slice, check_bands, check_grad, dev, lib,
                                       same_bits)

pytestmark = pytest.mark.gpu

ERR_ARG = 1
LAYOUTS = ("dense", "slices")


def operand(shape, layout, extra, off, value=None):
    """a [N,C,H,W] operand: dense, or ``off`` channels into its own NaN-filled buffer of C + extra channels"""
    return Slice(shape, extra, off, value) if layout == "slices" else Slice(shape, 0, 0, value)


def steps_dev(inp):
    return inp["steps"].to(dev()).contiguous()


@functools.lru_cache(maxsize=None)
def forward_ref(case, mode):
    inp = T.stepped_inputs(case)
    return T.stepped_raw(inp, mode), T.stepped_oracle(inp, mode, torch.float32)


@functools.lru_cache(maxsize=None)
def backward_ref(case, mode, seed):
    inp = T.stepped_inputs(case)
    r = T.stepped_raw(inp, mode)
    dlik = R.seed(r, seed, f"qtn.{case}.{mode}")
    return (r, dlik, T.stepped_oracle(inp, mode, torch.float64, dlik)[1],
            T.stepped_oracle(inp, mode, torch.float32, dlik)[1])


@functools.lru_cache(maxsize=None)
def yhat_ref(case):
    return T.yhat(T.stepped_inputs(case))


def qs_fwd(y, mu, sc, nz, steps, lik, yh, yh2, shape, steps_ptr=None):
    L = lib()
    N, Cc, H, W = shape
    return L.lib().icm_gc_likelihood_ste_qs_fwd(y.ptr, y.bs, mu.ptr, mu.bs, sc.ptr, sc.bs, nz.ptr, nz.bs,
                                                steps.data_ptr() if steps_ptr is None else steps_ptr, lik.ptr, lik.bs,
                                                yh.ptr, yh.bs, yh2.ptr, yh2.bs, N, Cc, H * W, SCALE_BOUND, LIK_BOUND,
                                                L.stream())


def qs_bwd(y, mu, sc, nz, steps, dl, dyh, dy, dmu, dsc, shape, accum, steps_ptr=None):
    L = lib()
    N, Cc, H, W = shape
    return L.lib().icm_gc_likelihood_ste_qs_bwd(y.ptr, y.bs, mu.ptr, mu.bs, sc.ptr, sc.bs, nz.ptr, nz.bs,
                                                steps.data_ptr() if steps_ptr is None else steps_ptr, dl.ptr, dl.bs,
                                                dyh.ptr, dyh.bs, dy.ptr, dy.bs, dmu.ptr, dmu.bs, dsc.ptr, dsc.bs, N, Cc,
                                                H * W, SCALE_BOUND, LIK_BOUND, accum, L.stream())


def codec_yhat(inp, y, mu, sc, shape):
    """y_hat of the codec's own kernels on the same device operands, image by image at that image's step:
    (icm_gc_code_q's, icm_dequantize_q's of the symbols it coded)"""
    L = lib()
    N, Cc, H, W = shape
    table = O.scale_table().to(dev()).contiguous()
    coded = torch.full(shape, NAN, dtype=torch.float32, device=dev())
    again = torch.full(shape, NAN, dtype=torch.float32, device=dev())
    per = Cc * H * W
    for n in range(N):
        step, inv = (float(v) for v in inp["steps"][n])
        sym = torch.empty((1, Cc, H, W), dtype=torch.int32, device=dev())
        idx = torch.empty_like(sym)
        L.check(L.lib().icm_gc_code_q(y.ptr + 4 * n * y.bs, y.bs, mu.ptr + 4 * n * mu.bs, mu.bs, sc.ptr + 4 * n * sc.bs,
                                      sc.bs, table.data_ptr(), table.numel(), SCALE_BOUND, step, inv, sym.data_ptr(),
                                      idx.data_ptr(), coded[n].data_ptr(), per, 1, Cc, H * W, L.stream()), "gc_code_q")
        L.check(L.lib().icm_dequantize_q(sym.data_ptr(), mu.ptr + 4 * n * mu.bs, mu.bs, step, again[n].data_ptr(), per,
                                         1, Cc, H * W, L.stream()), "dequantize_q")
        assert same_bits(sym, T.symbols(inp)[n:n + 1]), f"image {n}: the codec's symbols are not the reference's"
    return coded, again


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", ["strided", "tiny", "zero"])
def test_stepped_forward(case, mode, layout):
    shape = T.shape_of(case)
    inp = T.stepped_inputs(case)
    r, lik32 = forward_ref(case, mode)
    yh_ref = yhat_ref(case)
    steps = steps_dev(inp)
    y, mu, sc = (operand(shape, layout, 1, 0, inp["y"]), operand(shape, layout, 2, 1, inp["mu"]),
                 operand(shape, layout, 3, 3, inp["scale"]))
    nz = operand(shape, layout, 4, 2, inp["noise"]) if mode == "train" else Null
    coded, again = codec_yhat(inp, y, mu, sc, shape)
    assert same_bits(coded, yh_ref) and same_bits(again, yh_ref), "the codec's kernels and the numpy reference differ"
    for want_yh, want_yh2 in ((True, True), (False, True), (True, False), (False, False)):
        lik = operand(shape, layout, 5, 0)
        yh = operand(shape, layout, 6, 4) if want_yh else Null
        yh2 = operand(shape, layout, 7, 7) if want_yh2 else Null
        if layout == "slices" and mode == "train" and want_yh and want_yh2:
            assert len({s.bs for s in (y, mu, sc, nz, lik, yh, yh2)}) == 7
        lib().check(qs_fwd(y, mu, sc, nz, steps, lik, yh, yh2, shape), "gc_qs_fwd")
        what = f"stepped fwd {case} {mode} {layout} yh={int(want_yh)} yh2={int(want_yh2)}"
        for s in (y, mu, sc, lik) + ((nz,) if mode == "train" else ()) + ((yh,) if want_yh else ()) + ((yh2,) if want_yh2 else ()):
            assert s.outside_untouched(), what
        for s, v in ((y, inp["y"]), (mu, inp["mu"]), (sc, inp["scale"])):
            assert same_bits(s.cpu(), v), what + ": an input changed"
        assert same_bits(steps, inp["steps"]), what + ": the steps changed"
        for s, on in ((yh, want_yh), (yh2, want_yh2)):
            if on:
                assert same_bits(s.cpu(), yh_ref), what + ": y_hat is not the numpy reference's"
                assert same_bits(s.cpu(), coded) and same_bits(s.cpu(), again), what + ": y_hat is not the codec's"
        check_bands(what, lik.cpu(), lik32, r)
    if case == "zero":   # no step: the scalar kernel's y_hat
        assert same_bits(yh_ref, R.gaussian_yhat({k: inp[k] for k in ("y", "mu")}))


@pytest.mark.parametrize("mode", R.MODES)
def test_stepped_forward_long_grid(mode):
    shape = T.shape_of("long")
    assert int(np.prod(shape)) > 2048 * 256
    inp = T.stepped_inputs("long")
    r, lik32 = forward_ref("long", mode)
    y, mu, sc = (Slice(shape, 0, 0, inp[k]) for k in ("y", "mu", "scale"))
    nz = Slice(shape, 0, 0, inp["noise"]) if mode == "train" else Null
    lik, yh = Slice(shape, 0, 0), Slice(shape, 0, 0)
    lib().check(qs_fwd(y, mu, sc, nz, steps_dev(inp), lik, yh, Null, shape), "gc_qs_fwd")
    assert same_bits(yh.cpu(), yhat_ref("long"))
    coded, again = codec_yhat(inp, y, mu, sc, shape)
    assert same_bits(yh.cpu(), coded) and same_bits(yh.cpu(), again)
    check_bands(f"stepped fwd long {mode}", lik.cpu(), lik32, r)


# ------------------------------------------------------------------------------------------------ backward
def backward_case(case, mode, seed, layout, combos):
    shape = T.shape_of(case)
    inp = T.stepped_inputs(case)
    r, dlik, g64, g32 = backward_ref(case, mode, seed)
    live, floor, grey = R.classify(r)
    below, above, sgrey = R.scale_classes(inp["scale"])
    dyh_v = R.U(f"qtn.dyh.{case}", shape, -1.0, 1.0)
    prev_v = R.U(f"qtn.prev.{case}", shape, -2.0, 2.0)
    steps = steps_dev(inp)
    y, mu, sc = (operand(shape, layout, 1, 1, inp["y"]), operand(shape, layout, 2, 0, inp["mu"]),
                 operand(shape, layout, 3, 2, inp["scale"]))
    nz = operand(shape, layout, 4, 3, inp["noise"]) if mode == "train" else Null
    dl = operand(shape, layout, 5, 1, dlik)
    for use_dyh, accum in combos:
        what = f"stepped bwd {case} {mode} {seed} {layout} dyh={int(use_dyh)} accum={accum}"
        dyh = operand(shape, layout, 6, 6, dyh_v) if use_dyh else Null
        dy = operand(shape, layout, 7, 3, prev_v if accum else None)          # NaN inside too when not accumulating
        dmu, dsc = operand(shape, layout, 8, 4), operand(shape, layout, 9, 0)
        lib().check(qs_bwd(y, mu, sc, nz, steps, dl, dyh, dy, dmu, dsc, shape, accum), "gc_qs_bwd")
        for s in (dy, dmu, dsc):
            assert s.outside_untouched(), what
        got_dy, got_dmu, got_dsc = dy.cpu(), dmu.cpu(), dsc.cpu()
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
        # the two LowerBound gates, and the straight-through path: d y_hat reaches y unchanged and never mu
        off = floor & (dlik >= 0)
        if off.any():
            assert (got_dmu[off] == 0).all() and (got_dsc[off] == 0).all(), what + ": gradient through the floor"
            assert torch.equal(got_dy[off], add32[off]), what + ": dy through the floor"
        quiet = below & ~grey & (g64[2] == 0)
        assert (g64[2][below] <= 0).all()
        assert (got_dsc[quiet] == 0).all(), what + ": dscale below the scale bound"
        if mode == "eval":
            assert (got_dmu == 0).all(), what + ": dmu in eval mode"
            assert same_bits(got_dy, add32), what + ": dy in eval mode"
    return off, quiet


ALL_COMBOS = ((False, 0), (False, 1), (True, 0), (True, 1))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("seed", R.SEEDS)
@pytest.mark.parametrize("mode", R.MODES)
def test_stepped_backward(mode, seed, layout):
    off, quiet = backward_case("strided", mode, seed, layout, ALL_COMBOS)
    assert quiet.any() and (off.any() or seed == "bits")


@pytest.mark.parametrize("mode", R.MODES)
def test_stepped_backward_tiny_three_steps(mode):
    backward_case("tiny", mode, "mixed", "slices", ALL_COMBOS)
    backward_case("tiny", mode, "bits", "dense", ((True, 0),))


def test_stepped_backward_long_grid():
    backward_case("long", "train", "bits", "dense", ((True, 1),))


# ------------------------------------------------------------------------------------------------ refusals
def test_refused_calls_leave_the_outputs_alone():
    shape = T.shape_of("tiny")
    N, Cc, H, W = shape
    inp = T.stepped_inputs("tiny")
    steps = steps_dev(inp)
    y, mu, sc, nz = (Slice(shape, 1, 0, inp[k]) for k in ("y", "mu", "scale", "noise"))
    dl = Slice(shape, 1, 0, torch.ones(shape))
    L = lib().lib()
    st = lib().stream()

    def fwd(**kw):
        a = dict(y=y, mu=mu, sc=sc, steps=steps.data_ptr(), lik=lik, N=N, C=Cc, HW=H * W, bound=SCALE_BOUND)
        a.update(kw)
        return L.icm_gc_likelihood_ste_qs_fwd(a["y"].ptr, a["y"].bs, a["mu"].ptr, a["mu"].bs, a["sc"].ptr, a["sc"].bs,
                                              nz.ptr, nz.bs, a["steps"], a["lik"].ptr, a["lik"].bs, yh.ptr, yh.bs,
                                              yh2.ptr, yh2.bs, a["N"], a["C"], a["HW"], a["bound"], LIK_BOUND, st)

    def bwd(**kw):
        a = dict(y=y, mu=mu, sc=sc, steps=steps.data_ptr(), dl=dl, dy=dy, dmu=dmu, dsc=dsc, N=N, C=Cc, HW=H * W)
        a.update(kw)
        return L.icm_gc_likelihood_ste_qs_bwd(a["y"].ptr, a["y"].bs, a["mu"].ptr, a["mu"].bs, a["sc"].ptr, a["sc"].bs,
                                              nz.ptr, nz.bs, a["steps"], a["dl"].ptr, a["dl"].bs, 0, 0, a["dy"].ptr,
                                              a["dy"].bs, a["dmu"].ptr, a["dmu"].bs, a["dsc"].ptr, a["dsc"].bs, a["N"],
                                              a["C"], a["HW"], SCALE_BOUND, LIK_BOUND, 0, st)

    lik, yh, yh2 = Slice(shape, 1, 1), Slice(shape, 1, 0), Slice(shape, 1, 1)
    dy, dmu, dsc = Slice(shape, 1, 1), Slice(shape, 1, 0), Slice(shape, 1, 1)
    outs = (lik, yh, yh2, dy, dmu, dsc)
    refused = [("fwd steps null", fwd(steps=0)), ("fwd y null", fwd(y=Null)), ("fwd mu null", fwd(mu=Null)),
               ("fwd scale null", fwd(sc=Null)), ("fwd lik null", fwd(lik=Null)), ("fwd N 0", fwd(N=0)),
               ("fwd C 0", fwd(C=0)), ("fwd HW 0", fwd(HW=0)), ("fwd scale_bound 0", fwd(bound=0.0)),
               ("bwd steps null", bwd(steps=0)), ("bwd y null", bwd(y=Null)), ("bwd mu null", bwd(mu=Null)),
               ("bwd scale null", bwd(sc=Null)), ("bwd dlik null", bwd(dl=Null)), ("bwd dy null", bwd(dy=Null)),
               ("bwd dmu null", bwd(dmu=Null)), ("bwd dscale null", bwd(dsc=Null)), ("bwd N 0", bwd(N=0)),
               ("bwd C -1", bwd(C=-1)), ("bwd HW 0", bwd(HW=0))]
    torch.cuda.synchronize()
    for name, rc in refused:
        assert rc == ERR_ARG, f"{name}: returned {rc}"
    for s in outs:
        assert bool(torch.isnan(s.buf).all()), "a refused call wrote to an output"
    # ... and the same arguments, complete, are accepted
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert not torch.isnan(lik.cpu()).any() and not torch.isnan(dy.cpu()).any()


# ------------------------------------------------------------------------------------------------ weighted R-D loss
def flat(v=None, n=None):
    t = torch.full((n,), NAN, dtype=torch.float32, device=dev()) if v is None else v.to(dev()).contiguous()
    return t


def rdw_call(name, *args):
    L = lib()
    L.check(getattr(L.lib(), name)(*args, L.stream()), name)


@pytest.mark.parametrize("case", sorted(T.RDW_CASES))
def test_weighted_rd_loss(case):
    N, per, ny, nz = T.RDW_CASES[case]
    xv, xh, ly, lz, lam = T.rdw_inputs(case)
    npix = N * per // 3
    g = T.rdw_chains(N, per, ny, nz)
    assert (g["bpi"] > 1) == (case == "blocks")          # one workgroup per image, and several
    xd, hd, yd, zd, ld = (flat(t) for t in (xv, xh, ly, lz, lam))
    x64, h64, y64, z64, l64 = (t.double() for t in (xv, xh, ly, lz, lam))
    se_n = ((h64 - x64) ** 2).sum(1)
    ay, az = y64.log().abs().sum().item(), z64.log().abs().sum().item()
    den = math.log(2.0) * npix

    def run(entry, weights_dev):
        outs = []
        for _ in range(2):
            out, ws = flat(n=5), flat(n=8192)
            if entry == "icm_rd_loss_w_fwd":
                rdw_call(entry, xd.data_ptr(), hd.data_ptr(), N, per, yd.data_ptr(), ny, zd.data_ptr(), nz, npix,
                         weights_dev.data_ptr(), out.data_ptr(), ws.data_ptr())
            else:
                rdw_call(entry, xd.data_ptr(), hd.data_ptr(), N * per, yd.data_ptr(), ny, zd.data_ptr(), nz, npix,
                         weights_dev, out.data_ptr(), ws.data_ptr())
            outs.append(out.cpu())
        assert same_bits(outs[0], outs[1]), f"{entry}: two runs differ"
        assert torch.isfinite(outs[0]).all()
        return outs[0].double()

    def check(what, got, weights64):
        ref = T.rdw_loss(x64, h64, y64, z64, npix, weights64)
        P.check_sum(f"{what} bpp", got[0:1], ref[0:1], max(g["ky"], g["kz"]) + 4, (ay + az) / den)
        P.check_sum(f"{what} mse", got[1:2], ref[1:2], g["kx"] + 1, se_n.sum().item() / (N * per))
        P.check_sum(f"{what} sum log lik_y", got[3:4], ref[3:4], g["ky"], ay)
        P.check_sum(f"{what} sum log lik_z", got[4:5], ref[4:5], g["kz"], az)
        lim = T.rdw_loss_limit(x64, h64, y64, z64, npix, weights64)
        err = (got[2] - ref[2]).abs().item()
        print(f"{what} loss: gpu {err:.3e}, limit {lim:.3e}")
        assert err <= lim, f"{what} loss: {err:.3e} > limit {lim:.3e}"
        return lim

    check(f"rd_loss_w_fwd {case}", run("icm_rd_loss_w_fwd", ld), l64)
    # equal weights: the scalar loss, each within its own limit of the one float64 value
    lm = P.f32(0.0067)
    same = torch.full((N,), lm, dtype=torch.float32)
    got_w = run("icm_rd_loss_w_fwd", flat(same))
    lim_w = check(f"rd_loss_w_fwd {case} equal weights", got_w, same.double())
    got_s = run("icm_rd_loss_fwd", lm)
    ref = T.rdw_loss(x64, h64, y64, z64, npix, same.double())
    gs = P.rd_geometry(N * per, ny, nz)
    lim_s = (lm * 255.0 ** 2 * P.sum_limit(gs["k"][N * per] + 1, se_n.sum().item() / (N * per)) * (1 + 3 * P.ULP)
             + 3 * P.ULP * ref[2].abs().item() + P.sum_limit(max(gs["k"][ny], gs["k"][nz]) + 4, (ay + az) / den))
    assert (got_s[2] - ref[2]).abs().item() <= lim_s
    assert (got_w[2] - got_s[2]).abs().item() <= lim_w + lim_s
    assert (got_w[1] - got_s[1]).abs().item() <= 2 * P.sum_limit(max(g["kx"], gs["k"][N * per]) + 1,
                                                                  se_n.sum().item() / (N * per))
    # gradients
    for gscale in (1.0, 0.125):
        dxh, dly, dlz = flat(n=N * per), flat(n=ny), flat(n=nz)
        rdw_call("icm_rd_loss_w_bwd", xd.data_ptr(), hd.data_ptr(), N, per, yd.data_ptr(), ny, zd.data_ptr(), nz, npix,
                 ld.data_ptr(), gscale, dxh.data_ptr(), dly.data_ptr(), dlz.data_ptr())
        r64 = T.rdw_grads(x64, h64, y64, z64, npix, l64, gscale)
        r32 = T.rdw_grads(xv, xh, ly, lz, npix, lam, gscale)
        for name, o, a, b in zip(("dx_hat", "dlik_y", "dlik_z"), (dxh, dly, dlz), r32, r64):
            assert torch.isfinite(o).all()
            # the coefficients are formed in float32: six roundings, then a difference and a product / a quotient
            P.check_elementwise(f"rd_loss_w_bwd {case} gscale={gscale} {name}", o.cpu().reshape(b.shape), a, b,
                                5 * P.ULP * b.abs())


def test_weighted_rd_loss_refusals():
    N, per, ny, nz = T.RDW_CASES["odd"]
    xv, xh, ly, lz, lam = T.rdw_inputs("odd")
    xd, hd, yd, zd, ld = (flat(t) for t in (xv, xh, ly, lz, lam))
    out, ws = flat(n=5), flat(n=8192)
    dxh, dly, dlz = flat(n=N * per), flat(n=ny), flat(n=nz)
    L = lib().lib()
    st = lib().stream()
    p = lambda t: t.data_ptr()

    def fwd(N_=N, lam_=p(ld), out_=p(out), ws_=p(ws), per_=per, npix=N * per // 3):
        return L.icm_rd_loss_w_fwd(p(xd), p(hd), N_, per_, p(yd), ny, p(zd), nz, npix, lam_, out_, ws_, st)

    def bwd(N_=N, lam_=p(ld), dxh_=p(dxh)):
        return L.icm_rd_loss_w_bwd(p(xd), p(hd), N_, per, p(yd), ny, p(zd), nz, N * per // 3, lam_, 1.0, dxh_, p(dly),
                                   p(dlz), st)

    # 2731 images need 3 * 2731 = 8193 partial sums: one more than ICM_REDUCE_WS_FLOATS holds (never launched: the
    # buffers hold three images)
    rcs = [fwd(lam_=0), fwd(out_=0), fwd(ws_=0), fwd(N_=0), fwd(per_=0), fwd(npix=0), fwd(N_=2731), bwd(lam_=0),
           bwd(dxh_=0), bwd(N_=0), bwd(N_=2731)]
    torch.cuda.synchronize()
    assert rcs == [ERR_ARG] * len(rcs), rcs
    for t in (out, ws, dxh, dly, dlz):
        assert bool(torch.isnan(t).all()), "a refused call wrote to an output"
    assert fwd() == 0 and bwd() == 0
