"""The kernels of quality-map training through the C ABI against float64: the likelihood + STE pair with a quantiser step
per (image, latent position) (csrc/qstep.hip: icm_gc_likelihood_ste_qm_fwd / _bwd), the R-D loss with a distortion
weight per 16 x 16 cell (csrc/pointwise.hip: icm_rd_loss_m_fwd / _bwd) and the map painter (icm_qmap_paint).

Likelihoods are compared in bits and gradients element-wise, by the rule and constants of tests/_entropy_ref.py: every
limit is FACTOR times the error of the float32 restatement of tests/_qmtrain_ref.py against its float64 run on the same
inputs, plus that file's floor; none is taken from a kernel's output.  y_hat is compared bit for bit: with
tests/_qstep_ref.py's numpy arithmetic at each position's step, with the codec's map kernel where the map is shared by
the batch, and every output with the per-image pair's where the maps are uniform.  The sums of the loss follow
tests/_pointwise_ref.py's rule (gamma(k) of the longest chain of additions, restated from the launch geometry in
tests/_qmtrain_ref.py).  tests/test_qmtrain_ref.py asserts, without a GPU, what the inputs must provide.  pytest -s
prints each measured figure next to its limit."""
import functools
import math

import numpy as np
import pytest
import torch

import _entropy_ref as R
import _pointwise_ref as P
import _qmtrain_ref as M
import _qtrain_ref as T
from oracle import wacnn_oracle as O
from test_gpu_entropy_numerics import (LIK_BOUND, NAN, SCALE_BOUND, Null, Slice, check_bands, check_grad, dev, lib,
                                       same_bits)

pytestmark = pytest.mark.gpu

ERR_ARG = 1
LAYOUT = {"strided": "slices", "tiny": "slices", "long": "dense", "uniform": "dense"}


def operand(case, extra, off, value=None):
    """a [N,C,H,W] operand of the case: dense, or ``off`` channels into its own NaN-filled buffer of C + extra channels"""
    shape = M.shape_of(case)
    return Slice(shape, extra, off, value) if LAYOUT[case] == "slices" else Slice(shape, 0, 0, value)


@functools.lru_cache(maxsize=None)
def table_dev():
    return torch.from_numpy(M.step_table()).to(dev()).contiguous()


@functools.lru_cache(maxsize=None)
def forward_ref(case, mode):
    inp = M.inputs(case)
    return M.raw(inp, mode), M.oracle(inp, mode, torch.float32)


@functools.lru_cache(maxsize=None)
def backward_ref(case, mode, seed):
    inp = M.inputs(case)
    r = M.raw(inp, mode)
    dlik = R.seed(r, seed, f"qmn.{case}.{mode}")
    return r, dlik, M.oracle(inp, mode, torch.float64, dlik)[1], M.oracle(inp, mode, torch.float32, dlik)[1]


@functools.lru_cache(maxsize=None)
def yhat_ref(case):
    return M.yhat(M.inputs(case))


def qm_fwd(y, mu, sc, nz, qmap, lik, yh, yh2, shape, **kw):
    L = lib()
    N, Cc, H, W = shape
    a = dict(qmap_ptr=qmap.data_ptr(), table=table_dev().data_ptr(), N=N, C=Cc, HW=H * W, bound=SCALE_BOUND)
    a.update(kw)
    return L.lib().icm_gc_likelihood_ste_qm_fwd(y.ptr, y.bs, mu.ptr, mu.bs, sc.ptr, sc.bs, nz.ptr, nz.bs, a["qmap_ptr"],
                                                a["table"], lik.ptr, lik.bs, yh.ptr, yh.bs, yh2.ptr, yh2.bs, a["N"],
                                                a["C"], a["HW"], a["bound"], LIK_BOUND, L.stream())


def qm_bwd(y, mu, sc, nz, qmap, dl, dyh, dy, dmu, dsc, shape, accum, **kw):
    L = lib()
    N, Cc, H, W = shape
    a = dict(qmap_ptr=qmap.data_ptr(), table=table_dev().data_ptr(), N=N, C=Cc, HW=H * W)
    a.update(kw)
    return L.lib().icm_gc_likelihood_ste_qm_bwd(y.ptr, y.bs, mu.ptr, mu.bs, sc.ptr, sc.bs, nz.ptr, nz.bs, a["qmap_ptr"],
                                                a["table"], dl.ptr, dl.bs, dyh.ptr, dyh.bs, dy.ptr, dy.bs, dmu.ptr,
                                                dmu.bs, dsc.ptr, dsc.bs, a["N"], a["C"], a["HW"], SCALE_BOUND,
                                                LIK_BOUND, accum, L.stream())


def qs_fwd(y, mu, sc, nz, steps, lik, yh, yh2, shape):
    L = lib()
    N, Cc, H, W = shape
    return L.lib().icm_gc_likelihood_ste_qs_fwd(y.ptr, y.bs, mu.ptr, mu.bs, sc.ptr, sc.bs, nz.ptr, nz.bs,
                                                steps.data_ptr(), lik.ptr, lik.bs, yh.ptr, yh.bs, yh2.ptr, yh2.bs, N,
                                                Cc, H * W, SCALE_BOUND, LIK_BOUND, L.stream())


def qs_bwd(y, mu, sc, nz, steps, dl, dyh, dy, dmu, dsc, shape, accum):
    L = lib()
    N, Cc, H, W = shape
    return L.lib().icm_gc_likelihood_ste_qs_bwd(y.ptr, y.bs, mu.ptr, mu.bs, sc.ptr, sc.bs, nz.ptr, nz.bs,
                                                steps.data_ptr(), dl.ptr, dl.bs, dyh.ptr, dyh.bs, dy.ptr, dy.bs,
                                                dmu.ptr, dmu.bs, dsc.ptr, dsc.bs, N, Cc, H * W, SCALE_BOUND, LIK_BOUND,
                                                accum, L.stream())


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", M.MAP_CASES)
def test_map_forward(case, mode):
    shape = M.shape_of(case)
    inp = M.inputs(case)
    r, lik32 = forward_ref(case, mode)
    yh_ref = yhat_ref(case)
    qmap = inp["qmap"].to(dev()).contiguous()
    y, mu, sc = operand(case, 1, 0, inp["y"]), operand(case, 2, 1, inp["mu"]), operand(case, 3, 3, inp["scale"])
    nz = operand(case, 4, 2, inp["noise"]) if mode == "train" else Null
    for want_yh2 in (True, False):
        lik, yh = operand(case, 5, 0), operand(case, 6, 4)
        yh2 = operand(case, 7, 7) if want_yh2 else Null
        lib().check(qm_fwd(y, mu, sc, nz, qmap, lik, yh, yh2, shape), "gc_qm_fwd")
        what = f"map fwd {case} {mode} yh2={int(want_yh2)}"
        for s in (y, mu, sc, lik, yh) + ((nz,) if mode == "train" else ()) + ((yh2,) if want_yh2 else ()):
            assert s.outside_untouched(), what
        for s, v in ((y, inp["y"]), (mu, inp["mu"]), (sc, inp["scale"])):
            assert same_bits(s.cpu(), v), what + ": an input changed"
        assert torch.equal(qmap.cpu(), inp["qmap"]), what + ": the map changed"
        for s in (yh,) + ((yh2,) if want_yh2 else ()):
            assert same_bits(s.cpu(), yh_ref), what + ": y_hat is not the dequantised symbol of each position"
        check_bands(what, lik.cpu(), lik32, r)
        if case == "uniform":      # the per-image pair on the same operands: the same bits
            steps = M.per_image_steps(case).to(dev()).contiguous()
            lik_s, yh_s = operand(case, 5, 0), operand(case, 6, 4)
            yh2_s = operand(case, 7, 7) if want_yh2 else Null
            lib().check(qs_fwd(y, mu, sc, nz, steps, lik_s, yh_s, yh2_s, shape), "gc_qs_fwd")
            assert same_bits(lik.cpu(), lik_s.cpu()) and same_bits(yh.cpu(), yh_s.cpu()), what + ": not the _qs pair's"
            if want_yh2:
                assert same_bits(yh2.cpu(), yh2_s.cpu())


@pytest.mark.parametrize("case", ["strided", "long"])
def test_a_batch_shared_map_gives_the_codecs_yhat(case):
    """one map for the whole batch: y_hat is icm_gc_code_qmap's on the same device operands, bit for bit"""
    L = lib()
    shape = M.shape_of(case)
    N, Cc, H, W = shape
    inp = M.inputs(case)
    one = inp["qmap"][0].to(dev()).contiguous()
    shared = one.unsqueeze(0).expand(N, H, W).contiguous()
    y, mu, sc = operand(case, 1, 1, inp["y"]), operand(case, 2, 0, inp["mu"]), operand(case, 3, 2, inp["scale"])
    lik, yh = operand(case, 5, 0), operand(case, 6, 4)
    L.check(qm_fwd(y, mu, sc, Null, shared, lik, yh, Null, shape), "gc_qm_fwd")
    table = O.scale_table().to(dev()).contiguous()
    sym = torch.empty(shape, dtype=torch.int32, device=dev())
    idx = torch.empty_like(sym)
    coded = operand(case, 2, 1)
    L.check(L.lib().icm_gc_code_qmap(y.ptr, y.bs, mu.ptr, mu.bs, sc.ptr, sc.bs, table.data_ptr(), table.numel(),
                                     SCALE_BOUND, one.data_ptr(), table_dev().data_ptr(), sym.data_ptr(),
                                     idx.data_ptr(), coded.ptr, coded.bs, N, Cc, H * W, L.stream()), "gc_code_qmap")
    assert same_bits(yh.cpu(), coded.cpu())
    assert same_bits(yh.cpu()[0], yhat_ref(case)[0])          # image 0 under its own map: the numpy reference too


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("accum", [0, 1])
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", M.MAP_CASES)
def test_map_backward(case, mode, accum):
    shape = M.shape_of(case)
    inp = M.inputs(case)
    seed = "mixed" if accum and case != "long" else "bits"       # (the long case's float64 reference is made once)
    r, dlik, g64, g32 = backward_ref(case, mode, seed)
    live, floor, grey = R.classify(r)
    below, above, sgrey = R.scale_classes(inp["scale"])
    dyh_v = R.U(f"qmn.dyh.{case}", shape, -1.0, 1.0)
    prev_v = R.U(f"qmn.prev.{case}", shape, -2.0, 2.0)
    qmap = inp["qmap"].to(dev()).contiguous()
    y, mu, sc = operand(case, 1, 1, inp["y"]), operand(case, 2, 0, inp["mu"]), operand(case, 3, 2, inp["scale"])
    nz = operand(case, 4, 3, inp["noise"]) if mode == "train" else Null
    dl = operand(case, 5, 1, dlik)
    for use_dyh in ((True, False) if case in ("strided", "tiny") else (True,)):
        what = f"map bwd {case} {mode} {seed} dyh={int(use_dyh)} accum={accum}"
        dyh = operand(case, 6, 6, dyh_v) if use_dyh else Null

        def outs():
            return operand(case, 7, 3, prev_v if accum else None), operand(case, 8, 4), operand(case, 9, 0)
        dy, dmu, dsc = outs()
        lib().check(qm_bwd(y, mu, sc, nz, qmap, dl, dyh, dy, dmu, dsc, shape, accum), "gc_qm_bwd")
        for s in (dy, dmu, dsc):
            assert s.outside_untouched(), what
        got_dy, got_dmu, got_dsc = dy.cpu(), dmu.cpu(), dsc.cpu()
        add32, add64, dy32 = torch.zeros(shape), torch.zeros(shape, dtype=torch.float64), g32[0]
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
        if case == "uniform":
            steps = M.per_image_steps(case).to(dev()).contiguous()
            dy_s, dmu_s, dsc_s = outs()
            lib().check(qs_bwd(y, mu, sc, nz, steps, dl, dyh, dy_s, dmu_s, dsc_s, shape, accum), "gc_qs_bwd")
            for a, b in ((dy, dy_s), (dmu, dmu_s), (dsc, dsc_s)):
                assert same_bits(a.cpu(), b.cpu()), what + ": not the _qs pair's"
    if case == "strided":
        assert quiet.any() and (off.any() or seed == "bits")


# ------------------------------------------------------------------------------------------------ refusals
def test_refused_map_calls_leave_the_outputs_alone():
    case = "tiny"
    shape = M.shape_of(case)
    inp = M.inputs(case)
    qmap = inp["qmap"].to(dev()).contiguous()
    y, mu, sc, nz = (Slice(shape, 1, 0, inp[k]) for k in ("y", "mu", "scale", "noise"))
    dl = Slice(shape, 1, 0, torch.ones(shape))
    lik, yh, yh2 = Slice(shape, 1, 1), Slice(shape, 1, 0), Slice(shape, 1, 1)
    dy, dmu, dsc = Slice(shape, 1, 1), Slice(shape, 1, 0), Slice(shape, 1, 1)

    def fwd(y=y, mu=mu, sc=sc, lik=lik, **kw):
        return qm_fwd(y, mu, sc, nz, qmap, lik, yh, yh2, shape, **kw)

    def bwd(y=y, mu=mu, sc=sc, dl=dl, dy=dy, dmu=dmu, dsc=dsc, **kw):
        return qm_bwd(y, mu, sc, nz, qmap, dl, Null, dy, dmu, dsc, shape, 0, **kw)

    refused = [("fwd qmap null", fwd(qmap_ptr=0)), ("fwd step_table null", fwd(table=0)), ("fwd y null", fwd(y=Null)),
               ("fwd mu null", fwd(mu=Null)), ("fwd scale null", fwd(sc=Null)), ("fwd lik null", fwd(lik=Null)),
               ("fwd N 0", fwd(N=0)), ("fwd C 0", fwd(C=0)), ("fwd HW 0", fwd(HW=0)), ("fwd scale_bound 0", fwd(bound=0.0)),
               ("bwd qmap null", bwd(qmap_ptr=0)), ("bwd step_table null", bwd(table=0)), ("bwd y null", bwd(y=Null)),
               ("bwd mu null", bwd(mu=Null)), ("bwd scale null", bwd(sc=Null)), ("bwd dlik null", bwd(dl=Null)),
               ("bwd dy null", bwd(dy=Null)), ("bwd dmu null", bwd(dmu=Null)), ("bwd dscale null", bwd(dsc=Null)),
               ("bwd N 0", bwd(N=0)), ("bwd C -1", bwd(C=-1)), ("bwd HW 0", bwd(HW=0))]
    torch.cuda.synchronize()
    for name, rc in refused:
        assert rc == ERR_ARG, f"{name}: returned {rc}"
    for s in (lik, yh, yh2, dy, dmu, dsc):
        assert bool(torch.isnan(s.buf).all()), "a refused call wrote to an output"
    assert fwd() == 0 and bwd() == 0          # ... and the same arguments, complete, are accepted
    torch.cuda.synchronize()
    assert not torch.isnan(lik.cpu()).any() and not torch.isnan(dy.cpu()).any()


# ------------------------------------------------------------------------------------------------ per-cell R-D loss
def flat(v=None, n=None):
    return torch.full((n,), NAN, dtype=torch.float32, device=dev()) if v is None else v.to(dev()).contiguous()


def call(name, *args):
    L = lib()
    L.check(getattr(L.lib(), name)(*args, L.stream()), name)


@pytest.mark.parametrize("case", sorted(M.LOSS_CASES))
def test_per_cell_rd_loss(case):
    N, C, H, W = M.LOSS_CASES[case]
    xv, xh, ly, lz, qm = M.loss_inputs(case)
    ny, nz, npix, per = ly.numel(), lz.numel(), N * H * W, C * H * W
    g = M.m_chains(N, C, H, W, ny, nz)
    table = M.lmbda_table()
    xd, hd, yd, zd, td = (flat(t) for t in (xv, xh, ly, lz, table))
    x64, h64, y64, z64 = (t.double() for t in (xv, xh, ly, lz))
    se = ((h64 - x64) ** 2).sum().item()
    ay, az = y64.log().abs().sum().item(), z64.log().abs().sum().item()
    den = math.log(2.0) * npix

    def run_m(m):
        md = torch.from_numpy(m).to(dev()).contiguous()
        outs = []
        for _ in range(2):
            out, ws = flat(n=5), flat(n=8192)
            call("icm_rd_loss_m_fwd", xd.data_ptr(), hd.data_ptr(), N, C, H, W, 16, md.data_ptr(), td.data_ptr(),
                 yd.data_ptr(), ny, zd.data_ptr(), nz, npix, out.data_ptr(), ws.data_ptr())
            outs.append(out.cpu())
        assert same_bits(outs[0], outs[1]), "icm_rd_loss_m_fwd: two runs differ"
        assert torch.isfinite(outs[0]).all()
        return outs[0].double()

    def check(what, got, lam):
        ref = M.m_loss(x64, h64, y64, z64, npix, lam)
        P.check_sum(f"{what} bpp", got[0:1], ref[0:1], max(g["ky"], g["kz"]) + 4, (ay + az) / den)
        P.check_sum(f"{what} mse", got[1:2], ref[1:2], g["kx"] + 1, se / (N * per))
        P.check_sum(f"{what} sum log lik_y", got[3:4], ref[3:4], g["ky"], ay)
        P.check_sum(f"{what} sum log lik_z", got[4:5], ref[4:5], g["kz"], az)
        lim = M.m_loss_limit(x64, h64, y64, z64, npix, lam)
        err = (got[2] - ref[2]).abs().item()
        print(f"{what} loss: gpu {err:.3e}, limit {lim:.3e}")
        assert err <= lim, f"{what} loss: {err:.3e} > limit {lim:.3e}"
        return lim

    lam64 = M.pixel_weights(qm, table)
    check(f"rd_loss_m_fwd {case}", run_m(qm), lam64)
    # maps uniform over each image: the per-image pair, each within its own limit of the one float64 value
    ks = [(-16, 5, 32)[n] for n in range(N)]
    uni = np.ascontiguousarray(np.asarray(ks, dtype=np.int8).reshape(N, 1, 1) * np.ones((1, H // 16, W // 16), dtype=np.int8))
    lam_n = table[torch.tensor([k & 255 for k in ks])]
    got_m = run_m(uni)
    lim_m = check(f"rd_loss_m_fwd {case} uniform maps", got_m, M.pixel_weights(uni, table))
    out, ws = flat(n=5), flat(n=8192)
    call("icm_rd_loss_w_fwd", xd.data_ptr(), hd.data_ptr(), N, per, yd.data_ptr(), ny, zd.data_ptr(), nz, npix,
         flat(lam_n).data_ptr(), out.data_ptr(), ws.data_ptr())
    got_w = out.cpu().double()
    xf, hf = x64.reshape(N, per), h64.reshape(N, per)
    ref_w = T.rdw_loss(xf, hf, y64, z64, npix, lam_n.double())
    lim_w = T.rdw_loss_limit(xf, hf, y64, z64, npix, lam_n.double())
    assert (got_w[2] - ref_w[2]).abs().item() <= lim_w
    print(f"rd_loss_m_fwd {case} uniform maps against rd_loss_w_fwd: {(got_m[2] - got_w[2]).abs().item():.3e}, "
          f"limit {lim_m + lim_w:.3e}")
    assert (got_m[2] - got_w[2]).abs().item() <= lim_m + lim_w
    gw = T.rdw_chains(N, per, ny, nz)
    assert (got_m[1] - got_w[1]).abs().item() <= 2 * P.sum_limit(max(g["kx"], gw["kx"]) + 1, se / (N * per))
    # gradients, element-wise.  The coefficient is formed in float32: the pixel count's product, gscale * 255^2 (the
    # factor 2 is exact), the quotient, the weight's product; then the difference and the last product: six roundings
    # of half an ulp each (the likelihoods': ln 2 as a float, its product, two quotients)
    md = torch.from_numpy(qm).to(dev()).contiguous()
    for gscale in (1.0, 0.125):
        dxh, dly, dlz = flat(n=N * per), flat(n=ny), flat(n=nz)
        call("icm_rd_loss_m_bwd", xd.data_ptr(), hd.data_ptr(), N, C, H, W, 16, md.data_ptr(), td.data_ptr(),
             yd.data_ptr(), ny, zd.data_ptr(), nz, npix, gscale, dxh.data_ptr(), dly.data_ptr(), dlz.data_ptr())
        r64 = M.m_grads(x64, h64, y64, z64, npix, lam64, gscale)
        r32 = M.m_grads(xv, xh, ly, lz, npix, M.pixel_weights(qm, table, torch.float32), gscale)
        for name, o, a, b in zip(("dx_hat", "dlik_y", "dlik_z"), (dxh, dly, dlz), r32, r64):
            assert torch.isfinite(o).all()
            P.check_elementwise(f"rd_loss_m_bwd {case} gscale={gscale} {name}", o.cpu().reshape(b.shape), a, b,
                                3 * P.ULP * b.abs())


def test_per_cell_rd_loss_refusals():
    N, C, H, W = M.LOSS_CASES["odd"]
    xv, xh, ly, lz, qm = M.loss_inputs("odd")
    ny, nz, npix = ly.numel(), lz.numel(), N * H * W
    xd, hd, yd, zd, td = (flat(t) for t in (xv, xh, ly, lz, M.lmbda_table()))
    md = torch.from_numpy(qm).to(dev()).contiguous()
    out, ws = flat(n=5), flat(n=8192)
    dxh, dly, dlz = flat(n=xv.numel()), flat(n=ny), flat(n=nz)
    L = lib().lib()
    st = lib().stream()
    p = lambda t: t.data_ptr()

    def fwd(x=p(xd), xh_=p(hd), N_=N, C_=C, H_=H, W_=W, cell=16, m=p(md), t=p(td), y=p(yd), z=p(zd), npix_=npix,
            out_=p(out), ws_=p(ws)):
        return L.icm_rd_loss_m_fwd(x, xh_, N_, C_, H_, W_, cell, m, t, y, ny, z, nz, npix_, out_, ws_, st)

    def bwd(N_=N, H_=H, W_=W, cell=16, m=p(md), t=p(td), dxh_=p(dxh), dly_=p(dly), dlz_=p(dlz)):
        return L.icm_rd_loss_m_bwd(p(xd), p(hd), N_, C, H_, W_, cell, m, t, p(yd), ny, p(zd), nz, npix, 1.0, dxh_, dly_,
                                   dlz_, st)

    # 2049 images need 4 * 2049 = 8196 partial sums: more than ICM_REDUCE_WS_FLOATS holds (never launched: the buffers
    # hold three images); 40 and 88 are no multiples of 16; a 32-pixel cell does not divide 48 or 80
    rcs = [fwd(x=0), fwd(xh_=0), fwd(m=0), fwd(t=0), fwd(y=0), fwd(z=0), fwd(out_=0), fwd(ws_=0), fwd(N_=0), fwd(C_=0),
           fwd(H_=0), fwd(W_=0), fwd(npix_=0), fwd(cell=0), fwd(cell=-16), fwd(cell=32), fwd(H_=40), fwd(W_=88),
           fwd(N_=2049), bwd(m=0), bwd(t=0), bwd(dxh_=0), bwd(dly_=0), bwd(dlz_=0), bwd(N_=0), bwd(cell=0), bwd(H_=40),
           bwd(W_=88), bwd(N_=2049)]
    torch.cuda.synchronize()
    assert rcs == [ERR_ARG] * len(rcs), rcs
    for t_ in (out, ws, dxh, dly, dlz):
        assert bool(torch.isnan(t_).all()), "a refused call wrote to an output"
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(dxh).all()


# ------------------------------------------------------------------------------------------------ painter
def paint_rects(N, R_, h, w, rng):
    """[N, R, 5]: random rectangles, among them overlapping, empty and out-of-map ones (coordinates from -2 to side + 2)"""
    r = np.empty((N, R_, 5), dtype=np.int32)
    for a, side in ((0, h), (1, w)):
        r[..., a] = rng.integers(-2, side + 1, (N, R_))
        r[..., a + 2] = r[..., a] + rng.integers(0, side + 3, (N, R_))          # extent 0: empty
    r[..., 4] = rng.integers(-16, 33, (N, R_))
    if R_ >= 8:
        r[0, 1] = (0, 0, h, w, 7)              # the whole map, painted over by what follows
        r[0, 3, 2] = r[0, 3, 0]                # empty
        r[0, 5] = (h, w, h + 2, w + 2, -3)     # outside
    return r


@pytest.mark.parametrize("R_", [0, 1, 8])
@pytest.mark.parametrize("hw", [(1, 1), (4, 4), (5, 7), (16, 16)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_qmap_paint(hw, R_):
    h, w = hw
    N = 3
    rng = np.random.default_rng(100 * h + 10 * w + R_)
    base = rng.integers(-16, 33, N).astype(np.int8)
    rects = paint_rects(N, R_, h, w, rng)
    want = M.paint(base, rects, h, w)
    bd = torch.from_numpy(base).to(dev())
    rd = torch.from_numpy(rects.reshape(-1) if R_ else np.zeros(5, dtype=np.int32)).to(dev())     # R = 0: never read
    buf = torch.full((N * h * w + 64,), 99, dtype=torch.int8, device=dev())
    call("icm_qmap_paint", bd.data_ptr(), rd.data_ptr(), R_, buf.data_ptr() + 32, N, h, w)
    got = buf.cpu().numpy()
    assert (got[:32] == 99).all() and (got[32 + N * h * w:] == 99).all(), "the painter wrote outside the maps"
    assert np.array_equal(got[32:32 + N * h * w].reshape(N, h, w), want)
    if R_ == 8:
        assert not (want == base.reshape(N, 1, 1)).all()


def test_qmap_paint_refusals():
    L = lib().lib()
    st = lib().stream()
    base = torch.zeros(2, dtype=torch.int8, device=dev())
    rects = torch.zeros(2 * 5, dtype=torch.int32, device=dev())
    out = torch.full((2 * 4 * 4,), 99, dtype=torch.int8, device=dev())

    def paint(b=base.data_ptr(), r=rects.data_ptr(), R_=1, o=out.data_ptr(), N=2, h=4, w=4):
        return L.icm_qmap_paint(b, r, R_, o, N, h, w, st)
    rcs = [paint(b=0), paint(r=0), paint(o=0), paint(N=0), paint(h=0), paint(w=0), paint(R_=-1)]
    torch.cuda.synchronize()
    assert rcs == [ERR_ARG] * len(rcs), rcs
    assert (out == 99).all(), "a refused call wrote to the map"
    assert paint() == 0
    torch.cuda.synchronize()
    assert (out == 0).all()
