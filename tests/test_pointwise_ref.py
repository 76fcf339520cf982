"""tests/_pointwise_ref.py against torch float64 autograd and oracle/, without a GPU: each restatement matches the torch
op it restates to 1e-12 relative, the input generators reach the tails the GPU cases claim, and every GPU case yields
the split count / tiles per workgroup / finish kernel it is named for."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _pointwise_ref as R
from oracle import wacnn_oracle as O
from oracle import zigzag_oracle as Z

F64 = torch.float64


def close(a, b, rel=1e-12, scale=None):
    """max |a - b| <= rel * the largest magnitude of b (or of ``scale``: the terms b is a difference of)"""
    a, b = a.detach().double(), b.detach().double()
    scale = max((b if scale is None else scale.detach()).abs().max().item(), 1e-300)
    err = (a - b).abs().max().item()
    assert err <= rel * scale, f"{err:.3e} > {rel:.0e} * {scale:.3e}"


def leaf(name, shape, lo, hi):
    return R.u("t." + name, shape, lo, hi).double().requires_grad_(True)


# ------------------------------------------------------------------------------------------------ restatements
@pytest.mark.parametrize("C", [1, 3, 48])
def test_layernorm_matches_torch(C):
    N, HW = 2, 7
    x, g, b = leaf("x", (N, C, HW), -2, 3), leaf("g", (C,), 0.5, 1.5), leaf("b", (C,), -1, 1)
    y, mean, rstd = R.layernorm_fwd(x, g, b)
    want = F.layer_norm(x.permute(0, 2, 1), (C,), g, b, R.LN_EPS).permute(0, 2, 1)
    close(y, want)
    close(mean, x.mean(1))
    close(rstd, 1.0 / torch.sqrt(x.var(1, unbiased=False) + R.LN_EPS))
    dy = R.u("t.dy", (N, C, HW), -1, 1).double()
    dx_w, dg_w, db_w = torch.autograd.grad(want, (x, g, b), dy)
    dx, dg, db = R.layernorm_bwd(x.detach(), dy, g.detach(), mean.detach(), rstd.detach())
    terms = rstd.detach()[:, None] * dy * g.detach()[None, :, None]       # at C = 1 dx is a difference that vanishes
    close(dx, dx_w, scale=terms), close(dg, dg_w, scale=dy), close(db, db_w)
    extra, prev = R.u("t.e", (N, C, HW), -1, 1).double(), R.u("t.p", (N, C, HW), -1, 1).double()
    gp, bp = R.u("t.gp", (C,), -1, 1).double(), R.u("t.bp", (C,), -1, 1).double()
    dx, dg, db = R.layernorm_bwd(x.detach(), dy, g.detach(), mean.detach(), rstd.detach(), extra, prev, gp, bp)
    close(dx, dx_w + extra + prev), close(dg, dg_w + gp), close(db, db_w + bp)


def test_reductions_and_rd_loss_match_torch():
    x = R.u("t.cs", (2, 3, 11), -1, 1).double()
    close(R.channel_sum(x), torch.stack([x[:, c].sum() for c in range(3)]))
    close(R.sqnorm(x), torch.linalg.vector_norm(x) ** 2)
    img, xh = R.u("t.i", (600,), 0, 1).double(), leaf("xh", (600,), 0, 1)
    ly, lz = R.likelihoods("t.ly", 50).double().requires_grad_(True), R.likelihoods("t.lz", 7).double().requires_grad_(True)
    npix, lm = 200, 0.0067
    out = R.rd_loss_fwd(img, xh, ly, lz, npix, lm)
    mse = F.mse_loss(xh, img)
    bpp = torch.log(ly).sum() / (-math.log(2) * npix) + torch.log(lz).sum() / (-math.log(2) * npix)
    close(out, torch.stack([bpp, mse, lm * 255 ** 2 * mse + bpp, torch.log(ly).sum(), torch.log(lz).sum()]))
    for gs in (1.0, 0.125):
        want = torch.autograd.grad(out[2] * gs, (xh, ly, lz), retain_graph=True)
        got = R.rd_loss_bwd(img, xh.detach(), ly.detach(), lz.detach(), npix, lm, gs)
        for a, b in zip(got, want):
            close(a, b)


@pytest.mark.parametrize("clip", ["none", "active", "inactive"])
@pytest.mark.parametrize("gscale", [1.0, 0.125])
def test_adam_matches_torch_optim(clip, gscale):
    n, lr, b1, b2, eps = 33, 1e-3, 0.9, 0.999, 1e-8
    p0, g = R.u("t.ap", (n,), -1, 1).double(), R.u("t.ag", (n,), -30, 30).double()
    sq = None if clip == "none" else R.sqnorm(g).item()
    max_norm = 1.0 if clip == "active" else 1e9
    coef = R.clip_coef(sq, max_norm, gscale)
    if clip == "active":
        assert coef < 0.1 * gscale
    if clip == "inactive":
        assert coef == gscale
    p = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps)
    for _ in range(3):
        p.grad = g * gscale                              # the loss was scaled by gscale ...
        if sq is not None:                               # ... and the clip sees the scaled gradient (clip_grad_norm_'s rule)
            total = torch.linalg.vector_norm(p.grad)
            close(total, torch.tensor(math.sqrt(sq) * gscale, dtype=F64))
            p.grad = p.grad * torch.clamp(max_norm / (total + 1e-6), max=1.0)
        opt.step()
    got = R.adam_steps(p0, g, torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64), 3, lr, b1, b2, eps, coef)
    st = opt.state[p]
    close(got[0], p, 1e-11), close(got[1], st["exp_avg"], 1e-11), close(got[2], st["exp_avg_sq"], 1e-11)


def test_pointwise_match_torch():
    n = 300
    x = R.gelu_inputs("t.gx", n).double().requires_grad_(True)
    close(R.gelu(x), F.gelu(x))
    close(R.dgelu(x), torch.autograd.grad(F.gelu(x).sum(), x)[0])
    b = R.sigmoid_inputs("t.sb", n).double().requires_grad_(True)
    close(R.sigmoid(b), torch.sigmoid(b))
    # gate
    b = leaf("gb", (n,), -6, 6)
    res, g = leaf("gr", (n,), -1, 1), R.u("t.gg", (n,), -1, 1).double()
    out = F.gelu(x) * torch.sigmoid(b) + res
    close(R.gate_fwd(x, b, res), out)
    want = torch.autograd.grad(out, (x, b, res), g)
    pa, px = R.u("t.pa", (n,), -1, 1).double(), R.u("t.px", (n,), -1, 1).double()
    for a, w in zip(R.gate_bwd(g, x.detach(), b.detach()), want):
        close(a, w)
    got = R.gate_bwd(g, x.detach(), b.detach(), pa, px)
    close(got[0], want[0] + pa), close(got[2], want[2] + px)
    # add_grad
    close(R.add_grad(g, x.detach()), torch.autograd.grad(F.gelu(x), x, g)[0])
    close(R.add_grad(g, None, pa), g + pa)
    close(R.add_grad(g, x.detach(), pa), torch.autograd.grad(F.gelu(x), x, g)[0] + pa)
    # NonNegativeParametrizer: max(p, bound)^2 - pedestal, LowerBound's gradient rule
    p = R.nonneg_inputs("t.np", n).double().requires_grad_(True)
    close(R.nonneg_fwd(p, R.NONNEG_BOUND, R.NONNEG_PED), torch.clamp_min(p, R.NONNEG_BOUND) ** 2 - R.NONNEG_PED)
    pd = p.detach()
    gg = g * 2 * torch.clamp_min(pd, R.NONNEG_BOUND)
    want = torch.where((pd >= R.NONNEG_BOUND) | (gg < 0), gg, torch.zeros_like(gg))
    close(R.nonneg_bwd(pd, g, R.NONNEG_BOUND), want)
    inside = pd > R.NONNEG_BOUND
    auto = torch.autograd.grad((torch.clamp_min(p, R.NONNEG_BOUND) ** 2).sum(), p)[0] * g
    close(R.nonneg_bwd(pd, g, R.NONNEG_BOUND)[inside], auto[inside])
    close(R.nonneg_bwd(pd, g, R.NONNEG_BOUND, pa), want + pa)
    # GDN pre-pass: y = x * nrm^-1/2 (GDN) or x * nrm^1/2 (IGDN)
    xx = leaf("dx", (n,), -3, 3)
    nrm = R.log_uniform("t.nrm", n, -6, 3).double().requires_grad_(True)
    for inverse, power in ((0, -0.5), (1, 0.5)):
        y = xx * nrm ** power
        dxx, dn = torch.autograd.grad(y, (xx, nrm), g)
        got_dn, got_t1 = R.gdn_bwd_pre(g, xx.detach(), nrm.detach(), inverse)
        close(got_dn, dn), close(got_t1, dxx)
    # LRP tail: 0.5 * tanh(pre), t = tanh(pre)
    pre = leaf("lp", (n,), -3, 3)
    t = torch.tanh(pre)
    close(R.lrp_bwd(g, t.detach()), torch.autograd.grad(0.5 * t, pre, g)[0])
    # DropPath residual
    sc, br, s = leaf("rs", (3, 20), -1, 1), leaf("rb", (3, 20), -1, 1), R.u("t.rk", (3,), 0, 2).double()
    close(R.residual_scale(sc, br, s), sc + s.view(3, 1) * br)
    close(R.residual_scale(None, br, s), s.view(3, 1) * br)


def test_restatements_agree_with_the_oracle():
    """where oracle/ has the op: NonNegativeParametrizer with LowerBound's gradient rule, GELU, the R-D loss"""
    n = 300
    p = R.nonneg_inputs("t.op", n).double().requires_grad_(True)
    g = R.u("t.og", (n,), -1, 1).double()
    assert R.NONNEG_PED == O.PEDESTAL and R.NONNEG_BOUND == R.f32((1e-6 + O.PEDESTAL) ** 0.5)
    out = O.nonneg_param(p, 1e-6)
    b64 = (1e-6 + O.PEDESTAL) ** 0.5         # the oracle keeps its bound in double; the kernel is handed float32(b64)
    close(R.nonneg_fwd(p.detach(), b64, R.NONNEG_PED), out)
    dp = torch.autograd.grad(out, p, g)[0]
    close(R.nonneg_bwd(p.detach(), g, b64), dp)
    assert ((dp == 0) & (p.detach() < R.NONNEG_BOUND)).sum() > 20 and ((dp != 0) & (p.detach() < R.NONNEG_BOUND)).sum() > 20
    x = R.gelu_inputs("t.ox", n).double()
    close(R.gelu(x), O.gelu(x))
    img, xh = R.u("t.oi", (2, 3, 8, 8), 0, 1).double(), R.u("t.oh", (2, 3, 8, 8), 0, 1).double()
    ly, lz = R.likelihoods("t.oy", 70).double(), R.likelihoods("t.oz", 9).double()
    want = O.rd_loss(img, {"x_hat": xh, "likelihoods": {"y": ly, "z": lz}}, 0.0067)
    got = R.rd_loss_fwd(img.reshape(-1), xh.reshape(-1), ly, lz, 2 * 8 * 8, 0.0067)
    close(got[:3], torch.stack([want["bpp_loss"], want["mse_loss"], want["loss"]]))


def test_ste_round_offset():
    z = R.u("t.z", (2, 3, 50), -9, 9)
    q = R.u("t.q", (3, 1, 3), -2, 2)
    z[0, 0, :4] = q[0, 0, 1] + torch.tensor([0.5, -0.5, 1.5, 2.5])
    got = R.ste_round_offset(z, q)
    med = q[:, 0, 1].view(1, 3, 1)
    assert (got - (torch.round(z - med) + med)).abs().max().item() <= 2 ** -20       # round(z - med) + med to rounding
    assert got.dtype == torch.float32


# ------------------------------------------------------------------------------------------------ layout
def test_layout_restatements():
    x = R.u("t.lx", (2, 3, 6, 10), -1, 1)
    # PatchMerging: x0, x1, x2, x3 = even/even, odd/even, even/odd, odd/odd rows/columns
    k = R.space_to_depth2(x)
    C = 3
    assert torch.equal(k[:, C:2 * C], x[:, :, 1::2, 0::2]) and torch.equal(k[:, 2 * C:3 * C], x[:, :, 0::2, 1::2])
    xx = x.double().requires_grad_(True)
    g = R.u("t.lg", k.shape, -1, 1).double()
    assert torch.equal(R.depth_to_space2(g), torch.autograd.grad(R.space_to_depth2(xx), xx, g)[0])
    # pixel_unshuffle is the inverse of PixelShuffle(2)
    y = R.u("t.ly", (2, 3, 10, 14), -1, 1)
    assert torch.equal(F.pixel_shuffle(R.pixel_unshuffle2(y), 2), y)
    # permute_flip: a Conv2d weight as the ConvTranspose2d weight of the same map (stride 1, pad K-1-p)
    w = R.u("t.w", (5, 3, 3, 3), -1, 1).double()
    wt = R.permute_flip(w.reshape(5, 3, 9)).reshape(3, 5, 3, 3)
    img = R.u("t.img", (1, 3, 6, 7), -1, 1).double()
    close(F.conv_transpose2d(img, wt, padding=1), F.conv2d(img, w, padding=1))
    assert torch.equal(R.permute_flip(R.permute_flip(w.reshape(5, 3, 9))), w.reshape(5, 3, 9))
    # pad2d: positive pads fill, negative crop
    src = R.u("t.ps", R.PAD_SHAPE, -1, 1)
    H, W = R.PAD_SHAPE[2:]
    for top, left, OH, OW in R.PAD_CASES:
        out = R.pad2d(src, top, left, OH, OW, 0.25)
        assert out.shape[-2:] == (OH, OW)
        for yy in range(OH):
            for xc in range(OW):
                sy, sx = yy - top, xc - left
                want = src[0, 1, sy, sx] if 0 <= sy < H and 0 <= sx < W else torch.tensor(0.25)
                assert out[0, 1, yy, xc] == want
    assert any(OH > H for _, _, OH, _ in R.PAD_CASES) and any(OH < H for _, _, OH, _ in R.PAD_CASES)
    # im2col / col2im are adjoint, and im2col followed by a matmul is the convolution
    N, C, H, W = R.COL_SHAPE
    xi = R.u("t.ci", R.COL_SHAPE, -1, 1).double()
    for K, S, pad in R.COL_CASES:
        cols = R.im2col(xi, K, S, pad)
        wgt = R.u("t.cw", (4, C, K, K), -1, 1).double()
        conv = torch.einsum("ok,nkyx->noyx", wgt.reshape(4, -1), cols)
        close(conv, F.conv2d(xi, wgt, stride=S, padding=pad))
        gc = R.u("t.cg", cols.shape, -1, 1).double()
        close((R.col2im(gc, H, W, K, S, pad) * xi).sum(), (gc * cols).sum())
    assert any((H + 2 * p - K) % S != 0 for K, S, p in R.COL_CASES)


@pytest.mark.parametrize("ns,nh,nw", R.ZIGZAG_CASES)
def test_zigzag_agrees_with_oracle(ns, nh, nw):
    x = R.u("t.zz", (2, ns * 2, nh * 3, nw * 5), -1, 1)
    z = R.zigzag_splits(x, ns, nh, nw)
    if nh == nw:
        assert np.array_equal(z.numpy(), Z.zigzag_splits(x.numpy(), ns, nh))
    assert torch.equal(R.zigzag_reverse(z, ns, nh, nw), x)
    assert len(Z.zigzag_order(ns, nh, nw)) == ns * nh * nw <= 64


# ------------------------------------------------------------------------------------------------ input generators
def test_generators_reach_the_tails():
    n = 1025
    p = R.nonneg_inputs("nn.p", n)
    b = np.float32(R.NONNEG_BOUND)
    assert (p == b).any() and (p < b).sum() > 100 and (p > b).sum() > 100
    assert (p == np.nextafter(b, np.float32(0))).any() and (p == np.nextafter(b, np.float32(1))).any()
    x = R.gelu_inputs("ge.x", n)
    a = (x * np.float32(R.INV_SQRT2)).abs()             # what erf_bf sees
    assert (a > R.ERF_SWITCH).sum() > 100 and (a <= R.ERF_SWITCH).sum() > 50
    near = (a - R.ERF_SWITCH).abs() < 1e-6
    assert near.sum() >= 10 and (a[near] > R.ERF_SWITCH).any() and (a[near] <= R.ERF_SWITCH).any()
    assert (x == 0).sum() >= 2 and torch.signbit(x[x == 0]).any() and x.min() == -9 and x.max() == 9
    assert ((x < -5) & (1.0 + torch.erf(x.double() * R.INV_SQRT2) < 1e-6)).any()     # 1 + erf cancels
    s = R.sigmoid_inputs("sg.x", n)
    assert torch.isinf(torch.exp(-s[s < -89])).all() and (s < -89).sum() > 10        # expf overflows
    assert (torch.exp(-s[s > 89]) < 2.0 ** -126).all() and (s > 89).sum() > 10       # and vanishes
    assert s.min() == -100 and s.max() == 100
    l = R.likelihoods("lk", n)
    assert l.min().item() == R.f32(1e-9) and l.max().item() == 1.0
    dec = torch.floor(torch.log10(l.double())).clamp(-9, -1)
    assert all((dec == d).sum() > 50 for d in range(-9, 0))
    nrm = R.log_uniform("nrm", n, -6, 3)
    assert nrm.min() < 1e-5 and nrm.max() > 1e2


# ------------------------------------------------------------------------------------------------ launch geometry
@pytest.mark.parametrize("case", R.CHANNEL_SUM_CASES, ids=lambda c: c["id"])
def test_channel_sum_cases_reach_their_branch(case):
    N, C, HW = case["N"], case["C"], case["HW"]
    bs = C * HW + 2 if case["layout"] == "oddstride" else C * HW
    vec = HW % 4 == 0 and bs % 4 == 0 and case["layout"] != "misaligned"
    g = R.channel_sum_geometry(N, C, HW, R.channel_sum_ws_floats(case), vec)
    assert (g["S"], vec, g["finish"]) == (case["S"], case["vec"], case["finish"])
    if case["id"] == "float4-hw68-n3":
        assert 256 % (HW // 4) != 0 and N > 1
    assert g["k"] < 2200


def test_channel_sum_table_covers_every_branch():
    t = R.CHANNEL_SUM_CASES
    assert {c["finish"] for c in t} == {"none", "serial", "wave"}
    assert {c["layout"] for c in t} == {"plain", "slice", "misaligned", "oddstride"}
    assert any(c["HW"] % 4 and not c["vec"] for c in t) and any(c["ws"] is None for c in t)
    assert any(isinstance(c["ws"], int) and c["S"] < 32 for c in t)


def test_layernorm_cases_reach_their_branch():
    for C in R.LN_CS:
        for N, HW in R.LN_NHW:
            assert R.ln_fwd_geometry(N, C, HW)["tiles_per_wg"] == 1
    assert {N * HW for N, HW in R.LN_NHW} == {1, 63, 64, 65, 130} and (2, 65) in R.LN_NHW and 65 % 64 != 0
    for N, C, HW in R.LN_LONG:
        g = R.ln_fwd_geometry(N, C, HW)
        assert g["tiles"] > 4096 and g["grid"] == 4096 and g["tiles_per_wg"] == 2
    assert {C in R.LN_CACHED for _, C, _ in R.LN_LONG} == {True, False}
    # the small backward shape: which workspace sizes fuse
    N, HW = R.LN_BWD_SHAPE
    for C in R.LN_CS:
        for kind in R.LN_WS_KINDS:
            g = R.ln_bwd_geometry(N, C, HW, True, True, R.ln_ws_floats(kind, C))
            assert g["fused"] == (C in (48, 96, 192) and kind in ("fuse-min", "fuse-1024")), (C, kind)
            if not g["fused"]:
                assert g["S"] == 1
        assert R.ln_ws_floats("below-fuse", C) == 2 * 64 * C - 1
    for case in R.LN_BWD_BRANCH_CASES:
        g = R.ln_bwd_geometry(case["N"], case["C"], case["HW"], True, True, R.ln_ws_floats(case["ws"], case["C"]))
        for key, want in case["expect"].items():
            assert g[key] == want, (case["id"], key, g[key], want)
        # parameters only (dx null): never fused, the same split
        if not g["fused"]:
            g2 = R.ln_bwd_geometry(case["N"], case["C"], case["HW"], False, True, R.ln_ws_floats(case["ws"], case["C"]))
            assert (g2["S"], g2["finish"]) == (g["S"], g["finish"])
    fin = {(c["expect"]["finish"], c["expect"]["fused"]) for c in R.LN_BWD_BRANCH_CASES}
    assert fin == {("wave", True), ("none", False), ("serial", False), ("wave", False)}


def test_grid_stride_and_two_stage_cases():
    assert R.grid_for(R.LONG_N) == R.GRID_CAP and R.LONG_N > R.GRID_CAP * 256 * 4 > R.ELEMENT_NS[-2]
    assert R.grid_for(R.LONG_N1, 1) == R.GRID_CAP and R.LONG_N1 > R.GRID_CAP * 256
    assert R.grid_for(1025) == 2 and R.grid_for(256) == 1
    # rd loss: 8 elements per thread fill the capped grid; only the largest nx takes a trip more
    assert [R.rd_geometry(nx, 1, 1)["trips_x"] for nx in R.RD_NX] == [1, 8, 8, 9] and R.RD_NX[-1] > 2048 * 256 * 8
    assert [R.rd_geometry(nx, 1, 1)["nblk"] for nx in R.RD_NX] == [1, 1, 12, 2048]
    for nx in R.RD_NX:
        assert R.rd_ny(nx)[2] > nx              # lik_y longer than the image: its loop runs past the image's
    # sqnorm: 16 per thread; the misaligned form has no float4 part
    g = [R.sqnorm_geometry(n, True) for n in R.SQNORM_NS]
    assert [x["n4"] for x in g] == [0, 0, 1, 1, 256, 25000, 2098176]
    # 16 floats = 4 float4 loads per thread fill the capped grid; the largest n takes a fifth
    assert [x["trips4"] for x in g][-2:] == [4, 5] and R.grid_for(R.SQNORM_NS[-1], 16) == 2048
    assert R.SQNORM_NS[-1] > 2048 * 256 * 16
    assert all(R.sqnorm_geometry(n, False)["n4"] == 0 for n in R.SQNORM_NS)
    assert R.sqnorm_geometry(R.SQNORM_NS[-1], False)["k"] > R.sqnorm_geometry(R.SQNORM_NS[-1], True)["k"]


def test_limit_rule():
    ref = torch.tensor([1.0, 2.0, 30.0, 0.0], dtype=F64)
    r32 = torch.tensor([1.0 + 1e-7, 2.0, 30.0, 0.0], dtype=F64)
    lim = R.elementwise_limit(r32, ref, torch.zeros(4, dtype=F64))
    assert abs(lim[0].item() - 4e-7) < 1e-9 and lim[0] == lim[1] and lim[2].item() == R.TINY and lim[3].item() == R.TINY
    assert R.sum_limit(10, 1.0) == pytest.approx(10 * 2.0 ** -24, rel=1e-5)
    with pytest.raises(AssertionError):
        R.check_elementwise("x", torch.tensor([1.0, 2.0, 30.1, 0.0]), r32, ref, torch.zeros(4, dtype=F64))
    with pytest.raises(AssertionError):
        R.check_elementwise("x", torch.tensor([1.0, float("nan"), 30.0, 0.0]), r32, ref, torch.zeros(4, dtype=F64))
    with pytest.raises(AssertionError):
        R.check_sum("x", torch.tensor([1.0 + 1e-5]), torch.tensor([1.0], dtype=F64), 10, 1.0)
