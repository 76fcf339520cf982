"""Float64 restatements of what csrc/pointwise.hip computes, the limit rule of tests/test_gpu_pointwise_numerics.py,
its case tables and the launch geometry each case is named for.  CPU only; tests/test_pointwise_ref.py checks this
module against torch float64 autograd and against oracle/, and checks that every case reaches its branch.

Every restatement is written from the operation's definition (the formula in the kernel's header comment or the torch
op), takes the dtype of its inputs, and so serves twice: in float64 as the reference, in float32 as the "float32 CPU
restatement" whose own error scales the elementwise limit.

The limit rule (none of it is taken from a kernel's output)
  layout kernels, ste_round_offset, fill, clamp: bit equality; an accumulating form is one float32 add on top.
  elementwise kernels: per element |gpu - ref64| <= FACTOR * (max over the element's magnitude decade of
      |ref32 - ref64|) + floor.  The floor is one ulp (2^-23) of the largest intermediate of the formula, plus what the
      project documents for its approximations: erf_bf 5.8e-8 absolute (icm_common.h), v_rsq_f32 / v_exp_f32 2 ulp of
      their result, and the smallest normal float32 (denormal results may be flushed).
  sums: |gpu - ref64| <= gamma(k) * sum |terms|, gamma(k) = k u / (1 - k u), u = 2^-24: the worst-case bound of float32
      summation along the longest chain of additions k of the kernel's fixed tree for that launch."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import weights as W
from oracle import zigzag_oracle as Z

FACTOR = 4                      # the entropy suite's factor
U = 2.0 ** -24                  # unit roundoff of float32
ULP = 2.0 ** -23
TINY = 2.0 ** -126              # smallest normal float32
ERF_ABS = 5.8e-8                # erf_bf's documented maximum absolute error
ERF_SWITCH = 0.927734375        # |a| at which erf_bf changes branch; a = x / sqrt(2)
INV_SQRT2 = 0.70710678118654752440
F64 = torch.float64
GRID_CAP = 2048                 # workgroups of 256 threads an elementwise launch gets at the most
LONG_N = GRID_CAP * 256 * 4 + 77        # a second grid-stride trip at 4 elements per thread
LONG_N1 = GRID_CAP * 256 + 77           # ... at 1 per thread (col2im)
ELEMENT_NS = (1, 255, 256, 1025, LONG_N)
LN_EPS = 1e-5


def u(name, shape, lo, hi):
    return W._u("pw." + name, tuple(shape), lo, hi)


def f32(v):
    return float(np.float32(v))


# ================================================================================================ limit rule
def gamma(k):
    return k * U / (1.0 - k * U)


def sum_limit(k, abs_terms):
    """worst-case error of a float32 sum whose longest chain has k additions; abs_terms = sum |terms| (float64)"""
    return gamma(k) * abs_terms + TINY


def bands(ref64):
    """magnitude decade of every element (zeros and denormals share the lowest band)"""
    a = ref64.abs().clamp_min(1e-45)
    return (torch.floor(torch.log10(a)).long() + 50).clamp(0, 99)


def elementwise_limit(ref32, ref64, floor):
    """per element: FACTOR * (the float32 restatement's largest error in the element's decade) + floor"""
    err32 = (ref32.double() - ref64).abs().reshape(-1)
    err32 = torch.where(torch.isfinite(err32), err32, torch.zeros_like(err32))
    b = bands(ref64).reshape(-1)
    worst = torch.zeros(100, dtype=F64).scatter_reduce_(0, b, err32, "amax", include_self=True)
    return (FACTOR * worst[b]).reshape(ref64.shape) + floor + TINY


def check_elementwise(what, got, ref32, ref64, floor):
    """asserts the elementwise rule; returns (measured worst error / limit ratio) after printing figure and limit"""
    got = got.detach().cpu().double().reshape(ref64.shape)
    lim = elementwise_limit(ref32.reshape(ref64.shape), ref64, floor)
    err = (got - ref64).abs()
    bad = ~(err <= lim)                       # NaN counts as bad
    ratio = (err / lim)
    worst = int(torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio).argmax())
    e, l = err.reshape(-1)[worst].item(), lim.reshape(-1)[worst].item()
    own = (ref32.double().reshape(ref64.shape) - ref64).abs().reshape(-1)[worst].item()
    print(f"{what}: worst element gpu {e:.3e}, float32 restatement {own:.3e}, limit {l:.3e} ({e / l:.2f} of it)")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} elements over the limit, worst {e:.3e} > {l:.3e}"
    return e / l


def check_sum(what, got, ref64, k, abs_terms):
    got = got.detach().cpu().double().reshape(ref64.shape)
    lim = torch.as_tensor(sum_limit(k, abs_terms), dtype=F64).expand(ref64.shape)
    err = (got - ref64).abs()
    ratio = err / lim
    worst = int(torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio).argmax())
    e, l = err.reshape(-1)[worst].item(), lim.reshape(-1)[worst].item()
    print(f"{what}: k = {k}, gpu {e:.3e}, limit {l:.3e} ({e / l:.2f} of it)")
    assert bool((err <= lim).all()), f"{what}: {e:.3e} > limit {l:.3e} (k = {k})"
    return e / l


# ================================================================================================ launch geometry
# the host arithmetic, restated from the issue's case list (not imported from the library)
def cdiv(a, b):
    return -(-a // b)


def grid_for(n, per_thread=4):
    return max(1, min(cdiv(n, 256 * per_thread), GRID_CAP))


def finish_of(S):
    return "none" if S <= 1 else ("serial" if S <= 4 else "wave")


def finish_chain(S):
    """additions on the longest chain of the finish kernel: serial = S, wave = rows per lane + the 6-level xor tree"""
    return {"none": 0, "serial": S, "wave": cdiv(S, 64) + 6}[finish_of(S)]


def channel_sum_geometry(N, C, HW, ws_floats, vec):
    """ws_floats None = null workspace.  S = clamp(N*HW/16384, 1, 32), capped by ws_floats/C"""
    S = max(1, min(32, (N * HW) // 16384))
    S = 1 if ws_floats is None else max(1, min(S, ws_floats // C))
    items = cdiv(N * HW // 4 if vec else N * HW, S * 256)       # loads per thread
    k = items + (2 if vec else 0) + 6 + 2 + finish_chain(S) + 1  # + the accumulate / store add
    return {"S": S, "finish": finish_of(S), "k": k}


def ln_stat_chain(C):
    """additions on the longest chain of a per-pixel channel sum: cached = CPT serial + log2(NW) pairwise, generic =
    ceil(C/4) serial + 2 pairwise; + 1 for the division by C"""
    cached = {48: (12, 4), 96: (24, 4), 192: (24, 8), 384: (48, 8)}
    if C in cached:
        cpt, nw = cached[C]
        return cpt + int(math.log2(nw)) + 1
    return cdiv(C, 4) + 2 + 1


def ln_fwd_geometry(N, C, HW):
    tiles = cdiv(N * HW, 64)
    grid = min(tiles, 4096)
    return {"tiles": tiles, "grid": grid, "tiles_per_wg": cdiv(tiles, grid)}


def ln_bwd_geometry(N, C, HW, have_dx, have_params, ws_floats):
    """which kernels icm_layernorm_bwd launches and the chain length k of the parameter sums"""
    cached = C in (48, 96, 192, 384)
    tiles = cdiv(N * HW, 64)
    g = {"fused": False, "S": 0, "finish": "none", "tiles_per_wg": 0, "k": 0, "K": 2}
    if have_dx:
        nblk = min(tiles, 4096)
        if cached and C <= 192 and have_params and ws_floats is not None and ws_floats >= 2 * 64 * C:
            nblk = min(nblk, 1024, ws_floats // (2 * C))
            g.update(fused=True, S=nblk, finish="wave", tiles_per_wg=cdiv(tiles, nblk))
            # per lane one term per tile, the 6-level xor tree, then the wave finish over nblk rows; + 3 roundings
            # inside a term ((x - m) * r * dy)
            g["k"] = cdiv(tiles, nblk) + 6 + cdiv(nblk, 64) + 6 + 3 + 1
            g["grid"] = nblk
            return g
        g.update(grid=nblk, tiles_per_wg=cdiv(tiles, nblk))
    if have_params:
        S = max(1, min(cdiv(N * HW, 4096), cdiv(2048, C)))
        S = 1 if ws_floats is None else max(1, min(S, ws_floats // (2 * C)))
        g.update(S=S, finish=finish_of(S))
        g["k"] = cdiv(N * HW, S * 256) + 6 + 2 + finish_chain(S) + 3 + 1
    return g


def two_stage_chain(n, per_thread):
    """rd_reduce / sqnorm: grid_for(n, per_thread) workgroups, then one workgroup adds the partials in order"""
    nblk = grid_for(n, per_thread)
    return nblk, cdiv(nblk, 256) + 6 + 2


def rd_geometry(nx, ny, nz):
    nblk, fin = two_stage_chain(nx, 8)
    trips = lambda n: cdiv(n, nblk * 256)
    # + 2 roundings inside a term (d = xh - x, d * d; logf to an ulp)
    return {"nblk": nblk, "trips_x": trips(nx), "k": {n: trips(n) + 6 + 2 + fin + 2 for n in (nx, ny, nz)}}


def sqnorm_geometry(n, aligned):
    nblk, fin = two_stage_chain(n, 16)
    n4 = n // 4 if aligned else 0
    trips4, tail = cdiv(n4, nblk * 256), cdiv(n - 4 * n4, nblk * 256)
    # a float4 item is three additions deep before it joins the running sum; + 1 rounding of each square
    k = trips4 + (3 if n4 else 0) + tail + 6 + 2 + fin + 1
    return {"nblk": nblk, "n4": n4, "trips4": trips4, "k": k}


# ================================================================================================ case tables
def _cs(id, N, C, HW, layout, ws, S, vec, finish):
    return dict(id=id, N=N, C=C, HW=HW, layout=layout, ws=ws, S=S, vec=vec, finish=finish)


# ws: "full" = 32 * C floats, an int = that many floats, None = null pointer
CHANNEL_SUM_CASES = [
    _cs("scalar-hw35", 2, 3, 35, "plain", "full", 1, False, "none"),
    _cs("float4-hw36", 2, 5, 36, "plain", "full", 1, True, "none"),
    _cs("float4-hw36-slice", 2, 5, 36, "slice", "full", 1, True, "none"),
    _cs("scalar-misaligned-pointer", 2, 5, 36, "misaligned", "full", 1, False, "none"),
    _cs("scalar-odd-batch-stride", 2, 5, 36, "oddstride", "full", 1, False, "none"),
    _cs("float4-hw68-n3", 3, 2, 68, "plain", "full", 1, True, "none"),
    _cs("S2-serial-finish", 1, 2, 40960, "plain", "full", 2, True, "serial"),
    _cs("S5-wave-finish", 1, 2, 81940, "plain", "full", 5, True, "wave"),
    _cs("S32-wave-finish", 1, 1, 524292, "plain", "full", 32, True, "wave"),
    _cs("S3-capped-by-ws_floats", 1, 1, 524292, "plain", 3, 3, True, "serial"),
    _cs("S1-ws-null", 1, 1, 524292, "plain", None, 1, True, "none"),
]


def channel_sum_ws_floats(case):
    return 32 * case["C"] if case["ws"] == "full" else case["ws"]


LN_CACHED, LN_GENERIC = (48, 96, 192, 384), (1, 3, 40, 50)
LN_CS = LN_CACHED + LN_GENERIC
LN_NHW = ((1, 1), (1, 63), (1, 64), (1, 65), (2, 65))         # (N, HW); the last: a tile spans the batch boundary
LN_LONG = ((1, 5, 262225), (1, 48, 262225))                   # more than 4096 tiles: the persistent loop
LN_BWD_SHAPE = (2, 65)
LN_WS_KINDS = ("null", "below-fuse", "fuse-min", "fuse-1024")


def ln_ws_floats(kind, C):
    return {"null": None, "below-fuse": 2 * 64 * C - 1, "fuse-min": 2 * 64 * C, "fuse-1024": 2 * 1024 * C,
            "6C": 6 * C}[kind]


def _lb(id, N, C, HW, ws, **expect):
    return dict(id=id, N=N, C=C, HW=HW, ws=ws, expect=expect)


# (the geometry with dx and both parameter gradients requested must equal ``expect``)
LN_BWD_BRANCH_CASES = [
    _lb("fused-4-tiles-per-workgroup-C48", 1, 48, 64 * 64 * 3 + 5, "fuse-min", fused=True, S=64, tiles_per_wg=4, finish="wave"),
    _lb("fused-4-tiles-per-workgroup-C96", 1, 96, 64 * 64 * 3 + 5, "fuse-min", fused=True, S=64, tiles_per_wg=4, finish="wave"),
    _lb("fused-4-tiles-per-workgroup-C192", 1, 192, 64 * 64 * 3 + 5, "fuse-min", fused=True, S=64, tiles_per_wg=4, finish="wave"),
    _lb("unfused-persistent-loop-C48-ws-null", 1, 48, 262225, "null", fused=False, S=1, tiles_per_wg=2, finish="none"),
    _lb("unfused-persistent-loop-C5-generic-ws-null", 1, 5, 262225, "null", fused=False, S=1, tiles_per_wg=2, finish="none"),
    _lb("split-S2-serial-K2-C384", 1, 384, 4097, "fuse-1024", fused=False, S=2, finish="serial"),
    _lb("split-S6-wave-K2-C384", 1, 384, 20481, "fuse-1024", fused=False, S=6, finish="wave"),
    _lb("split-S10-wave-C40", 1, 40, 36867, "fuse-1024", fused=False, S=10, finish="wave"),
    _lb("split-S3-capped-by-ws_floats-C40", 1, 40, 36867, "6C", fused=False, S=3, finish="serial"),
]

PERMUTE_FLIP_CASES = ((3, 5, 1), (5, 3, 9), (2, 7, 25))
PAD_CASES = (  # (top, left, OH, OW) on a (2, 3, 5, 7) source
    (2, 3, 9, 12), (-1, -2, 3, 4), (-1, 2, 6, 6), (2, 3, 4, 5), (-1, -2, 7, 9))
PAD_SHAPE = (2, 3, 5, 7)
COL_CASES = ((5, 2, 2), (3, 1, 1), (3, 2, 0))                 # (K, stride, pad)
COL_SHAPE = (2, 3, 10, 9)                                     # H = 10: (H + 2p - K) % S != 0 for both stride-2 cases
ZIGZAG_CASES = ((1, 1, 1), (2, 2, 2), (4, 2, 2), (3, 1, 2))
RD_NX = (1, 2047, 24576, 4194304 + 12345)
RD_NZ = (1, 384)
SQNORM_NS = (1, 3, 4, 5, 1027, 100003, 8388608 + 4099)
ADAM_NS = (1, 1025, 100003)


def rd_ny(nx):
    return (1, 10240, nx + 7)


# ================================================================================================ input generators
def gelu_inputs(name, n):
    """[-9, 9] with +-0, the erf_bf switch point x = +-0.927734375 * sqrt(2) and the float32 values around it"""
    x = u(name, (n,), -9.0, 9.0)
    c = np.float32(ERF_SWITCH * math.sqrt(2.0))
    sp = [0.0, -0.0]
    for s in (c, -c):
        lo, hi = np.nextafter(s, np.float32(-10)), np.nextafter(s, np.float32(10))
        sp += [s, lo, hi, np.nextafter(lo, np.float32(-10)), np.nextafter(hi, np.float32(10))]
    sp += [-9.0, 9.0, -5.5, -7.25]                         # the negative tail, where 1 + erf cancels
    sp = torch.tensor(np.array(sp, dtype=np.float32))
    m = min(n, sp.numel())
    x[:m] = sp[:m]
    return x


def sigmoid_inputs(name, n):
    """[-100, 100]: expf(-x) overflows below about -88.7 and vanishes above 88.7"""
    x = u(name, (n,), -100.0, 100.0)
    sp = torch.tensor([-100.0, 100.0, -89.0, 89.0, -88.0, 88.0, 0.0, -0.0, -20.0, 20.0])
    m = min(n, sp.numel())
    x[:m] = sp[:m]
    return x


NONNEG_BOUND = f32(math.sqrt(1e-6 + 2.0 ** -36))       # NonNegativeParametrizer(minimum 1e-6): bound, pedestal 2^-36
NONNEG_PED = f32(2.0 ** -36)


def nonneg_inputs(name, n):
    """values on both sides of the bound and exactly at it"""
    p = u(name, (n,), -2.0 * NONNEG_BOUND, 4.0 * NONNEG_BOUND)
    b = np.float32(NONNEG_BOUND)
    sp = torch.tensor(np.array([b, np.nextafter(b, np.float32(0)), np.nextafter(b, np.float32(1)), 0.0, -b, 1.5],
                               dtype=np.float32))
    m = min(n, sp.numel())
    p[:m] = sp[:m]
    return p


def likelihoods(name, n):
    """log-uniform over [1e-9, 1], with both ends present"""
    l = torch.from_numpy(np.float32(10.0) ** u(name, (n,), -9.0, 0.0).numpy()).clamp(1e-9, 1.0)
    sp = torch.tensor([1.0, 1e-9, 0.5])
    m = min(n, 3)
    l[:m] = sp[:m]
    return l


def log_uniform(name, n, lo_exp, hi_exp):
    return torch.from_numpy(np.float32(10.0) ** u(name, (n,), lo_exp, hi_exp).numpy())


# ================================================================================================ LayerNorm
def layernorm_fwd(x, gamma_, beta, eps=LN_EPS):
    """x [N, C, HW] normalised over C.  Returns y [N, C, HW], mean [N, HW], rstd [N, HW]"""
    mean = x.mean(1)
    d = x - mean[:, None]
    rstd = 1.0 / torch.sqrt((d * d).mean(1) + eps)
    return d * rstd[:, None] * gamma_[None, :, None] + beta[None, :, None], mean, rstd


def layernorm_bwd(x, dy, gamma_, mean, rstd, dx_extra=None, dx_prev=None, dgamma_prev=None, dbeta_prev=None):
    """dx = rstd * (g*gamma - mean_c(g*gamma) - xhat * mean_c(g*gamma*xhat)) [+ dx_extra] [+ dx_prev];
    dgamma = sum_{n,p} dy * xhat [+ prev]; dbeta = sum dy [+ prev]"""
    xh = (x - mean[:, None]) * rstd[:, None]
    gg = dy * gamma_[None, :, None]
    dx = rstd[:, None] * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))
    if dx_extra is not None:
        dx = dx + dx_extra
    if dx_prev is not None:
        dx = dx + dx_prev
    dgamma, dbeta = (dy * xh).sum((0, 2)), dy.sum((0, 2))
    if dgamma_prev is not None:
        dgamma, dbeta = dgamma + dgamma_prev, dbeta + dbeta_prev
    return dx, dgamma, dbeta


def layernorm_fwd_limits(x64, gamma64, beta64, y64, mean64, rstd64, eps=LN_EPS):
    """(limit of mean, limit of rstd, floor of y): the statistics are sums over C with chain k = ln_stat_chain(C)"""
    C = x64.shape[1]
    k = ln_stat_chain(C)
    lim_mean = sum_limit(k, x64.abs().sum(1) / C)
    d = x64 - mean64[:, None]
    var = (d * d).mean(1)
    # var' = sum (d - dm)^2 / C = var + dm^2, each term 3 roundings more; rsqrt halves the relative error; v_rsq_f32 is
    # given 2 ulp and the rounding of its argument (the quotient by C, the sum with eps) one more
    rel_var = gamma(k + 3) * (d * d).sum(1) / C / (var + eps) + lim_mean ** 2 / (var + eps) \
        + 2 * gamma(2) * d.abs().sum(1) / C * lim_mean / (var + eps)
    lim_rstd = rstd64 * (0.5 * rel_var + 3 * ULP) + TINY
    g = gamma64[None, :, None].abs()
    floor_y = g * rstd64[:, None] * lim_mean[:, None] + g * d.abs() * lim_rstd[:, None] \
        + ULP * (g * d.abs() * rstd64[:, None] + beta64[None, :, None].abs())
    return lim_mean, lim_rstd, floor_y


def layernorm_bwd_floor(x64, dy64, gamma64, mean64, rstd64, extra64=None, prev64=None):
    """floor of dx: the two per-pixel channel means are sums with chain ln_stat_chain(C) (+ 3 roundings in a term)"""
    C = x64.shape[1]
    k = ln_stat_chain(C) + 3
    xh = (x64 - mean64[:, None]) * rstd64[:, None]
    gg = dy64 * gamma64[None, :, None]
    e1 = gamma(k) * gg.abs().sum(1, keepdim=True) / C
    e2 = gamma(k) * (gg * xh).abs().sum(1, keepdim=True) / C
    s1, s2 = gg.mean(1, keepdim=True).abs(), (gg * xh).mean(1, keepdim=True).abs()
    r = rstd64[:, None]
    scale = r * (gg.abs() + s1 + xh.abs() * s2)
    floor = r * (e1 + xh.abs() * e2) + 4 * ULP * scale
    for t in (extra64, prev64):
        if t is not None:
            floor = floor + ULP * (t.abs() + scale)
    return floor


@functools.lru_cache(maxsize=4)
def layernorm_case(N, C, HW):
    """inputs and float64 / float32 references of one LayerNorm shape, computed once"""
    x = u(f"ln.x.{C}", (N, C, HW), -2.0, 3.0) * u(f"ln.xs.{C}", (N, 1, HW), 0.2, 2.0)
    gam, bet = u(f"ln.g.{C}", (C,), 0.5, 1.5), u(f"ln.b.{C}", (C,), -0.5, 0.5)
    dy = u(f"ln.dy.{C}", (N, C, HW), -1.0, 1.0)
    gprev, bprev = u(f"ln.gp.{C}", (C,), -3.0, 3.0), u(f"ln.bp.{C}", (C,), -3.0, 3.0)
    y64, m64, r64 = layernorm_fwd(x.double(), gam.double(), bet.double())
    y32, m32, r32 = layernorm_fwd(x, gam, bet)
    return dict(x=x, gamma=gam, beta=bet, dy=dy, gprev=gprev, bprev=bprev, y64=y64, mean64=m64,
                rstd64=r64, y32=y32, mean32=m64.float(), rstd32=r64.float())


@functools.lru_cache(maxsize=2)
def layernorm_extras(N, C, HW):
    """(dx_extra, the previous content of dx) of the accumulating backward cases"""
    return u(f"ln.ex.{C}", (N, C, HW), -1.0, 1.0), u(f"ln.pv.{C}", (N, C, HW), -2.0, 2.0)


# ================================================================================================ reductions, optimiser
def channel_sum(x):
    """x [N, C, HW] -> [C]"""
    return x.sum((0, 2))


def rd_loss_fwd(x, xh, ly, lz, npix, lmbda):
    """(bpp, mse, loss, sum log lik_y, sum log lik_z): loss = lmbda * 255^2 * mse + bpp"""
    sy, sz = torch.log(ly).sum(), torch.log(lz).sum()
    mse = ((xh - x) ** 2).mean()
    bpp = sy / (-math.log(2.0) * npix) + sz / (-math.log(2.0) * npix)
    return torch.stack([bpp, mse, lmbda * 255.0 ** 2 * mse + bpp, sy, sz])


def rd_loss_bwd(x, xh, ly, lz, npix, lmbda, gscale):
    """gscale * d loss / d (x_hat, lik_y, lik_z)"""
    cl = gscale / (-math.log(2.0) * npix)
    return gscale * lmbda * 255.0 ** 2 * 2.0 / x.numel() * (xh - x), cl / ly, cl / lz


def sqnorm(g):
    return (g * g).sum()


def clip_coef(sq, max_norm, gscale):
    """min(1, max_norm / (||g|| * gscale + 1e-6)) * gscale; sq None = no clipping"""
    if sq is None:
        return gscale
    return min(1.0, max_norm / (math.sqrt(sq) * gscale + 1e-6)) * gscale


def adam_steps(p, g, m, v, steps, lr, b1, b2, eps, coef):
    """torch.optim.Adam (no weight decay, no amsgrad) on the gradient g * coef, the same g every step, in p's dtype.
    Returns p, m, v and, for the floor, sum |update|, sum step_size / denom and the smallest v met."""
    p, m, v = p.clone(), m.clone(), v.clone()
    moved, sens, vmin = torch.zeros_like(p), torch.zeros_like(p), torch.full_like(p, math.inf)
    for t in range(1, steps + 1):
        gv = g * coef
        m = b1 * m + (1.0 - b1) * gv
        v = b2 * v + (1.0 - b2) * gv * gv
        step_size = lr / (1.0 - b1 ** t)
        denom = torch.sqrt(v) / math.sqrt(1.0 - b2 ** t) + eps
        upd = step_size * (m / denom)
        moved, sens, vmin = moved + upd.abs(), sens + step_size / denom, torch.minimum(vmin, v)
        p = p - upd
    return p, m, v, moved, sens, vmin


def adam_floors(p0, g, m0, v, coef, steps, moved, sens, vmin):
    """(floor of p, of m, of v) after ``steps`` steps, all float64; v = the reference's final v.  The kernel forms the
    clip coefficient in float32 (sqrt, two products, a sum, a quotient: 6 roundings), so g * coef carries 7 u.  m adds 3
    roundings a step and is bounded by max(|m0|, |g coef|).  v is a sum of positive terms, so its relative error is that
    of its worst term: the squared gradient's 14 u and 4 roundings a step.  An update step_size * m / (sqrt(v) / c + eps)
    inherits m's absolute error through step_size / denom, half of v's relative error, and 6 roundings of its own."""
    gv = (g * coef).abs()
    f_m = steps * 10 * U * torch.maximum(m0.abs(), gv)
    f_v = steps * 18 * U * v
    rel_v = f_v / vmin.clamp_min(TINY)
    f_p = sens * f_m + moved * (0.5 * rel_v + 6 * U) + steps * ULP * (p0.abs() + moved)
    return f_p, f_m, f_v


def adam_hyper(lr, b1, b2, step):
    """the two step-dependent scalars as the host forms them: in double, then rounded to float32"""
    return np.array([lr / (1.0 - b1 ** step), math.sqrt(1.0 - b2 ** step)], dtype=np.float64).astype(np.float32)


# ================================================================================================ pointwise
def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * INV_SQRT2))


def dgelu(x):
    return 0.5 * (1.0 + torch.erf(x * INV_SQRT2)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def sigmoid(x):
    return 1.0 / (1.0 + torch.exp(-x))


def gelu_floor(x64):
    """erf_bf's absolute error through 0.5 * x * (1 + erf)"""
    return 0.5 * x64.abs() * ERF_ABS


def dgelu_floor(x64):
    """erf_bf through the cdf; v_exp_f32 (2 ulp) and the rounding of its argument x^2/2 through x * pdf"""
    pdf = torch.exp(-0.5 * x64 * x64) / math.sqrt(2.0 * math.pi)
    return 0.5 * ERF_ABS + x64.abs() * pdf * ULP * (3.0 + 0.5 * x64 * x64) + ULP * dgelu(x64).abs()


def nonneg_fwd(p, bound, ped):
    v = torch.clamp_min(p, bound)
    return v * v - ped


def nonneg_bwd(p, g, bound, prev=None):
    """g * 2 * max(p, bound) where p >= bound, or where the gradient pushes p up (gg < 0); else 0"""
    gg = g * 2.0 * torch.clamp_min(p, bound)
    r = torch.where((p >= bound) | (gg < 0), gg, torch.zeros_like(gg))
    return r if prev is None else r + prev


def gdn_bwd_pre(g, x, nrm, inverse):
    """(dn, t1).  GDN y = x * nrm^-1/2: t1 = g * nrm^-1/2, dn = -g x nrm^-3/2 / 2; IGDN y = x * nrm^1/2: t1 = g * nrm^1/2,
    dn = g x nrm^-1/2 / 2"""
    if inverse:
        s = torch.sqrt(nrm)
        return 0.5 * g * x / s, g * s
    return -0.5 * g * x * nrm ** -1.5, g / torch.sqrt(nrm)


def gate_fwd(a, b, x):
    return gelu(a) * sigmoid(b) + x


def gate_bwd(g, a, b, da_prev=None, dx_prev=None):
    s = sigmoid(b)
    da, db, dx = g * s * dgelu(a), g * gelu(a) * s * (1.0 - s), g
    return (da if da_prev is None else da + da_prev), db, (dx if dx_prev is None else dx + dx_prev)


def gate_bwd_floors(g64, a64, b64, da_prev64=None):
    s = sigmoid(b64)
    ga = g64.abs()
    f_da = ga * s * (dgelu_floor(a64) + 3 * ULP * dgelu(a64).abs())
    if da_prev64 is not None:
        f_da = f_da + ULP * (da_prev64.abs() + (g64 * s * dgelu(a64)).abs())
    # s carries 3 ulp (v_exp_f32 2, the division 1); 1 - s turns that into an absolute error of 3 ulp * s
    f_db = ga * (gelu_floor(a64) * s * (1 - s) + gelu(a64).abs() * 3 * ULP * s * (1 + (1 - 2 * s).abs())
                 + 2 * ULP * gelu(a64).abs() * s * (1 - s))
    return f_da, f_db


def add_grad(src, pre=None, prev=None):
    v = src if pre is None else src * dgelu(pre)
    return v if prev is None else v + prev


def lrp_bwd(g, t):
    return g * 0.5 * (1.0 - t * t)


def residual_scale(shortcut, branch, scale):
    """[N, per]: shortcut + scale[n] * branch"""
    v = scale[:, None] * branch
    return v if shortcut is None else shortcut + v


def ste_round_offset(z, quantiles):
    """float32 numpy: ((rint(t) - t) + t) + med with t = z - med; z [N, C, HW], quantiles [C, 1, 3]"""
    z = z.numpy().astype(np.float32)
    med = quantiles.numpy().astype(np.float32)[:, 0, 1][None, :, None]
    t = z - med
    return torch.from_numpy(((np.rint(t) - t) + t) + med)


# ================================================================================================ layout
def pixel_unshuffle2(x):
    return F.pixel_unshuffle(x, 2)


def pad2d(x, top, left, OH, OW, value):
    """F.pad with (left, right, top, bottom); negative pads crop"""
    H, W = x.shape[-2:]
    return F.pad(x, (left, OW - W - left, top, OH - H - top), value=value)


def im2col(x, K, S, pad):
    """[N, C, H, W] -> [N, C*K*K, OH, OW]"""
    N, C, H, W = x.shape
    OH, OW = (H + 2 * pad - K) // S + 1, (W + 2 * pad - K) // S + 1
    return F.unfold(x, K, padding=pad, stride=S).reshape(N, C * K * K, OH, OW)


def col2im(cols, H, W, K, S, pad, bias=None, prev=None):
    N = cols.shape[0]
    out = F.fold(cols.reshape(N, cols.shape[1], -1), (H, W), K, padding=pad, stride=S)
    if bias is not None:
        out = out + bias[None, :, None, None]
    return out if prev is None else out + prev


def space_to_depth2(x):
    """PatchMerging's gather: cat of the four strided views, channel blocks in the order (0,0), (1,0), (0,1), (1,1)"""
    return torch.cat([x[:, :, 0::2, 0::2], x[:, :, 1::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 1::2]], 1)


def depth_to_space2(g):
    """the gradient of space_to_depth2: every block back to its strided positions"""
    N, C4, H2, W2 = g.shape
    C = C4 // 4
    out = torch.zeros(N, C, 2 * H2, 2 * W2, dtype=g.dtype)
    for k, (dy, dx) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        out[:, :, dy::2, dx::2] = g[:, k * C:(k + 1) * C]
    return out


def permute_flip(w):
    """[A, B, K] -> [B, A, K] with the taps reversed"""
    return w.flip(2).transpose(0, 1).contiguous()


def zigzag_splits(x, ns, nh, nw):
    """[B, C, H, W] -> [B, ns*nh*nw, C/ns, H/nh, W/nw] in the zigzag oracle's block order"""
    B, C, H, W = x.shape
    v = x.reshape(B, ns, C // ns, nh, H // nh, nw, W // nw)
    return torch.stack([v[:, c, :, h, :, w, :] for (c, h, w) in Z.zigzag_order(ns, nh, nw)], 1).contiguous()


def zigzag_reverse(z, ns, nh, nw):
    return torch.from_numpy(Z.zigzag_reverse(z.numpy(), ns, nh, nw))
