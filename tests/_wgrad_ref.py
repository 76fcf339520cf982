"""Reference, inputs, limit rule, case tables and host-path predicates of the weight-gradient numerics tests
(tests/test_wgrad_ref.py on the CPU, tests/test_gpu_wgrad_numerics.py on the GPU).

Reference: wgrad64 is the header formula of include/icm_hip.h (icm_wgrad_args) in float64 torch, an explicit gather
with zero fill per tap:
    dW[a][b][t] = sum_{n,p} actS(gs[n,a,p]) * actB(gb[n,b,p*stride - pad + t]),   dbias[a] = sum_{n,p} actS(gs[n,a,p])

Two input sets
  grid: every operand element and every accumulation prefill is an integer in [-2, 2]; activations NONE / SQUARE.  Every
        product and every partial sum in any order is an integer below 2^24 (asserted per case by grid_headroom), so the
        kernels must return wgrad64(...).float() bit for bit whatever their tiling, split count or reduction order.
  real: uniform [-1, 1).  Limit per output tensor (none of it is taken from a kernel's output)
            |gpu - ref64|_max <= FACTOR * |ref32 - ref64|_max + FACTOR * 2^-24 * |ref64|_max  (+ the erf_bf floor with GELU)
        ref32 = the same formula in float32, summed in the order the planner reports for the launch: the pixel list cut
        into ntiles consecutive chunks, chunk q dealt to split q mod nsplit, one serial chain per split, the slabs added
        in split order.  Winograd launches: nsplit from the workspace size, chunks of 8 tiles (32 pixels).
        GELU floor: sum over terms of |other operand| * 0.5 * |x| * 5.8e-8 (erf_bf's documented absolute error).

Host paths: the predicates below restate, as formulas over the arguments and the plan, the branches that
wgrad_direct_grouped and fill_reduce (csrc/conv_wgrad.hip) take; the plan itself is asked of the library
(icm_debug_wgrad_plan: host code)."""
import ctypes
import functools
from collections import namedtuple

import numpy as np
import torch

from oracle import weights as W

FACTOR = 4                      # the project's headroom factor (winattn, entropy, pointwise)
U = 2.0 ** -24
ERF_ABS = 5.8e-8                # erf_bf's documented maximum absolute error (icm_common.h)
F64 = torch.float64
NONE, GELU, SQUARE = 0, 1, 2
ACT_NAMES = {NONE: "none", GELU: "gelu", SQUARE: "square"}
OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 3
DIRECT, WINOGRAD = 0, 1
NVARIANTS = 15
# family of every row of kWgVariants (csrc/conv_wgrad.hip) and its (a, b) block in channels
FAMILY = ["general"] * 3 + ["t33"] * 4 + ["t33_tapw", "tap9", "tap9", "tap25"] + ["dma1"] * 4
BLOCK = [(64, 32), (64, 64), (128, 128), (96, 96), (192, 192), (96, 192), (192, 96), (96, 96), (96, 96), (64, 64),
         (96, 32), (192, 192), (96, 192), (192, 96), (96, 96)]
DMA_FAMILIES = ("tap9", "tap25", "dma1")

Geom = namedtuple("Geom", "N Ca Cb OH OW H W KH KW stride pad")


def geom(N, OH, OW, k, stride, pad, ch=(40, 24), HW=None):
    """small grid OH x OW (gs), kernel k (int or (KH, KW)); the big grid (gb) is the smallest that gives OH x OW unless
    HW names it (stride 2: a last row / column that only some taps reach)"""
    KH, KW = (k, k) if isinstance(k, int) else k
    H, Wd = HW if HW else ((OH - 1) * stride + KH - 2 * pad, (OW - 1) * stride + KW - 2 * pad)
    assert H >= 1 and Wd >= 1 and (H + 2 * pad - KH) // stride + 1 == OH and (Wd + 2 * pad - KW) // stride + 1 == OW
    return Geom(N, ch[0], ch[1], OH, OW, H, Wd, KH, KW, stride, pad)


def gname(g):
    return "N%d-%dx%d-k%dx%ds%dp%d-c%dx%d-big%dx%d" % (g.N, g.OH, g.OW, g.KH, g.KW, g.stride, g.pad, g.Ca, g.Cb, g.H, g.W)


# ================================================================================================ inputs
def _key(g, name, member):
    return "wg.%s.%s.m%d" % (gname(g), name, member)


@functools.lru_cache(maxsize=None)
def make_input(g, which, name, member=0):
    """operand gs / gb, or prefill dw / dbias, of input set `which` for member `member` of a group (cached: read-only)"""
    shape = {"gs": (g.N, g.Ca, g.OH, g.OW), "gb": (g.N, g.Cb, g.H, g.W), "dw": (g.Ca, g.Cb, g.KH * g.KW),
             "dbias": (g.Ca,)}[name]
    n = int(np.prod(shape))
    if which == "grid":
        v = np.floor(5.0 * W.uniform01(_key(g, name, member), n)) - 2.0
        assert v.min() >= -2 and v.max() <= 2
        return torch.from_numpy(v.astype(np.float32)).reshape(shape)
    assert which == "real"
    return W._u(_key(g, name, member), shape, -1.0, 1.0)


# ================================================================================================ reference
def act64(x, act):
    if act == GELU:
        return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752440))
    if act == SQUARE:
        return x * x
    assert act == NONE
    return x


def gather_taps(b, g):
    """[N, Cb, H, W] -> [taps, Cb, N*OH*OW]: element (t, b, (n, p)) = b[n, b, p*stride - pad + t], 0 outside the image"""
    N, Cb = b.shape[:2]
    ph, pw = (g.OH - 1) * g.stride + g.KH, (g.OW - 1) * g.stride + g.KW      # extent the taps reach, from -pad
    padded = torch.zeros((N, Cb, max(ph, g.H + g.pad), max(pw, g.W + g.pad)), dtype=b.dtype)
    padded[:, :, g.pad:g.pad + g.H, g.pad:g.pad + g.W] = b
    out = torch.empty((g.KH * g.KW, Cb, N * g.OH * g.OW), dtype=b.dtype)
    for kh in range(g.KH):
        for kw in range(g.KW):
            patch = padded[:, :, kh:kh + (g.OH - 1) * g.stride + 1:g.stride, kw:kw + (g.OW - 1) * g.stride + 1:g.stride]
            out[kh * g.KW + kw] = patch.permute(1, 0, 2, 3).reshape(Cb, -1)
    return out


def wgrad64(gs, gb, g, act_s=NONE, act_b=NONE):
    """(dW [Ca, Cb, taps], dbias [Ca]) in float64"""
    S = act64(gs.double(), act_s).permute(1, 0, 2, 3).reshape(g.Ca, -1)
    B = gather_taps(act64(gb.double(), act_b), g)
    dw = torch.einsum("ap,tbp->abt", S, B)
    return dw.contiguous(), S.sum(1)


def abs_terms(gs, gb, g, act_s=NONE, act_b=NONE):
    """(sum |terms| of every dW element, of every dbias element), float64"""
    S = act64(gs.double(), act_s).abs().permute(1, 0, 2, 3).reshape(g.Ca, -1)
    B = gather_taps(act64(gb.double(), act_b).abs(), g)
    return torch.einsum("ap,tbp->abt", S, B), S.sum(1)


def gelu_floor(gs, gb, g, act_s, act_b):
    """erf_bf's absolute error carried through the sum, per dW element and per dbias element (0 without GELU)"""
    s64, b64 = gs.double(), gb.double()
    As, Ab = act64(s64, act_s).abs(), act64(b64, act_b).abs()
    Es = 0.5 * s64.abs() * ERF_ABS if act_s == GELU else torch.zeros_like(s64)
    Eb = 0.5 * b64.abs() * ERF_ABS if act_b == GELU else torch.zeros_like(b64)
    flat = lambda t: t.permute(1, 0, 2, 3).reshape(t.shape[1], -1)
    fw = torch.einsum("ap,tbp->abt", flat(Es), gather_taps(Ab + Eb, g)) + torch.einsum("ap,tbp->abt", flat(As), gather_taps(Eb, g))
    return fw, flat(Es).sum(1)


def split_order(npix, ntiles, nsplit):
    """the pixel list cut into ntiles consecutive chunks, chunk q dealt to split q mod nsplit: an index array
    [steps, nsplit] of the pixel every split adds at every step of its serial chain (npix = the padding: a zero pixel)"""
    ntiles = max(1, min(ntiles, npix))
    nsplit = max(1, min(nsplit, ntiles))
    chunks = np.array_split(np.arange(npix, dtype=np.int64), ntiles)
    lists = [np.concatenate(chunks[s::nsplit]) for s in range(nsplit)]
    steps = max(len(l) for l in lists)
    idx = np.full((steps, nsplit), npix, dtype=np.int64)
    for s, l in enumerate(lists):
        idx[:len(l), s] = l
    return idx


def wgrad32_ordered(gs, gb, g, act_s, act_b, ntiles, nsplit):
    """the formula in float32 in the summation order of split_order: every product rounded, every addition rounded, the
    nsplit slabs added in order.  Activations are the float64 ones rounded once to float32."""
    S = act64(gs.double(), act_s).float().permute(1, 0, 2, 3).reshape(g.Ca, -1)
    B = gather_taps(act64(gb.double(), act_b).float(), g)
    npix = S.shape[1]
    S = torch.cat([S, torch.zeros(g.Ca, 1)], 1).t().contiguous()                       # [npix + 1, Ca]
    B = torch.cat([B, torch.zeros(B.shape[0], g.Cb, 1)], 2).permute(2, 0, 1).contiguous()   # [npix + 1, taps, Cb]
    idx = torch.from_numpy(split_order(npix, ntiles, nsplit))
    ns = idx.shape[1]
    acc = torch.zeros((ns, g.Ca, B.shape[1], g.Cb), dtype=torch.float32)
    bacc = torch.zeros((ns, g.Ca), dtype=torch.float32)
    for j in range(idx.shape[0]):
        s, b = S[idx[j]], B[idx[j]]
        acc += s[:, :, None, None] * b[:, None, :, :]
        bacc += s
    dw, db = acc[0].clone(), bacc[0].clone()
    for k in range(1, ns):
        dw += acc[k]
        db += bacc[k]
    return dw.permute(0, 2, 1).contiguous(), db


Ref = namedtuple("Ref", "dw db floor_w floor_b")


@functools.lru_cache(maxsize=None)
def reference(g, which, act_s=NONE, act_b=NONE, member=0):
    """cached per (geometry, input set, activations, member): float64 results and the GELU floors"""
    gs, gb = make_input(g, which, "gs", member), make_input(g, which, "gb", member)
    dw, db = wgrad64(gs, gb, g, act_s, act_b)
    if GELU in (act_s, act_b):
        fw, fb = gelu_floor(gs, gb, g, act_s, act_b)
    else:
        fw, fb = torch.zeros_like(dw), torch.zeros_like(db)
    return Ref(dw, db, fw, fb)


@functools.lru_cache(maxsize=None)
def reference32(g, act_s, act_b, ntiles, nsplit, member=0):
    """cached float32 restatement on the `real` inputs in the launch's summation order"""
    gs, gb = make_input(g, "real", "gs", member), make_input(g, "real", "gb", member)
    return wgrad32_ordered(gs, gb, g, act_s, act_b, ntiles, nsplit)


def limit(ref32, ref64, floor=None):
    """FACTOR * |ref32 - ref64|_max + FACTOR * 2^-24 * |ref64|_max (+ max of the GELU floor); also returns ref32's error"""
    e32 = (ref32.double() - ref64).abs().max().item()
    lim = FACTOR * e32 + FACTOR * U * ref64.abs().max().item()
    if floor is not None:
        lim += floor.max().item()
    return lim, e32


def wino_transformed_terms(gs, gb, g):
    """max over (xi, a, b) of sum_tiles |A dY A^T|[xi] * |B^T d B|[xi]: the magnitudes the F(2x2, 3x3) kernel sums"""
    A = torch.tensor([[1, 0], [1, 1], [1, -1], [0, -1]], dtype=F64)
    Bt = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=F64)
    N, TH, TW = g.N, (g.H + 1) // 2, (g.W + 1) // 2
    y = torch.zeros((N, g.Ca, 2 * TH, 2 * TW), dtype=F64)
    y[:, :, :g.H, :g.W] = gs.double()
    x = torch.zeros((N, g.Cb, 2 * TH + 2, 2 * TW + 2), dtype=F64)
    x[:, :, 1:1 + g.H, 1:1 + g.W] = gb.double()
    yt = y.unfold(2, 2, 2).unfold(3, 2, 2)                     # [N, Ca, TH, TW, 2, 2]
    xt = x.unfold(2, 4, 2).unfold(3, 4, 2)                     # [N, Cb, TH, TW, 4, 4]
    dM = torch.einsum("ir,nchwrs,js->cijnhw", A, yt, A).abs().reshape(g.Ca, 16, -1)
    V = torch.einsum("ir,nchwrs,js->cijnhw", Bt, xt, Bt).abs().reshape(g.Cb, 16, -1)
    return torch.einsum("axp,bxp->abx", dM, V).max().item()


def grid_headroom(g, act_s, act_b, accum, algo=DIRECT, member=0):
    """largest magnitude any partial sum of a `grid` launch can reach; bit equality needs it below 2^24"""
    tw, tb = abs_terms(make_input(g, "grid", "gs", member), make_input(g, "grid", "gb", member), g, act_s, act_b)
    m = max(tw.max().item(), tb.max().item()) + (2 if accum else 0)
    if algo == WINOGRAD:
        m = max(m, 16 * wino_transformed_terms(make_input(g, "grid", "gs", member), make_input(g, "grid", "gb", member), g)
                + (2 if accum else 0))
    return m


# ================================================================================================ the planner (host code)
def _lib():
    from icm_amd import _lib as L
    return L


def wargs(g, act_s=NONE, act_b=NONE, algo=DIRECT):
    a = _lib().WgradArgs()
    a.gs, a.gb = 16, 16            # never dereferenced by the planner
    a.Ca, a.OH, a.OW, a.Cb, a.H, a.W, a.N = g.Ca, g.OH, g.OW, g.Cb, g.H, g.W, g.N
    a.KH, a.KW, a.stride, a.pad, a.act_s, a.act_b, a.algo = g.KH, g.KW, g.stride, g.pad, act_s, act_b, algo
    a.gs_bs, a.gb_bs = g.Ca * g.OH * g.OW, g.Cb * g.H * g.W
    return a


Plan = namedtuple("Plan", "rc variant npx TW TH TI tpg nsplit lds ntiles tiles_x family")


@functools.lru_cache(maxsize=None)
def plan(g, act_s=NONE, act_b=NONE, n=1, variant=-1):
    """icm_debug_wgrad_plan with `variant` forced (restored afterwards), plus what follows from it"""
    L = _lib().lib()
    out = (ctypes.c_int32 * 8)()
    a = wargs(g, act_s, act_b)
    try:
        L.icm_debug_force_wgrad_cfg(variant, -1)
        rc = L.icm_debug_wgrad_plan(ctypes.byref(a), n, out)
    finally:
        L.icm_debug_force_wgrad_cfg(-1, -1)
    if rc:
        return Plan(rc, *([0] * 10), None)
    v, lgNPX, lgTW, lgTH, lgTI, tpg, nsplit, lds = list(out)
    TW, TH, TI = 1 << lgTW, 1 << lgTH, 1 << lgTI
    tx, ty, tn = -(-g.OW // TW), -(-g.OH // TH), -(-g.N // TI)
    return Plan(0, v, 1 << lgNPX, TW, TH, TI, tpg, nsplit, lds, tx * ty * tn, tx, FAMILY[v])


def trips(p):
    """(fewest, most) staging-loop trips of a workgroup: niter = ceil((ntiles - split) / nsplit)"""
    return (p.ntiles - (p.nsplit - 1) + p.nsplit - 1) // p.nsplit, -(-p.ntiles // p.nsplit)


def workspace_floats(g, act_s=NONE, act_b=NONE, n=1, variant=-1, algo=DIRECT):
    L = _lib().lib()
    a = wargs(g, act_s, act_b, algo)
    try:
        L.icm_debug_force_wgrad_cfg(variant, -1)
        return int(L.icm_wgrad_workspace_floats_grouped(ctypes.byref(a), n))
    finally:
        L.icm_debug_force_wgrad_cfg(-1, -1)


def wino_splits(g, n=1):
    """(nsplit, chunks of 8 tiles) of a Winograd launch, from the workspace query"""
    ws = workspace_floats(g, n=n, algo=WINOGRAD)
    assert ws > 0 and ws % (16 * g.Ca * g.Cb + g.Ca) == 0
    ntiles = g.N * ((g.H + 1) // 2) * ((g.W + 1) // 2)
    return ws // (16 * g.Ca * g.Cb + g.Ca), -(-ntiles // 8)


# ================================================================================================ operand layouts
STRIDES = ("natural", "slice", "odd")


def batch_stride(C, plane, kind):
    """natural; + 4 planes (a channel slice of a wider buffer, alignment kept); + 2 floats (16-byte paths off)"""
    return C * plane + {"natural": 0, "slice": 4 * plane, "odd": 2}[kind]


Layout = namedtuple("Layout", "gs_bs gb_bs gs_lead gb_lead dw_lead ws_lead dw_ld dw_col0 ws_extra ws_floats_arg")


def layout(g, need_ws, gs_stride="natural", gb_stride="natural", dw_ld=0, misalign=None, ws_mode="exact"):
    """where every operand of a call lies in its own NaN-filled allocation (floats): `lead` guard floats in front (4 =
    16-byte aligned, 5 = 4 bytes off), the block of a wider dw starting dw_col0 columns into its rows"""
    assert gs_stride in STRIDES and gb_stride in STRIDES and misalign in (None, "gs", "gb", "dw", "ws")
    assert ws_mode in ("unchecked", "exact", "larger")
    lead = lambda name: 5 if misalign == name else 4
    ld = dw_ld if dw_ld else g.Cb
    col0 = 0 if ld == g.Cb else (4 if (ld - g.Cb) >= 4 else ld - g.Cb)
    extra = 1000 if ws_mode == "larger" else 0
    return Layout(batch_stride(g.Ca, g.OH * g.OW, gs_stride), batch_stride(g.Cb, g.H * g.W, gb_stride),
                  lead("gs"), lead("gb"), lead("dw"), lead("ws"), ld, col0, extra,
                  0 if ws_mode == "unchecked" else need_ws + extra)


# ================================================================================================ host-path predicates
def host_paths(g, p, lay, act_s=NONE, act_b=NONE, algo=DIRECT):
    """which forms a direct launch of plan p with operands laid out as `lay` takes (conv_wgrad.hip: wgrad_direct_grouped
    for the loaders and the kernel form, fill_reduce for the reduction)"""
    taps = g.KH * g.KW
    al = lambda lead, off=0: (lead + off) % 4 == 0          # allocations are 16-byte aligned themselves
    gs_al, gb_al, ws_al = al(lay.gs_lead), al(lay.gb_lead), al(lay.ws_lead)
    dw_al = al(lay.dw_lead, lay.dw_col0 * taps)
    red_taps = 16 if algo == WINOGRAD else taps
    red4 = red_taps == 1 and (g.Ca * g.Cb) % 4 == 0 and ws_al and dw_al and \
        (lay.dw_ld == g.Cb or (g.Cb % 4 == 0 and lay.dw_ld % 4 == 0))
    out = {"reduce": "wino" if algo == WINOGRAD else ("float4" if red4 else "taps")}
    if algo == WINOGRAD:
        return out
    PW, PH = (p.TW - 1) * g.stride + g.KW, (p.TH - 1) * g.stride + g.KH
    pg_vec4 = taps == 1 and g.stride == 1 and g.pad == 0 and p.npx >= 32 and p.TW % 4 == 0 and g.W % 4 == 0 and \
        lay.gb_bs % 4 == 0 and (g.H * g.W) % 4 == 0 and PW % 4 == 0 and (PW * PH) % 4 == 0 and gb_al
    gs_vec4 = p.npx >= 32 and p.TW % 4 == 0 and g.OW % 4 == 0 and lay.gs_bs % 4 == 0 and (g.OH * g.OW) % 4 == 0 and gs_al
    out["pg"] = "vec4" if pg_vec4 else ("dma" if act_b == NONE else "planes")
    out["gs_vec4"] = bool(gs_vec4)          # loader-wave kernels only (the DMA-only families stage gs by DMA)
    out["dma16"] = bool(p.family == "dma1" and p.npx == 64 and p.TW >= 4 and g.OW % 4 == 0 and lay.gs_bs % 4 == 0 and
                        lay.gb_bs % 4 == 0 and gs_al and gb_al)
    return out


def int32_guard_refuses(g, gb_bs):
    """wgrad_direct_grouped: PlaneMap byte offsets are int32"""
    return (g.N * gb_bs + 8 * g.H * g.W) * 4 >= 2 ** 31


# ================================================================================================ case tables
def case(cid, g, **kw):
    c = dict(id=cid, g=g, inputs="grid", act_s=NONE, act_b=NONE, accum=0, dbias=True, accum_bias=0, dw_ld=0,
             gs_stride="natural", gb_stride="natural", misalign=None, ws_mode="exact", variant=-1, algo=DIRECT)
    assert set(kw) <= set(c), kw
    c.update(kw)
    return c


def kname(g):
    return "%dx%ds%dp%d" % (g.KH, g.KW, g.stride, g.pad)


ONE_TRIP = [geom(3, 11, 13, 1, 1, 0), geom(3, 11, 13, 3, 1, 1), geom(3, 11, 13, 3, 1, 0), geom(3, 11, 13, 3, 2, 1, HW=(22, 26)),
            geom(3, 11, 13, 5, 2, 2, HW=(22, 26)), geom(3, 11, 13, 5, 1, 2)]
TINY = [geom(5, 4, 4, 3, 1, 1), geom(5, 2, 3, 3, 1, 1), geom(7, 1, 1, 3, 1, 1)]
TINY_TI = [4, 8, 32]             # images per pixel tile each of them must get
MULTI_TRIP = [geom(10, 61, 63, 1, 1, 0), geom(10, 61, 63, 3, 1, 1), geom(10, 61, 63, 5, 1, 2),
              geom(9, 61, 63, 5, 2, 2, HW=(122, 126)), geom(9, 61, 63, 1, 1, 0), geom(9, 61, 63, 3, 1, 1)]
MULTI_TRIP_VEC = geom(9, 61, 64, 1, 1, 0)
BLOCKS = [geom(2, 24, 24, 3, 1, 1, ch=(200, 196)), geom(2, 48, 48, 1, 1, 0, ch=(200, 196)),
          geom(2, 48, 48, 5, 2, 2, ch=(200, 196), HW=(96, 96)), geom(2, 24, 24, 3, 1, 1, ch=(100, 70)),
          geom(2, 48, 48, 1, 1, 0, ch=(100, 70)), geom(2, 48, 48, 5, 2, 2, ch=(100, 70), HW=(96, 96))]
CONVT = [geom(2, 9, 11, 5, 2, 2, ch=(24, 40), HW=(18, 22)), geom(2, 9, 11, 5, 2, 2, ch=(24, 40), HW=(17, 21))]
ODD_KERNELS = [geom(2, 10, 14, 2, 2, 0), geom(2, 10, 14, 4, 2, 1), geom(2, 10, 14, (1, 3), 1, 1), geom(2, 10, 14, (3, 5), 1, 1)]
DEEP_REDUCE = [geom(4, 64, 64, 1, 1, 0, ch=(32, 32)), geom(4, 64, 64, 3, 1, 1, ch=(96, 96)), geom(4, 64, 64, 5, 1, 2, ch=(96, 32))]
DEEP_VARIANT = [None, 8, 10]     # the automatic choice each of them must get (None: any)
REFUSED_KERNELS = [(geom(2, 10, 12, (5, 6), 1, 0), ERR_UNSUPPORTED), (geom(2, 10, 12, (4, 8), 1, 0), ERR_UNSUPPORTED),
                   (geom(2, 10, 12, 7, 1, 3), ERR_ARG)]
ONE_TRIP_CROSS = [ONE_TRIP[0], ONE_TRIP[1], ONE_TRIP[4]]       # 1x1, 3x3, 5x5 s2: the argument cross

ALL_GEOMS = ONE_TRIP + TINY + MULTI_TRIP + [MULTI_TRIP_VEC] + BLOCKS + CONVT + ODD_KERNELS + DEEP_REDUCE


def variant_table(geoms):
    """every row of kWgVariants on every geometry: (g, v, plan return code); admitted rows are launches, the others
    refusal cases with the planner's own code"""
    return [(g, v, plan(g, variant=v).rc) for g in geoms for v in range(NVARIANTS)]


def geometry_cases():
    """the automatic choice on every base geometry, `grid` inputs, bias set; the `blocks` geometries also with the
    64 x 32 blocks of variant 0 (several blocks in both directions whatever the automatic choice is)"""
    return [case("auto-" + gname(g), g) for g in ALL_GEOMS] + [case("v0-" + gname(g), g, variant=0) for g in BLOCKS]


def real_cases():
    """`real` inputs: the automatic choice on every geometry whose float32 restatement stays around a second (left out:
    the 5x5 shape at (200, 196) and the 5x5 of `deep-reduce`, tens of seconds each), and the 64 x 32 blocks of variant 0 on the 3x3
    `blocks` shapes"""
    gs = ONE_TRIP + TINY + MULTI_TRIP[:4] + [MULTI_TRIP_VEC] + BLOCKS[0:2] + BLOCKS[3:6] + CONVT + ODD_KERNELS + DEEP_REDUCE[:2]
    return [case("real-" + gname(g), g, inputs="real") for g in gs] + \
        [case("real-v0-" + gname(g), g, inputs="real", variant=0) for g in (BLOCKS[0], BLOCKS[3])]


def real_variant_rows(g):
    """forced rows that also run on `real` inputs: all of them on a one-trip geometry, on a multi-trip geometry the first
    admitted row of every family (the float32 restatement is cached per split count)"""
    adm = [v for v in range(NVARIANTS) if plan(g, variant=v).rc == OK]
    if g in ONE_TRIP:
        return adm
    return [next(v for v in adm if FAMILY[v] == f) for f in FAMILIES if any(FAMILY[v] == f for v in adm)]


FAMILIES = ("general", "t33", "t33_tapw", "tap9", "tap25", "dma1")


def forced_variants(g, act_s=NONE, act_b=NONE):
    """asked of the planner: for every family that admits (g, act_s, act_b), the first admitted row that is not the
    automatic choice (whose plan a forced launch would only repeat).  A one-row family that is itself the automatic
    choice has no entry: the `auto` cases are its cases."""
    auto = plan(g, act_s, act_b).variant
    out = []
    for fam in FAMILIES:
        rows = [v for v in range(NVARIANTS) if FAMILY[v] == fam and v != auto and plan(g, act_s, act_b, 1, v).rc == OK]
        if rows:
            out.append(rows[0])
    return out


def admitted_families(g, act_s=NONE, act_b=NONE):
    return {FAMILY[v] for v in range(NVARIANTS) if plan(g, act_s, act_b, 1, v).rc == OK}


@functools.lru_cache(maxsize=None)
def _cross_cases():
    out = []
    vname = lambda v: "auto" if v < 0 else "v%d" % v
    for g in ONE_TRIP_CROSS:
        k = kname(g)
        for a_s in (NONE, GELU, SQUARE):
            for a_b in (NONE, GELU, SQUARE):
                if (a_s, a_b) == (NONE, NONE):
                    continue
                which = "real" if GELU in (a_s, a_b) else "grid"
                for v in [-1] + forced_variants(g, a_s, a_b):
                    out.append(case("%s-%s-act-%s-%s" % (k, vname(v), ACT_NAMES[a_s], ACT_NAMES[a_b]), g, inputs=which,
                                    act_s=a_s, act_b=a_b, variant=v))
        for v in [-1] + forced_variants(g):
            vn = vname(v)
            for accum, dbias, ab in ((1, True, 0), (0, False, 0), (1, True, 1), (0, True, 1), (1, False, 0)):
                for which in ("grid", "real"):
                    out.append(case("%s-%s-%s-accum%d-%s-accumbias%d" % (k, vn, which, accum, "bias" if dbias else "nobias", ab),
                                    g, inputs=which, accum=accum, dbias=dbias, accum_bias=ab, variant=v))
            for ld in (g.Cb, g.Cb + 8, g.Cb + 3):
                for accum in (0, 1):
                    out.append(case("%s-%s-dwld%d-accum%d" % (k, vn, ld, accum), g, dw_ld=ld, accum=accum, variant=v))
            for name in ("gs_stride", "gb_stride"):
                for kind in ("slice", "odd"):
                    out.append(case("%s-%s-%s-%s" % (k, vn, name, kind), g, variant=v, **{name: kind}))
            for m in ("gs", "gb", "dw", "ws"):
                out.append(case("%s-%s-misaligned-%s" % (k, vn, m), g, misalign=m, variant=v))
            for wm in ("unchecked", "larger"):
                out.append(case("%s-%s-ws-%s" % (k, vn, wm), g, ws_mode=wm, variant=v))
        # dbias = sum actS(gs) on the square, with accumulation
        out.append(case("%s-auto-square-bias-accum" % k, g, act_s=SQUARE, accum=1, accum_bias=1))
    # bias with several b-blocks and two tap groups: only (bt, tg) = (0, 0) writes the partial
    out.append(case("blocks-5x5-v0-bias-two-tap-groups", BLOCKS[2], variant=0, accum_bias=1))
    out.append(case("blocks-5x5-v0-bias-two-tap-groups-small", BLOCKS[5], variant=0, accum_bias=1))
    return tuple(out)


def cross_cases():
    """the argument cross on one-trip 1x1, 3x3 and 5x5 s2: the automatic choice and one forced row of every family that
    admits the combination (forced_variants)"""
    return [dict(c) for c in _cross_cases()]


# the vec shapes: every 16-byte form taken in one case and knocked out in a sibling by exactly one of its conditions
VEC_G = MULTI_TRIP_VEC
VEC_ONE = geom(1, 64, 64, 1, 1, 0)
VEC_RAGGED = [geom(2, 8, 12, 1, 1, 0), geom(2, 8, 20, 1, 1, 0), geom(2, 8, 68, 1, 1, 0)]


def vec_cases():
    """(case, expected host paths): keys of host_paths that the case is there for"""
    out = []
    add = lambda c, **exp: out.append((c, exp))
    for g, tag in ((VEC_G, "multi-trip-vec"), (VEC_ONE, "N1-64x64")):
        add(case(tag + "-v3-all-16-byte", g, variant=3), gs_vec4=True, pg="vec4", reduce="float4")
        add(case(tag + "-v3-gs-misaligned", g, variant=3, misalign="gs"), gs_vec4=False, pg="vec4", reduce="float4")
        add(case(tag + "-v3-gs-odd-stride", g, variant=3, gs_stride="odd"), gs_vec4=False, pg="vec4")
        add(case(tag + "-v3-gb-misaligned", g, variant=3, misalign="gb"), gs_vec4=True, pg="dma")
        add(case(tag + "-v3-gb-odd-stride", g, variant=3, gb_stride="odd"), gs_vec4=True, pg="dma")
        add(case(tag + "-v3-act-b-square", g, variant=3, act_b=SQUARE), gs_vec4=True, pg="vec4")
        add(case(tag + "-v3-act-s-square", g, variant=3, act_s=SQUARE), gs_vec4=True, pg="vec4")
        add(case(tag + "-v3-act-s-gelu", g, variant=3, act_s=GELU, inputs="real"), gs_vec4=True, pg="vec4")
        add(case(tag + "-v3-act-s-gelu-gs-misaligned", g, variant=3, act_s=GELU, inputs="real", misalign="gs"), gs_vec4=False)
        add(case(tag + "-v3-ws-misaligned", g, variant=3, misalign="ws"), reduce="taps")
        add(case(tag + "-v3-dw-misaligned", g, variant=3, misalign="dw"), reduce="taps")
        add(case(tag + "-v3-dwld-plus3", g, variant=3, dw_ld=g.Cb + 3), reduce="taps")
        add(case(tag + "-v3-dwld-plus8", g, variant=3, dw_ld=g.Cb + 8), reduce="float4")
        add(case(tag + "-v14-dma16", g, variant=14), dma16=True, reduce="float4")
        add(case(tag + "-v14-gs-misaligned", g, variant=14, misalign="gs"), dma16=False)
        add(case(tag + "-v14-gb-misaligned", g, variant=14, misalign="gb"), dma16=False)
        add(case(tag + "-v14-gs-odd-stride", g, variant=14, gs_stride="odd"), dma16=False)
        add(case(tag + "-v14-gb-odd-stride", g, variant=14, gb_stride="odd"), dma16=False)
        add(case(tag + "-v14-slices", g, variant=14, gs_stride="slice", gb_stride="slice"), dma16=True)
        add(case(tag + "-auto", g), reduce="float4")
    # same geometry one column narrower: OW % 4 != 0 knocks every 16-byte operand form out
    g63 = MULTI_TRIP[0]
    add(case("multi-trip-OW63-v3", g63, variant=3), gs_vec4=False, pg="dma", reduce="float4")
    add(case("multi-trip-OW63-v14", g63, variant=14), dma16=False)
    # plain staging (an activation on the big-grid operand, no 16-byte form)
    add(case("multi-trip-OW63-v3-act-b-square", g63, variant=3, act_b=SQUARE), pg="planes")
    # 3x3 with an activation on the big-grid operand: plain stage_planes next to a 16-byte small-grid loader
    add(case("3x3-OW64-v1-act-b-square", geom(2, 16, 64, 3, 1, 1), variant=1, act_b=SQUARE), gs_vec4=True, pg="planes")
    add(case("3x3-OW64-v1", geom(2, 16, 64, 3, 1, 1), variant=1), gs_vec4=True, pg="dma")
    add(case("3x3-OW64-v1-act-s-square", geom(2, 16, 64, 3, 1, 1), variant=1, act_s=SQUARE), gs_vec4=True, pg="dma")
    add(case("3x3-OW64-v7-act-s-gelu", geom(2, 16, 64, 3, 1, 1), variant=7, act_s=GELU, inputs="real"), gs_vec4=True, pg="dma")
    for g in VEC_RAGGED:              # a ragged last float4 column of the pixel tile
        add(case("ragged-OW%d-v3" % g.OW, g, variant=3), gs_vec4=True, pg="vec4")
        add(case("ragged-OW%d-v14" % g.OW, g, variant=14), dma16=True)
    # Ca * Cb % 4 != 0: the float4 reduction is off whatever the alignment
    add(case("1x1-CaCb-odd", geom(3, 11, 13, 1, 1, 0, ch=(5, 3))), reduce="taps")
    return out


GROUP_GEOMS = [ONE_TRIP[1], BLOCKS[3], geom(2, 48, 48, 1, 1, 0), geom(2, 48, 48, 3, 1, 1)]
GROUP_NS = [1, 2, 3, 32]


def group_members(g, n, which, algo=DIRECT):
    """members differ in data, accum, dw_ld and in dbias being null or set"""
    lds = (0, g.Cb + 8, g.Cb + 3, g.Cb)
    return [case("m%d" % i, g, inputs=which, accum=i & 1, dbias=(i % 3) != 1, accum_bias=(i >> 1) & 1, dw_ld=lds[i % 4],
                 algo=algo) for i in range(n)]


WINO_GEOMS = [geom(1, 1, 1, 3, 1, 1), geom(2, 5, 7, 3, 1, 1), geom(3, 11, 13, 3, 1, 1), geom(9, 61, 63, 3, 1, 1, ch=(72, 40)),
              geom(2, 24, 24, 3, 1, 1, ch=(200, 130))]


def wino_cases():
    out = []
    for g in WINO_GEOMS:
        for which in ("grid", "real"):
            out.append(case("wino-%s-%s" % (gname(g), which), g, inputs=which, algo=WINOGRAD))
    g = WINO_GEOMS[2]
    for which in ("grid", "real"):
        for accum, dbias, ab in ((1, True, 1), (1, False, 0), (0, True, 1)):
            out.append(case("wino-%s-accum%d-%s-accumbias%d" % (which, accum, "bias" if dbias else "nobias", ab), g, inputs=which,
                            accum=accum, dbias=dbias, accum_bias=ab, algo=WINOGRAD))
    for ld in (g.Cb + 8, g.Cb + 3):
        for accum in (0, 1):
            out.append(case("wino-dwld%d-accum%d" % (ld, accum), g, dw_ld=ld, accum=accum, algo=WINOGRAD))
    for name in ("gs_stride", "gb_stride"):
        for kind in ("slice", "odd"):
            out.append(case("wino-%s-%s" % (name, kind), g, algo=WINOGRAD, **{name: kind}))
            out.append(case("wino-even-W-%s-%s" % (name, kind), geom(2, 6, 8, 3, 1, 1), algo=WINOGRAD, **{name: kind}))
    for m in ("gs", "gb", "dw", "ws"):
        out.append(case("wino-even-W-misaligned-%s" % m, geom(2, 6, 8, 3, 1, 1), algo=WINOGRAD, misalign=m))
    return out


# near the int32 limit of the big-grid byte offsets
INT32_G = geom(2, 16, 16, 3, 1, 1, ch=(40, 8))
INT32_REFUSED_BS = 2 ** 28
INT32_LARGEST_BS = (2 ** 29 - 8 * 16 * 16 - 1) // 2
