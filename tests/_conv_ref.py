"""Reference, inputs, limit rule, case tables and host-path predicates of the forward / input-gradient convolution
numerics tests (tests/test_conv_ref.py on the CPU, tests/test_gpu_conv_numerics.py on the GPU).

Reference: conv64 is the header formula of include/icm_hip.h (icm_conv_args) in float64 torch -- not F.conv2d: an
explicit gather (transposed = 0) or scatter (transposed = 1) of the operand per tap with zero fill, contracted with the
canonical weights W[o][i][kh][kw] (nothing packed):
    gather:  y[n,o,p] = sum_{i,t} W[o][i][t] * act(x[n,i,p*stride - pad + t])
    scatter: y[n,o,q] = sum_{i,t,p : p*stride - pad + t == q} W[o][i][t] * act(x[n,i,p])
around it the operand activation (NONE / exact-erf GELU / SQUARE), the blocked channel map x_seg_len / x_seg_gap, the
optional bias, every ICM_EPI_* kind as epi_apply (csrc/conv_common.h) and the header state it, accum, the second output
(side value of GDN / IGDN / LRP, gelu(y after the add) for NONE / RES / RES_GELU, the y2 == y form) and the
pixel_shuffle = 2 store.  It also returns abs_terms (sum |terms| per accumulator element).

Two input sets (oracle/weights.py's generator)
  grid: every element of x, w, bias, res, aux, aux2 and of the y prefill is an integer in [-2, 2] (GDN / IGDN: SQUARE
        operand, weights in [0, 2], bias in [1, 2], as the model's non-negative parametrisation gives: norm >= 1).  Every
        product and partial sum is an integer, in the Winograd form a multiple of 1/4 (G g G^T) times an integer
        (B^T d B); grid_headroom asserts per case that none can reach 2^24 (direct: sum |terms| + |prefill|; Winograd: 4 x
        the transform-domain sum, i.e. the same bound in units of 1/4).  Where the epilogue is exact arithmetic (NONE, RES,
        AXPY2, accum, y2 = the GDN / IGDN norm, pro_act NONE / SQUARE) the kernels must return conv64(...).float() bit for
        bit under any tiling, K split or transform.  The kinds that end in gelu_f, dgelu_f, tanhf, sqrtf or rsqrtf have
        an exact accumulator; they are held to the rule below with the accumulator terms at zero: the function floor and
        the roundings of the multiply / add that follow the function.
  real: uniform [-1, 1); the only set for a GELU operand, and the one that shows a lower-precision matrix instruction.

Limit per output tensor on `real` (none of it is taken from a kernel's output)
    |gpu - ref64|_max <= FACTOR * |ref32 - ref64|_max + FACTOR * 2^-24 * |ref64|_max + function floor
  ref32 = the same formula with every product and addition rounded to float32, summed in the order the code documents
  for the family the planner reports: staged and pointwise kernels one serial chain over sub-steps (8-channel group,
  tap), channels inside the group; KS rows 10-12 sub-step q of a staged chunk to chain q mod KS, the K-split kernel
  sub-step q to chain q mod 8, chains added in order; Winograd float32 transforms, a per-point channel chain and a
  float32 output transform.
  Function floors: gelu_f / dgelu_f -- tests/_pointwise_ref.py's gelu_floor / dgelu_floor (erf_bf 5.8e-8); rsqrtf /
  sqrtf -- the 2 ulp _pointwise_ref grants v_rsq_f32; tanhf -- the documentation installed with ROCm (the share/doc
  tree of the installation, searched for "tanh": no match in any file) states no accuracy for it, so there is no file
  and line to quote and 2 ulp of the result are GRANTED, not measured.  Every floor is carried through the arithmetic that follows the function, and the accumulator's own limit
  (FACTOR * |acc32 - acc64|_max + FACTOR * 2^-24 * |acc64|_max + the GELU-operand floor) through the function's
  derivative.

Host paths: plan() asks the library (icm_debug_conv_plan: host code); the predicates restate plan_class, plan_ks8,
plan_conv1x1 and plan_conv_wino (csrc/conv_igemm.hip, conv_1x1.hip, conv_wino.hip) as formulas over the arguments and
the plan, so that "taken" / "knocked out by exactly this condition" is asserted on the CPU."""
import ctypes
import functools
import math
from collections import namedtuple

import numpy as np
import torch

import _pointwise_ref as PR
from oracle import weights as W

FACTOR = 4
U = 2.0 ** -24
ULP = 2.0 ** -23
F64 = torch.float64
NONE, GELU, SQUARE = 0, 1, 2
ACT_NAMES = {NONE: "none", GELU: "gelu", SQUARE: "square"}
E_NONE, E_RES, E_RES_GELU, E_GDN, E_IGDN, E_MUL_DGELU, E_AXPY2, E_LRP, E_RES_MUL_DGELU = range(9)
EPI_NAMES = ["none", "res", "res_gelu", "gdn", "igdn", "mul_dgelu", "axpy2", "lrp", "res_mul_dgelu"]
EPI_ALL = tuple(range(9))
EPI_KS8 = (E_NONE, E_RES, E_RES_GELU, E_MUL_DGELU, E_LRP, E_RES_MUL_DGELU)
EPI_WINO = EPI_KS8
EPI_EXACT = (E_NONE, E_RES, E_AXPY2)                 # exact arithmetic on `grid`
OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 3
DIRECT, WINOGRAD = 0, 1
STAGED, KS8, P1, WINO44, WINO8 = range(5)
FAMILY_NAMES = ["staged", "ks8", "pointwise", "wino44", "wino8"]
CFG_AUTO, CFG_KS8_64, CFG_KS8_128 = -1, 100, 101
NROWS = 13
# rows of kCfgs (csrc/conv_igemm.hip): (wco, wpx, tco, tpx, ks); rows of kCfgs1x1 (csrc/conv_1x1.hip): (tco, tpx)
ROWS = [(1, 4, 3, 2, 1), (1, 4, 6, 1, 1), (1, 4, 2, 2, 1), (1, 4, 1, 2, 1), (1, 4, 3, 1, 1), (1, 4, 5, 1, 1), (2, 2, 2, 1, 1),
        (2, 2, 1, 1, 1), (4, 1, 1, 1, 1), (1, 4, 1, 1, 1), (2, 1, 1, 1, 2), (1, 2, 1, 1, 2), (1, 1, 1, 1, 4)]
ROWS_1X1 = [(6, 1), (5, 1), (4, 1), (3, 2), (2, 2), (1, 2), (3, 1), (2, 1)]
EFF_1X1 = [1.0, 1.0, 0.97, 1.0, 0.7, 0.6, 0.95, 0.6]
MAX_TAPS, MAX_GROUPS = 32, 12


def cdiv(a, b):
    return -(-a // b)


def clog2(v):
    return max(0, int(v - 1).bit_length())


Geom = namedtuple("Geom", "N Cin Cout H W OH OW KH KW stride pad transposed")


def geom(N, OH, OW, k, stride, pad, transposed=0, ch=(40, 24), HW=None):
    """output grid OH x OW, kernel k (int or (KH, KW)); the input grid is the smallest that gives (gather) or reaches
    (scatter) OH x OW unless HW names it"""
    KH, KW = (k, k) if isinstance(k, int) else k
    if HW:
        H, Wd = HW
    elif not transposed:
        H, Wd = (OH - 1) * stride + KH - 2 * pad, (OW - 1) * stride + KW - 2 * pad
    else:
        H, Wd = max(1, cdiv(OH - 1 + pad - (KH - 1), stride) + 1), max(1, cdiv(OW - 1 + pad - (KW - 1), stride) + 1)
    assert H >= 1 and Wd >= 1
    if not transposed:
        assert (H + 2 * pad - KH) // stride + 1 == OH and (Wd + 2 * pad - KW) // stride + 1 == OW
    return Geom(N, ch[0], ch[1], H, Wd, OH, OW, KH, KW, stride, pad, transposed)


def gname(g):
    return "%sN%d-%dx%d-k%dx%ds%dp%d-c%dx%d-in%dx%d" % ("T" if g.transposed else "", g.N, g.OH, g.OW, g.KH, g.KW, g.stride,
                                                        g.pad, g.Cin, g.Cout, g.H, g.W)


# ================================================================================================ cases
def case(cid, g, **kw):
    """one launch member.  strides: kind per operand ("natural" / "slice" / "odd"); x_off: floats x lies off 16-byte
    alignment; y2: "none" / "sep" / "same"; seg: (x_seg_len, x_seg_gap) or None; cfg / f1x1: the forced configuration"""
    c = dict(id=cid, g=g, inputs="grid", pro_act=NONE, epi=E_NONE, bias=True, accum=0, y2="none", ps=0, seg=None,
             strides={}, x_off=0, cfg=CFG_AUTO, f1x1=-1, algo=DIRECT, xv=False, member=0, ngroups=1, nonneg=False)
    assert set(kw) <= set(c), kw
    c.update(kw)
    if c["epi"] in (E_GDN, E_IGDN):
        assert c["pro_act"] == SQUARE and c["bias"], "GDN / IGDN cases take the model's operands: the norm stays >= 1"
    if c["pro_act"] == GELU:
        assert c["inputs"] == "real", "a GELU operand has no exact set"
    return c


def phys_channels(c):
    g = c["g"]
    if not c["seg"]:
        return g.Cin
    L, gap = c["seg"]
    return g.Cin + ((g.Cin - 1) // L) * gap


def channel_planes(c):
    g = c["g"]
    ch = torch.arange(g.Cin)
    if not c["seg"]:
        return ch
    L, gap = c["seg"]
    return ch + (ch // L) * gap


def out_shape(c):
    g = c["g"]
    return (g.N, g.Cout // 4, 2 * g.OH, 2 * g.OW) if c["ps"] == 2 else (g.N, g.Cout, g.OH, g.OW)


def _key(c, name):
    return "cv.%s.%s.m%d" % (gname(c["g"]), name, c["member"])


@functools.lru_cache(maxsize=None)
def _input(key, shape, which, lo, hi):
    n = int(np.prod(shape))
    if which == "grid":
        span = int(hi - lo) + 1
        v = np.floor(span * W.uniform01(key, n)) + lo
        assert v.min() >= lo and v.max() <= hi
        return torch.from_numpy(v.astype(np.float32)).reshape(shape)
    assert which == "real"
    return W._u(key, shape, float(lo), float(hi))


NONNEG_BOUND, NONNEG_PED = PR.NONNEG_BOUND, PR.NONNEG_PED


def make_inputs(c):
    """dict of float32 tensors (cached, read-only): x [N, physical planes, H, W], w [Cout, Cin, KH, KW] (logical o, i),
    bias [Cout], res / aux / aux2 / prefill in the layout of y.  nonneg: "w_raw" is what gets packed, w the float32
    evaluation of max(w_raw, bound)^2 - pedestal and "w64" its float64 value"""
    if c["nonneg"]:
        t = dict(make_inputs(dict(c, nonneg=False)))
        t["w_raw"] = t["w"]
        b = torch.clamp_min(t["w"], NONNEG_BOUND)
        t["w"] = b * b - NONNEG_PED
        b = torch.clamp_min(t["w_raw"].double(), float(NONNEG_BOUND))
        t["w64"] = b * b - float(NONNEG_PED)
        return t
    g, which = c["g"], c["inputs"]
    gdn = c["epi"] in (E_GDN, E_IGDN)
    lo, hi = (-2, 2) if which == "grid" else (-1, 1)
    osh = out_shape(c)
    t = {"x": _input(_key(c, "x%d" % phys_channels(c)), (g.N, phys_channels(c), g.H, g.W), which, lo, hi),
         "w": _input(_key(c, "w" + ("+" if gdn else "")), (g.Cout, g.Cin, g.KH, g.KW), which, 0 if gdn else lo, hi),
         "bias": _input(_key(c, "b" + ("+" if gdn else "")), (g.Cout,), which, 1 if gdn else lo, 2 if gdn else hi)}
    for name in ("res", "aux", "aux2", "prefill"):
        t[name] = _input(_key(c, name + ("ps" if c["ps"] else "")), osh, which, lo, hi)
    return t


# ================================================================================================ reference
def act64(x, act):
    if act == GELU:
        return PR.gelu(x)
    if act == SQUARE:
        return x * x
    assert act == NONE
    return x


def tap_operands(xl, g):
    """[N, Cin, H, W] (logical channels, activation applied) -> T [N, Cin, taps, OH*OW]: the operand element tap t of
    output pixel p multiplies, 0 where the formula has none (outside the image / no p with p*stride - pad + t == q)"""
    N, Ci = xl.shape[:2]
    T = torch.zeros((N, Ci, g.KH * g.KW, g.OH, g.OW), dtype=xl.dtype)
    iy, ix = torch.arange(g.H), torch.arange(g.W)
    oy, ox = torch.arange(g.OH), torch.arange(g.OW)
    for kh in range(g.KH):
        for kw in range(g.KW):
            if g.transposed:            # q = p * stride - pad + t
                qy, qx = iy * g.stride - g.pad + kh, ix * g.stride - g.pad + kw
                my, mx = (qy >= 0) & (qy < g.OH), (qx >= 0) & (qx < g.OW)
                sy, sx, dy, dx = iy[my], ix[mx], qy[my], qx[mx]
            else:                       # source = p * stride - pad + t
                py, px = oy * g.stride - g.pad + kh, ox * g.stride - g.pad + kw
                my, mx = (py >= 0) & (py < g.H), (px >= 0) & (px < g.W)
                sy, sx, dy, dx = py[my], px[mx], oy[my], ox[mx]
            if len(sy) and len(sx):
                T[:, :, kh * g.KW + kw, dy[:, None], dx[None, :]] = xl[:, :, sy[:, None], sx[None, :]]
    return T.reshape(N, Ci, g.KH * g.KW, g.OH * g.OW)


def ckey(c):
    """what the contraction of a case depends on"""
    return (c["g"], c["seg"], c["pro_act"], c["inputs"], c["member"], c["epi"] in (E_GDN, E_IGDN), c["nonneg"])


_CONTRACT, _ACC32 = {}, {}


def contract64(x, w, c):
    """(accumulator [N, Cout, OH, OW], sum |terms|) in float64: operand activation, channel map, the tap formula"""
    g = c["g"]
    xl = act64(x.double()[:, channel_planes(c)], c["pro_act"])
    T = tap_operands(xl, g)
    w3 = w.double().reshape(g.Cout, g.Cin, g.KH * g.KW)          # nonneg cases pass their float64 weights as w
    acc = torch.einsum("oit,nitp->nop", w3, T).reshape(g.N, g.Cout, g.OH, g.OW)
    ab = torch.einsum("oit,nitp->nop", w3.abs(), T.abs()).reshape(g.N, g.Cout, g.OH, g.OW)
    return acc, ab


def shuffle2(v):
    """the pixel_shuffle = 2 store: [N, C, OH, OW] -> [N, C/4, 2 OH, 2 OW], channel co to plane co >> 2, row
    2 oy + ((co >> 1) & 1), column 2 ox + (co & 1)"""
    N, Cc, H, Wd = v.shape
    return v.reshape(N, Cc // 4, 2, 2, H, Wd).permute(0, 1, 4, 2, 5, 3).reshape(N, Cc // 4, 2 * H, 2 * Wd)


def side_kind(epi):
    return epi in (E_GDN, E_IGDN, E_LRP)


def may_gelu(epi):
    return epi in (E_NONE, E_RES, E_RES_GELU)


Out = namedtuple("Out", "y y2 v side")      # v: the value epi_apply returns (after accum), before materialisation


def epilogue(acc, c, t, fn):
    """everything after the contraction, on tensors of acc's dtype: fn = dict of the functions (gelu, dgelu, tanh,
    sqrt, rsqrt) so that the float32 restatement rounds them once.  acc: [N, Cout, OH, OW]."""
    dt = acc.dtype
    v = acc + t["bias"].to(dt).view(1, -1, 1, 1) if c["bias"] else acc
    if c["ps"] == 2:
        v = shuffle2(v)
    res, aux, aux2 = t["res"].to(dt), t["aux"].to(dt), t["aux2"].to(dt)
    e, side = c["epi"], None
    if e == E_RES:
        v = v + res
    elif e == E_RES_GELU:
        v = v + fn["gelu"](res)
    elif e in (E_GDN, E_IGDN):
        side = v
        v = aux * (fn["rsqrt"](v) if e == E_GDN else fn["sqrt"](v))
    elif e == E_MUL_DGELU:
        v = v * fn["dgelu"](aux)
    elif e == E_RES_MUL_DGELU:
        v = (v + res) * fn["dgelu"](aux)
    elif e == E_AXPY2:
        v = aux2 + (2.0 * aux) * v
    elif e == E_LRP:
        side = fn["tanh"](v)
        v = aux + 0.5 * side
    else:
        assert e == E_NONE
    if c["accum"]:
        v = v + t["prefill"].to(dt)
    y, y2 = v, None
    if c["y2"] != "none":
        if side_kind(e):
            assert c["y2"] == "sep"
            y2 = side
        elif may_gelu(e):
            gv = fn["gelu"](v)
            if c["y2"] == "same":
                y = gv
            else:
                y2 = gv
    return Out(y, y2, v, side)


FN64 = dict(gelu=PR.gelu, dgelu=PR.dgelu, tanh=torch.tanh, sqrt=torch.sqrt, rsqrt=torch.rsqrt)
FN32 = {k: (lambda f: (lambda x: f(x.double()).float()))(f) for k, f in FN64.items()}   # correctly rounded float32


def conv64(c, t=None):
    """(Out of float64 tensors in the layout of y, accumulator, abs_terms)"""
    if t is None:
        t = make_inputs(c)
        if ckey(c) not in _CONTRACT:
            _CONTRACT[ckey(c)] = contract64(t["x"], t.get("w64", t["w"]), c)
        acc, ab = _CONTRACT[ckey(c)]
    else:
        acc, ab = contract64(t["x"], t["w"], c)
    return epilogue(acc, c, t, FN64), acc, ab


# ---- float32 restatements in the documented summation orders
Tap = namedtuple("Tap", "kidx dy dx")
Class = namedtuple("Class", "cy cx iy0 ix0 ey ex taps")


def _axis_taps(K, s, pad, cpar):
    ks, dis = [], []
    for k in range(K):
        v = cpar + pad - k
        if v % s:
            continue
        ks.append(k)
        dis.append(v // s if v >= 0 else -((-v) // s))
    return ks, dis


def build_classes(g):
    """the tap classes of a launch (build_classes of csrc/conv_igemm.hip): one for a gather, stride^2 output-parity
    classes for a scatter"""
    if not g.transposed:
        taps = [Tap(kh * g.KW + kw, kh, kw) for kh in range(g.KH) for kw in range(g.KW)]
        return [Class(0, 0, -g.pad, -g.pad, g.KH, g.KW, taps)]
    out = []
    for cy in range(g.stride):
        for cx in range(g.stride):
            khs, dys = _axis_taps(g.KH, g.stride, g.pad, cy)
            kws, dxs = _axis_taps(g.KW, g.stride, g.pad, cx)
            miny, maxy = (min(dys), max(dys)) if dys else (0, 0)
            minx, maxx = (min(dxs), max(dxs)) if dxs else (0, 0)
            taps = [Tap(khs[a] * g.KW + kws[b], dys[a] - miny, dxs[b] - minx) for a in range(len(khs)) for b in range(len(kws))]
            out.append(Class(cy, cx, miny, minx, maxy - miny + 1, maxx - minx + 1, taps))
    return out


def class_grid(g, cl):
    """virtual output grid of a class: (OHv, OWv)"""
    if not g.transposed:
        return g.OH, g.OW
    return max(0, cdiv(g.OH - cl.cy, g.stride)), max(0, cdiv(g.OW - cl.cx, g.stride))


def acc32_direct(x, w, c, orders=("serial",), fault=None):
    """the contraction in float32, every product and every addition rounded: per tap class the sub-steps (8-channel
    group, tap of the class) in order, channels inside the group; orders = one per class (or one for all) of
    ("serial",), ("ks", KS, ckm): sub-step q of a staged chunk of ckm groups to chain q mod KS, or ("ks8",): sub-step q to
    chain q mod 8; chains added in order.
    fault (tests only): "tap" drops the last tap from the output tile [:8, :8] of image 0, "channel" drops the last
    channel of the last K group, "pixel" gives output pixel (1, 1) of image 0 its left neighbour's value."""
    g = c["g"]
    xl = act64(x.double()[:, channel_planes(c)], c["pro_act"]).float()
    T = tap_operands(xl, g)                                   # [N, Cin, taps, P]
    w3 = w.float().reshape(g.Cout, g.Cin, g.KH * g.KW)
    if isinstance(orders[0], str):
        orders = [orders] * (g.stride ** 2 if g.transposed else 1)
    out = torch.zeros((g.N, g.Cout, g.OH * g.OW), dtype=torch.float32)
    oy = torch.arange(g.OH).view(-1, 1).expand(g.OH, g.OW).reshape(-1)
    ox = torch.arange(g.OW).view(1, -1).expand(g.OH, g.OW).reshape(-1)
    for cl, order in zip(build_classes(g), orders):
        nch = {"serial": 1, "ks": order[1] if len(order) > 1 else 1, "ks8": 8}[order[0]]
        pix = ((oy % g.stride == cl.cy) & (ox % g.stride == cl.cx)).nonzero().reshape(-1) if g.transposed else torch.arange(g.OH * g.OW)
        if not len(pix) or not cl.taps:
            continue
        Tc = T[:, :, :, pix]
        accs = torch.zeros((nch, g.N, g.Cout, len(pix)), dtype=torch.float32)
        nt, ngrp = len(cl.taps), cdiv(g.Cin, 8)
        for grp in range(ngrp):
            for ti, tp in enumerate(cl.taps):
                q = grp * nt + ti
                if order[0] == "ks":
                    q = (grp % order[2]) * nt + ti
                a = accs[q % nch]
                for ch in range(grp * 8, min(grp * 8 + 8, g.Cin)):
                    if fault == "channel" and ch == g.Cin - 1:
                        continue
                    term = w3[None, :, ch, tp.kidx, None] * Tc[:, None, ch, tp.kidx, :]
                    if fault == "tap" and ti == nt - 1:
                        tile = ((oy[pix] < 8) & (ox[pix] < 8)).float()
                        term = term.clone()
                        term[0] *= (1.0 - tile)
                    a += term
        tot = accs[0]
        for k in range(1, nch):
            tot = tot + accs[k]
        out[:, :, pix] = tot
    out = out.reshape(g.N, g.Cout, g.OH, g.OW)
    if fault == "pixel":
        out[0, :, min(1, g.OH - 1), min(1, g.OW - 1)] = out[0, :, min(1, g.OH - 1), 0]
    return out


WINO_BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=F64)
WINO_G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=F64)
WINO_AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=F64)


def wino_domain(x, w, c, dt):
    """(U [16, Cout, Cin], V [16, Cin, tiles]) of F(2x2, 3x3) in dtype dt.  The input-gradient orientation
    (transposed: a scatter with W = a gather with the kernel rotated by 180 degrees) flips the taps."""
    g = c["g"]
    xl = act64(x.double()[:, channel_planes(c)], c["pro_act"]).to(dt)
    TH, TW = cdiv(g.H, 2), cdiv(g.W, 2)
    xp = torch.zeros((g.N, g.Cin, 2 * TH + 2, 2 * TW + 2), dtype=dt)
    xp[:, :, 1:1 + g.H, 1:1 + g.W] = xl
    d = xp.unfold(2, 4, 2).unfold(3, 4, 2)                                 # [N, Cin, TH, TW, 4, 4]
    Bt, G = WINO_BT.to(dt), WINO_G.to(dt)
    V = torch.einsum("ar,nchwrs,bs->abcnhw", Bt, d, Bt).reshape(16, g.Cin, -1)
    k = w.to(dt)
    if g.transposed:
        k = k.flip(2, 3)
    Uw = torch.einsum("ap,oipq,bq->aboi", G, k, G).reshape(16, g.Cout, g.Cin)
    return Uw, V


def acc32_wino(x, w, c, fault=None):
    """F(2x2, 3x3) in float32: float32 transforms, one serial channel chain per transform point, float32 output
    transform"""
    g = c["g"]
    Uw, V = wino_domain(x, w, c, torch.float32)
    M = torch.zeros((16, g.Cout, V.shape[2]), dtype=torch.float32)
    for ch in range(g.Cin):
        if fault == "channel" and ch == g.Cin - 1:
            continue
        M += Uw[:, :, ch, None] * V[:, None, ch, :]
    TH, TW = cdiv(g.H, 2), cdiv(g.W, 2)
    M = M.reshape(4, 4, g.Cout, g.N, TH, TW)
    if fault == "tap":                                                     # one transform point of one tile block
        M[3, 3, :, 0, :4, :4] = 0
    At = WINO_AT.float()
    Y = torch.einsum("ia,abonhw,jb->nohiwj", At, M, At).reshape(g.N, g.Cout, 2 * TH, 2 * TW)[:, :, :g.H, :g.W].contiguous()
    if fault == "pixel":
        Y[0, :, min(1, g.H - 1), min(1, g.W - 1)] = Y[0, :, min(1, g.H - 1), 0]
    return Y


def wino_headroom(c, t=None):
    """largest transform-domain sum of a Winograd launch in units of 1/4: 4 * max_xi sum_ci |U| |V| (grid: U is a multiple
    of 1/4, V an integer); the output transform adds at most 9 such sums"""
    t = t or make_inputs(c)
    Uw, V = wino_domain(t["x"], t["w"], c, F64)
    return 4.0 * 9.0 * torch.einsum("aoi,aip->aop", Uw.abs(), V.abs()).max().item()


def summation_order(p):
    """the order of acc32_direct for a direct plan"""
    if p.family == KS8:
        return ("ks8",)
    if p.family == STAGED and ROWS[p.row][4] > 1:
        return ("ks", ROWS[p.row][4], p.ckm)
    return ("serial",)


def acc32(c, p, fault=None):
    """float32 restatement of the accumulator of case c under plan p, or under the plans of its classes (cached:
    read-only)"""
    t = make_inputs(c)
    ps = p if isinstance(p, (list, tuple)) and not isinstance(p, Plan) else [p] * (c["g"].stride ** 2 if c["g"].transposed else 1)
    order = ("wino",) if c["algo"] == WINOGRAD else tuple(summation_order(q) for q in ps)
    k = (ckey(c), order, fault)
    if k not in _ACC32:
        _ACC32[k] = acc32_wino(t["x"], t["w"], c, fault) if c["algo"] == WINOGRAD else acc32_direct(t["x"], t["w"], c, order, fault)
    return _ACC32[k]


def operand_floor(c, t):
    """erf_bf's absolute error of a GELU operand carried through the sum: sum |w| * 0.5 |x| * 5.8e-8 per accumulator"""
    if c["pro_act"] != GELU:
        return 0.0
    g = c["g"]
    E = tap_operands(PR.gelu_floor(t["x"].double()[:, channel_planes(c)]), g)
    return torch.einsum("oit,nitp->nop", t["w"].double().abs().reshape(g.Cout, g.Cin, -1), E).max().item()


Limits = namedtuple("Limits", "y y2 e32_y e32_y2 acc")


def limits(c, a32, t=None, ref=None):
    """the limit of y and of y2 (None where the call writes none) from the float32 restatement a32 of the accumulator;
    also ref32's own errors and the accumulator's limit.  `grid` with an exact accumulator: pass a32 = acc64.float()."""
    t = t or make_inputs(c)
    o64, acc64, _ = ref or conv64(c, t)
    o32 = epilogue(a32, c, t, FN32)
    acc_lim = FACTOR * (a32.double() - acc64).abs().max().item() + FACTOR * U * acc64.abs().max().item() + operand_floor(c, t)
    if c["inputs"] == "grid" and c["pro_act"] != GELU:
        assert torch.equal(a32.double(), acc64)
        acc_lim = 0.0
    e = c["epi"]
    v64 = (shuffle2(acc64) if c["ps"] == 2 else acc64)
    if c["bias"]:
        b = t["bias"].double().view(1, -1, 1, 1).expand_as(acc64)
        v64 = v64 + (shuffle2(b) if c["ps"] == 2 else b)
    res, aux = t["res"].double(), t["aux"].double()
    zero = torch.zeros_like(v64)
    fy, fs = zero + acc_lim, None                                   # linear kinds: the accumulator's limit itself
    if e == E_RES_GELU:
        fy = acc_lim + PR.gelu_floor(res)
    elif e == E_GDN:
        fs = zero + acc_lim
        fy = aux.abs() * (2 * ULP * torch.rsqrt(v64) + 0.5 * v64 ** -1.5 * acc_lim)
    elif e == E_IGDN:
        fs = zero + acc_lim
        fy = aux.abs() * (2 * ULP * torch.sqrt(v64) + 0.5 * v64 ** -0.5 * acc_lim)
    elif e == E_MUL_DGELU:
        fy = v64.abs() * PR.dgelu_floor(aux) + PR.dgelu(aux).abs() * acc_lim
    elif e == E_RES_MUL_DGELU:
        fy = (v64 + res).abs() * PR.dgelu_floor(aux) + PR.dgelu(aux).abs() * acc_lim
    elif e == E_AXPY2:
        fy = (2 * aux).abs() * acc_lim
    elif e == E_LRP:
        th = torch.tanh(v64)
        fs = 2 * ULP * th.abs() + (1 - th * th) * acc_lim
        fy = 0.5 * fs
    f2 = fs
    if c["y2"] != "none" and may_gelu(e):                           # gelu(v): floor at v, the value's floor through gelu'
        fg = PR.gelu_floor(o64.v) + PR.dgelu(o64.v).abs() * fy
        if c["y2"] == "same":
            fy = fg
        else:
            f2 = fg

    def lim(r32, r64, fl):
        e32 = (r32.double() - r64).abs().max().item()
        return FACTOR * e32 + FACTOR * U * r64.abs().max().item() + fl.max().item(), e32
    ly, ey = lim(o32.y, o64.y, fy)
    l2, e2 = lim(o32.y2, o64.y2, f2) if o64.y2 is not None else (None, None)
    return Limits(ly, l2, ey, e2, acc_lim)


def exact_on_grid(c):
    """(y exact, y2 exact): bit equality expected on `grid`"""
    if c["inputs"] != "grid" or c["pro_act"] == GELU:
        return False, False
    y = c["epi"] in EPI_EXACT and c["y2"] != "same"
    y2 = c["epi"] in (E_GDN, E_IGDN)
    return y, y2


def grid_headroom(c, t=None):
    """largest magnitude a partial sum of a `grid` launch can reach (Winograd: in units of 1/4); must stay below 2^24"""
    t = t or make_inputs(c)
    _, _, ab = conv64(c, t)
    m = ab.max().item() + 2 + (2 if c["accum"] else 0)
    if c["epi"] == E_AXPY2:
        m = 4 * m + 2
    if c["algo"] == WINOGRAD:
        m = max(m, wino_headroom(c, t))
    return m


# ================================================================================================ the planner (host code)
def _L():
    from icm_amd import _lib as L
    return L


def batch_stride(C, plane, kind):
    """natural; + 4 planes (a channel slice of a wider buffer, alignment kept); + 2 floats (16-byte paths off)"""
    return C * plane + {"natural": 0, "slice": 4 * plane, "odd": 2}[kind]


def strides_of(c):
    g = c["g"]
    osh = out_shape(c)
    oc, opl = osh[1], osh[2] * osh[3]
    s = {"x": batch_stride(phys_channels(c), g.H * g.W, c["strides"].get("x", "natural"))}
    for name in ("y", "res", "aux", "aux2", "y2"):
        s[name] = batch_stride(oc, opl, c["strides"].get(name, "natural"))
    if c["y2"] == "same":
        s["y2"] = s["y"]
    return s


def reads(epi):
    return {"res": epi in (E_RES, E_RES_GELU, E_RES_MUL_DGELU),
            "aux": epi in (E_GDN, E_IGDN, E_MUL_DGELU, E_AXPY2, E_LRP, E_RES_MUL_DGELU), "aux2": epi == E_AXPY2}


def conv_args(c, ptrs=None):
    """icm_conv_args of a case; ptrs = dict of device addresses (the planner looks at null-ness and alignment only)"""
    g = c["g"]
    s = strides_of(c)
    a = _L().ConvArgs()
    rd = reads(c["epi"])
    p = ptrs or {"x": 64 + 4 * c["x_off"], "wp": 64, "y": 64, "bias": 64 if c["bias"] else 0,
                 "res": 64 if rd["res"] else 0, "aux": 64 if rd["aux"] else 0, "aux2": 64 if rd["aux2"] else 0,
                 "y2": 0 if c["y2"] == "none" else (64 if c["y2"] == "same" else 128), "xv": 64 if c["xv"] else 0}
    a.x, a.x_bs, a.N, a.Cin, a.H, a.W = p["x"], s["x"], g.N, g.Cin, g.H, g.W
    a.wp, a.bias, a.y, a.y_bs, a.Cout, a.OH, a.OW = p["wp"], p["bias"], p["y"], s["y"], g.Cout, g.OH, g.OW
    a.KH, a.KW, a.stride, a.pad, a.transposed = g.KH, g.KW, g.stride, g.pad, g.transposed
    a.pro_act, a.epi = c["pro_act"], c["epi"]
    a.res, a.res_bs, a.aux, a.aux_bs, a.aux2, a.aux2_bs = p["res"], s["res"], p["aux"], s["aux"], p["aux2"], s["aux2"]
    a.y2, a.y2_bs, a.accum, a.pixel_shuffle = p["y2"], s["y2"], c["accum"], c["ps"]
    a.x_seg_len, a.x_seg_gap = c["seg"] if c["seg"] else (0, 0)
    a.algo, a.xv = c["algo"], p["xv"]
    return a


Plan = namedtuple("Plan", "rc classes family row lgTW lgTH lgTI ckm ncb nblk lds block vec4 dma off")


class forced:
    """icm_debug_force_conv_cfg / icm_debug_force_conv1x1 for the duration of a with block"""

    def __init__(self, cfg=CFG_AUTO, f1x1=-1):
        self.cfg, self.f1x1 = cfg, f1x1

    def __enter__(self):
        L = _L().lib()
        L.icm_debug_force_conv_cfg(self.cfg)
        L.icm_debug_force_conv1x1(self.f1x1)

    def __exit__(self, *exc):
        L = _L().lib()
        L.icm_debug_force_conv_cfg(CFG_AUTO)
        L.icm_debug_force_conv1x1(-1)


def plan_args(a, ngroups=1, cls=0, cfg=CFG_AUTO, f1x1=-1):
    arr = (_L().ConvArgs * max(1, ngroups))(*([a] * max(1, ngroups)))
    out = (ctypes.c_int64 * 16)()
    with forced(cfg, f1x1):
        rc = _L().lib().icm_debug_conv_plan(arr, ngroups, cls, out)
    return Plan(rc, *list(out)[:14])


def plan_array(args, n, cfg=CFG_AUTO, f1x1=-1):
    """icm_debug_conv_plan's code for an array of member arguments (class 0)"""
    arr = (_L().ConvArgs * len(args))(*args)
    out = (ctypes.c_int64 * 16)()
    with forced(cfg, f1x1):
        return _L().lib().icm_debug_conv_plan(arr, n, 0, out)


def plan(c, ngroups=None, cls=0):
    """icm_debug_conv_plan of a case (of c["ngroups"] members unless said) under its forced configuration.  Winograd plans: row = co tiles per workgroup,
    lgTW / lgTH = lgTX / lgTY, ckm = nsteps, vec4 = vpre, dma = px_fast"""
    return plan_args(conv_args(c), c["ngroups"] if ngroups is None else ngroups, cls, c["cfg"], c["f1x1"])


def class_plans(c, ngroups=None):
    n = len(build_classes(c["g"]))
    return [plan(c, ngroups, k) for k in range(n)] if c["algo"] == DIRECT else [plan(c, ngroups, 0)]


def trips(c, p, cls=0):
    """staging trips of a direct plan: ceil(8-channel groups / ckm)"""
    return cdiv(cdiv(c["g"].Cin, 8), max(1, p.ckm))


# ---- predicates: the conditions of the planner, restated
def patch(c, p, cls=0):
    """(TW, TH, TI, PW, PH, PWrow, PP, CS) of a staged / K-split plan (make_geometry)"""
    g = c["g"]
    cl = build_classes(g)[cls]
    S = 1 if g.transposed else g.stride
    TW, TH, TI = 1 << p.lgTW, 1 << p.lgTH, 1 << p.lgTI
    PW, PH = (TW - 1) * S + cl.ex, (TH - 1) * S + cl.ey
    PWrow = 2 * ((PW + 1) // 2) if S == 2 else PW
    return TW, TH, TI, PW, PH, PWrow, PH * PWrow, TI * PH * PWrow


def vec4_conditions(c, p, cls=0):
    """every condition of the 16-byte halo-free staging (plan_class), by name"""
    g = c["g"]
    cl = build_classes(g)[cls]
    S = 1 if g.transposed else g.stride
    TW, TH, TI, PW, PH, PWrow, PP, CS = patch(c, p, cls)
    return {"stride-1 sampling": S == 1, "one tap": cl.ex == 1 and cl.ey == 1 and cl.ix0 == 0, "PW % 4": PW % 4 == 0,
            "TW % 4": TW % 4 == 0, "W % 4": g.W % 4 == 0, "x_bs % 4": strides_of(c)["x"] % 4 == 0,
            "H*W % 4": (g.H * g.W) % 4 == 0, "plane4": TI * PH * (PW // 4) <= 256,
            "patch % 4": CS % 4 == 0 and PWrow % 4 == 0 and PP % 4 == 0, "x aligned": c["x_off"] % 4 == 0,
            "no channel map": not c["seg"]}


def dma_conditions(c, p, cls=0):
    g = c["g"]
    S = 1 if g.transposed else g.stride
    TW, TH, TI, PW, PH, PWrow, PP, CS = patch(c, p, cls)
    return {"not vec4": not all(vec4_conditions(c, p, cls).values()), "stride-1 sampling": S == 1,
            "no activation": c["pro_act"] == NONE, "linear patch": PWrow == PW and PP == PH * PW}


def staging_form(c, p, cls=0):
    """("vec4" | "dma" | "planes", the conditions that knock the better forms out)"""
    v, d = vec4_conditions(c, p, cls), dma_conditions(c, p, cls)
    if all(v.values()):
        return "vec4", []
    if all(d.values()):
        return "dma", [k for k, ok in v.items() if not ok]
    return "planes", [k for k, ok in d.items() if not ok]


def pointwise_eligible(c):
    """plan_class + plan_conv1x1: the launch may take the barrier-free pointwise kernel"""
    g = c["g"]
    cl = build_classes(g)[0]
    return (g.KH == 1 and g.KW == 1 and g.stride == 1 and g.pad == 0 and not c["ps"] and g.Cin % 8 == 0 and g.OH == g.H and
            g.OW == g.W and not c["seg"] and c["cfg"] == CFG_AUTO and c["f1x1"] != 0 and c["algo"] == DIRECT and
            cl.iy0 == 0 and cl.ix0 == 0)


def pointwise_row(g, ngroups=1):
    """plan_conv1x1's score restated: (row, waves) -- no padded co tiles if avoidable, then min(waves, 2048) * eff, ties to
    the earlier row"""
    ncot, NP = cdiv(g.Cout, 32), g.N * g.H * g.W
    best_pad = min(cdiv(ncot, t) * t for t, _ in ROWS_1X1)
    best, score = -1, -1.0
    for i, (tco, tpx) in enumerate(ROWS_1X1):
        if cdiv(ncot, tco) * tco != best_pad:
            continue
        waves = cdiv(NP, 32 * tpx) * cdiv(ncot, tco) * ngroups
        s = np.float32(min(waves, 2048)) * np.float32(EFF_1X1[i])
        if s > score:
            best, score = i, s
    tco, tpx = ROWS_1X1[best]
    return best, cdiv(NP, 32 * tpx) * cdiv(ncot, tco) * ngroups


def pointwise_auto(g, ngroups=1):
    """the automatic threshold: >= 1024 waves (512 for Cin <= 384)"""
    return pointwise_row(g, ngroups)[1] >= (512 if g.Cin <= 384 else 1024)


def ks8_admits(c):
    """plan_ks8's argument conditions (its geometry conditions are the planner's own)"""
    g = c["g"]
    S = 1 if g.transposed else g.stride
    return S == 1 and c["pro_act"] == NONE and c["epi"] in EPI_KS8 and not c["seg"]


def wino_supported(c):
    g = c["g"]
    return (g.KH == 3 and g.KW == 3 and g.stride == 1 and g.pad == 1 and not c["ps"] and g.OH == g.H and g.OW == g.W and
            c["epi"] in EPI_WINO)


def wino_plan_expect(c, ngroups=1):
    """plan_conv_wino restated: (family, tco, px_fast, co blocks, workgroups)"""
    g = c["g"]
    tw, th = cdiv(g.W, 2), cdiv(g.H, 2)
    lgTX = min(3, clog2(tw))
    lgTY = min(5 - lgTX, clog2(th))
    lgTI = 5 - lgTX - lgTY
    pblocks = cdiv(tw, 1 << lgTX) * cdiv(th, 1 << lgTY) * cdiv(g.N, 1 << lgTI)
    ncot = cdiv(g.Cout, 32)
    b2, b1 = pblocks * cdiv(ncot, 2) * ngroups, pblocks * ncot * ngroups
    tco = 1 if (ncot == 1 or math.ceil(b1 / 256.0) * 1.08 < math.ceil(b2 / 256.0) * 2.0) else 2
    w8 = bool(c["xv"])
    if w8:
        t8, bestc = 2, 1e300
        for t in (4, 3, 2):
            cst = math.ceil(pblocks * cdiv(ncot, t) * ngroups / 256.0) * (t + 0.6)
            if cst < bestc - 1e-9:
                bestc, t8 = cst, t
        if pblocks * cdiv(ncot, t8) * ngroups >= 150:
            tco = t8
        else:
            w8 = False
    wbytes, abytes = 64.0 * g.Cin * g.Cout, 4.0 * g.Cin * g.N * g.H * g.W
    px_fast = int(wbytes > 3.0e6 and wbytes > abytes)
    return (WINO8 if w8 else WINO44), tco, px_fast, cdiv(ncot, tco), pblocks * cdiv(ncot, tco)


def wino_transform_vec(g):
    """run_wino_transform: the 16-byte row form of the input transform"""
    return g.W % 2 == 0 and g.W >= 4


def int32_guard_refuses(g, x_bs):
    """validate(): PlaneMap byte offsets are int32"""
    return (g.N * x_bs + 8 * g.H * g.W) * 4 >= 2 ** 31


# ================================================================================================ case tables
K_ONE_TRIP = [(1, 1, 0), (3, 1, 1), (3, 1, 0), (3, 1, 2), (3, 2, 1), (5, 1, 2), (5, 2, 2), (2, 2, 0), ((1, 3), 1, 1),
              ((3, 5), 1, 1), (4, 1, 1), ((4, 8), 1, 2)]
ONE_TRIP = [geom(3, 11, 13, k, s, p, tr) for k, s, p in K_ONE_TRIP for tr in (0, 1)]
REFUSED_KERNEL = geom(2, 6, 6, 6, 1, 2)                       # 36 taps
G1, G3, G5T = geom(3, 11, 13, 1, 1, 0), geom(3, 11, 13, 3, 1, 1), geom(3, 11, 13, 5, 2, 2, 1)
# 3x3 stride 1 pad 1 as a scatter with H = OH: validate() has no consistency check for a scatter, and the same numbers are a
# valid gather too, so a member that differs from it in ONE field is still valid on its own (the refusal is check_group's)
G3T = geom(3, 11, 13, 3, 1, 1, 1, HW=(11, 13))
G3S2, G5S2 = geom(3, 11, 13, 3, 2, 1), geom(3, 11, 13, 5, 2, 2)
# transposed stride 2: all four classes; even (2H) and odd (2H - 1) output sizes; OH = 1 (the cy = 1 classes are empty)
TRANSPOSED_S2 = [geom(2, oh, ow, k, 2, p, 1, HW=hw) for k, p in ((5, 2), (3, 1), (2, 0))
                 for oh, ow, hw in ((12, 14, (6, 7)), (11, 13, (6, 7)), (1, 13, (1, 7)))]
TINY = [geom(5, 4, 4, 3, 1, 1), geom(9, 2, 2, 3, 1, 1), geom(33, 1, 1, 3, 1, 1), geom(9, 2, 2, 1, 1, 0),
        geom(5, 4, 4, 5, 2, 2, 1, HW=(2, 2))]
# a finding, not a bug: the smallest pixel tile is 32 pixels, on a 1x1 output map 32 images whatever N is, and 32 patches
# of 5x5 exceed the staging plane map (ICM_MAXJ * 64 = 768 elements) under every row: a 5x5 kernel with a 1x1 output map
# is refused as unsupported (3x3: 288 elements, accepted)
TINY_REFUSED = geom(33, 1, 1, 5, 1, 2)
BLOCKS = [geom(2, 19, 37, 3, 1, 1, ch=(24, 200)), geom(2, 19, 37, 1, 1, 0, ch=(24, 200)),
          geom(2, 19, 37, 5, 2, 2, 1, ch=(24, 200), HW=(10, 19))]
PS_G = geom(3, 11, 13, 3, 1, 1, ch=(24, 40))


@functools.lru_cache(maxsize=None)
def multi_trip_geom(k, cfg=CFG_AUTO):
    """smallest Cin (a ragged last 8-channel group, a ragged last staged chunk) that gives >= 3 staging trips under the ckm
    the planner reports, on an 8x7 map"""
    for n8 in range(3, 200):
        g = geom(2, 8, 7, k, 1, k // 2, ch=(8 * n8 - 4, 24))
        p = plan(case("probe", g, cfg=cfg))
        if p.rc == OK and p.family != P1 and cdiv(n8, p.ckm) >= 3 and n8 % p.ckm:
            return g
    raise AssertionError("no multi-trip Cin for k = %d" % k)


def forced_configs():
    return list(range(NROWS)) + [CFG_KS8_64, CFG_KS8_128]


def cfg_name(cfg):
    return {CFG_AUTO: "auto", CFG_KS8_64: "ks8-64x64", CFG_KS8_128: "ks8-32x128"}.get(cfg, "row%d" % cfg)


def forced_row_geoms():
    return [G3, G3S2, G5S2, G5T, multi_trip_geom(3)]


def forced_row_table():
    """every staged row and both K-split blocks on the five geometries: (g, cfg, planner's code of class 0)"""
    return [(g, cfg, max(p.rc for p in class_plans(case("probe", g, cfg=cfg)))) for g in forced_row_geoms()
            for cfg in forced_configs()]


def other_family_cfgs(c):
    """for a case: one forced configuration of every other direct family that admits it and does not repeat the automatic plan"""
    auto = plan(c)
    out = []
    for cfgs in ((6, 9, 12), (CFG_KS8_64,)):
        for cfg in cfgs:
            p = plan(dict(c, cfg=cfg))
            if p.rc == OK and (p.family, p.row) != (auto.family, auto.row):
                out.append(cfg)
                break
    return out


def epi_case_kwargs(epi, pro_act):
    """the operands a kind needs: GDN / IGDN take the SQUARE operand"""
    kw = dict(epi=epi, pro_act=pro_act)
    if epi in (E_GDN, E_IGDN):
        kw["pro_act"] = SQUARE
    return kw


@functools.lru_cache(maxsize=None)
def _cross_cases():
    out = []
    for g, tag in ((G1, "1x1"), (G3, "3x3"), (G5T, "T5x5s2")):
        base = case("probe", g)
        cfgs = [CFG_AUTO] + other_family_cfgs(base)
        if tag == "1x1":
            cfgs.append("p1")                      # the pointwise kernel, forced on (the shape is below its threshold)
        for cf in cfgs:
            fk = dict(f1x1=1) if cf == "p1" else dict(cfg=cf)
            cn = "p1" if cf == "p1" else cfg_name(cf)
            for pa in (NONE, GELU, SQUARE):
                for epi in EPI_ALL:
                    if epi in (E_GDN, E_IGDN) and pa != SQUARE:
                        continue
                    for which in (("real",) if pa == GELU else ("grid", "real")):
                        if which == "real" and pa == SQUARE and epi not in (E_GDN, E_IGDN):
                            continue               # SQUARE is exact on grid; real adds nothing the NONE operand lacks
                        y2 = "sep" if side_kind(epi) else "none"
                        out.append(case("%s-%s-%s-%s-%s" % (tag, cn, ACT_NAMES[pa], EPI_NAMES[epi], which), g, inputs=which,
                                        pro_act=pa, epi=epi, y2=y2, **fk))
            for which in ("grid", "real"):
                out.append(case("%s-%s-nobias-%s" % (tag, cn, which), g, inputs=which, bias=False, **fk))
                out.append(case("%s-%s-accum-%s" % (tag, cn, which), g, inputs=which, accum=1, **fk))
                for y2 in ("sep", "same"):
                    for accum in (0, 1):
                        out.append(case("%s-%s-y2%s-accum%d-%s" % (tag, cn, y2, accum, which), g, inputs=which, y2=y2,
                                        accum=accum, epi=E_RES if accum else E_NONE, **fk))
            for L in (20, 12):
                out.append(case("%s-%s-seg%d" % (tag, cn, L), g, seg=(L, 4), **fk))
            for name in ("x", "y", "res", "aux", "aux2", "y2"):
                for kind in ("slice", "odd"):
                    epi = {"res": E_RES, "aux": E_MUL_DGELU, "aux2": E_AXPY2}.get(name, E_NONE)
                    out.append(case("%s-%s-%s_bs-%s" % (tag, cn, name, kind), g, epi=epi, y2="sep" if name == "y2" else "none",
                                    strides={name: kind}, **fk))
            out.append(case("%s-%s-x-4-bytes-off" % (tag, cn), g, x_off=1, **fk))
        if not g.transposed:
            gp = g._replace(Cin=24, Cout=40)
            for y2 in ("none", "sep"):
                out.append(case("%s-pixel-shuffle-y2%s" % (tag, y2), gp, ps=2, y2=y2, epi=E_RES))
                out.append(case("%s-pixel-shuffle-y2%s-real" % (tag, y2), gp, ps=2, y2=y2, epi=E_RES, inputs="real"))
    return tuple(out)


def cross_cases():
    return [dict(c) for c in _cross_cases()]


# staging forms: each taken in one case and knocked out in a sibling by exactly one of its conditions
VEC_G = geom(2, 8, 16, 1, 1, 0)          # 1x1 on a W = 16 map under a forced staged row
DMA_G = geom(2, 8, 16, 3, 1, 1)


def staging_cases():
    """(case, form, what knocked the better form out: the one condition, the tuple of conditions that go together, or
    None where the better form is taken or was never in reach)"""
    v = dict(cfg=9)
    return [
        (case("vec4-taken", VEC_G, **v), "vec4", None),
        (case("vec4-W%4", geom(2, 8, 18, 1, 1, 0), **v), "dma", "W % 4"),   # W = 18: tile 32 x 4, the patch stays % 4
        (case("vec4-x_bs%4", VEC_G, strides={"x": "odd"}, **v), "dma", "x_bs % 4"),
        (case("vec4-x-4-bytes-off", VEC_G, x_off=1, **v), "dma", "x aligned"),
        (case("vec4-x_seg_len", VEC_G, seg=(20, 4), **v), "dma", "no channel map"),
        (case("vec4-pro_act-stays", VEC_G, pro_act=SQUARE, **v), "vec4", None),
        (case("dma-taken", DMA_G, **v), "dma", None),
        (case("dma-pro_act", DMA_G, pro_act=SQUARE, **v), "planes", "no activation"),
        # stride-2 sampling stores the patch column-parity-split: the linear-patch condition goes with it
        (case("dma-stride-2", geom(2, 8, 16, 3, 2, 1), **v), "planes", ("stride-1 sampling", "linear patch")),
        (case("dma-x_seg_len-stays", DMA_G, seg=(12, 4), **v), "dma", None),
        (case("planes-gelu", DMA_G, pro_act=GELU, inputs="real", **v), "planes", "no activation"),
        (case("dma-1x1-x_bs%4-act", VEC_G, strides={"x": "odd"}, pro_act=SQUARE, **v), "planes", "no activation"),
    ]


# the pointwise kernel: Cin = 8 for the large ones
def pointwise_sweep(ncots=range(1, 25), members=(1, 2, 12), max_lg=20):
    """plan_conv1x1 through icm_debug_conv_plan (forced on): {row: (waves, members, ncot, pixels)} of the cheapest
    geometry that reaches each row"""
    first = {}
    pix = sorted({v for lg in range(5, max_lg + 1) for v in (1 << lg, (1 << lg) + 1, 3 << (lg - 2))} | {189, 64, 96})
    for n in members:
        for ncot in ncots:
            for P in pix:
                g = Geom(1, 8, 32 * ncot, 1, P, 1, P, 1, 1, 1, 0, 0)
                p = plan(case("sweep", g, f1x1=1), n)
                assert p.rc == OK and p.family == P1
                assert p.row == pointwise_row(g, n)[0], (g, n, p.row)
                cost = (P * ncot * n, n, ncot, P)
                if p.row not in first or cost < first[p.row]:
                    first[p.row] = cost
    return first


def pointwise_geom(ncot, pixels, Cin=8):
    """one image of H x 61 >= `pixels` pixels (61: no multiple of a 32-pixel strip), a co tail of 12 channels"""
    H = cdiv(pixels, 61)
    return Geom(1, Cin, 32 * ncot - 12, H, 61, H, 61, 1, 1, 1, 0, 0)


@functools.lru_cache(maxsize=None)
def pointwise_row_cases():
    """{row: (members, geometry)}: for every row plan_conv1x1's score (restated: pointwise_row) can select, the launch with
    the fewest pixels per member that selects it -- members in (1, 2, 12), co tiles 1 - 6, Cin = 8 so that the float64
    reference of the large ones stays cheap.  tests/test_conv_ref.py asks the library whether each lands on its row."""
    out = {}
    for row in range(len(ROWS_1X1)):
        best = None
        for n in (12, 2, 1):
            for ncot in range(1, 7):
                lo, hi = 1, 1 << 21
                if pointwise_row(pointwise_geom(ncot, hi), n)[0] != row and pointwise_row(pointwise_geom(ncot, 64), n)[0] != row:
                    continue
                for H in range(1, 4096):                       # rows change only at saturation: a linear scan suffices
                    g = pointwise_geom(ncot, 61 * H)
                    if pointwise_row(g, n)[0] == row:
                        cand = (g.H * ncot, n, g)
                        if best is None or cand[:2] < best[:2]:
                            best = cand
                        break
        if best:
            out[row] = (best[1], best[2])
    return out


POINTWISE_UNREACHABLE = (7,)            # <2,1>: never wins against row 5 <1,2> (a tie goes to the earlier row)
POINTWISE_CHUNKS = [Geom(3, 8 * n8, 84, 9, 7, 9, 7, 1, 1, 1, 0, 0) for n8 in (1, 3, 40)]


WINO_GEOMS = [geom(3, 11, 13, 3, 1, 1), geom(2, 5, 2, 3, 1, 1), geom(2, 5, 3, 3, 1, 1), geom(5, 2, 2, 3, 1, 1),
              geom(2, 6, 8, 3, 1, 1, ch=(4, 24)), geom(2, 6, 8, 3, 1, 1, ch=(24, 40)), geom(2, 7, 9, 3, 1, 1, ch=(40, 72)),
              geom(2, 11, 13, 3, 1, 1, 1, HW=(11, 13)), geom(2, 6, 8, 3, 1, 1, 1, ch=(24, 40), HW=(6, 8))]
WINO_PXFAST_G = geom(1, 4, 4, 3, 1, 1, ch=(224, 224))
# the eight-MFMA-wave kernel wants >= 150 workgroups: 12 members on a 16-wide strip of 104 rows (13 pixel blocks each)
WINO_W8_N = 12
WINO_W8_G = {t: geom(1, 104, 16, 3, 1, 1, ch=(8, 32 * t - 12)) for t in (2, 3, 4)}
W8_CASES = [case("wino8-tco%d-%s" % (t, which), g, inputs=which, algo=WINOGRAD, xv=True, ngroups=WINO_W8_N)
            for t, g in WINO_W8_G.items() for which in ("grid", "real")]
# the eight-wave kernel's own per-image arithmetic and epilogue: 25 images of a 4x16 map, two per tile (13 pixel blocks,
# a batch tail inside the last), every batch stride in a form of its own, the kinds, accum, a null bias, y2 in both forms
WINO_W8_BATCH_G = {t: geom(25, 4, 16, 3, 1, 1, ch=(8, 32 * t - 12)) for t in (2, 3, 4)}
W8_VARIANTS = [("res-slice", dict(epi=E_RES, strides={"x": "slice", "y": "odd", "res": "slice"})),
               ("lrp-y2-odd", dict(epi=E_LRP, y2="sep", strides={"x": "odd", "y": "slice", "aux": "odd"})),
               ("mul_dgelu-aux-slice", dict(epi=E_MUL_DGELU, strides={"aux": "slice"})),
               ("accum-nobias-y2", dict(accum=1, bias=False, y2="sep", strides={"y2": "slice"})),
               ("res_gelu-y2same-accum", dict(epi=E_RES_GELU, y2="same", accum=1, strides={"y": "slice", "res": "odd"}))]
W8_CASES += [case("wino8-tco%d-N25-%s-%s" % (t, vn, which), g, inputs=which, algo=WINOGRAD, xv=True, ngroups=WINO_W8_N, **kw)
             for t, g in WINO_W8_BATCH_G.items() for vn, kw in W8_VARIANTS for which in ("grid", "real")]
# two co tiles per workgroup of the 4 + 4 wave kernel want more than one round of the chip with one co tile each
WINO_TCO2_G = geom(1, 88, 16, 3, 1, 1, ch=(8, 40))
W8_CASES += [case("wino44-tco2-%s-%s" % ("xv" if xv else "raw", which), WINO_TCO2_G, inputs=which, algo=WINOGRAD, xv=xv,
                  ngroups=WINO_W8_N) for xv in (False, True) for which in ("grid", "real")]
# the automatic K-split choice: one nearly full round of the chip (160..256 workgroups of 64 co x 64 px)
KS8_AUTO_N = 12
KS8_AUTO = case("ks8-auto", geom(4, 16, 16, 3, 1, 1, ch=(24, 40)), ngroups=KS8_AUTO_N)


def wino_cases():
    out = []
    for g in WINO_GEOMS:
        for xv in (False, True):
            for which in ("grid", "real"):
                out.append(case("wino-%s-%s-%s" % (gname(g), "xv" if xv else "raw", which), g, inputs=which, algo=WINOGRAD, xv=xv))
    g = WINO_GEOMS[0]
    for xv in (False, True):
        tag = "xv" if xv else "raw"
        for epi in EPI_WINO:
            for which in ("grid", "real"):
                out.append(case("wino-%s-%s-%s" % (tag, EPI_NAMES[epi], which), g, inputs=which, algo=WINOGRAD, xv=xv, epi=epi,
                                y2="sep" if epi == E_LRP else "none"))
        out.append(case("wino-%s-gelu-operand" % tag, g, inputs="real", algo=WINOGRAD, xv=xv, pro_act=GELU))
        out.append(case("wino-%s-square-operand" % tag, g, algo=WINOGRAD, xv=xv, pro_act=SQUARE))
        out.append(case("wino-%s-seg20" % tag, g, algo=WINOGRAD, xv=xv, seg=(20, 4)))
        out.append(case("wino-%s-seg12-square" % tag, g, algo=WINOGRAD, xv=xv, seg=(12, 4), pro_act=SQUARE))
        out.append(case("wino-%s-nobias-accum" % tag, g, algo=WINOGRAD, xv=xv, bias=False, accum=1))
        for y2 in ("sep", "same"):
            out.append(case("wino-%s-y2%s-accum" % (tag, y2), g, algo=WINOGRAD, xv=xv, y2=y2, accum=1, inputs="real"))
        for name in ("x", "y", "res", "aux", "y2"):          # one operand strided, y natural: a wrong stride field shows
            for kind in ("slice", "odd"):
                out.append(case("wino-%s-%s_bs-%s" % (tag, name, kind), g, algo=WINOGRAD, xv=xv, strides={name: kind},
                                epi={"res": E_RES, "aux": E_MUL_DGELU}.get(name, E_NONE), y2="sep" if name == "y2" else "none"))
        out.append(case("wino-%s-x-4-bytes-off" % tag, WINO_GEOMS[5], algo=WINOGRAD, xv=xv, x_off=1))
    for which in ("grid", "real"):
        out.append(case("wino-px_fast-%s" % which, WINO_PXFAST_G, inputs=which, algo=WINOGRAD))
        out.append(case("wino-px_fast-xv-%s" % which, WINO_PXFAST_G, inputs=which, algo=WINOGRAD, xv=True))
    return out


GROUP_NS = [1, 2, 3, 12]
GROUP_GEOMS = [G3, G1, G5T]

INT32_G = geom(2, 8, 8, 3, 1, 1, ch=(8, 24))
INT32_REFUSED_BS = 2 ** 28
INT32_LARGEST_BS = (2 ** 29 - 8 * 8 * 8 - 1) // 2
