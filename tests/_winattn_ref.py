"""Reference, inputs, limit and case list for the window-attention kernels (csrc/winattn.hip, csrc/winattn_mfma.hip).

``core`` is the attention between the qkv and proj Linears in plain torch ops on the kernels' layouts
(include/icm_hip.h: qkv [N][3C][H][W], channel = which*C + head*hd + d; out [N][C][H][W]); it runs in float64 (the
reference, gradients by autograd) and in float32 (the yardstick: ``limit`` is formed from ITS error against float64,
never from a kernel's output).  tests/test_winattn_ref.py checks, without a GPU, that ``core`` restates the oracle and
that the ``hot`` and ``leak`` inputs reach the regimes they are meant to; tests/test_gpu_winattn_numerics.py runs the
kernels on the same cases."""
import collections
import functools

import torch

from oracle import wacnn_oracle as O
from oracle import weights as Wt

FACTOR = 4.0                 # the project's margin for kernel-versus-float32-oracle comparisons
U32 = 2.0 ** -24             # float32 unit roundoff
TENSORS = ("out", "dq", "dk", "dv", "dtable")
ROUTE_VALU, ROUTE_MFMA, ROUTE_MFMA16 = 0, 1, 2
ERR_ARG, ERR_UNSUPPORTED = 1, 3
LEAKS = (60, 100, 140)


def core(qkv, table, heads, ws, shift, want_probs=False):
    """qkv [N,3C,H,W], table [(2ws-1)^2, heads] -> out [N,C,H,W] (and the softmax [windows, heads, T, T])"""
    N, C3, H, W = qkv.shape
    C = C3 // 3
    hd, T = C // heads, ws * ws
    t = qkv.permute(0, 2, 3, 1)
    if shift > 0:
        t = torch.roll(t, shifts=(-shift, -shift), dims=(1, 2))
    win = t.reshape(N, H // ws, ws, W // ws, ws, C3).permute(0, 1, 3, 2, 4, 5).reshape(-1, T, C3)
    Bn = win.shape[0]
    x = win.reshape(Bn, T, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = x[0] * (hd ** -0.5), x[1], x[2]
    attn = q @ k.transpose(-2, -1)
    idx = O.relative_position_index(ws).reshape(-1)
    attn = attn + table[idx].reshape(T, T, heads).permute(2, 0, 1).unsqueeze(0)
    if shift > 0:
        mask = O.shift_mask(H, W, ws, shift).to(attn.dtype)
        nW = mask.shape[0]
        attn = (attn.reshape(Bn // nW, nW, heads, T, T) + mask[None, :, None]).reshape(-1, heads, T, T)
    p = torch.softmax(attn, dim=-1)
    o = (p @ v).transpose(1, 2).reshape(Bn, T, C)
    o = o.reshape(N, H // ws, W // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(N, H, W, C)
    if shift > 0:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    o = o.permute(0, 3, 1, 2).contiguous()
    return (o, p) if want_probs else o


def evaluate(qkv, table, dout, heads, ws, shift, dtype):
    """out, dq, dk, dv, dtable of ``core`` evaluated in ``dtype`` (gradients by autograd against ``dout``)"""
    q = qkv.to(dtype).clone().requires_grad_(True)
    t = table.to(dtype).clone().requires_grad_(True)
    out = core(q, t, heads, ws, shift)
    gq, gt = torch.autograd.grad(out, (q, t), dout.to(dtype))
    C = out.shape[1]
    return {"out": out.detach(), "dq": gq[:, :C], "dk": gq[:, C:2 * C], "dv": gq[:, 2 * C:], "dtable": gt}


def limit(x32, x64, fallback_scale=0.0):
    """FACTOR * the float32 evaluation's own error + FACTOR * unit roundoff * the tensor's scale"""
    scale = x64.abs().max().item()
    if scale == 0.0:
        scale = fallback_scale
    return FACTOR * (x32.double() - x64).abs().max().item() + FACTOR * U32 * scale


# ------------------------------------------------------------------------------------------------ cases
# route = (forward, backward): what icm_debug_winattn_route must report (a negative entry: the call refuses)
Case = collections.namedtuple("Case", "name N heads hd H W ws shift force route")


def _c(name, N, heads, hd, H, W, ws, shift, force=0, route=None):
    if route is None:
        r = ROUTE_VALU if force else {8: ROUTE_MFMA, 4: ROUTE_MFMA16}.get(ws, ROUTE_VALU)
        route = (r, r)
    return Case(name, N, heads, hd, H, W, ws, shift, force, route)


V = (ROUTE_VALU, ROUTE_VALU)
MATRIX = [
    # matrix cores, 8x8 windows: 1, 3, 5, 9, 13 windows (no multiple of the 8 XCDs); heads 5 wraps the four waves
    _c("mfma8-hd8", 1, 5, 8, 8, 8, 8, 0),
    _c("mfma8-hd16", 1, 3, 16, 8, 24, 8, 1),                # H == ws with a shift
    _c("mfma8-hd24", 1, 2, 24, 40, 8, 8, 4),
    _c("mfma8-hd32", 1, 1, 32, 24, 24, 8, 7),
    # the backward of head dim 48 needs 210 KB of LDS: the forward is the matrix cores', the backward the VALU kernel's
    _c("mfma8-hd48", 1, 2, 48, 8, 104, 8, 4, route=(ROUTE_MFMA, ROUTE_VALU)),
    # matrix cores, 4x4 windows: 1, 2, 3, 5, 8 windows per row (group of four, ragged last group); wave tasks
    # heads * N * rows * groups = 2, 9, 10, 6, 2
    _c("mfma4-hd8", 1, 1, 8, 8, 4, 4, 0),
    _c("mfma4-hd16", 3, 3, 16, 4, 8, 4, 1),
    _c("mfma4-hd24", 1, 5, 24, 8, 12, 4, 2),
    _c("mfma4-hd32", 3, 1, 32, 4, 20, 4, 3),
    _c("mfma4-hd40", 1, 1, 40, 4, 32, 4, 1),
    # VALU, 8x8 windows: the live path for head dims the matrix cores do not take, forced for the others
    _c("valu8-hd10", 1, 3, 10, 8, 16, 8, 3, route=V),
    _c("valu8-hd40", 1, 2, 40, 16, 8, 8, 0, route=V),
    _c("valu8-hd8-forced", 1, 5, 8, 8, 8, 8, 5, force=1),
    _c("valu8-hd16-forced", 1, 1, 16, 8, 16, 8, 0, force=1),
    _c("valu8-hd24-forced", 1, 2, 24, 16, 16, 8, 2, force=1),
    _c("valu8-hd32-forced", 1, 3, 32, 8, 8, 8, 6, force=1),
    # VALU, 4x4 windows, four heads per wave: heads = 5 leaves the second wave one head
    _c("valu4-hd10", 1, 5, 10, 8, 8, 4, 1, route=V),
    _c("valu4-hd48", 1, 2, 48, 4, 12, 4, 0, route=V),
    _c("valu4-hd8-forced", 1, 5, 8, 4, 4, 4, 2, force=1),
    _c("valu4-hd16-forced", 1, 3, 16, 8, 4, 4, 3, force=1),
    _c("valu4-hd24-forced", 1, 1, 24, 4, 8, 4, 0, force=1),
    _c("valu4-hd32-forced", 1, 2, 32, 8, 8, 4, 1, force=1),
    _c("valu4-hd40-forced", 1, 5, 40, 4, 4, 4, 2, force=1),
    # VALU, every other window size: 64 / T heads per wave, idle lanes for T = 9, 25, 36, 49
    _c("valu1-hd8", 1, 2, 8, 3, 5, 1, 0),
    _c("valu2-hd8", 1, 5, 8, 4, 6, 2, 1),
    _c("valu3-hd8", 1, 2, 8, 6, 9, 3, 2),
    _c("valu5-hd8", 1, 3, 8, 10, 5, 5, 2),
    _c("valu6-hd8", 1, 2, 8, 6, 12, 6, 5),
    _c("valu7-hd8", 1, 3, 8, 7, 14, 7, 3),
    _c("valu5-hd10", 1, 1, 10, 5, 10, 5, 4),
    _c("valu7-hd16", 1, 2, 16, 14, 7, 7, 0),
    _c("valu2-hd48", 1, 3, 48, 4, 4, 2, 1),
]
# 8x8 windows, head dim 48, five heads, VALU forced: four forward waves need 164 864 bytes of LDS (over the 160 KB a
# workgroup may ask for), the two backward waves 107 008
LDS_CASE = _c("valu8-hd48-forced", 1, 5, 48, 8, 8, 8, 3, force=1, route=(-ERR_UNSUPPORTED, ROUTE_VALU))
# table-gradient reduction plans (heads 1, head dim 8): S = 2 with a ragged last chunk; the capped S on each route
REDUCTION = [
    _c("reduce-valu-33win", 1, 1, 8, 6, 22, 2, 0),
    _c("reduce-valu-1056win", 1, 1, 8, 64, 66, 2, 0),
    _c("reduce-mfma8-289win", 1, 1, 8, 136, 136, 8, 0),
    _c("reduce-mfma4-288slabs", 1, 1, 8, 128, 144, 4, 0),
]
# one row per route for the leak(60) / leak(140) sets, the backward contract and the repeatability check
PER_ROUTE = ("mfma8-hd16", "mfma4-hd24", "valu5-hd8")
BY_NAME = {c.name: c for c in MATRIX + [LDS_CASE] + REDUCTION}


def geometry(case):
    """the argument tail of the C ABI: N, C, H, W, heads, ws, shift"""
    return case.N, case.heads * case.hd, case.H, case.W, case.heads, case.ws, case.shift


def input_sets(case):
    sets = ["mild", "hot"]
    if case.shift > 0:
        sets.append("leak100")
        if case.name in PER_ROUTE:
            sets += ["leak60", "leak140"]
    return sets


def reduction_plan(slabs):
    """S, chunk of the table-gradient reduction over ``slabs`` slabs (csrc/winattn.hip, dtable_chunks)"""
    S = max(1, min(64, slabs // 16))
    chunk = -(-slabs // S)
    return -(-slabs // chunk), chunk


# ------------------------------------------------------------------------------------------------ inputs
def region_code(H, W, shift):
    """[H, W] int64 in the image frame: bit 1 = the pixel lies in the last ``shift`` rows of the ROLLED frame, bit 0
    the same for columns.  Tokens of one window carry different shift-mask labels exactly when their codes differ."""
    r = (torch.arange(H) >= H - shift).long()
    c = (torch.arange(W) >= W - shift).long()
    code = 2 * r[:, None] + c[None, :]
    return torch.roll(code, shifts=(shift, shift), dims=(0, 1))


def inputs(case, kind):
    """float32 qkv, table, dout for one of ``mild``, ``hot``, ``leak<L>``"""
    N, heads, hd, H, W, ws = case.N, case.heads, case.hd, case.H, case.W, case.ws
    C = heads * hd
    key = f"winattn.{case.name}.{kind}"
    qkv = Wt._u(key + ".qkv", (N, 3 * C, H, W), -1.0, 1.0)
    table = Wt._u(key + ".table", ((2 * ws - 1) ** 2, heads), -0.5, 0.5)
    dout = Wt._u(key + ".dout", (N, C, H, W), -1.0, 1.0)
    if kind == "hot":
        # logit = hd^-1/2 sum_d q_d k_d with q, k uniform in +-a: standard deviation a^2 / 3 = 6
        a = (3.0 * 6.0) ** 0.5
        qkv[:, :2 * C] *= a
        table = table * 8.0
    elif kind.startswith("leak"):
        assert case.shift > 0 and hd >= 4
        L = float(kind[4:])
        amp = (L * hd ** 0.5) ** 0.5            # hd^-1/2 * amp^2 = L
        onehot = torch.nn.functional.one_hot(region_code(H, W, case.shift), 4).permute(2, 0, 1).float()   # [4,H,W]
        q = qkv[:, :C].reshape(N, heads, hd, H, W)
        k = qkv[:, C:2 * C].reshape(N, heads, hd, H, W)
        q[:, :, :4] -= amp * onehot
        k[:, :, :4] += amp * onehot
    elif kind != "mild":
        raise KeyError(kind)
    return qkv.contiguous(), table.contiguous(), dout


Ref = collections.namedtuple("Ref", "qkv table dout x64 x32 lim")


@functools.lru_cache(maxsize=None)
def reference(name, kind):
    """inputs, float64 reference, float32 evaluation and the per-tensor limits of one (case, input set); computed once
    and shared -- callers must not write to it"""
    case = BY_NAME[name]
    qkv, table, dout = inputs(case, kind)
    x64 = evaluate(qkv, table, dout, case.heads, case.ws, case.shift, torch.float64)
    x32 = evaluate(qkv, table, dout, case.heads, case.ws, case.shift, torch.float32)
    fb = max(x64[t].abs().max().item() for t in ("dq", "dk", "dv"))
    lim = {t: limit(x32[t], x64[t], fb) for t in TENSORS}
    return Ref(qkv, table, dout, x64, x32, lim)


def oracle_error(ref):
    return {t: (ref.x32[t].double() - ref.x64[t]).abs().max().item() for t in TENSORS}


def probabilities(case, kind):
    """float64 softmax [windows, heads, T, T] and, for shift > 0, the mask of suppressed keys [windows, T, T]"""
    qkv, table, _ = inputs(case, kind)
    _, p = core(qkv.double(), table.double(), case.heads, case.ws, case.shift, want_probs=True)
    masked = None
    if case.shift > 0:
        m = O.shift_mask(case.H, case.W, case.ws, case.shift) != 0
        masked = m.repeat(case.N, 1, 1)
    return p, masked
