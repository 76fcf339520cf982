"""Graph table, float64 mirror, inputs and limit rule of the engine-graph numerics tests (tests/test_engine_ref.py on
the CPU, tests/test_gpu_engine_graphs.py on the GPU).

What is under test is the layer ABOVE the kernels: icm_amd/engine.py's Tape and op wrappers, i.e. which buffer a gradient
lands in, whether a launch overwrites or accumulates, whether an identity-path gradient rides on a dgrad epilogue, private
buffers of grouped launches, and how weight-gradient problems are batched.  Every graph of GRAPHS is a pair
    build(tape, T, o)   the engine calls on device tensors T (o: gelu on / off, the engine module, act_out)
    mirror(m, T, o)     the same computation in plain torch ops (m: the op set M below) on CPU tensors of m's dtype
and the reference is torch autograd on the mirror in float64: the gradient of sum_k <out_k, g_k> for one fixed upstream
gradient g_k per output, with respect to every leaf (data and parameters alike).

Two input sets (oracle/weights.py's named generator, as tests/_conv_ref.py)
  grid: data and upstream gradients integers in [-2, 2], weights in {-1, 0, 1}, biases integers in [-2, 2].  Only graphs of
        exact operations have a grid form (o.gelu False: every virtual activation is NONE, the wiring is the same).  Every
        value, gradient and partial sum is an integer below 2^24 (tests/test_engine_ref.py proves it on the mirror run on
        |inputs|, |weights|; the Winograd transforms make multiples of 1/4, hence the factor 4 there), so the GPU must
        return mirror(...).float() BIT FOR BIT under any tiling, split, Winograd form, flush timing or stream, and a
        bookkeeping error is a whole-integer difference.
  real: uniform [-1, 1) (GDN parameters: |u| + 0.05, above the bound of the non-negative parametrisation, where its
        backward is the derivative).  The only set for GELU, GDN, LayerNorm, tanh and attention.

Limit per tensor on `real` (none of it is taken from a kernel's output)
    |gpu - ref64|_max <= FACTOR * |ref32 - ref64|_max + FACTOR * 2^-24 * |ref64|_max + function floor
  ref32 = the same mirror in float32 on the CPU.  Function floor: the mirror is run again in float64 with every function
  evaluation moved by its whole floor -- gelu by _pointwise_ref.gelu_floor, gelu' (in the backward) by dgelu_floor, the
  rsqrt of LayerNorm, the rsqrt / sqrt of GDN and the tanh of the LRP tail by the 2 ulp _conv_ref.py grants them, each as
  the saved value the backward reuses -- with all signs +, all signs -, and two seeded sign patterns; the floor of a
  tensor is the largest deviation of the four runs from the unperturbed one.  That carries each floor through the actual
  derivative of everything that follows it (forward and backward).  It is a directional carry: never more than the sum
  of absolute path products an analytical bound would grant.

Sizes: N = 2, maps 8x8 (16x16 in front of a stride-2 stage), channels 8 / 16 / 24 / 40 plus one odd pair (5 -> 3),
windows 4x4 with 2 heads, at most three convolutions deep: the smallest at which the paths are taken and at which the
grid sums stay below 2^24."""
import functools
from collections import OrderedDict, namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import _pointwise_ref as PR
import _winattn_ref as WA
from oracle import wacnn_oracle as O
from oracle import weights as W

FACTOR = 4
U = 2.0 ** -24
ULP = 2.0 ** -23
F64, F32 = torch.float64, torch.float32
FD_COORDS, FD_TOL = 8, 1e-6
PERTS = ("+", "-", "r0", "r1")


class NS(dict):
    __getattr__ = dict.__getitem__


# ================================================================================================ mirror op set
class _Gelu(torch.autograd.Function):
    """exact-erf GELU with its own backward, so that the function and its derivative can each be moved by their floor"""

    @staticmethod
    def forward(ctx, x, sf, sd):
        ctx.save_for_backward(x)
        ctx.sd = sd
        y = PR.gelu(x)
        return y if sf is None else y + sf * PR.gelu_floor(x)

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        d = PR.dgelu(x)
        if ctx.sd is not None:
            d = d + ctx.sd * PR.dgelu_floor(x)
        return g * d, None, None


class M:
    """the plain-torch operations a mirror is written in; dtype float64 (reference) or float32 (yardstick).  pert: None,
    or one of PERTS: every function evaluation is moved by its floor times a sign (float64 only)"""

    def __init__(self, dtype=F64, pert=None):
        assert pert is None or dtype == F64
        self.dtype, self.pert, self._n = dtype, pert, 0
        self.ste_record, self.ste_replay, self._k = None, None, 0      # fd_check: see ste_round

    def _sign(self, like):
        if self.pert is None:
            return None
        if self.pert in "+-":
            return 1.0 if self.pert == "+" else -1.0
        self._n += 1
        u = W.uniform01("eg.pert.%s.%d" % (self.pert, self._n), like.numel())
        return torch.from_numpy(np.where(u < 0.5, -1.0, 1.0)).reshape(like.shape)

    def _rel(self, v, ulps=2.0):
        s = self._sign(v)
        return v if s is None else v * (1.0 + s * ulps * ULP)

    # ---- exact operations
    conv = staticmethod(lambda x, w, b=None, stride=1, pad=0: F.conv2d(x, w, b, stride=stride, padding=pad))
    convT = staticmethod(lambda x, w, b=None, stride=1, pad=0, opad=0:
                         F.conv_transpose2d(x, w, b, stride=stride, padding=pad, output_padding=opad))
    ps2 = staticmethod(lambda x: F.pixel_shuffle(x, 2))

    @staticmethod
    def lin(x, w, b=None):
        return F.conv2d(x, w.reshape(w.shape[0], w.shape[1], 1, 1), b)

    # ---- functions
    def gelu(self, x):
        if self.dtype == F32:
            return F.gelu(x)
        return _Gelu.apply(x, self._sign(x), self._sign(x))

    def act(self, x, on):
        return self.gelu(x) if on else x

    def ln(self, x, gamma, beta):
        if self.pert is None:
            return F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), gamma, beta, PR.LN_EPS).permute(0, 3, 1, 2)
        mean = x.mean(1, keepdim=True)
        var = ((x - mean) ** 2).mean(1, keepdim=True)
        rstd = self._rel(torch.rsqrt(var + PR.LN_EPS))
        return (x - mean) * rstd * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)

    def gdn(self, x, beta, gamma, inverse):
        """layers/gdn.py:62-75 with the non-negative parametrisation of both parameters"""
        Cc = x.shape[1]
        norm = F.conv2d(x * x, O.nonneg_param(gamma, 0.0).reshape(Cc, Cc, 1, 1).to(x.dtype),
                        O.nonneg_param(beta, 1e-6).to(x.dtype))
        return x * self._rel(torch.sqrt(norm) if inverse else torch.rsqrt(norm))

    def ste_round(self, x):
        """round(x) with the gradient of the identity (compressai/ops/ops.py:20-34).  The straight-through gradient is by
        definition not the derivative of the staircase: fd_check differentiates the function it IS the derivative of,
        x + (round(x0) - x0) with the offset frozen at the unperturbed point (recorded, then replayed)"""
        if self.ste_replay is not None:
            self._k += 1
            return x + self.ste_replay[self._k - 1]
        if self.ste_record is not None:
            self.ste_record.append((torch.round(x) - x).detach())
        return O.ste_round(x)

    def lrp(self, aux, v):
        return aux + 0.5 * self._rel(torch.tanh(v))

    @staticmethod
    def attn(qkv, table, heads, ws, shift):
        return WA.core(qkv, table, heads, ws, shift)

    def swin_block(self, x, T, p, heads, ws, shift, dp=None):
        """stf.py:149-193 on an NCHW map; dp: None or [2, N] DropPath scales"""
        sc = (lambda v, i: v) if dp is None else (lambda v, i: v * dp[i].view(-1, 1, 1, 1))
        n1 = self.ln(x, T[p + ".norm1.weight"], T[p + ".norm1.bias"])
        o = self.attn(self.lin(n1, T[p + ".attn.qkv.weight"], T[p + ".attn.qkv.bias"]),
                      T[p + ".attn.relative_position_bias_table"], heads, ws, shift)
        x1 = x + sc(self.lin(o, T[p + ".attn.proj.weight"], T[p + ".attn.proj.bias"]), 0)
        n2 = self.ln(x1, T[p + ".norm2.weight"], T[p + ".norm2.bias"])
        h = self.gelu(self.lin(n2, T[p + ".mlp.fc1.weight"], T[p + ".mlp.fc1.bias"]))
        return x1 + sc(self.lin(h, T[p + ".mlp.fc2.weight"], T[p + ".mlp.fc2.bias"]), 1)

    def residual_unit(self, xa, T, p):
        """layers/layers.py:52-72 on the ACTIVATED input xa; returns the pre-activation of the unit's output"""
        u1 = self.conv(xa, T[p + ".conv.0.weight"], T[p + ".conv.0.bias"])
        u2 = self.conv(self.gelu(u1), T[p + ".conv.2.weight"], T[p + ".conv.2.bias"], pad=1)
        return self.conv(self.gelu(u2), T[p + ".conv.4.weight"], T[p + ".conv.4.bias"]) + xa


# ================================================================================================ the table
# tensors: name -> (shape, kind); kind "x" data, "w" weight, "b" bias (all leaves), "pos" a GDN parameter (leaf, real
# only), "q" EntropyBottleneck quantiles (leaf), "k" a constant operand given as a tuple of values and "k:<kind>" a generated
# one (no gradient; "n": quantisation noise in [-0.5, 0.5)).  outs: the outputs that get an upstream
# gradient; free: outputs compared in value only (no upstream gradient: their gout is None).  stops: leaves the build
# stops (tape.stop): grad_of must return None for them.  prebound: leaf -> name of the "x"-kind tensor its gradient
# buffer is pre-filled with (Tape.bind_grad(leaf, value, True)).  grid: the graph has an exact twin.  like: the graph
# whose inputs and upstream gradients this one shares (default: its own).  zero: leaves no output with a gradient depends on
# (autograd: None) but which lie behind a node that writes all its input gradients: the engine owes exact zeros there.
Graph = namedtuple("Graph", "name branch tensors outs free stops prebound grid build mirror note like zero")
GRAPHS: "OrderedDict[str, Graph]" = OrderedDict()
# every branch the table must cover, with what it exists for.  S1 - S4: the four defects this table was written to
# expose ("Engine graph numerics": shared weight in one grouped wgrad launch, LayerNorm's beta gradient,
# stale tape.mat entry, GELU term into a non-contiguous target)
BRANCHES = OrderedDict([
    ("chain", "virtual GELU between layers, materialised or not, direct and Winograd"),
    ("ride", "the identity-path gradient rides on the first convolution's dgrad (EPI_RES / EPI_RES_MUL_DGELU)"),
    ("ride_mismatch", "take_res_grad refuses a term of the other activation: _flush_res"),
    ("ride_preempted", "grad_for_write flushes a pending term before another writer"),
    ("ride_leftover", "a pending term nobody carried is flushed at the end of Tape.backward"),
    ("ride_twice", "a second defer_res_grad flushes the first"),
    ("ride_slice", "S4: a GELU term into a non-contiguous target, no ride possible (private buffers)"),
    ("fanout", "five consumers of one tensor: accum 0 then 1 in unwinding order; a pre-bound gradient"),
    ("group_shared", "members that share inputs write private buffers; slices, LRP tail, residuals, pixel shuffle"),
    ("group_mixed_accum", "members whose gradients are partly written already: zero_() and accum = 1"),
    ("group_partial_want", "a stopped member input leaves the others unchanged"),
    ("group_missing", "a member without a gradient: RuntimeError; none with a gradient: nothing is launched"),
    ("bias_paths", "bias gradient fused into the wgrad, through channel_sum, absent, behind pixel shuffle and LRP"),
    ("shared_weight", "S1: one weight in two layers of one geometry, of two geometries, and through conv2d_thin_out"),
    ("thin", "conv2d_thin_in (x wanted / stopped), convT2d_thin_out, conv2d_thin_out K = 3 and K = 1"),
    ("gdn_chain", "GDN / IGDN between layers with the EPI_AXPY2 dgrad accumulating; beta, gamma stopped alone"),
    ("swin", "swin_block with and without DropPath, patch merging / split; S2: LayerNorm gamma, beta stopped alone"),
    ("gate", "attention_gate with the branches paired and unpaired"),
    ("aliased_views", "zigzag block views and nested channel prefixes bound into one zeroed gradient buffer"),
    ("entropy_tail", "ste_round_medians + eb_likelihood (noise / medians), gc_likelihood_ste with d lik, d y_hat, both"),
    ("inference", "need_grad=False: values only, activated-in-place stores; S3: a stale tape.mat entry"),
    ("autograd_bridge", "tape_function: requires_grad mix, an unused output, a non-contiguous upstream gradient"),
])


# branches that have no graph of their own: they run graphs of other branches a second way (tests/test_gpu_engine_graphs.py)
NOT_IN_TABLE = {"inference": "chain and ride with need_grad=False; the S3 case is written out in the test",
                "autograd_bridge": "chain through tape_function"}


def graph(name, branch, tensors, outs, *, free=(), stops=(), prebound=None, grid=True, note="", like=None, zero=()):
    assert branch in BRANCHES, branch

    def deco(pair):
        build, mirror = pair()
        GRAPHS[name] = Graph(name, branch, OrderedDict(tensors), tuple(outs), tuple(free), tuple(stops),
                             dict(prebound or {}), grid, build, mirror, note, like or name, tuple(zero))
        return pair
    return deco


def opts(E, which, **kw):
    """the options a build / mirror pair reads: gelu (virtual activations on: the real set), A (the engine's flag for
    it), E (the engine module; None for a mirror), act_out"""
    gelu = which == "real"
    o = NS(gelu=gelu, E=E, A=(1 if gelu else 0), act_out=True, which=which)
    o.update(kw)
    return o


def _ru(p, dim):
    h = dim // 2
    return [(p + ".conv.0.weight", ((h, dim, 1, 1), "w")), (p + ".conv.0.bias", ((h,), "b")),
            (p + ".conv.2.weight", ((h, h, 3, 3), "w")), (p + ".conv.2.bias", ((h,), "b")),
            (p + ".conv.4.weight", ((dim, h, 1, 1), "w")), (p + ".conv.4.bias", ((dim,), "b"))]


def _conv(p, co, ci, k, bias=True, transposed=False):
    t = [(p + ".w", ((ci, co, k, k) if transposed else (co, ci, k, k), "w"))]
    return t + ([(p + ".b", ((co,), "b"))] if bias else [])


# ---------------------------------------------------------------------------------------------- chain
@graph("chain", "chain", [("x", ((2, 8, 8, 8), "x"))] + _conv("c1", 16, 8, 3) + _conv("c2", 16, 16, 3) + _conv("c3", 24, 16, 1),
       ["y"])
def _chain():
    def build(tape, T, o):
        E, VT = o.E, o.E.VT
        u1 = E.conv2d(tape, VT(T.x), T["c1.w"], T["c1.b"], pad=1, act_out=o.act_out)
        u2 = E.conv2d(tape, VT(u1, o.A), T["c2.w"], T["c2.b"], pad=1, act_out=o.act_out)
        return {"y": E.conv2d(tape, VT(u2, o.A), T["c3.w"], T["c3.b"])}

    def mirror(m, T, o):
        u1 = m.conv(T.x, T["c1.w"], T["c1.b"], pad=1)
        u2 = m.conv(m.act(u1, o.gelu), T["c2.w"], T["c2.b"], pad=1)
        return {"y": m.conv(m.act(u2, o.gelu), T["c3.w"], T["c3.b"])}
    return build, mirror


@graph("chain_odd", "chain", [("x", ((2, 5, 8, 8), "x"))] + _conv("c1", 3, 5, 3) + _conv("c2", 8, 3, 1), ["y"],
       note="the odd pair 5 -> 3: channel tails of both directions and of the weight gradient")
def _chain_odd():
    def build(tape, T, o):
        E, VT = o.E, o.E.VT
        u1 = E.conv2d(tape, VT(T.x, o.A), T["c1.w"], T["c1.b"], pad=1, act_out=True)
        return {"y": E.conv2d(tape, VT(u1, o.A), T["c2.w"], T["c2.b"])}

    def mirror(m, T, o):
        u1 = m.conv(m.act(T.x, o.gelu), T["c1.w"], T["c1.b"], pad=1)
        return {"y": m.conv(m.act(u1, o.gelu), T["c2.w"], T["c2.b"])}
    return build, mirror


# ---------------------------------------------------------------------------------------------- ride family
def _ride(act_in):
    def pair():
        def build(tape, T, o):
            E, VT = o.E, o.E.VT
            xv = VT(T.x, o.A if act_in else 0)
            if o.gelu:
                return {"y": E.residual_unit(tape, xv, T, "ru").t}
            u1 = E.conv2d(tape, xv, T["ru.conv.0.weight"], T["ru.conv.0.bias"], act_out=o.act_out)      # the unit's wiring,
            u2 = E.conv2d(tape, VT(u1), T["ru.conv.2.weight"], T["ru.conv.2.bias"], pad=1, act_out=o.act_out)   # activations NONE
            return {"y": E.conv2d(tape, VT(u2), T["ru.conv.4.weight"], T["ru.conv.4.bias"], res=xv, act_out=o.act_out)}

        def mirror(m, T, o):
            xa = m.act(T.x, o.gelu and act_in)
            u1 = m.conv(xa, T["ru.conv.0.weight"], T["ru.conv.0.bias"])
            u2 = m.conv(m.act(u1, o.gelu), T["ru.conv.2.weight"], T["ru.conv.2.bias"], pad=1)
            return {"y": m.conv(m.act(u2, o.gelu), T["ru.conv.4.weight"], T["ru.conv.4.bias"]) + xa}
        return build, mirror
    return pair


graph("ride", "ride", [("x", ((2, 16, 8, 8), "x"))] + _ru("ru", 16), ["y"])(_ride(False))
graph("ride_gelu", "ride", [("x", ((2, 16, 8, 8), "x"))] + _ru("ru", 16), ["y"])(_ride(True))


def _ride_mismatch(first_act):
    def pair():
        def build(tape, T, o):
            E, VT = o.E, o.E.VT
            u1 = E.conv2d(tape, VT(T.x, o.A if first_act else 0), T["c1.w"], T["c1.b"], pad=1, act_out=True)
            return {"y": E.conv2d(tape, VT(u1, o.A), T["c2.w"], T["c2.b"], res=VT(T.x, 0 if first_act else o.A))}

        def mirror(m, T, o):
            u1 = m.conv(m.act(T.x, o.gelu and first_act), T["c1.w"], T["c1.b"], pad=1)
            return {"y": m.conv(m.act(u1, o.gelu), T["c2.w"], T["c2.b"]) + m.act(T.x, o.gelu and not first_act)}
        return build, mirror
    return pair


_MIS = [("x", ((2, 16, 8, 8), "x"))] + _conv("c1", 8, 16, 3) + _conv("c2", 16, 8, 1)
graph("ride_mismatch_gelu_first", "ride_mismatch", _MIS, ["y"])(_ride_mismatch(True))
graph("ride_mismatch_gelu_res", "ride_mismatch", _MIS, ["y"])(_ride_mismatch(False))


@graph("ride_preempted", "ride_preempted", _MIS + [("z", ((2, 16, 8, 8), "x"))], ["y", "s"])
def _ride_preempted():
    def build(tape, T, o):
        E, VT = o.E, o.E.VT
        u1 = E.conv2d(tape, VT(T.x), T["c1.w"], T["c1.b"], pad=1, act_out=True)      # the would-be carrier
        s = E.add(tape, T.x, T.z)                                                     # unwinds between the two
        return {"y": E.conv2d(tape, VT(u1, o.A), T["c2.w"], T["c2.b"], res=VT(T.x)), "s": s}

    def mirror(m, T, o):
        u1 = m.conv(T.x, T["c1.w"], T["c1.b"], pad=1)
        return {"y": m.conv(m.act(u1, o.gelu), T["c2.w"], T["c2.b"]) + T.x, "s": T.x + T.z}
    return build, mirror


@graph("ride_leftover", "ride_leftover", [("x", ((2, 16, 8, 8), "x")), ("z", ((2, 8, 8, 8), "x"))] + _conv("c2", 16, 8, 1),
       ["y"])
def _ride_leftover():
    def build(tape, T, o):
        E, VT = o.E, o.E.VT
        return {"y": E.conv2d(tape, VT(T.z, o.A), T["c2.w"], T["c2.b"], res=VT(T.x, o.A))}

    def mirror(m, T, o):
        return {"y": m.conv(m.act(T.z, o.gelu), T["c2.w"], T["c2.b"]) + m.act(T.x, o.gelu)}
    return build, mirror


@graph("ride_twice", "ride_twice", [("x", ((2, 16, 8, 8), "x")), ("z", ((2, 8, 8, 8), "x"))] + _conv("c2", 16, 8, 1)
       + _conv("c3", 16, 8, 3), ["y1", "y2"])
def _ride_twice():
    def build(tape, T, o):
        E, VT = o.E, o.E.VT
        y1 = E.conv2d(tape, VT(T.z), T["c2.w"], T["c2.b"], res=VT(T.x, o.A))
        return {"y1": y1, "y2": E.conv2d(tape, VT(T.z), T["c3.w"], T["c3.b"], pad=1, res=VT(T.x))}

    def mirror(m, T, o):
        return {"y1": m.conv(T.z, T["c2.w"], T["c2.b"]) + m.act(T.x, o.gelu),
                "y2": m.conv(T.z, T["c3.w"], T["c3.b"], pad=1) + T.x}
    return build, mirror


@graph("ride_slice", "ride_slice", [("X", ((2, 24, 8, 8), "x"))] + _conv("ga", 8, 16, 3) + _conv("gb", 8, 16, 3)
       + _conv("c3", 16, 8, 1), ["y", "v"],
       note="S4.  x = X[:, 4:20]; its gradient is bound to the same slice of one zeroed buffer the size of X")
def _ride_slice():
    def build(tape, T, o):
        E, VT = o.E, o.E.VT
        x = T.X[:, 4:20]
        dX = E.zeros(T.X.shape, T.X.device)
        tape.bind_grad(T.X, dX, True)
        tape.bind_grad(x, dX[:, 4:20], True)
        us = E.conv2d_group(tape, [VT(x, o.A), VT(x, o.A)], [T["ga.w"], T["gb.w"]], [T["ga.b"], T["gb.b"]], pad=1,
                            act_out=True)
        return {"y": E.conv2d(tape, VT(us[0], o.A), T["c3.w"], T["c3.b"], res=VT(x, o.A)), "v": us[1]}

    def mirror(m, T, o):
        xa = m.act(T.X[:, 4:20], o.gelu)
        ua, ub = m.conv(xa, T["ga.w"], T["ga.b"], pad=1), m.conv(xa, T["gb.w"], T["gb.b"], pad=1)
        return {"y": m.conv(m.act(ua, o.gelu), T["c3.w"], T["c3.b"]) + xa, "v": ub}
    return build, mirror


# ---------------------------------------------------------------------------------------------- fanout
_FAN = ([("x", ((2, 8, 16, 16), "x")), ("z", ((2, 8, 16, 16), "x"))] + _conv("a", 16, 8, 1) + _conv("b", 8, 8, 3)
        + _conv("c", 16, 8, 5) + _conv("d", 8, 8, 3, transposed=True))


def _fanout(pre):
    def pair():
        def build(tape, T, o):
            E, VT = o.E, o.E.VT
            if pre:
                tape.bind_grad(T.x, T.g0.clone(), True)
            return {"a": E.conv2d(tape, VT(T.x), T["a.w"], T["a.b"]),
                    "b": E.conv2d(tape, VT(T.x), T["b.w"], T["b.b"], pad=1),
                    "c": E.conv2d(tape, VT(T.x), T["c.w"], T["c.b"], stride=2, pad=2),
                    "d": E.conv2d(tape, VT(T.x), T["d.w"], T["d.b"], stride=2, pad=1, output_padding=1, transposed=True),
                    "e": E.add(tape, T.x, T.z)}

        def mirror(m, T, o):
            return {"a": m.conv(T.x, T["a.w"], T["a.b"]), "b": m.conv(T.x, T["b.w"], T["b.b"], pad=1),
                    "c": m.conv(T.x, T["c.w"], T["c.b"], stride=2, pad=2),
                    "d": m.convT(T.x, T["d.w"], T["d.b"], stride=2, pad=1, opad=1), "e": T.x + T.z}
        return build, mirror
    return pair


graph("fanout", "fanout", _FAN, list("abcde"))(_fanout(False))
graph("fanout_prebound", "fanout", _FAN + [("g0", ((2, 8, 16, 16), "k:x"))], list("abcde"),
      prebound={"x": "g0"})(_fanout(True))


# ---------------------------------------------------------------------------------------------- grouped layers
def _members(n, co, ci, k=3):
    t = []
    for i in range(n):
        t += _conv("m%d" % i, co, ci, k)
    return t


def _grp(T, n):
    return [T["m%d.w" % i] for i in range(n)], [T["m%d.b" % i] for i in range(n)]


def _group_shared(kind):
    def pair():
        def build(tape, T, o):
            E, VT = o.E, o.E.VT
            ws, bs_ = _grp(T, 4)
            xs = [VT(T.x0, o.A), VT(T.x0, o.A), VT(T.x1, o.A), VT(T.x1, o.A)]
            kw, leaf = {}, {}
            if kind == "slices":        # outputs and LRP operands are channel slices of wider buffers
                wide, aux = E.new((2, 40, 8, 8), T.x0.device), E.new((2, 40, 8, 8), T.x0.device)
                for i in range(4):
                    aux[:, 2 + 8 * i:10 + 8 * i] = T["aux%d" % i]
                    leaf["aux%d" % i] = aux[:, 2 + 8 * i:10 + 8 * i]
                kw = dict(outs=[wide[:, 2 + 8 * i:10 + 8 * i] for i in range(4)],
                          lrp_auxs=[leaf["aux%d" % i] for i in range(4)])
            elif kind == "ress":
                kw = dict(ress=[VT(T["r%d" % i], o.A) for i in range(4)], act_out=True)
            elif kind == "ps":
                kw = dict(pixel_shuffle=2)
            ys = E.conv2d_group(tape, xs, ws, bs_, pad=1, **kw)
            return dict({"y%d" % i: y for i, y in enumerate(ys)}, _leaf=leaf)

        def mirror(m, T, o):
            out = {}
            for i in range(4):
                v = m.conv(m.act(T["x%d" % (i // 2)], o.gelu), T["m%d.w" % i], T["m%d.b" % i], pad=1)
                if kind == "slices":
                    v = m.lrp(T["aux%d" % i], v)
                elif kind == "ress":
                    v = v + m.act(T["r%d" % i], o.gelu)
                elif kind == "ps":
                    v = m.ps2(v)
                out["y%d" % i] = v
            return out
        return build, mirror
    return pair


_GX = [("x0", ((2, 16, 8, 8), "x")), ("x1", ((2, 16, 8, 8), "x"))]
_Y4 = ["y0", "y1", "y2", "y3"]
graph("group_shared", "group_shared", _GX + _members(4, 8, 16), _Y4)(_group_shared("plain"))
graph("group_shared_slices_lrp", "group_shared", _GX + _members(4, 8, 16) + [("aux%d" % i, ((2, 8, 8, 8), "x")) for i in range(4)],
      _Y4, grid=False, note="tanh: no exact twin")(_group_shared("slices"))
graph("group_shared_ress", "group_shared", _GX + _members(4, 8, 16) + [("r%d" % i, ((2, 8, 8, 8), "x")) for i in range(4)],
      _Y4)(_group_shared("ress"))
graph("group_shared_ps", "group_shared", _GX + _members(4, 8, 16), _Y4)(_group_shared("ps"))


@graph("group_mixed_accum", "group_mixed_accum", [("x%d" % i, ((2, 16, 8, 8), "x")) for i in range(3)] + _members(3, 8, 16)
       + _conv("late", 8, 16, 1), ["y0", "y1", "y2", "l"])
def _group_mixed():
    def build(tape, T, o):
        E, VT = o.E, o.E.VT
        ws, bs_ = _grp(T, 3)
        ys = E.conv2d_group(tape, [VT(T["x%d" % i], o.A) for i in range(3)], ws, bs_, pad=1)
        late = E.conv2d(tape, VT(T.x1, o.A), T["late.w"], T["late.b"])      # unwinds first: d(x1) exists already
        return dict({"y%d" % i: y for i, y in enumerate(ys)}, l=late)

    def mirror(m, T, o):
        out = {"y%d" % i: m.conv(m.act(T["x%d" % i], o.gelu), T["m%d.w" % i], T["m%d.b" % i], pad=1) for i in range(3)}
        out["l"] = m.conv(m.act(T.x1, o.gelu), T["late.w"], T["late.b"])
        return out
    return build, mirror


def _group_plain3():
    def build(tape, T, o):
        E, VT = o.E, o.E.VT
        ws, bs_ = _grp(T, 3)
        ys = E.conv2d_group(tape, [VT(T["x%d" % i], o.A) for i in range(3)], ws, bs_, pad=1)
        return {"y%d" % i: y for i, y in enumerate(ys)}

    def mirror(m, T, o):
        return {"y%d" % i: m.conv(m.act(T["x%d" % i], o.gelu), T["m%d.w" % i], T["m%d.b" % i], pad=1) for i in range(3)}
    return build, mirror


_G3 = [("x%d" % i, ((2, 16, 8, 8), "x")) for i in range(3)] + _members(3, 8, 16)
graph("group_all_wanted", "group_partial_want", _G3, ["y0", "y1", "y2"])(_group_plain3)
graph("group_partial_want", "group_partial_want", _G3, ["y0", "y1", "y2"], stops=["x1"], like="group_all_wanted")(_group_plain3)
graph("group_missing_one", "group_missing", _G3, ["y0", "y2"], free=["y1"],
      note="y1 gets no gradient: backward raises RuntimeError")(_group_plain3)
graph("group_missing_all", "group_missing", _G3, [], free=["y0", "y1", "y2"],
      note="no member gets a gradient: backward returns, no gradient exists, nothing is launched")(_group_plain3)


# ---------------------------------------------------------------------------------------------- bias paths
@graph("bias_paths", "bias_paths", [("x", ((2, 8, 8, 8), "x"))] + _conv("f", 16, 8, 3) + _conv("t", 8, 8, 3, transposed=True)
       + _conv("s", 16, 8, 1) + _conv("n", 16, 8, 3, bias=False) + _conv("p", 16, 8, 3), list("ftsnp"), stops=["s.w"])
def _bias_paths():
    def build(tape, T, o):
        E, VT = o.E, o.E.VT
        x = VT(T.x, o.A)
        return {"f": E.conv2d(tape, x, T["f.w"], T["f.b"], pad=1),                                   # fused into the wgrad
                "t": E.conv2d(tape, x, T["t.w"], T["t.b"], stride=2, pad=1, output_padding=1, transposed=True),
                "s": E.conv2d(tape, x, T["s.w"], T["s.b"]),                                          # weight stopped
                "n": E.conv2d(tape, x, T["n.w"], None, pad=1),
                "p": E.conv2d(tape, x, T["p.w"], T["p.b"], pad=1, pixel_shuffle=2)}

    def mirror(m, T, o):
        x = m.act(T.x, o.gelu)
        return {"f": m.conv(x, T["f.w"], T["f.b"], pad=1), "t": m.convT(x, T["t.w"], T["t.b"], stride=2, pad=1, opad=1),
                "s": m.conv(x, T["s.w"], T["s.b"]), "n": m.conv(x, T["n.w"], None, pad=1),
                "p": m.ps2(m.conv(x, T["p.w"], T["p.b"], pad=1))}
    return build, mirror


@graph("bias_lrp", "bias_paths", [("x", ((2, 8, 8, 8), "x")), ("aux", ((2, 16, 8, 8), "x"))] + _conv("f", 16, 8, 3), ["y"],
       grid=False, note="tanh: no exact twin")
def _bias_lrp():
    def build(tape, T, o):
        E = o.E
        return {"y": E.conv2d(tape, E.VT(T.x, o.A), T["f.w"], T["f.b"], pad=1, lrp_aux=T.aux)}

    def mirror(m, T, o):
        return {"y": m.lrp(T.aux, m.conv(m.act(T.x, o.gelu), T["f.w"], T["f.b"], pad=1))}
    return build, mirror


# ---------------------------------------------------------------------------------------------- shared weight (S1)
@graph("shared_weight_same", "shared_weight", [("x", ((2, 8, 8, 8), "x")), ("z", ((2, 8, 8, 8), "x"))] + _conv("sh", 8, 8, 3),
       ["y1", "y2"], note="S1: two problems of one geometry on one dw / dbias")
def _shared_same():
    def build(tape, T, o):
        E, VT = o.E, o.E.VT
        return {"y1": E.conv2d(tape, VT(T.x), T["sh.w"], T["sh.b"], pad=1),
                "y2": E.conv2d(tape, VT(T.z), T["sh.w"], T["sh.b"], pad=1)}

    def mirror(m, T, o):
        return {"y1": m.conv(T.x, T["sh.w"], T["sh.b"], pad=1), "y2": m.conv(T.z, T["sh.w"], T["sh.b"], pad=1)}
    return build, mirror


@graph("shared_weight_chain", "shared_weight", [("x", ((2, 8, 8, 8), "x"))] + _conv("sh", 8, 8, 3), ["y"],
       note="S1 with the two layers in series (the second reads the first through a virtual GELU)")
def _shared_chain():
    def build(tape, T, o):
        E, VT = o.E, o.E.VT
        u = E.conv2d(tape, VT(T.x, o.A), T["sh.w"], T["sh.b"], pad=1)
        return {"y": E.conv2d(tape, VT(u, o.A), T["sh.w"], T["sh.b"], pad=1)}

    def mirror(m, T, o):
        u = m.conv(m.act(T.x, o.gelu), T["sh.w"], T["sh.b"], pad=1)
        return {"y": m.conv(m.act(u, o.gelu), T["sh.w"], T["sh.b"], pad=1)}
    return build, mirror


@graph("shared_weight_sizes", "shared_weight", [("x", ((2, 8, 8, 8), "x")), ("z", ((2, 8, 16, 16), "x")),
                                                ("q", ((2, 8, 16, 16), "x"))] + _conv("sh", 8, 8, 3) + _conv("o", 8, 8, 3),
       ["y1", "y2", "y3"],
       note="one weight at two map sizes, with another weight's problem of the second geometry queued BEFORE the "
            "overwriting one: the launches of a flush must follow the queue, not the geometry table")
def _shared_sizes():
    def build(tape, T, o):
        E, VT = o.E, o.E.VT
        y2 = E.conv2d(tape, VT(T.z), T["sh.w"], T["sh.b"], pad=1)       # unwinds last: accumulates (16x16)
        y1 = E.conv2d(tape, VT(T.x), T["sh.w"], T["sh.b"], pad=1)       # unwinds second: overwrites (8x8)
        y3 = E.conv2d(tape, VT(T.q), T["o.w"], T["o.b"], pad=1)         # unwinds first: opens the 16x16 group
        return {"y1": y1, "y2": y2, "y3": y3}

    def mirror(m, T, o):
        return {"y1": m.conv(T.x, T["sh.w"], T["sh.b"], pad=1), "y2": m.conv(T.z, T["sh.w"], T["sh.b"], pad=1),
                "y3": m.conv(T.q, T["o.w"], T["o.b"], pad=1)}
    return build, mirror


@graph("shared_weight_thin", "shared_weight", [("x", ((2, 8, 8, 8), "x")), ("z", ((2, 8, 8, 8), "x"))] + _conv("sh", 3, 8, 3),
       ["y1", "y2"], note="conv2d_thin_out twice: every call has its own temporary weight and gradient")
def _shared_thin():
    def build(tape, T, o):
        E, VT = o.E, o.E.VT
        return {"y1": E.conv2d_thin_out(tape, VT(T.x, o.A), T["sh.w"], T["sh.b"], pad=1),
                "y2": E.conv2d_thin_out(tape, VT(T.z, o.A), T["sh.w"], T["sh.b"], pad=1)}

    def mirror(m, T, o):
        return {"y1": m.conv(m.act(T.x, o.gelu), T["sh.w"], T["sh.b"], pad=1),
                "y2": m.conv(m.act(T.z, o.gelu), T["sh.w"], T["sh.b"], pad=1)}
    return build, mirror


# ---------------------------------------------------------------------------------------------- thin-channel forms
def _thin_in(stop_x):
    def pair():
        def build(tape, T, o):
            E, VT = o.E, o.E.VT
            u = E.conv2d_thin_in(tape, T.x, T["ti.w"], T["ti.b"], stride=2, pad=2)
            return {"y": E.conv2d(tape, VT(u, o.A), T["c.w"], T["c.b"], pad=1)}

        def mirror(m, T, o):
            u = m.conv(T.x, T["ti.w"], T["ti.b"], stride=2, pad=2)
            return {"y": m.conv(m.act(u, o.gelu), T["c.w"], T["c.b"], pad=1)}
        return build, mirror
    return pair


_TI = [("x", ((2, 3, 16, 16), "x"))] + _conv("ti", 16, 3, 5) + _conv("c", 8, 16, 3)
graph("thin_in", "thin", _TI, ["y"])(_thin_in(False))
graph("thin_in_stopped", "thin", _TI, ["y"], stops=["x"])(_thin_in(True))


@graph("thin_convT_out", "thin", [("x", ((2, 8, 8, 8), "x"))] + _conv("c", 16, 8, 3) + _conv("to", 3, 16, 5, transposed=True),
       ["y"])
def _thin_convT():
    def build(tape, T, o):
        E, VT = o.E, o.E.VT
        u = E.conv2d(tape, VT(T.x), T["c.w"], T["c.b"], pad=1, act_out=True)
        return {"y": E.convT2d_thin_out(tape, VT(u, o.A), T["to.w"], T["to.b"], stride=2, pad=2, output_padding=1)}

    def mirror(m, T, o):
        u = m.conv(T.x, T["c.w"], T["c.b"], pad=1)
        return {"y": m.convT(m.act(u, o.gelu), T["to.w"], T["to.b"], stride=2, pad=2, opad=1)}
    return build, mirror


def _thin_out(K):
    def pair():
        def build(tape, T, o):
            E, VT = o.E, o.E.VT
            u = E.conv2d(tape, VT(T.x), T["c.w"], T["c.b"], pad=1, act_out=True)
            return {"y": E.conv2d_thin_out(tape, VT(u, o.A), T["to.w"], T["to.b"], pad=K // 2)}

        def mirror(m, T, o):
            u = m.conv(T.x, T["c.w"], T["c.b"], pad=1)
            return {"y": m.conv(m.act(u, o.gelu), T["to.w"], T["to.b"], pad=K // 2)}
        return build, mirror
    return pair


for _K in (3, 1):
    graph("thin_out_k%d" % _K, "thin", [("x", ((2, 8, 8, 8), "x"))] + _conv("c", 16, 8, 3) + _conv("to", 3, 16, _K),
          ["y"])(_thin_out(_K))


# ---------------------------------------------------------------------------------------------- GDN
def _gdn(inverse):
    def pair():
        def build(tape, T, o):
            E, VT = o.E, o.E.VT
            u = E.conv2d(tape, VT(T.x), T["c1.w"], T["c1.b"], pad=1)
            v = E.gdn(tape, u, T.beta, T.gamma, inverse)
            s = E.add(tape, u, v)                     # unwinds first: the AXPY2 dgrad of the GDN accumulates onto it
            if inverse:
                return {"y": E.conv2d(tape, VT(s), T["c2.w"], T["c2.b"], stride=2, pad=1, output_padding=1, transposed=True)}
            return {"y": E.conv2d(tape, VT(s), T["c2.w"], T["c2.b"], pad=1)}

        def mirror(m, T, o):
            u = m.conv(T.x, T["c1.w"], T["c1.b"], pad=1)
            s = u + m.gdn(u, T.beta, T.gamma, inverse)
            if inverse:
                return {"y": m.convT(s, T["c2.w"], T["c2.b"], stride=2, pad=1, opad=1)}
            return {"y": m.conv(s, T["c2.w"], T["c2.b"], pad=1)}
        return build, mirror
    return pair


for _inv in (False, True):
    for _stop in ((), ("beta",), ("gamma",)):
        graph("gdn_chain%s%s" % ("_inverse" if _inv else "", "".join("_stop_" + s for s in _stop)), "gdn_chain",
              [("x", ((2, 8, 8, 8), "x"))] + _conv("c1", 16, 8, 3) + [("beta", ((16,), "pos")), ("gamma", ((16, 16), "pos"))]
              + _conv("c2", 8, 16, 3, transposed=_inv), ["y"], stops=_stop, grid=False,
              note="rsqrt / sqrt: no exact twin")(_gdn(_inv))


# ---------------------------------------------------------------------------------------------- swin
def _swin_t(p, dim, ws=4, heads=2):
    return [(p + ".norm1.weight", ((dim,), "w")), (p + ".norm1.bias", ((dim,), "b")),
            (p + ".attn.relative_position_bias_table", (((2 * ws - 1) ** 2, heads), "w")),
            (p + ".attn.qkv.weight", ((3 * dim, dim), "w")), (p + ".attn.qkv.bias", ((3 * dim,), "b")),
            (p + ".attn.proj.weight", ((dim, dim), "w")), (p + ".attn.proj.bias", ((dim,), "b")),
            (p + ".norm2.weight", ((dim,), "w")), (p + ".norm2.bias", ((dim,), "b")),
            (p + ".mlp.fc1.weight", ((4 * dim, dim), "w")), (p + ".mlp.fc1.bias", ((4 * dim,), "b")),
            (p + ".mlp.fc2.weight", ((dim, 4 * dim), "w")), (p + ".mlp.fc2.bias", ((dim,), "b"))]


def _swin(dp, shift):
    def pair():
        def build(tape, T, o):
            return {"y": o.E.swin_block(tape, T.x, T, "blk", 2, 4, shift, dp=T.dp if dp else None)}

        def mirror(m, T, o):
            return {"y": m.swin_block(T.x, T, "blk", 2, 4, shift, T.dp if dp else None)}
        return build, mirror
    return pair


_SW = [("x", ((2, 16, 8, 8), "x"))] + _swin_t("blk", 16)
_DP = [("dp", ((2, 2), "k", (0.0, 2.0, 2.0, 0.0)))]
graph("swin", "swin", _SW, ["y"], grid=False, note="dp=None, shifted windows")(_swin(False, 2))
graph("swin_droppath", "swin", _SW + _DP, ["y"], grid=False,
      note="DropPath scales {0, 2} per sample: residual_scale, whose shortcut term rides on the LayerNorm backward")(_swin(True, 0))
graph("swin_stop_gamma", "swin", _SW, ["y"], grid=False, stops=["blk.norm1.weight", "blk.norm2.weight"],
      note="S2: beta's gradient must still be written")(_swin(False, 0))
graph("swin_stop_beta", "swin", _SW, ["y"], grid=False, stops=["blk.norm1.bias", "blk.norm2.bias"],
      note="gamma's gradient alone")(_swin(False, 0))


@graph("swin_merge_split", "swin", [("x", ((2, 8, 16, 16), "x")), ("pm.norm.weight", ((32,), "w")), ("pm.norm.bias", ((32,), "b")),
                                    ("pm.reduction.weight", ((16, 32), "w"))] + _swin_t("blk", 16)
       + [("sp.norm.weight", ((16,), "w")), ("sp.norm.bias", ((16,), "b")), ("sp.reduction.weight", ((32, 16), "w"))], ["y"],
       grid=False, note="patch_merging -> swin_block -> patch_split")
def _merge_split():
    def build(tape, T, o):
        E = o.E
        a = E.patch_merging(tape, T.x, T, "pm")
        return {"y": E.patch_split(tape, E.swin_block(tape, a, T, "blk", 2, 4, 0), T, "sp")}

    def mirror(m, T, o):
        x = T.x
        g4 = torch.cat([x[:, :, 0::2, 0::2], x[:, :, 1::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 1::2]], 1)   # stf.py:221-225
        a = m.lin(m.ln(g4, T["pm.norm.weight"], T["pm.norm.bias"]), T["pm.reduction.weight"])
        b = m.swin_block(a, T, "blk", 2, 4, 0)
        return {"y": m.ps2(m.lin(m.ln(b, T["sp.norm.weight"], T["sp.norm.bias"]), T["sp.reduction.weight"]))}
    return build, mirror


# ---------------------------------------------------------------------------------------------- gate
def _gate_t(p, dim, ws=4, heads=2):
    t = []
    for i in range(3):
        t += _ru("%s.conv_a.%d" % (p, i), dim)
    a = p + ".conv_b.0.attn"
    t += [(a + ".relative_position_bias_table", (((2 * ws - 1) ** 2, heads), "w")), (a + ".qkv.weight", ((3 * dim, dim), "w")),
          (a + ".qkv.bias", ((3 * dim,), "b")), (a + ".proj.weight", ((dim, dim), "w")), (a + ".proj.bias", ((dim,), "b"))]
    for i in (1, 2, 3):
        t += _ru("%s.conv_b.%d" % (p, i), dim)
    return t + [(p + ".conv_b.4.weight", ((dim, dim, 1, 1), "w")), (p + ".conv_b.4.bias", ((dim,), "b"))]


@graph("gate", "gate", [("x", ((2, 16, 8, 8), "x"))] + _gate_t("g", 16), ["y"], grid=False,
       note="layers/layers.py:83-89; run with PAIR_GATE_BRANCHES both ways")
def _gate():
    def build(tape, T, o):
        return {"y": o.E.attention_gate(tape, T.x, T, "g", 2, 4, 0)}

    def mirror(m, T, o):
        x = T.x
        a = x                                        # the first unit reads x itself, the later ones gelu(previous)
        for i in range(3):
            a = m.residual_unit(a if i == 0 else m.gelu(a), T, "g.conv_a.%d" % i)
        p = "g.conv_b.0.attn"
        att = m.attn(m.lin(x, T[p + ".qkv.weight"], T[p + ".qkv.bias"]), T[p + ".relative_position_bias_table"], 2, 4, 0)
        b = x + m.lin(att, T[p + ".proj.weight"], T[p + ".proj.bias"])
        for i in (1, 2, 3):
            b = m.residual_unit(b if i == 1 else m.gelu(b), T, "g.conv_b.%d" % i)
        b4 = m.conv(m.gelu(b), T["g.conv_b.4.weight"], T["g.conv_b.4.bias"])
        return {"y": m.gelu(a) * torch.sigmoid(b4) + x}
    return build, mirror


# ---------------------------------------------------------------------------------------------- aliased views
@graph("aliased_zigzag", "aliased_views", [("x", ((2, 16, 8, 8), "x"))] + _conv("k0", 8, 8, 3) + _conv("k1", 8, 8, 3)
       + _conv("k2", 8, 8, 1) + _conv("k3", 8, 8, 3) + [("z2", ((2, 8, 8, 4, 4), "x"))], ["y", "r"],
       note="zigzag_splits -> per-block convs on the bound views (block 2: two consumers, block 5: none) -> "
            "zigzag_reverse of another leaf")
def _aliased_zigzag():
    def build(tape, T, o):
        E, VT = o.E, o.E.VT
        z = E.zigzag_splits(tape, T.x, 2)                       # [2, 8, 8, 4, 4]
        ys = [E.conv2d(tape, VT(z[:, 0], o.A), T["k0.w"], T["k0.b"], pad=1),
              E.conv2d(tape, VT(z[:, 2], o.A), T["k1.w"], T["k1.b"], pad=1),
              E.conv2d(tape, VT(z[:, 2], o.A), T["k2.w"], T["k2.b"]),
              E.conv2d(tape, VT(z[:, 7], o.A), T["k3.w"], T["k3.b"], pad=1)]
        y = E.add(tape, E.add(tape, ys[0], ys[1]), E.add(tape, ys[2], ys[3]))
        return {"y": y, "r": E.zigzag_reverse(tape, T.z2, 2)}

    def mirror(m, T, o):
        z = PR.zigzag_splits(T.x, 2, 2, 2)
        y = (m.conv(m.act(z[:, 0], o.gelu), T["k0.w"], T["k0.b"], pad=1) + m.conv(m.act(z[:, 2], o.gelu), T["k1.w"], T["k1.b"], pad=1)
             + m.conv(m.act(z[:, 2], o.gelu), T["k2.w"], T["k2.b"]) + m.conv(m.act(z[:, 7], o.gelu), T["k3.w"], T["k3.b"], pad=1))
        r = torch.zeros(2, 2, 8, 2, 4, 2, 4, dtype=T.z2.dtype)
        for n, (c, h, w) in enumerate(PR.Z.zigzag_order(2, 2, 2)):
            r[:, c, :, h, :, w, :] = T.z2[:, n]
        return {"y": y, "r": r.reshape(2, 16, 8, 8)}
    return build, mirror


@graph("aliased_nested", "aliased_views", [("B", ((2, 24, 8, 8), "x"))] + _conv("k0", 8, 24, 3) + _conv("k1", 8, 8, 3)
       + _conv("k2", 8, 16, 1) + _conv("k3", 8, 8, 3), ["y0", "y1", "y2", "y3"],
       note="slices.py:239-246: a buffer, two nested prefixes and one disjoint slice, all bound into one zeroed buffer")
def _aliased_nested():
    def build(tape, T, o):
        E, VT = o.E, o.E.VT
        B = T.B
        dB = E.zeros(B.shape, B.device)
        views = [B, B[:, :8], B[:, :16], B[:, 16:24]]
        for v, dv in zip(views, [dB, dB[:, :8], dB[:, :16], dB[:, 16:24]]):
            tape.bind_grad(v, dv, True)
        return {"y%d" % i: E.conv2d(tape, VT(v, o.A), T["k%d.w" % i], T["k%d.b" % i], pad=(0 if i == 2 else 1))
                for i, v in enumerate(views)}

    def mirror(m, T, o):
        B = T.B
        views = [B, B[:, :8], B[:, :16], B[:, 16:24]]
        return {"y%d" % i: m.conv(m.act(v, o.gelu), T["k%d.w" % i], T["k%d.b" % i], pad=(0 if i == 2 else 1))
                for i, v in enumerate(views)}
    return build, mirror


# ---------------------------------------------------------------------------------------------- entropy tail
_FILT = (1, 3, 3, 3, 3, 1)
_EB = ([("eb._matrix%d" % i, ((8, _FILT[i + 1], _FILT[i]), "w")) for i in range(5)]
       + [("eb._bias%d" % i, ((8, _FILT[i + 1], 1), "b")) for i in range(5)]
       + [("eb._factor%d" % i, ((8, _FILT[i + 1], 1), "w")) for i in range(4)] + [("eb.quantiles", ((8, 1, 3), "q"))])
ROUND_MARGIN = 1e-4      # no rounded value of an entropy graph lies nearer a half-integer (test_engine_ref.py)


def _eb_tail(noisy):
    def pair():
        def build(tape, T, o):
            E = o.E
            z = E.conv2d(tape, E.VT(T.x), T["c.w"], T["c.b"], pad=1)
            zh = E.ste_round_medians(tape, z, T["eb.quantiles"])
            zt, lik = E.eb_likelihood(tape, z, T, "eb", noise=T.noise if noisy else None, want_zt=True)
            return {"zh": zh, "zt": zt, "lik": lik}

        def mirror(m, T, o):
            z = m.conv(T.x, T["c.w"], T["c.b"], pad=1)
            med = T["eb.quantiles"][:, 0, 1].detach().view(1, -1, 1, 1)      # ste_round(z - med) + med: d / d med = 0
            zt, lik = O.eb_likelihood(z, T, "eb", T.noise if noisy else None)
            return {"zh": m.ste_round(z - med) + med, "zt": zt, "lik": lik, "_rounded": z - med}
        return build, mirror
    return pair


_EBT = [("x", ((2, 8, 8, 8), "x"))] + _conv("c", 8, 8, 3) + _EB + [("noise", ((2, 8, 8, 8), "k:n"))]
graph("entropy_eb_noise", "entropy_tail", _EBT, ["zh", "zt", "lik"], grid=False,
      note="round and the density: no exact twin.  z~ = z + noise: its gradient is added to z's")(_eb_tail(True))
graph("entropy_eb_medians", "entropy_tail", _EBT, ["zh", "zt", "lik"], grid=False,
      note="no noise: the gradients of the likelihood and of z~ with respect to the medians land in "
           "quantiles[:, 0, 1]")(_eb_tail(False))


def _gc_tail():
    def build(tape, T, o):
        E, VT = o.E, o.E.VT
        mu = E.conv2d(tape, VT(T.x), T["mu.w"], T["mu.b"], pad=1)
        sc = E.conv2d(tape, VT(T.xs), T["sc.w"], T["sc.b"], pad=1)
        lik, yh = E.new(T.y), E.new(T.y)
        E.gc_likelihood_ste(tape, T.y, mu, sc, T.noise, lik, yh)
        t = E.conv2d(tape, VT(T.y), T["k.w"], T["k.b"], pad=1)      # unwinds first: the Gaussian step accumulates into d(y)
        return {"lik": lik, "yh": yh, "t": t}

    def mirror(m, T, o):
        mu = m.conv(T.x, T["mu.w"], T["mu.b"], pad=1)
        sc = m.conv(T.xs, T["sc.w"], T["sc.b"], pad=1)
        _, lik = O.gaussian_likelihood(T.y, sc, mu, T.noise)
        return {"lik": lik, "yh": m.ste_round(T.y - mu) + mu, "t": m.conv(T.y, T["k.w"], T["k.b"], pad=1),
                "_rounded": T.y - mu, "_scale": sc}
    return build, mirror


_GCT = ([("x", ((2, 8, 8, 8), "x")), ("xs", ((2, 8, 8, 8), "pos")), ("y", ((2, 8, 8, 8), "x"))] + _conv("mu", 8, 8, 3)
        + [("sc.w", ((8, 8, 3, 3), "pos")), ("sc.b", ((8,), "pos"))] + _conv("k", 8, 8, 3) + [("noise", ((2, 8, 8, 8), "k:n"))])
_GCN = "erfc and round: no exact twin.  The scale layer's operands are positive: every scale lies above the 0.11 bound"
graph("entropy_gc", "entropy_tail", _GCT, ["lik", "yh", "t"], grid=False, note=_GCN)(_gc_tail)
graph("entropy_gc_dlik_alone", "entropy_tail", _GCT, ["lik", "t"], free=["yh"], grid=False, note=_GCN, like="entropy_gc")(_gc_tail)
graph("entropy_gc_dyh_alone", "entropy_tail", _GCT, ["yh", "t"], free=["lik"], grid=False, note=_GCN, like="entropy_gc",
      zero=["xs", "sc.w", "sc.b"])(_gc_tail)


# ---------------------------------------------------------------------------------------------- many problems
@graph("many33", "chain", [("x", ((1, 8, 4, 4), "x"))] + [t for i in range(33) for t in _conv("k%d" % i, 8, 8, 3)],
       ["y%d" % i for i in range(33)], note="33 same-geometry weight-gradient problems: launches of 32 + 1")
def _many33():
    def build(tape, T, o):
        E = o.E
        return {"y%d" % i: E.conv2d(tape, E.VT(T.x), T["k%d.w" % i], T["k%d.b" % i], pad=1) for i in range(33)}

    def mirror(m, T, o):
        return {"y%d" % i: m.conv(T.x, T["k%d.w" % i], T["k%d.b" % i], pad=1) for i in range(33)}
    return build, mirror


# ================================================================================================ inputs
def whiches(g):
    return ("grid", "real") if g.grid else ("real",)


def leaves(g):
    return [k for k, v in g.tensors.items() if not v[1].startswith("k")]


@functools.lru_cache(maxsize=None)
def _input(key, shape, kind, which):
    n = int(np.prod(shape))
    u = W.uniform01(key, n)
    if which == "grid":
        assert kind in ("x", "w", "b"), "no exact form"
        lo, span = (-1, 3) if kind == "w" else (-2, 5)
        v = np.floor(span * u) + lo
    elif kind == "pos":
        v = np.abs(2.0 * u - 1.0) + 0.05
    elif kind == "n":                       # quantisation noise
        v = u - 0.5
    elif kind == "q":                       # EntropyBottleneck.quantiles [C, 1, 3]: medians in [-1, 1)
        v = (2.0 * u - 1.0) + np.tile([-10.0, 0.0, 10.0], n // 3)
    else:
        v = 2.0 * u - 1.0
    return torch.from_numpy(v.astype(np.float32)).reshape(shape)


def make_inputs(g, which):
    """name -> float32 CPU tensor (cached: do not write to them)"""
    t = OrderedDict()
    for name, spec in g.tensors.items():
        shape, kind = spec[0], spec[1]
        if kind == "k":
            t[name] = torch.tensor(spec[2], dtype=F32).reshape(shape)
        else:
            t[name] = _input("eg.%s.%s" % (g.like, name), tuple(shape), kind.split(":")[-1], which)
    return t


def upstream(g, which, shapes):
    """the fixed upstream gradient of every output of g.outs; shapes: name -> shape"""
    return OrderedDict((k, _input("eg.%s.g.%s" % (g.like, k), tuple(shapes[k]), "x", which)) for k in g.outs)


# ================================================================================================ reference
Ref = namedtuple("Ref", "outs grads")


def loss_of(g, outs, T, ups):
    tot = 0.0
    for k in g.outs:
        tot = tot + (outs[k] * ups[k].to(outs[k].dtype)).sum()
    for leaf, pre in g.prebound.items():
        tot = tot + (T[leaf] * T[pre]).sum()
    return tot


def evaluate(g, which, dtype=F64, pert=None, absolute=False, override=None):
    """the mirror and its autograd gradients; absolute: on |inputs|, |weights| (sums of absolute terms)"""
    base = make_inputs(g, which)
    T = NS()
    for k, v in base.items():
        v = v.to(dtype)
        if absolute:
            v = v.abs()
        T[k] = v.clone().requires_grad_(k in leaves(g))
    if override:
        for k, v in override.items():
            T[k] = v
    m, o = M(dtype, pert), opts(None, which)
    with torch.enable_grad():
        outs = g.mirror(m, T, o)
        ups = upstream(g, which, {k: outs[k].shape for k in g.outs})
        if absolute:
            ups = OrderedDict((k, v.abs()) for k, v in ups.items())
        want = [k for k in leaves(g) if k not in g.stops]
        grads = {}
        if g.outs or g.prebound:
            gr = torch.autograd.grad(loss_of(g, outs, T, ups), [T[k] for k in want], allow_unused=True)
            grads = {k: v for k, v in zip(want, gr)}
    return Ref({k: v.detach() for k, v in outs.items() if not k.startswith("_")},       # "_...": the mirror's diagnostics
               {k: (None if v is None else v.detach()) for k, v in grads.items()}), T


@functools.lru_cache(maxsize=None)
def reference(name, which, dtype=F64, pert=None, absolute=False):
    return evaluate(GRAPHS[name], which, dtype, pert, absolute)[0]


def tensors_of(ref):
    """(label, tensor) of every output and gradient of a Ref"""
    for k, v in ref.outs.items():
        yield k, v
    for k, v in ref.grads.items():
        if v is not None:
            yield "d." + k, v


@functools.lru_cache(maxsize=None)
def limits(name):
    """label -> (limit, ref32's error, floor) on `real`"""
    r64, r32 = reference(name, "real"), reference(name, "real", F32)
    perts = [dict(tensors_of(reference(name, "real", F64, p))) for p in PERTS]
    t32 = dict(tensors_of(r32))
    out = {}
    for k, v in tensors_of(r64):
        e32 = (t32[k].double() - v).abs().max().item()
        floor = max((p[k] - v).abs().max().item() for p in perts)
        out[k] = (FACTOR * e32 + FACTOR * U * v.abs().max().item() + floor, e32, floor)
    return out


def grid_headroom(name, wino=False):
    """largest magnitude any value, gradient or partial sum of the grid twin can reach (Winograd: in units of 1/4)"""
    r = reference(name, "grid", F64, None, True)
    m = max(v.abs().max().item() for _, v in tensors_of(r))
    return 4 * m if wino else m


def fd_check(g, coords=FD_COORDS, h=1e-5):
    """worst |autograd - central difference| / |gradient|_max over `coords` seeded coordinates of every leaf (real),
    the central difference taken at h and h / 2 and extrapolated (h = 1e-5 keeps the roundoff of the loss, a sum of
    thousands of terms, below 1e-7 of the smaller gradients; the extrapolation removes the h^2 term the gate's six
    residual units make visible at that step); a
    leaf whose gradient is all zero is held to the largest gradient of the graph"""
    ref, T = evaluate(g, "real")
    rec = M(F64)
    rec.ste_record = []
    with torch.no_grad():
        outs = g.mirror(rec, T, opts(None, "real"))
    ups = upstream(g, "real", {k: outs[k].shape for k in g.outs})

    def outs_at(leaf, i, delta):
        m = M(F64)
        m.ste_replay = rec.ste_record
        v = T[leaf].detach().clone()
        v.view(-1)[i] += delta
        Tn = NS(T)
        Tn[leaf] = v
        with torch.no_grad():
            return g.mirror(m, Tn, opts(None, "real")), Tn

    def loss_difference(leaf, i, step):
        """loss(+step) - loss(-step), the outputs subtracted element by element BEFORE the sum: what the coordinate does
        not reach cancels exactly instead of leaving the roundoff of a large sum"""
        (op, Tp), (om, Tm) = outs_at(leaf, i, step), outs_at(leaf, i, -step)
        tot = sum(((op[k] - om[k]) * ups[k].double()).sum().item() for k in g.outs)
        return tot + sum(((Tp[a] - Tm[a]) * T[b]).sum().item() for a, b in g.prebound.items())
    top = max(gr.abs().max().item() for gr in ref.grads.values() if gr is not None)
    worst = 0.0
    for leaf, gr in ref.grads.items():
        if gr is None:
            continue
        idx = np.unique((W.uniform01("eg.fd.%s.%s" % (g.name, leaf), coords) * gr.numel()).astype(np.int64))
        scale = gr.abs().max().item() or top
        for i in idx.tolist():
            d = [loss_difference(leaf, i, step) / (2 * step) for step in (h, 0.5 * h)]      # Richardson: the h^2 term goes
            worst = max(worst, abs((4.0 * d[1] - d[0]) / 3.0 - gr.view(-1)[i].item()) / scale)
    return worst


def rounding_margin(name, dtype=F64):
    """(smallest distance of a rounded value of the graph from a half-integer, the rounded values) in dtype"""
    g = GRAPHS[name]
    T = NS((k, v.to(dtype)) for k, v in make_inputs(g, "real").items())
    with torch.no_grad():
        outs = g.mirror(M(dtype), T, opts(None, "real"))
    v = outs["_rounded"]
    return ((v - torch.floor(v)) - 0.5).abs().min().item(), v, outs.get("_scale")
