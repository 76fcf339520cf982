"""Inputs, float64 references and error yardsticks for the entropy-model kernels (csrc/entropy.hip).  CPU only; shared by
tests/test_entropy_ref.py (which asserts the conditions the GPU tests rely on) and tests/test_gpu_entropy_numerics.py.

The rate is -log2(likelihood) and its gradient 1/likelihood, so a likelihood's error is measured in bits,
|log2 a - log2 b|.  The reference is the oracle of oracle/wacnn_oracle.py run on ``.double()`` copies of the float32
inputs; the same oracle run in float32 is the yardstick every tolerance is derived from (FACTOR times its own error
against float64 on the same inputs, plus a small floor), never the thing under test.

Elements are classified by the float64 likelihood before the bound, ``r``:
  live   r >= 4e-9      compared by value, in three bands
  floor  r <= 2.5e-10   the likelihood is the bound itself, exactly
  grey   in between     float32 and float64 may decide the bound differently: left out of element-wise comparisons
and, for the scale gradient, by the scale: safely below / safely above the bound, or ``grey`` (0.11 and its two float
neighbours: float32(0.11) < 0.11, so float32 and float64 place 0.11 itself on different sides).
"""
import functools
import math

import numpy as np
import torch

from oracle import wacnn_oracle as O
from oracle import weights as W

FACTOR = 4.0            # limit = FACTOR * (float32 oracle's error) + floor; DESIGN.md "Entropy-kernel numerics"
BITS_FLOOR = 1e-6       # bits, added to every log2 limit
REL_FLOOR = 1e-6        # times the largest reference magnitude of the group, added to every gradient limit
LIVE, FLOOR = 4e-9, 2.5e-10
BAND_EDGES = (4e-9, 1e-6, 1e-3)
BAND_NAMES = ("[4e-9,1e-6)", "[1e-6,1e-3)", "[1e-3,1]")
LN2 = math.log(2.0)

_B32 = np.float32(O.SCALE_BOUND)
SCALE_BELOW = float(np.nextafter(_B32, np.float32(0)))      # the two float neighbours of float32(0.11)
SCALE_ABOVE = float(np.nextafter(_B32, np.float32(1)))

EB_NAMES = [f"_matrix{i}" for i in range(5)] + [f"_bias{i}" for i in range(5)] + [f"_factor{i}" for i in range(4)]
EB = "entropy_bottleneck"
EB_SHIFT = 3.0          # added to _matrix0: steep enough for the density to fall below 2.5e-10 within ~35 of the median

GC_SHAPE = (2, 40, 24, 23)          # HW = 552: no multiple of 4 or 64
GC_LONG_SHAPE = (2, 320, 32, 33)    # 675 840 elements: past the 2048 x 256 threads of the capped grid
# (N, C, HW) -> L = N * HW = 1, 63, 256, 257, 999, and how far from the median the last channel's offsets reach
EB_SHAPES = ((1, 5, 1), (1, 5, 63), (2, 24, 128), (1, 7, 257), (3, 24, 333))
EB_REACH = {(1, 5, 1): 43.0}       # five elements: one in each band and two on the floor, in both modes
EB_REACH_DEFAULT = 110.0
MODES = ("eval", "train")
SEEDS = ("bits", "mixed")


def U(key, shape, lo, hi):
    return W._u(key, shape, lo, hi)


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def gaussian_inputs(shape=GC_SHAPE, key="gcn"):
    """{y, mu, scale, noise}, float32 [N,C,H,W].  scale walks the 64-entry table (each entry times a factor in
    [0.8, 1.25]) and holds the corner values around the bound; y = mu + k + f with integer k out to 6.5 sigma and
    |f| <= 0.45, so that round(y - mu) is the same in float32 and float64."""
    n = int(np.prod(shape))
    table = O.scale_table()
    scale = table[torch.arange(n) % table.numel()] * U(key + ".fac", (n,), 0.8, 1.25)
    scale[:7] = torch.tensor([0.11, SCALE_BELOW, SCALE_ABOVE, 0.0, -1.0, 1e-3, 300.0])
    mu = U(key + ".mu", (n,), -3.0, 3.0)
    reach = 6.5 * torch.clamp(scale, min=O.SCALE_BOUND)
    u = U(key + ".k", (n,), -1.0, 1.0)
    k = torch.round(torch.sign(u) * u.abs() ** 1.5 * reach)     # thinner towards the far end, where the grey zone lies
    f = U(key + ".f", (n,), -0.45, 0.45)
    y = mu + (k + f)
    noise = U(key + ".noise", (n,), -0.5, 0.5)
    return {"y": y.reshape(shape), "mu": mu.reshape(shape), "scale": scale.reshape(shape),
            "noise": noise.reshape(shape)}


@functools.lru_cache(maxsize=None)
def eb_params(C, key="ebn", shift=EB_SHIFT):
    """state-dict of an EntropyBottleneck(C): the formula of tests/golden/make_golden.py's fill_module, with _matrix0
    shifted up so that the tails reach the likelihood bound (the model-sized formula weights stop at 1.3e-4)"""
    filt = (1, 3, 3, 3, 3, 1)
    sd = {}
    for i in range(5):
        init = math.log(math.expm1(1 / (10 ** 0.2) / filt[i + 1]))
        sd[f"{EB}._matrix{i}"] = init + (shift if i == 0 else 0.0) + U(f"{key}._matrix{i}", (C, filt[i + 1], filt[i]), -0.3, 0.3)
        sd[f"{EB}._bias{i}"] = U(f"{key}._bias{i}", (C, filt[i + 1], 1), -0.5, 0.5)
        if i < 4:
            sd[f"{EB}._factor{i}"] = U(f"{key}._factor{i}", (C, filt[i + 1], 1), -0.5, 0.5)
    sd[f"{EB}.quantiles"] = U(f"{key}.quantiles", (C, 1, 3), -0.4, 0.4) + torch.tensor([-10.0, 0.0, 10.0])
    return sd


@functools.lru_cache(maxsize=None)
def eb_inputs(shape, key="ebn"):
    """{z, noise}, float32 [N,C,HW]: z = median + k + f with |f| <= 0.45; |k| grows with the channel index up to
    EB_REACH, so the first channels sit at the mode and the last ones deep in the tails"""
    N, C, HW = shape
    reach = EB_REACH.get(shape, EB_REACH_DEFAULT)
    med = eb_params(C)[f"{EB}.quantiles"][:, 0, 1].reshape(1, C, 1)
    tag = f"{key}.{N}x{C}x{HW}"
    t = (torch.arange(C, dtype=torch.float32).reshape(1, C, 1) + U(tag + ".t", shape, 0.0, 1.0)) / C
    sign = torch.where(U(tag + ".s", shape, -1.0, 1.0) < 0, -1.0, 1.0)
    k = torch.round(sign * t * reach)
    f = U(tag + ".f", shape, -0.45, 0.45)
    z = med + (k + f)
    return {"z": z.contiguous(), "noise": U(tag + ".noise", shape, -0.5, 0.5)}


def cast(d, dtype):
    return {k: v.detach().to(dtype) for k, v in d.items()}


# ------------------------------------------------------------------------------------------------ classification
def classify(r):
    """(live, floor, grey) boolean masks of a float64 raw likelihood"""
    live, floor = r >= LIVE, r <= FLOOR
    return live, floor, ~(live | floor)


def bands(r):
    """the three live bands as boolean masks"""
    e = BAND_EDGES
    return [(r >= e[0]) & (r < e[1]), (r >= e[1]) & (r < e[2]), r >= e[2]]


def groups(r):
    """the groups a gradient tolerance is formed over: the three live bands and the floor"""
    return bands(r) + [r <= FLOOR]


def scale_classes(scale):
    """(below, above, grey) of the float32 scales around the bound"""
    below, above = scale < SCALE_BELOW, scale > SCALE_ABOVE
    return below, above, ~(below | above)


def bits_err(a, r):
    return (torch.log2(a.double()) - torch.log2(r.double())).abs()


def band_bits(lik, r):
    """per band: max |log2 lik - log2 r| over the band (0.0 for an empty band)"""
    err = bits_err(lik, r)
    return [err[m].max().item() if m.any() else 0.0 for m in bands(r)]


def band_limits(lik32, r):
    """per band: FACTOR * the float32 oracle's error + BITS_FLOOR"""
    return [FACTOR * e + BITS_FLOOR for e in band_bits(lik32, r)]


def grad_tolerance(g32, g64, r, keep):
    """element-wise limit for a gradient: per group of ``groups(r)``, FACTOR * max |g32 - g64| + REL_FLOOR * max |g64|,
    both maxima over the group's elements inside ``keep``.  Elements outside every group (grey) get inf."""
    tol = torch.full(g64.shape, float("inf"), dtype=torch.float64)
    err = (g32.double() - g64).abs()
    for m in groups(r):
        m = m & keep
        if m.any():
            tol[m] = FACTOR * err[m].max().item() + REL_FLOOR * g64[m].abs().max().item()
    return tol


def tensor_tolerance(g32, g64):
    """limit for a reduced gradient (a sum over L): relative to the tensor's largest float64 magnitude"""
    return FACTOR * (g32.double() - g64).abs().max().item() + REL_FLOOR * g64.abs().max().item()


def seed(r, kind, key, zero_grey=False):
    """float32 d loss / d likelihood.  bits: what training sends, -1 / (r ln 2) on live elements and -1 elsewhere;
    mixed: uniform in +-1, both arms of each bound.  zero_grey: no gradient into grey elements (for sums over L)"""
    live, _, grey = classify(r)
    if kind == "bits":
        g = torch.where(live, -1.0 / (r.clamp_min(1e-300) * LN2), torch.full_like(r, -1.0))
    else:
        g = U(key + ".seed", tuple(r.shape), -1.0, 1.0).double()
    if zero_grey:
        g = torch.where(grey, torch.zeros_like(g), g)
    return g.float()


# ------------------------------------------------------------------------------------------------ Gaussian references
def gaussian_round(inp):
    """the float32 rounding decisions round(y - mu)"""
    return torch.round(inp["y"] - inp["mu"])


def gaussian_yhat(inp):
    """((rt - t) + t) + mu in float32, the value of ste_round(y - mu) + mu"""
    t = inp["y"] - inp["mu"]
    return ((torch.round(t) - t) + t) + inp["mu"]


def gaussian_raw(inp, mode):
    """float64 likelihood before the bound (formula of oracle.gaussian_likelihood)"""
    d = cast(inp, torch.float64)
    out = (gaussian_round(inp).double() + d["mu"]) if mode == "eval" else d["y"] + d["noise"]
    s = torch.clamp(d["scale"], min=O.SCALE_BOUND)
    v = (out - d["mu"]).abs()
    c = -(2 ** -0.5)
    return 0.5 * torch.erfc(c * ((0.5 - v) / s)) - 0.5 * torch.erfc(c * ((-0.5 - v) / s))


def gaussian_oracle(inp, mode, dtype, dlik=None):
    """oracle.gaussian_likelihood in ``dtype``: lik, and with a seed (dy, dmu, dscale) of the likelihood alone"""
    d = cast(inp, dtype)
    y, mu, sc = (d[k].requires_grad_(dlik is not None) for k in ("y", "mu", "scale"))
    if mode == "eval":
        _, lik = O.gaussian_likelihood(y, sc, mu, None, round_to=gaussian_round(inp))
    else:
        _, lik = O.gaussian_likelihood(y, sc, mu, d["noise"])
    if dlik is None:
        return lik.detach()
    gs = torch.autograd.grad(lik, [y, mu, sc], dlik.to(dtype), allow_unused=True)
    gs = [torch.zeros_like(y) if g is None else g for g in gs]
    return lik.detach(), gs


def gaussian_round_flips(inp):
    d = cast(inp, torch.float64)
    return int((torch.round(d["y"] - d["mu"]) != gaussian_round(inp).double()).sum())


# ------------------------------------------------------------------------------------------------ bottleneck references
def eb_round(z, sd):
    """float32 round(z - median), [N,C,HW]"""
    return torch.round(z - sd[f"{EB}.quantiles"][:, 0, 1].reshape(1, -1, 1))


def eb_value(inp, sd, mode):
    """float32 value the likelihood is taken at (the kernel's zt)"""
    if mode == "train":
        return inp["z"] + inp["noise"]
    med = sd[f"{EB}.quantiles"][:, 0, 1].reshape(1, -1, 1)
    return torch.round(inp["z"] - med) + med


def eb_round_flips(inp, sd):
    med = sd[f"{EB}.quantiles"][:, 0, 1].reshape(1, -1, 1).double()
    return int((torch.round(inp["z"].double() - med) != eb_round(inp["z"], sd).double()).sum())


def eb_raw(inp, sd, mode):
    """float64 likelihood before the bound, [N,C,HW]"""
    s = cast(sd, torch.float64)
    d = cast(inp, torch.float64)
    N, C, HW = d["z"].shape
    vals = d["z"].transpose(0, 1).reshape(C, 1, -1)
    med = s[f"{EB}.quantiles"][:, :, 1:2]
    out = (torch.round(vals - med) + med) if mode == "eval" else vals + d["noise"].transpose(0, 1).reshape(C, 1, -1)
    lo = O.eb_logits_cumulative(out - 0.5, s, EB, False)
    up = O.eb_logits_cumulative(out + 0.5, s, EB, False)
    sg = -torch.sign(lo + up)
    r = (torch.sigmoid(sg * up) - torch.sigmoid(sg * lo)).abs()
    return r.reshape(C, N, HW).transpose(0, 1).contiguous()


def eb_oracle(inp, sd, mode, dtype, dlik=None):
    """oracle.eb_likelihood in ``dtype``: lik, and with a seed {"z": dz, "quantiles": dq, name: dparam ...} where a
    parameter the likelihood does not depend on gets zeros"""
    s = {k: v.detach().to(dtype).requires_grad_(dlik is not None) for k, v in sd.items()}
    d = cast(inp, dtype)
    z = d["z"].requires_grad_(dlik is not None)
    _, lik = O.eb_likelihood(z, s, EB, d["noise"] if mode == "train" else None)
    if dlik is None:
        return lik.detach()
    names = EB_NAMES + ["quantiles"]
    leaves = [z] + [s[f"{EB}.{n}"] for n in names]
    gs = torch.autograd.grad(lik, leaves, dlik.to(dtype), allow_unused=True)
    gs = [torch.zeros_like(t) if g is None else g for g, t in zip(gs, leaves)]
    return lik.detach(), dict(zip(["z"] + names, gs))


def eb_aux(sd, dtype):
    """(loss, dquantiles) of oracle.eb_aux_loss in ``dtype``; the target is the float32 one the kernel is given"""
    s = {k: v.detach().to(dtype) for k, v in sd.items()}
    q = s[f"{EB}.quantiles"].requires_grad_(True)
    t = float(np.float32(math.log(2 / 1e-9 - 1)))
    target = torch.tensor([-t, 0.0, t], dtype=dtype)
    loss = torch.abs(O.eb_logits_cumulative(q, s, EB, True) - target).sum()
    (dq,) = torch.autograd.grad(loss, [q])
    return loss.detach(), dq


# ------------------------------------------------------------------------------------------------ tables
def gc_pmf(table, centers, max_length, dtype):
    """pmf [ns, max_length] and tail mass [ns] of GaussianConditional.update for given integer centers.
    oracle.gc_update_tables casts to float32 inside, so its formula is restated here for the float64 run."""
    sc = table.to(dtype).unsqueeze(1)
    v = (torch.arange(max_length).unsqueeze(0) - centers.to(torch.int64).unsqueeze(1)).abs().to(dtype)
    c = -(2 ** -0.5)
    up = 0.5 * torch.erfc(c * ((0.5 - v) / sc))
    lo = 0.5 * torch.erfc(c * ((-0.5 - v) / sc))
    return up - lo, 2 * lo[:, 0]


def gc_multiplier(tail_mass=1e-9):
    import scipy.stats
    return float(-scipy.stats.norm.ppf(tail_mass / 2))


def share(mask):
    return mask.double().mean().item()
