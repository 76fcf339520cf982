"""Inputs and float64 references for variable-rate training: the stepped likelihood + STE pair of csrc/qstep.hip
(icm_gc_likelihood_ste_qs_fwd / _bwd) and the per-image weighted R-D loss of csrc/pointwise.hip (icm_rd_loss_w_fwd /
_bwd).  CPU only; shared by tests/test_qtrain_ref.py (which asserts what the GPU tests rely on) and the GPU tests.

The stepped likelihood is restated in torch from its definition, in the dtype of its inputs, with the gradients by
autograd through the oracle's own LowerBound: run on ``.double()`` copies of the float32 inputs it is the reference, run
in float32 it is the yardstick every tolerance is formed from, by the rule and the constants of tests/_entropy_ref.py
(FACTOR times the float32 restatement's own error plus a floor; never anything a kernel returned).  y_hat has no
tolerance: it is tests/_qstep_ref.py's ``dequantize(symbols(...))``, bit for bit.

Per image n the inputs are those of ``_entropy_ref.gaussian_inputs`` in units of the image's step D_n = 2^(K_n / 8):
y = mu + D_n (k + f) with integer k out to 6.5 sigma / D_n and |f| <= 0.45, so that round((y - mu) / D_n) is the same
symbol in float32 and float64.

Everything here reads the (step, inv) pair of an element through ``pair_of``, so it serves a pair per position as well:
tests/_qmtrain_ref.py builds its inputs with ``inputs_at`` and uses these references as they stand."""
import functools
import math

import numpy as np
import torch

import _entropy_ref as R
import _qstep_ref as Q
from oracle import wacnn_oracle as O

SHAPES = {"strided": R.GC_SHAPE, "tiny": (3, 7, 1, 1), "long": R.GC_LONG_SHAPE}
# step index of each image; "zero": no step at all, where the stepped kernels must restate the scalar ones
QSTEPS = {"strided": (-16, 32), "tiny": (-16, 5, 32), "long": (5, 32), "zero": (0, 0)}
CASES = ("strided", "tiny", "long", "zero")
BANDED = ("strided", "long", "zero")     # 21 elements cannot populate five classes at 2 % each: "tiny" is exempt


def shape_of(case):
    return SHAPES.get(case, R.GC_SHAPE)


def step_pairs(case):
    """float32 [N, 2]: (step, inv) of each image, the pairs of bitstream.step_of (restated in _qstep_ref.step_of)"""
    return torch.tensor(np.array([Q.step_of(k) for k in QSTEPS[case]], dtype=np.float32))


def inputs_at(key, shape, step, inv):
    """{y, mu, scale, noise} float32 [N,C,H,W] in units of the float32 ``step`` / ``inv``, which broadcast against
    ``shape``: y = mu + step (k + f), integer k out to 6.5 sigma inv and |f| <= 0.45.  ``key`` prefixes the RNG keys."""
    n = int(np.prod(shape))
    step, inv = (a.expand(shape).reshape(-1) for a in (step, inv))
    table = O.scale_table()
    scale = table[torch.arange(n) % table.numel()] * R.U(key + ".fac", (n,), 0.8, 1.25)
    scale[:7] = torch.tensor([0.11, R.SCALE_BELOW, R.SCALE_ABOVE, 0.0, -1.0, 1e-3, 300.0])
    mu = R.U(key + ".mu", (n,), -3.0, 3.0)
    # in symbols; at a large step many scales fall far below one symbol, where the tail is the symbol next to the mean
    reach = torch.clamp(6.5 * torch.clamp(scale, min=O.SCALE_BOUND) * inv, min=0.75)
    u = R.U(key + ".k", (n,), -1.0, 1.0)
    k = torch.round(torch.sign(u) * u.abs() ** 1.5 * reach)
    f = R.U(key + ".f", (n,), -0.45, 0.45)
    y = mu + step * (k + f)
    noise = R.U(key + ".noise", (n,), -0.5, 0.5)
    return {"y": y.reshape(shape), "mu": mu.reshape(shape), "scale": scale.reshape(shape),
            "noise": noise.reshape(shape)}


def pair_of(inp):
    """float32 (step, inv) of an input set, broadcasting against [N,C,H,W]: its "step" / "inv" where it carries them
    ([N,1,H,W], a pair per position: tests/_qmtrain_ref.py), else the columns of "steps" [N, 2] as [N,1,1,1]"""
    if "inv" in inp:
        return inp["step"], inp["inv"]
    return tuple(inp["steps"][:, c].reshape(-1, 1, 1, 1) for c in (0, 1))


@functools.lru_cache(maxsize=None)
def stepped_inputs(case):
    """{y, mu, scale, noise} float32 [N,C,H,W] and "steps" float32 [N, 2]"""
    shape = shape_of(case)
    steps = step_pairs(case)
    assert steps.shape[0] == shape[0]
    return {**inputs_at("qtn." + case, shape, *pair_of({"steps": steps})), "steps": steps}


def symbols(inp):
    """the float32 symbols round((y - mu) * inv), int32 [N,C,H,W]: tests/_qstep_ref.py's, with the pair of each element"""
    shape = inp["y"].shape
    return torch.from_numpy(Q.symbols(inp["y"].numpy(), inp["mu"].numpy(), pair_of(inp)[1].expand(shape).numpy()))


def yhat(inp):
    """float32 y_hat = (float)symbol * step + mu, two roundings: tests/_qstep_ref.py's dequantize"""
    shape = inp["y"].shape
    return torch.from_numpy(Q.dequantize(symbols(inp).numpy(), inp["mu"].numpy(),
                                         pair_of(inp)[0].expand(shape).numpy()))


def round_flips(inp):
    """symbols float64 arithmetic would round differently"""
    t = (inp["y"].double() - inp["mu"].double()) * pair_of(inp)[1].double()
    return int((torch.round(t) != symbols(inp).double()).sum())


def stepped_value(inp, mode, dtype, y=None, mu=None):
    """the value the likelihood is taken at, in symbol units: the float32 symbol (eval), or (y - mu) * inv + noise"""
    if mode == "eval":
        return symbols(inp).to(dtype)
    y = inp["y"].to(dtype) if y is None else y
    mu = inp["mu"].to(dtype) if mu is None else mu
    return (y - mu) * pair_of(inp)[1].to(dtype) + inp["noise"].to(dtype)


def _cdf_diff(v, s):
    c = -(2 ** -0.5)
    a = v.abs()
    return 0.5 * torch.erfc(c * ((0.5 - a) / s)) - 0.5 * torch.erfc(c * ((-0.5 - a) / s))


def stepped_raw(inp, mode):
    """float64 likelihood before the bound"""
    s = torch.clamp(inp["scale"].double(), min=O.SCALE_BOUND) * pair_of(inp)[1].double()
    return _cdf_diff(stepped_value(inp, mode, torch.float64), s)


def stepped_oracle(inp, mode, dtype, dlik=None):
    """the stepped likelihood in ``dtype``: lik, and with a seed (dy, dmu, dscale) of the likelihood alone"""
    y, mu, sc = (inp[k].detach().to(dtype).requires_grad_(dlik is not None) for k in ("y", "mu", "scale"))
    s = O.lower_bound(sc, O.SCALE_BOUND) * pair_of(inp)[1].to(dtype)
    lik = O.lower_bound(_cdf_diff(stepped_value(inp, mode, dtype, y, mu), s), O.LIK_BOUND)
    if dlik is None:
        return lik.detach()
    gs = torch.autograd.grad(lik, [y, mu, sc], dlik.to(dtype), allow_unused=True)
    return lik.detach(), [torch.zeros_like(y) if g is None else g for g in gs]


# ------------------------------------------------------------------------------------------------ weighted R-D loss
RDW_CASES = {"odd": (3, 3 * 17 * 19, 5 * 320 + 3, 97), "blocks": (2, 3 * 64 * 64, 2 * 320 * 16, 2 * 192)}


@functools.lru_cache(maxsize=None)
def rdw_inputs(case):
    """(x, x_hat [N, img_elems], lik_y, lik_z, lmbda_n [N]) float32; the weights span the range training draws from"""
    import _pointwise_ref as P
    N, per, ny, nz = RDW_CASES[case]
    x = P.u(f"rdw.x.{case}", (N, per), 0.0, 1.0)
    xh = x + P.u(f"rdw.e.{case}", (N, per), -0.1, 0.1) * torch.arange(1, N + 1, dtype=torch.float32).reshape(N, 1)
    lam = torch.tensor([0.0067 * 2.0 ** (-k * 2.0 / 8.0) for k in (-16, 5, 32)[:N]], dtype=torch.float64).float()
    return x, xh, P.likelihoods(f"rdw.ly.{case}", ny), P.likelihoods(f"rdw.lz.{case}", nz), lam


def rdw_loss(x, xh, ly, lz, npix, lam):
    """(bpp, mse, loss, sum log lik_y, sum log lik_z) in the inputs' dtype: loss = 255^2 mean_n(lam_n mse_n) + bpp"""
    sy, sz = torch.log(ly).sum(), torch.log(lz).sum()
    mse_n = ((xh - x) ** 2).mean(1)
    bpp = sy / (-math.log(2.0) * npix) + sz / (-math.log(2.0) * npix)
    return torch.stack([bpp, mse_n.mean(), 255.0 ** 2 * (lam * mse_n).mean() + bpp, sy, sz])


def rdw_grads(x, xh, ly, lz, npix, lam, gscale):
    """gscale * d loss / d (x_hat, lik_y, lik_z) by autograd"""
    xh, ly, lz = (t.detach().clone().requires_grad_(True) for t in (xh, ly, lz))
    loss = rdw_loss(x, xh, ly, lz, npix, lam)[2] * gscale
    return torch.autograd.grad(loss, [xh, ly, lz])


def rdw_loss_limit(x, xh, ly, lz, npix, lam):
    """limit of |gpu - float64| for out[2] of icm_rd_loss_w_fwd on these float64 inputs ([N, img_elems] images): the
    summation bound gamma(k) sum |terms| of tests/_pointwise_ref.py along the chains of ``rdw_chains`` for the weighted
    distortion (one more rounding per term for lmbda_n * se_n, then the quotient and the product by 255^2) and for
    bpp (two sums, the constant's product, two quotients and a sum), and three roundings of the result"""
    import _pointwise_ref as P
    N, per = x.shape
    g = rdw_chains(N, per, ly.numel(), lz.numel())
    se_n = ((xh - x) ** 2).sum(1)
    den = math.log(2.0) * npix
    bpp_terms = (ly.log().abs().sum().item() + lz.log().abs().sum().item()) / den
    wterms = 255.0 ** 2 * (lam * se_n).sum().item() / (N * per)
    ref = rdw_loss(x, xh, ly, lz, npix, lam)[2].abs().item()
    return (P.sum_limit(g["kx"] + 4, wterms) + P.sum_limit(max(g["ky"], g["kz"]) + 4, bpp_terms) + 3 * P.ULP * ref)


def rdw_chains(N, per, ny, nz):
    """longest chains of float32 additions of the weighted reduction, restated from its launch geometry: bpi workgroups
    per image (what the scalar loss gives one image, 2048 in all at the most), T = N bpi in flat order for the two
    likelihood sums; a thread's trips, 6 butterfly steps + 2 across the waves, the finishing workgroup's trips + 8, and
    for the image sums N - 1 more across the images; + 2 roundings inside a term"""
    import _pointwise_ref as P
    bpi = max(1, min(P.grid_for(per, 8), 2048 // N))
    T = N * bpi
    fin = lambda nblk: P.cdiv(nblk, 256) + 8
    kx = P.cdiv(per, bpi * 256) + 8 + fin(bpi) + (N - 1) + 2
    kl = lambda n: P.cdiv(n, T * 256) + 8 + fin(T) + 2
    return {"bpi": bpi, "kx": kx, "ky": kl(ny), "kz": kl(nz)}
