"""Inputs and float64 references for quality-map training: the likelihood + STE pair with a quantiser step per (image,
latent position) of csrc/qstep.hip (icm_gc_likelihood_ste_qm_fwd / _bwd), the R-D loss with a distortion weight per
16 x 16 cell of csrc/pointwise.hip (icm_rd_loss_m_fwd / _bwd) and the map painter (icm_qmap_paint).  CPU only; shared by
tests/test_qmtrain_ref.py (which asserts what the GPU tests rely on) and the GPU tests.

The rule, the input generator and the likelihood references are tests/_qtrain_ref.py's own, read with a (step, inv) pair
per POSITION where that module's cases carry one per image: the inputs are ``_qtrain_ref.inputs_at`` in units of each
position's step D = 2^(k / 8), k the map's entry, and y_hat is tests/_qstep_ref.py's numpy arithmetic with the step of
each position, bit for bit.  This module holds what is the map's own: the maps, the step table, the per-cell loss and
the painter."""
import functools
import math

import numpy as np
import torch

import _entropy_ref as R
import _pointwise_ref as P
import _qstep_ref as Q
import _qtrain_ref as T

MAP_CASES = ("strided", "tiny", "long", "uniform")
BANDED = ("strided", "long", "uniform")      # 21 elements cannot populate five classes: "tiny" is exempt
KS = tuple(range(Q.QSTEP_MIN, Q.QSTEP_MAX + 1))
assert len(KS) == 49


def shape_of(case):
    return T.SHAPES.get(case, R.GC_SHAPE)


def step_table():
    """float32 [256, 2]: row b the (step, inv) of the map byte b read as unsigned, (1, 1) for bytes that are no valid k
    (bitstream.step_table restated with tests/_qstep_ref.py's step_of)"""
    t = np.ones((256, 2), dtype=np.float32)
    for k in KS:
        t[k & 0xFF] = Q.step_of(k)
    return t


@functools.lru_cache(maxsize=None)
def maps(case):
    """int8 [N, H, W]: a map per image"""
    N, _, H, W = shape_of(case)
    if case == "strided":        # every image's cells cycle through all 49 step indexes, each image from its own start
        idx = np.arange(H * W).reshape(1, H, W) + 7 * np.arange(N).reshape(N, 1, 1)
        m = np.asarray(KS)[idx % 49]
    elif case == "tiny":
        m = np.asarray([-16, 5, 32]).reshape(3, 1, 1)
    elif case == "long":         # two levels: a rectangle in a background, the levels swapped in the second image
        m = np.full((N, H, W), 12)
        m[0, 8:24, 5:20] = -8
        m[1] = -8
        m[1, 3:30, 11:29] = 12
    elif case == "uniform":
        m = np.asarray(T.QSTEPS["strided"]).reshape(N, 1, 1) * np.ones((1, H, W), dtype=np.int64)
    else:
        raise KeyError(case)
    return np.ascontiguousarray(m, dtype=np.int8)


def pairs(m):
    """(step, inv) float32 arrays [N, 1, H, W] of an int8 map [N, H, W]"""
    t = step_table()[np.asarray(m).view(np.uint8)]
    return t[..., 0][:, None], t[..., 1][:, None]


@functools.lru_cache(maxsize=None)
def inputs(case):
    """{y, mu, scale, noise} float32 [N,C,H,W], "qmap" int8 [N,H,W], "step" / "inv" float32 [N,1,H,W]"""
    m = maps(case)
    step, inv = (torch.from_numpy(a) for a in pairs(m))
    return {**T.inputs_at("qmn." + case, shape_of(case), step, inv), "qmap": torch.from_numpy(m), "step": step,
            "inv": inv}


def per_image_steps(case):
    """float32 [N, 2] (step, inv) of a case whose maps are uniform over each image: what the _qs pair takes"""
    m = maps(case)
    assert (m == m[:, :1, :1]).all()
    return torch.tensor(np.array([Q.step_of(int(k)) for k in m[:, 0, 0]], dtype=np.float32))


# the references of tests/_qtrain_ref.py read "step" / "inv" where an input set carries them
symbols, yhat, round_flips, raw, oracle = T.symbols, T.yhat, T.round_flips, T.stepped_raw, T.stepped_oracle


# ------------------------------------------------------------------------------------------------ per-cell R-D loss
CELL = 16
LMBDA, LMBDA_EXP = 0.0067, 2.0
# (N, C, H, W): one cell; 3 x 5 cells, odd counts, 80-pixel rows (three rows per pass of a workgroup, whose chunks end
# inside cells); maps spanning -16 .. 32
LOSS_CASES = {"cell": (1, 3, 16, 16), "odd": (3, 3, 48, 80), "span": (2, 3, 64, 64)}


def lmbda_table(lmbda=LMBDA, exp=LMBDA_EXP):
    """float32 [256]: entry k & 255 = lmbda 2^(-k exp / 8) formed in double, the k = 0 value for bytes that are no k"""
    t = np.full(256, lmbda, dtype=np.float64)
    for k in KS:
        t[k & 0xFF] = lmbda * 2.0 ** (-k * exp / 8.0)
    return torch.from_numpy(t).float()


@functools.lru_cache(maxsize=None)
def loss_maps(case):
    N, _, H, W = LOSS_CASES[case]
    h, w = H // CELL, W // CELL
    if case == "cell":
        m = np.full((1, 1, 1), 5)
    elif case == "odd":
        m = np.asarray(KS)[(11 * np.arange(N * h * w)) % 49].reshape(N, h, w)
    else:
        m = np.round(np.linspace(-16, 32, N * h * w)).astype(np.int64).reshape(N, h, w)
        assert m.min() == -16 and m.max() == 32
    return np.ascontiguousarray(m, dtype=np.int8)


def pixel_weights(m, table, dtype=torch.float64):
    """[N, 1, H, W]: the table entry of the cell that holds each pixel, from an int8 map [N, h, w]"""
    lam = table.to(dtype)[torch.from_numpy(np.asarray(m).view(np.uint8).astype(np.int64))]
    return lam.repeat_interleave(CELL, 1).repeat_interleave(CELL, 2)[:, None]


@functools.lru_cache(maxsize=None)
def loss_inputs(case):
    """(x, x_hat [N,C,H,W], lik_y, lik_z, qmap int8 [N,h,w]) float32"""
    N, C, H, W = LOSS_CASES[case]
    ny, nz = N * 40 * (H // CELL) * (W // CELL) + 3, 97 * N
    x = P.u(f"rdm.x.{case}", (N, C, H, W), 0.0, 1.0)
    xh = x + P.u(f"rdm.e.{case}", (N, C, H, W), -0.1, 0.1) * torch.arange(1, N + 1, dtype=torch.float32).reshape(N, 1, 1, 1)
    return x, xh, P.likelihoods(f"rdm.ly.{case}", ny), P.likelihoods(f"rdm.lz.{case}", nz), loss_maps(case)


def m_loss(x, xh, ly, lz, npix, lam):
    """(bpp, mse, loss, sum log lik_y, sum log lik_z) in the inputs' dtype, ``lam`` [N,1,H,W] the weight of each pixel:
    loss = 255^2 sum_i(lam_i (x_hat_i - x_i)^2) / (N C H W) + bpp"""
    sy, sz = torch.log(ly).sum(), torch.log(lz).sum()
    sq = (xh - x) ** 2
    bpp = sy / (-math.log(2.0) * npix) + sz / (-math.log(2.0) * npix)
    return torch.stack([bpp, sq.mean(), 255.0 ** 2 * (lam * sq).sum() / sq.numel() + bpp, sy, sz])


def m_grads(x, xh, ly, lz, npix, lam, gscale):
    """gscale * d loss / d (x_hat, lik_y, lik_z) by autograd"""
    xh, ly, lz = (t.detach().clone().requires_grad_(True) for t in (xh, ly, lz))
    return torch.autograd.grad(m_loss(x, xh, ly, lz, npix, lam)[2] * gscale, [xh, ly, lz])


def m_chains(N, C, H, W, ny, nz):
    """longest chains of float32 additions of the per-cell reduction, restated from its launch geometry: a workgroup
    takes rpb = 256 / W rows of W pixels per pass (1 from W = 256 on), a thread 8 rows, so bpi = ceil(C H / (8 rpb))
    workgroups per image, 2048 in all at the most; T = N bpi partials per sum.  A thread's trips (rows it takes times
    256-pixel strides of a row), 6 butterfly steps + 2 across the waves, the finishing workgroup's trips + 8 over the T
    partials; + 2 roundings inside a term (+ 1 in the weighted sum, for the weight's product)"""
    rows, rpb = C * H, (1 if W >= 256 else 256 // W)
    bpi = max(1, min(P.cdiv(rows, 8 * rpb), 2048 // N))
    T_ = N * bpi
    fin = P.cdiv(T_, 256) + 8
    kx = P.cdiv(rows, bpi * rpb) * P.cdiv(W, 256) + 8 + fin + 2
    kl = lambda n: P.cdiv(n, T_ * 256) + 8 + fin + 2
    return {"bpi": bpi, "rpb": rpb, "T": T_, "kx": kx, "kw": kx + 1, "ky": kl(ny), "kz": kl(nz)}


def m_loss_limit(x, xh, ly, lz, npix, lam):
    """limit of |gpu - float64| for out[2] of icm_rd_loss_m_fwd on these float64 inputs, the form of
    ``_qtrain_ref.rdw_loss_limit``: gamma(k) sum |terms| along the chains of ``m_chains`` for the weighted distortion
    (then the quotient and the product by 255^2) and for bpp (two sums, the constant's product, two quotients and a
    sum), and three roundings of the result"""
    N, C, H, W = x.shape
    g = m_chains(N, C, H, W, ly.numel(), lz.numel())
    den = math.log(2.0) * npix
    bpp_terms = (ly.log().abs().sum().item() + lz.log().abs().sum().item()) / den
    wterms = 255.0 ** 2 * (lam * (xh - x) ** 2).sum().item() / x.numel()
    ref = m_loss(x, xh, ly, lz, npix, lam)[2].abs().item()
    return P.sum_limit(g["kw"] + 4, wterms) + P.sum_limit(max(g["ky"], g["kz"]) + 4, bpp_terms) + 3 * P.ULP * ref


# ------------------------------------------------------------------------------------------------ painter
def paint(base, rects, h, w):
    """int8 [N, h, w]: every cell of image n holds base[n], then its rectangles (y0, x0, y1, x1, k), cells, half open,
    are painted in order, later ones winning; a rectangle is clipped to the map, an empty one paints nothing"""
    base, rects = np.asarray(base), np.asarray(rects)
    N = base.shape[0]
    out = np.empty((N, h, w), dtype=np.int8)
    for n in range(N):
        out[n] = base[n]
        for y0, x0, y1, x1, k in rects[n].reshape(-1, 5).tolist():
            y0, x0, y1, x1 = max(y0, 0), max(x0, 0), min(y1, h), min(x1, w)
            if y1 > y0 and x1 > x0:
                out[n, y0:y1, x0:x1] = k
    return out
