"""RateDistortionLoss (train.py:44-76; loss form of train_czigzag.py:63,71) on the fused HIP reductions, with the
MS-SSIM distortion of upstream CompressAI's RateDistortionLoss(metric="ms-ssim") as an option."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from ._lib import check, ptr
from .bitstream import QSTEP_MAX, QSTEP_MIN, check_qmap


class _RDFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, x_hat, lik_y, lik_z, lmbda):
        x, x_hat, lik_y, lik_z = (t.contiguous() for t in (x, x_hat, lik_y, lik_z))
        N, _, H, W = x.shape
        out = torch.empty(5, dtype=torch.float32, device=x.device)
        ws = torch.empty(L.REDUCE_WS_FLOATS, dtype=torch.float32, device=x.device)
        check(L.lib().icm_rd_loss_fwd(ptr(x), ptr(x_hat), x.numel(), ptr(lik_y), lik_y.numel(), ptr(lik_z),
                                      lik_z.numel(), N * H * W, lmbda, ptr(out), ptr(ws), L.stream()), "rd_loss_fwd")
        ctx.save_for_backward(x, x_hat, lik_y, lik_z)
        ctx.lmbda, ctx.npix = lmbda, N * H * W
        return out[2], out[0], out[1]

    @staticmethod
    def backward(ctx, g_loss, g_bpp, g_mse):
        x, x_hat, lik_y, lik_z = ctx.saved_tensors
        dxh, dly, dlz = torch.empty_like(x_hat), torch.empty_like(lik_y), torch.empty_like(lik_z)
        check(L.lib().icm_rd_loss_bwd(ptr(x), ptr(x_hat), x.numel(), ptr(lik_y), lik_y.numel(), ptr(lik_z),
                                      lik_z.numel(), ctx.npix, ctx.lmbda, 1.0, ptr(dxh), ptr(dly), ptr(dlz),
                                      L.stream()), "rd_loss_bwd")
        g = g_loss if g_loss is not None else torch.ones((), device=x.device)
        return None, dxh * g, dly * g, dlz * g, None


class _RDWFn(torch.autograd.Function):
    """_RDFn with a distortion weight per image, lmbda_n [N] on the device (icm_rd_loss_w_fwd / _bwd)"""

    @staticmethod
    def forward(ctx, x, x_hat, lik_y, lik_z, lmbda_n):
        x, x_hat, lik_y, lik_z = (t.contiguous() for t in (x, x_hat, lik_y, lik_z))
        N, _, H, W = x.shape
        out = torch.empty(5, dtype=torch.float32, device=x.device)
        ws = torch.empty(L.REDUCE_WS_FLOATS, dtype=torch.float32, device=x.device)
        check(L.lib().icm_rd_loss_w_fwd(ptr(x), ptr(x_hat), N, x[0].numel(), ptr(lik_y), lik_y.numel(), ptr(lik_z),
                                        lik_z.numel(), N * H * W, ptr(lmbda_n), ptr(out), ptr(ws), L.stream()),
              "rd_loss_w_fwd")
        ctx.save_for_backward(x, x_hat, lik_y, lik_z, lmbda_n)
        ctx.npix = N * H * W
        return out[2], out[0], out[1]

    @staticmethod
    def backward(ctx, g_loss, g_bpp, g_mse):
        x, x_hat, lik_y, lik_z, lmbda_n = ctx.saved_tensors
        dxh, dly, dlz = torch.empty_like(x_hat), torch.empty_like(lik_y), torch.empty_like(lik_z)
        check(L.lib().icm_rd_loss_w_bwd(ptr(x), ptr(x_hat), x.shape[0], x[0].numel(), ptr(lik_y), lik_y.numel(),
                                        ptr(lik_z), lik_z.numel(), ctx.npix, ptr(lmbda_n), 1.0, ptr(dxh), ptr(dly),
                                        ptr(dlz), L.stream()), "rd_loss_w_bwd")
        g = g_loss if g_loss is not None else torch.ones((), device=x.device)
        return None, dxh * g, dly * g, dlz * g, None


CELL = 16   # pixels per latent position and side: a quality map's cell


def qmap_lmbda_table(lmbda: float, lmbda_exp: float = 2.0) -> torch.Tensor:
    """The distortion weight of every map byte, as the per-cell loss takes it (host f32 [256], indexed by the byte read
    as unsigned): entry k & 255 holds lmbda * 2^(-k * lmbda_exp / 8) for each step index k, formed in double as
    ``trainer.qstep_tables`` forms it; bytes that are no valid k hold the k = 0 value."""
    t = [float(lmbda)] * 256
    for k in range(QSTEP_MIN, QSTEP_MAX + 1):
        t[k & 255] = float(lmbda) * 2.0 ** (-k * float(lmbda_exp) / 8.0)
    return torch.tensor(t, dtype=torch.float64).to(torch.float32)


class _RDMFn(torch.autograd.Function):
    """_RDFn with a distortion weight per 16 x 16 cell: qmap [N, H/16, W/16] int8 and the 256-entry weight table, both
    on the device (icm_rd_loss_m_fwd / _bwd)"""

    @staticmethod
    def forward(ctx, x, x_hat, lik_y, lik_z, qmap, table):
        x, x_hat, lik_y, lik_z = (t.contiguous() for t in (x, x_hat, lik_y, lik_z))
        N, Cc, H, W = x.shape
        out = torch.empty(5, dtype=torch.float32, device=x.device)
        ws = torch.empty(L.REDUCE_WS_FLOATS, dtype=torch.float32, device=x.device)
        check(L.lib().icm_rd_loss_m_fwd(ptr(x), ptr(x_hat), N, Cc, H, W, CELL, ptr(qmap), ptr(table), ptr(lik_y),
                                        lik_y.numel(), ptr(lik_z), lik_z.numel(), N * H * W, ptr(out), ptr(ws),
                                        L.stream()), "rd_loss_m_fwd")
        ctx.save_for_backward(x, x_hat, lik_y, lik_z, qmap, table)
        return out[2], out[0], out[1]

    @staticmethod
    def backward(ctx, g_loss, g_bpp, g_mse):
        x, x_hat, lik_y, lik_z, qmap, table = ctx.saved_tensors
        N, Cc, H, W = x.shape
        dxh, dly, dlz = torch.empty_like(x_hat), torch.empty_like(lik_y), torch.empty_like(lik_z)
        check(L.lib().icm_rd_loss_m_bwd(ptr(x), ptr(x_hat), N, Cc, H, W, CELL, ptr(qmap), ptr(table), ptr(lik_y),
                                        lik_y.numel(), ptr(lik_z), lik_z.numel(), N * H * W, 1.0, ptr(dxh), ptr(dly),
                                        ptr(dlz), L.stream()), "rd_loss_m_bwd")
        g = g_loss if g_loss is not None else torch.ones((), device=x.device)
        return None, dxh * g, dly * g, dlz * g, None, None


def _maps(qmap, target):
    """the maps as the kernels take them: a contiguous int8 [N, H/16, W/16] tensor on the target's device, from one map
    per image or one [H/16, W/16] map for the batch; every map checked by ``bitstream.check_qmap``"""
    N, _, H, W = target.shape
    if H % CELL or W % CELL:
        raise ValueError(f"qmap: the image sides must be multiples of {CELL}, got {H}x{W}")
    hw = (H // CELL, W // CELL)
    a = qmap.detach().cpu().numpy() if torch.is_tensor(qmap) else np.asarray(qmap)
    if a.ndim == 2:
        a = np.broadcast_to(check_qmap(a, hw, 0, "loss: "), (N,) + hw)
    elif a.ndim == 3 and a.shape[0] == N:
        a = np.stack([check_qmap(m, hw, 0, "loss: ") for m in a])
    else:
        raise ValueError(f"qmap: expected a map {hw} or one per image {(N,) + hw}, got shape {tuple(a.shape)}")
    return torch.from_numpy(np.ascontiguousarray(a)).to(target.device)


def _weights(lmbda_n, target):
    """the per-image weights as the kernels take them: a contiguous f32 [N] tensor on the target's device"""
    w = torch.as_tensor(lmbda_n, dtype=torch.float32).to(target.device).contiguous()
    if tuple(w.shape) != (target.shape[0],):
        raise ValueError(f"lmbda_n: expected {target.shape[0]} weights, one per image, got shape {tuple(w.shape)}")
    return w


METRICS = ("mse", "ms-ssim")


class RateDistortionLoss(nn.Module):
    """metric="mse" (default): loss = lmbda * 255^2 * mse + bpp; returns {"loss","bpp_loss","mse_loss"} like the
    reference.  metric="ms-ssim" (CompressAI's form): loss = lmbda * (1 - ms_ssim(x_hat, target)) + bpp; returns
    {"loss","bpp_loss","ms_ssim_loss"} with ms_ssim_loss = 1 - ms_ssim.
    ``forward(output, target, lmbda_n)`` (mse only): a weight per image instead of ``lmbda``, loss =
    255^2 * mean_n(lmbda_n * mse_n) + bpp -- what variable-rate training minimises (``Trainer(qstep_range=...)``);
    mse_loss stays the plain mean.
    ``forward(output, target, qmap=maps, lmbda_exp=E)`` (mse only): a weight per 16 x 16 cell of pixels from a quality
    map (one [H/16, W/16] for the batch or one per image), lmbda_i = lmbda * 2^(-k_i * E / 8) at the cell's step index
    k_i: loss = 255^2 * mean_i(lmbda_i * (x_hat_i - x_i)^2) + bpp -- what quality-map training minimises
    (``Trainer(qmap_rects=...)``)."""

    def __init__(self, lmbda=1e-2, metric="mse"):
        super().__init__()
        if metric not in METRICS:
            raise NotImplementedError(f"{metric} is not implemented!")
        self.lmbda = float(lmbda)
        self.metric = metric

    def forward(self, output, target, lmbda_n=None, qmap=None, lmbda_exp=2.0):
        lik = output["likelihoods"]
        if qmap is not None:
            if self.metric != "mse":
                raise ValueError("qmap: the MS-SSIM loss takes a scalar lmbda")
            if lmbda_n is not None:
                raise ValueError("qmap and lmbda_n are two weightings of the distortion; give one")
            table = qmap_lmbda_table(self.lmbda, lmbda_exp).to(target.device)
            loss, bpp, mse = _RDMFn.apply(target, output["x_hat"], lik["y"], lik["z"], _maps(qmap, target), table)
            return {"loss": loss, "bpp_loss": bpp.detach(), "mse_loss": mse.detach()}
        if lmbda_n is not None:
            if self.metric != "mse":
                raise ValueError("lmbda_n: the MS-SSIM loss takes a scalar lmbda")
            loss, bpp, mse = _RDWFn.apply(target, output["x_hat"], lik["y"], lik["z"], _weights(lmbda_n, target))
            return {"loss": loss, "bpp_loss": bpp.detach(), "mse_loss": mse.detach()}
        if self.metric == "mse":
            loss, bpp, mse = _RDFn.apply(target, output["x_hat"], lik["y"], lik["z"], self.lmbda)
            return {"loss": loss, "bpp_loss": bpp.detach(), "mse_loss": mse.detach()}
        from .ops import ms_ssim
        # the rate term from the same fused reduction (lmbda = 0: its loss output is bpp, with the bpp gradient)
        rate, bpp, _ = _RDFn.apply(target, output["x_hat"], lik["y"], lik["z"], 0.0)
        dist = 1.0 - ms_ssim(output["x_hat"], target, data_range=1.0)
        return {"loss": self.lmbda * dist + rate, "bpp_loss": bpp.detach(), "ms_ssim_loss": dist.detach()}
