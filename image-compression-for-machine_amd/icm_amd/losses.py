"""RateDistortionLoss (train.py:44-76; loss form of train_czigzag.py:63,71) on the fused HIP reductions, with the
MS-SSIM distortion of upstream CompressAI's RateDistortionLoss(metric="ms-ssim") as an option."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib as L
from ._lib import check, ptr


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
    mse_loss stays the plain mean."""

    def __init__(self, lmbda=1e-2, metric="mse"):
        super().__init__()
        if metric not in METRICS:
            raise NotImplementedError(f"{metric} is not implemented!")
        self.lmbda = float(lmbda)
        self.metric = metric

    def forward(self, output, target, lmbda_n=None):
        lik = output["likelihoods"]
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
