"""compressai/ops mirror: ste_round (ops.py:20-34), LowerBound (bound_ops.py:21-65),
NonNegativeParametrizer (parametrizers.py:23-49).  On the hot path these are fused into the GDN and
likelihood kernels; the standalone forms below exist for API parity and call the same HIP kernels."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib as L
from ._lib import check, ptr


class _SteRound(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        xc = x.contiguous()
        y = torch.empty_like(xc)
        q = torch.zeros(3, dtype=torch.float32, device=x.device)
        check(L.lib().icm_ste_round_offset(ptr(xc), ptr(q), ptr(y), 1, 1, xc.numel(), L.stream()), "ste_round")
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, g):
        return g


def ste_round(x: torch.Tensor) -> torch.Tensor:
    """Rounding with identity gradient: (round(x) - x) + x."""
    return _SteRound.apply(x)


class _LowerBoundFn(torch.autograd.Function):
    """max(x, bound); backward passes g where (x >= bound) | (g < 0)."""

    @staticmethod
    def forward(ctx, x, bound):
        ctx.save_for_backward(x, bound)
        return torch.max(x, bound)

    @staticmethod
    def backward(ctx, g):
        x, bound = ctx.saved_tensors
        return ((x >= bound) | (g < 0)) * g, None


class LowerBound(nn.Module):
    bound: torch.Tensor

    def __init__(self, bound: float):
        super().__init__()
        self.register_buffer("bound", torch.Tensor([float(bound)]))

    def forward(self, x):
        return _LowerBoundFn.apply(x, self.bound)


class _NonNegFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bound, pedestal):
        xc = x.contiguous()
        out = torch.empty_like(xc)
        check(L.lib().icm_nonneg_fwd(ptr(xc), ptr(out), xc.numel(), bound, pedestal, L.stream()), "nonneg_fwd")
        ctx.save_for_backward(xc)
        ctx.bound = bound
        return out.view(x.shape)

    @staticmethod
    def backward(ctx, g):
        (xc,) = ctx.saved_tensors
        gc = g.contiguous()
        dx = torch.empty_like(xc)
        check(L.lib().icm_nonneg_bwd(ptr(xc), ptr(gc), ptr(dx), xc.numel(), ctx.bound, 0, L.stream()), "nonneg_bwd")
        return dx.view(g.shape), None, None


class NonNegativeParametrizer(nn.Module):
    pedestal: torch.Tensor

    def __init__(self, minimum: float = 0, reparam_offset: float = 2 ** -18):
        super().__init__()
        self.minimum = float(minimum)
        self.reparam_offset = float(reparam_offset)
        pedestal = self.reparam_offset ** 2
        self.register_buffer("pedestal", torch.Tensor([pedestal]))
        self._bound = (self.minimum + self.reparam_offset ** 2) ** 0.5
        self._pedestal = pedestal
        self.lower_bound = LowerBound(self._bound)

    def init(self, x):
        return torch.sqrt(torch.max(x + self.pedestal, self.pedestal))

    def forward(self, x):
        return _NonNegFn.apply(x, self._bound, self._pedestal)


# ---------------------------------------------------------------- MS-SSIM (icm_msssim_fwd / icm_msssim_bwd)
MS_SSIM_MIN_SIDE = 160   # (11 - 1) * 2^4: both sides must exceed it


def _msssim_check(x: torch.Tensor, y: torch.Tensor) -> None:
    if not (torch.is_tensor(x) and torch.is_tensor(y)):
        raise ValueError("ms_ssim expects two tensors")
    if x.dim() != 4 or y.dim() != 4:
        raise ValueError(f"ms_ssim expects [N,C,H,W] inputs, got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.shape != y.shape:
        raise ValueError(f"ms_ssim: shapes differ: {tuple(x.shape)} vs {tuple(y.shape)}")
    if not (x.is_cuda and y.is_cuda):
        raise ValueError("ms_ssim runs on the GPU only (no CPU fallback)")
    if x.dtype != torch.float32 or y.dtype != torch.float32:
        raise ValueError("ms_ssim expects float32 inputs")
    if min(x.shape[2], x.shape[3]) <= MS_SSIM_MIN_SIDE:
        raise ValueError(f"ms_ssim: image sides must exceed {MS_SSIM_MIN_SIDE} pixels (five levels of an 11-tap "
                         f"window), got {x.shape[2]}x{x.shape[3]}")


def msssim_workspace(x: torch.Tensor) -> torch.Tensor:
    """the caller-owned scratch of icm_msssim_fwd / icm_msssim_bwd for inputs shaped like x"""
    N, Cc, H, W = x.shape
    n = L.lib().icm_msssim_workspace_floats(N, Cc, H, W)
    if n <= 0:
        raise ValueError(f"ms_ssim: unsupported geometry {tuple(x.shape)}")
    return torch.empty(n, dtype=torch.float32, device=x.device)


class _MsSsimFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, data_range):
        x, y = x.contiguous(), y.contiguous()
        N, Cc, H, W = x.shape
        ws = msssim_workspace(x)
        ms = torch.empty((N, Cc), dtype=torch.float32, device=x.device)
        out = torch.empty(2, dtype=torch.float32, device=x.device)
        check(L.lib().icm_msssim_fwd(ptr(x), ptr(y), N, Cc, H, W, float(data_range), ptr(ms), ptr(out), 0.0, 0,
                                     ptr(ws), ws.numel(), L.stream()), "msssim_fwd")
        ctx.save_for_backward(x, y, ws)
        return ms, out[0]

    @staticmethod
    def backward(ctx, g_ms, g_mean):
        x, y, ws = ctx.saved_tensors
        N, Cc, H, W = x.shape
        # upstream weight of every plane: the [N,C] output's own gradient plus the mean's share
        g = torch.zeros((N, Cc), dtype=torch.float32, device=x.device)
        if g_ms is not None:
            g = g + g_ms
        if g_mean is not None:
            g = g + g_mean / (N * Cc)
        g = g.contiguous()
        dx = torch.empty_like(x)
        check(L.lib().icm_msssim_bwd(ptr(x), ptr(y), N, Cc, H, W, ptr(g), 1.0, ptr(dx), ptr(ws), ws.numel(),
                                     L.stream()), "msssim_bwd")
        return dx, None, None


def ms_ssim(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0, size_average: bool = True) -> torch.Tensor:
    """MS-SSIM of x against y, [N,C,H,W] float32 device tensors in [0, data_range] (the definition and defaults of
    ``pytorch_msssim.ms_ssim``).  Returns the mean over (n, c), or the [N,C] values with ``size_average=False``.
    Differentiable in x only (y is the target)."""
    _msssim_check(x, y)
    ms, mean = _MsSsimFn.apply(x, y, float(data_range))
    return mean if size_average else ms
