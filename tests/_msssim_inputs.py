"""Deterministic inputs of the MS-SSIM tests: a smooth target (sines) and a noisy reconstruction of it."""
import math

import torch

CASES = {
    "crop256": (2, 3, 256, 256),     # the training crop
    "odd175x201": (1, 3, 175, 201),  # odd sizes on several levels: pooling padding and its adjoint
    "min161": (1, 3, 161, 161),      # smallest legal size; the last level has 1x1 statistics
    "gray192x224": (2, 1, 192, 224),
}


def make_pair(shape, seed=0):
    """(target, x_hat) float32 CPU tensors in [0, 1]: target = smooth sines + 0.02 * randn, x_hat = clamp(target +
    0.05 * randn)"""
    N, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    yy = torch.arange(H, dtype=torch.float64).view(1, 1, H, 1)
    xx = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W)
    n = torch.arange(N, dtype=torch.float64).view(N, 1, 1, 1)
    c = torch.arange(C, dtype=torch.float64).view(1, C, 1, 1)
    smooth = 0.5 + 0.25 * torch.sin(2 * math.pi * yy / 37.0 + 0.7 * c + 0.3 * n) * torch.cos(2 * math.pi * xx / 53.0 - 0.4 * c) \
        + 0.15 * torch.sin(2 * math.pi * (xx + 2.0 * yy) / 19.0 + 1.1 * n)
    target = (smooth + 0.02 * torch.randn(shape, generator=g, dtype=torch.float64)).clamp(0, 1)
    x_hat = (target + 0.05 * torch.randn(shape, generator=g, dtype=torch.float64)).clamp(0, 1)
    return target.to(torch.float32), x_hat.to(torch.float32)


def clamp_corner_pair(seed=0):
    """x_hat = 1 - target on a random target: anti-correlated, so some level's cs is non-positive"""
    g = torch.Generator().manual_seed(seed)
    target = torch.rand((1, 3, 192, 192), generator=g, dtype=torch.float32)
    return target, 1.0 - target
