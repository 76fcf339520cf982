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


LOWQ_SHAPE = FLAT_SHAPE = (1, 3, 192, 208)

# name -> shape of the inputs of tests/test_gpu_msssim_numerics.py; numerics_pair(name) builds them
NUMERICS_CASES = {
    "planes258": (43, 6, 161, 161),      # more planes than the finish kernel has threads, at the smallest legal size
    "tile_exact": (1, 2, 170, 202),      # statistics map 160 x 192: a whole number of 32 x 32 tiles
    "tile_plus1": (1, 2, 171, 203),      # one row and one column past that
    "wide": (1, 1, 161, 700),            # 22 tiles along x, 5 along y
    "tall": (1, 1, 700, 163),
    "range255": CASES["odd175x201"],     # the odd175x201 pair times 255, data_range = 255
    "lowq_noise": LOWQ_SHAPE,            # x_hat = clamp(target + 0.35 * randn)
    "lowq_contrast": LOWQ_SHAPE,         # x_hat = clamp(0.5 * target + 0.25 + 0.2 * randn)
    "flat_blocks": FLAT_SHAPE,           # a block of exactly 1.0 and a block of exactly 0.0 in both images
    "flat_blocks_dim": FLAT_SHAPE,       # the same, the reconstruction's bright block at 0.98
    "entry161x175": (2, 3, 161, 175),    # the direct C entry in the trainer's form
    "stage192x224": (1, 3, 192, 224),    # W % 4 == 0 on the first levels: vector or scalar staging by alignment
    "odd175x201": CASES["odd175x201"],
}
LOWQ_CASES = ("lowq_noise", "lowq_contrast")


def numerics_pair(name):
    """(target, x_hat, data_range) of a NUMERICS_CASES entry, float32 CPU tensors in [0, data_range]"""
    shape = NUMERICS_CASES[name]
    t, xh = make_pair(shape)
    if name == "range255":
        return t * 255.0, xh * 255.0, 255.0
    if name in LOWQ_CASES:
        g = torch.Generator().manual_seed(1)
        noise = torch.randn(shape, generator=g, dtype=torch.float64)
        t64 = t.double()
        x64 = t64 + 0.35 * noise if name == "lowq_noise" else 0.5 * t64 + 0.25 + 0.2 * noise
        return t, x64.clamp(0, 1).to(torch.float32), 1.0
    if name in ("flat_blocks", "flat_blocks_dim"):
        for img, bright in ((t, 1.0), (xh, 1.0 if name == "flat_blocks" else 0.98)):
            img[:, :, :64, :80] = bright
            img[:, :, 100:, 120:] = 0.0
    return t, xh, 1.0


ONE_LEVEL_CLAMP_PLANE = 1


def one_level_clamp_pair(a=0.1):
    """A make_pair whose plane ONE_LEVEL_CLAMP_PLANE carries columns of alternating sign, +a (-1)^x in the target and
    -a (-1)^x in the reconstruction.  The stripes are the only content a level-0 window sees much variance in, and
    they are anti-correlated, so the level-0 cs of that plane is negative; every side is even on levels 0..3
    (192 -> 96 -> 48 -> 24), so the first 2x2 pooling removes the stripes exactly and levels 1..4 see the plain pair."""
    t, xh = make_pair((1, 3, 192, 192))
    stripes = a * (1.0 - 2.0 * (torch.arange(192) % 2).float()).view(1, 192)
    p = ONE_LEVEL_CLAMP_PLANE
    t[:, p] = 0.8 * t[:, p] + 0.1 + stripes       # stays inside [0, 1]
    xh[:, p] = 0.8 * xh[:, p] + 0.1 - stripes
    return t, xh


def clamp_corner_pair(seed=0):
    """x_hat = 1 - target on a random target: anti-correlated, so some level's cs is non-positive"""
    g = torch.Generator().manual_seed(seed)
    target = torch.rand((1, 3, 192, 192), generator=g, dtype=torch.float32)
    return target, 1.0 - target
