"""CPU restatement of MS-SSIM as this project defines it (the defaults of ``pytorch_msssim.ms_ssim``; Wang, Simoncelli,
Bovik 2003), dtype-generic, differentiable by autograd.  Tests only: nothing under icm_amd/ imports it.

1. window: 11 taps exp(-(k-5)^2 / (2 * 1.5^2)), normalised; separable, per channel, valid (no padding);
2. per level: mu, sigma from the filtered products; cs_map, ssim_map; spatial means cs[n,c], ssim[n,c];
3. five levels, weights WEIGHTS; levels 0..3 contribute relu(cs), level 4 relu(ssim); between levels
   avg_pool2d(2, 2, padding=(h % 2, w % 2)) with the padded zeros counted in the divisor;
4. ms[n,c] = prod_l v_l ** w_l; the scalar is the mean over (n, c);
5. min(H, W) must exceed (11 - 1) * 2^4 = 160.
"""
import torch
import torch.nn.functional as F

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
WIN, SIGMA = 11, 1.5


def window(dtype=torch.float64):
    k = torch.arange(WIN, dtype=dtype) - WIN // 2
    g = torch.exp(-(k ** 2) / (2 * SIGMA ** 2))
    return g / g.sum()


def gaussian_filter(x, g):
    C = x.shape[1]
    x = F.conv2d(x, g.view(1, 1, -1, 1).expand(C, 1, -1, 1), groups=C)      # along H
    return F.conv2d(x, g.view(1, 1, 1, -1).expand(C, 1, 1, -1), groups=C)   # along W


def pool(x):
    return F.avg_pool2d(x, kernel_size=2, stride=2, padding=(x.shape[2] % 2, x.shape[3] % 2))


def ssim_level(X, Y, g, data_range=1.0):
    """(ssim[n,c], cs[n,c]) of one level"""
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mu1, mu2 = gaussian_filter(X, g), gaussian_filter(Y, g)
    s1 = gaussian_filter(X * X, g) - mu1 * mu1
    s2 = gaussian_filter(Y * Y, g) - mu2 * mu2
    s12 = gaussian_filter(X * Y, g) - mu1 * mu2
    cs_map = (2 * s12 + C2) / (s1 + s2 + C2)
    ssim_map = (2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * cs_map
    return ssim_map.flatten(2).mean(-1), cs_map.flatten(2).mean(-1)


def level_values(X, Y, data_range=1.0):
    """[5, N, C]: relu(cs) of levels 0..3, relu(ssim) of level 4"""
    if X.dim() != 4 or X.shape != Y.shape:
        raise ValueError(f"expected two equal [N,C,H,W] shapes, got {tuple(X.shape)} and {tuple(Y.shape)}")
    if min(X.shape[2], X.shape[3]) <= (WIN - 1) * 2 ** 4:
        raise ValueError(f"image sides must exceed {(WIN - 1) * 2 ** 4} pixels, got {X.shape[2]}x{X.shape[3]}")
    g = window(X.dtype)
    vals = []
    for l in range(len(WEIGHTS)):
        ssim, cs = ssim_level(X, Y, g, data_range)
        if l < len(WEIGHTS) - 1:
            vals.append(torch.relu(cs))
            X, Y = pool(X), pool(Y)
        else:
            vals.append(torch.relu(ssim))
    return torch.stack(vals, 0)


def ms_ssim(X, Y, data_range=1.0, size_average=True):
    v = level_values(X, Y, data_range)
    w = torch.tensor(WEIGHTS, dtype=X.dtype).view(-1, 1, 1)
    ms = torch.prod(v ** w, dim=0)
    return ms.mean() if size_average else ms
