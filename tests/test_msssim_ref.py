"""The float64 CPU restatement of MS-SSIM (tests/_msssim_ref.py) against hand-checkable cases, the conditions
that the inputs of the GPU numerics tests (tests/_msssim_inputs.py) must meet, and the host-side surface of the
feature that exists without a GPU (loss constructor, CLI parsers)."""
import pytest
import torch

import _msssim_ref as R
from _msssim_inputs import (LOWQ_CASES, NUMERICS_CASES, ONE_LEVEL_CLAMP_PLANE, make_pair, numerics_pair,
                            one_level_clamp_pair)


def test_identical_images_give_exactly_one():
    t, _ = make_pair((1, 3, 192, 200))
    t = t.double()
    assert R.ms_ssim(t, t.clone()).item() == 1.0
    assert torch.equal(R.ms_ssim(t, t.clone(), size_average=False), torch.ones(1, 3, dtype=torch.float64))


def test_symmetric_in_its_arguments():
    t, xh = make_pair((1, 2, 170, 181))
    a = R.ms_ssim(xh.double(), t.double(), size_average=False)
    b = R.ms_ssim(t.double(), xh.double(), size_average=False)
    assert torch.allclose(a, b, rtol=0, atol=1e-15)


@pytest.mark.parametrize("a,b", [(0.3, 0.6), (0.9, 0.1)])
def test_constant_images(a, b):
    # zero variance and covariance: cs = C2 / C2 = 1 on every level; only the luminance term of level 4 remains.
    # 176 -> 88 -> 44 -> 22 -> 11 and 192 -> 96 -> 48 -> 24 -> 12: every pooled level is even-sized, so no padded zeros
    # are mixed in and the images stay constant down the pyramid
    X = torch.full((1, 1, 176, 192), a, dtype=torch.float64)
    Y = torch.full((1, 1, 176, 192), b, dtype=torch.float64)
    v = R.level_values(X, Y)
    assert torch.allclose(v[:4], torch.ones_like(v[:4]), rtol=0, atol=1e-12)
    C1 = 0.01 ** 2
    want = ((2 * a * b + C1) / (a * a + b * b + C1)) ** 0.1333
    assert R.ms_ssim(X, Y).item() == pytest.approx(want, rel=1e-12)


def test_pooling_of_an_odd_level():
    x = torch.tensor([[1., 2., 3.], [4., 5., 6.], [7., 8., 9.]], dtype=torch.float64).view(1, 1, 3, 3)
    # padding (1, 1) puts a zero row / column in FRONT; windows start at -1: rows {-1,0}, {1,2}; the divisor is always 4
    want = torch.tensor([[1 / 4, (2 + 3) / 4], [(4 + 7) / 4, (5 + 6 + 8 + 9) / 4]], dtype=torch.float64)
    assert torch.equal(R.pool(x).view(2, 2), want)
    # mixed parity: 3 rows (padded), 4 columns (not)
    y = torch.arange(12, dtype=torch.float64).view(1, 1, 3, 4)
    want = torch.tensor([[(0 + 1) / 4, (2 + 3) / 4], [(4 + 5 + 8 + 9) / 4, (6 + 7 + 10 + 11) / 4]], dtype=torch.float64)
    assert torch.equal(R.pool(y).view(2, 2), want)


def test_size_limit():
    with pytest.raises(ValueError):
        R.ms_ssim(torch.rand(1, 1, 160, 256, dtype=torch.float64), torch.rand(1, 1, 160, 256, dtype=torch.float64))
    v = R.ms_ssim(torch.rand(1, 1, 161, 161, dtype=torch.float64), torch.rand(1, 1, 161, 161, dtype=torch.float64))
    assert torch.isfinite(v)
    with pytest.raises(ValueError):
        R.ms_ssim(torch.rand(1, 1, 200, 200), torch.rand(1, 1, 200, 201))


def test_window():
    g = R.window()
    assert g.sum().item() == pytest.approx(1.0, abs=1e-15)
    assert torch.equal(g, g.flip(0)) and g.argmax().item() == 5


# ---- input conditions of tests/test_gpu_msssim_numerics.py, in float64
@pytest.mark.parametrize("name", list(NUMERICS_CASES))
def test_numerics_inputs_keep_relu_inactive(name):
    # every level value well above 0: the gradient is smooth there and "4x the f32-vs-f64 distance" means something
    t, xh, dr = numerics_pair(name)
    assert tuple(t.shape) == tuple(xh.shape) == NUMERICS_CASES[name]
    assert t.dtype == xh.dtype == torch.float32
    assert min(t.min().item(), xh.min().item()) >= 0.0 and max(t.max().item(), xh.max().item()) <= dr
    lv = R.level_values(xh.double(), t.double(), dr)
    assert lv.min().item() > 0.05
    if name in LOWQ_CASES:
        w = torch.tensor(R.WEIGHTS, dtype=torch.float64).view(-1, 1, 1)
        ms = torch.prod(lv ** w, dim=0).mean().item()
        assert 0.5 <= ms <= 0.85 and lv.min().item() < 0.35


def test_numerics_shapes_sit_where_they_claim():
    T, HALO = 32, 10                                  # tile edge and window halo of csrc/msssim.hip
    N, C, H, W = NUMERICS_CASES["planes258"]
    assert N * C > 256 and min(H, W) == 161           # the finish kernel has 256 threads
    _, _, H, W = NUMERICS_CASES["tile_exact"]
    assert (H - HALO) % T == 0 and (W - HALO) % T == 0
    _, _, H, W = NUMERICS_CASES["tile_plus1"]
    assert (H - HALO) % T == 1 and (W - HALO) % T == 1
    for name, long_side, short_side in (("wide", 3, 2), ("tall", 2, 3)):
        s = NUMERICS_CASES[name]
        assert -(-(s[long_side] - HALO) // T) >= 20 and -(-(s[short_side] - HALO) // T) == 5
    assert NUMERICS_CASES["stage192x224"][3] % 4 == 0
    assert NUMERICS_CASES["range255"] == NUMERICS_CASES["odd175x201"]


def test_flat_blocks_are_exactly_flat():
    for name, bright in (("flat_blocks", 1.0), ("flat_blocks_dim", 0.98)):
        t, xh, _ = numerics_pair(name)
        assert (t[:, :, :64, :80] == 1.0).all() and (xh[:, :, :64, :80] == torch.tensor(bright)).all()
        assert (t[:, :, 100:, 120:] == 0.0).all() and (xh[:, :, 100:, 120:] == 0.0).all()
        assert t[:, :, 64:100].std().item() > 0.05     # and the rest is not


def test_range255_is_the_unscaled_pair():
    # MS-SSIM does not change when data_range scales with the images
    t, xh, _ = numerics_pair("odd175x201")
    t, xh = t.double(), xh.double()
    x = xh.clone().requires_grad_(True)
    y = t.clone().requires_grad_(True)
    one = R.ms_ssim(x, y, size_average=False)
    one.sum().backward()
    scaled = R.ms_ssim(xh * 255.0, t * 255.0, data_range=255.0, size_average=False)
    assert (scaled - one.detach()).abs().max().item() <= 1e-12
    # the case itself holds the product rounded to float32: each pixel moves by at most 2^-24 of itself, which to
    # first order moves a plane's value by at most 2^-24 * sum |pixel * d ms / d pixel| (twice that is allowed here)
    t255, x255, dr = numerics_pair("range255")
    assert dr == 255.0
    got = R.ms_ssim(x255.double(), t255.double(), data_range=255.0, size_average=False)
    first_order = 2.0 ** -24 * ((x.grad * xh).abs().sum((2, 3)) + (y.grad * t).abs().sum((2, 3)))
    assert ((got - one.detach()).abs() <= 2.0 * first_order).all() and first_order.max().item() < 1e-7
    # data_range matters: the same images at data_range = 1 are further away than any bound of the GPU tests (which
    # ask for 100x the case's value bound, 1.1e-4)
    assert (R.ms_ssim(x255.double(), t255.double(), size_average=False) - got).abs().min().item() > 2e-4


def test_one_level_clamp_pair_clamps_exactly_one_level():
    t, xh = one_level_clamp_pair()
    assert min(t.min().item(), xh.min().item()) >= 0.0 and max(t.max().item(), xh.max().item()) <= 1.0
    p = ONE_LEVEL_CLAMP_PLANE
    others = [q for q in range(3) if q != p]
    _, cs0 = R.ssim_level(xh.double(), t.double(), R.window())
    assert cs0[0, p].item() < -0.05                   # clearly negative before the relu, not a rounding away from 0
    lv = R.level_values(xh.double(), t.double())[:, 0]
    assert lv[0, p].item() == 0.0 and lv[1:, p].min().item() > 0.05
    assert lv[:, others].min().item() > 0.05
    assert R.ms_ssim(xh.double(), t.double(), size_average=False)[0, p].item() == 0.0


# ---- host-side surface (no GPU needed)
def test_loss_constructor_metrics():
    from icm_amd.losses import RateDistortionLoss
    assert RateDistortionLoss(0.01).metric == "mse"
    crit = RateDistortionLoss(8.73, metric="ms-ssim")
    assert crit.metric == "ms-ssim" and crit.lmbda == 8.73
    with pytest.raises(NotImplementedError, match="psnr-hvs"):
        RateDistortionLoss(0.01, metric="psnr-hvs")


def test_train_parser_metric():
    from icm_amd import train as T
    assert T.parse_args(["-d", "/data"]).metric == "mse"
    assert T.parse_args(["-d", "/data", "--metric", "ms-ssim"]).metric == "ms-ssim"
    with pytest.raises(SystemExit):
        T.parse_args(["-d", "/data", "--metric", "psnr-hvs"])


def test_eval_parser_metric():
    from icm_amd import eval_model as EM
    p = EM.setup_args()
    assert EM.parse_metrics(p.parse_args(["-d", "/data"]).metric) == ["psnr"]
    assert EM.parse_metrics(p.parse_args(["-d", "/data", "--metric", "ms-ssim"]).metric) == ["ms-ssim"]
    assert EM.parse_metrics(p.parse_args(["-d", "/data", "--metric", "psnr,ms-ssim"]).metric) == ["psnr", "ms-ssim"]
    assert EM.parse_metrics(p.parse_args(["-d", "/data", "--metric", "ms-ssim", "--metric", "psnr"]).metric) == ["psnr", "ms-ssim"]
    with pytest.raises(ValueError):
        EM.parse_metrics(["psnr-hvs"])


def test_ops_ms_ssim_rejects_bad_inputs_without_a_gpu():
    from icm_amd.ops import ms_ssim
    with pytest.raises(ValueError):
        ms_ssim(torch.rand(1, 3, 256, 256), torch.rand(1, 3, 256, 256))   # CPU tensors
    with pytest.raises(ValueError):
        ms_ssim(torch.rand(3, 256, 256), torch.rand(3, 256, 256))         # wrong rank
