"""The float64 CPU restatement of MS-SSIM (tests/_msssim_ref.py) against hand-checkable cases, and the host-side
surface of the feature that exists without a GPU (loss constructor, CLI parsers)."""
import pytest
import torch

import _msssim_ref as R
from _msssim_inputs import make_pair


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
