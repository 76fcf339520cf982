"""MI355X: the MS-SSIM kernels (csrc/msssim.hip) against the float64 CPU restatement of the definition
(tests/_msssim_ref.py) on the same inputs, and the layers above them: ops.ms_ssim, RateDistortionLoss(metric="ms-ssim"),
Trainer(metric="ms-ssim") eager and graphed, eval_model --metric.

Tolerances.  The kernel is one more f32 evaluation of the definition, so it is allowed 4x the distance between the
float32 and the float64 run of the restatement on the same input (value: max abs over the [N,C] values; gradient:
max abs difference over the gradient's max abs).  Measured on the CPU on the inputs of tests/_msssim_inputs.py (seed 0):

    case          ms-ssim (f64)  smallest level value  f32-vs-f64 value  f32-vs-f64 gradient
    crop256       0.98687        0.8809                2.37e-07          8.54e-06
    odd175x201    0.98698        0.8812                6.85e-07          2.23e-05
    min161        0.98682        0.8802                1.50e-06          2.97e-05
    gray192x224   0.98683        0.8815                8.77e-08          7.37e-06
"""
import json
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "image-compression-for-machine_amd"))
import _msssim_ref as R  # noqa: E402
from _msssim_inputs import CASES, clamp_corner_pair, make_pair  # noqa: E402
from oracle import weights as W  # noqa: E402

pytestmark = pytest.mark.gpu

# (f32-vs-f64 value, f32-vs-f64 gradient) of the restatement, from the table above; the bounds are 4x these
F32_VS_F64 = {
    "crop256": (2.37e-07, 8.54e-06),
    "odd175x201": (6.85e-07, 2.23e-05),
    "min161": (1.50e-06, 2.97e-05),
    "gray192x224": (8.77e-08, 7.37e-06),
}
FACTOR = 4.0


def _ref(t, xh):
    x = xh.double().requires_grad_(True)
    lv = R.level_values(x, t.double())
    ms = R.ms_ssim(x, t.double(), size_average=False)
    ms.mean().backward()
    return ms.detach(), x.grad, lv.detach()


@pytest.mark.parametrize("case", list(CASES))
def test_forward_and_gradient_match_float64(case):
    from icm_amd.ops import ms_ssim
    t, xh = make_pair(CASES[case])
    ms_ref, g_ref, lv = _ref(t, xh)
    assert lv.min().item() > 0.05, "input condition: relu must be inactive on every level"
    x = xh.cuda().requires_grad_(True)
    ms = ms_ssim(x, t.cuda(), size_average=False)
    mean = ms_ssim(x, t.cuda())
    mean.backward()
    dv = (ms.detach().cpu().double() - ms_ref).abs().max().item()
    dm = abs(mean.item() - ms_ref.mean().item())
    dg = (x.grad.cpu().double() - g_ref).abs().max().item() / g_ref.abs().max().item()
    bv, bg = FACTOR * F32_VS_F64[case][0], FACTOR * F32_VS_F64[case][1]
    print(f"{case}: value diff {dv:.3e} (bound {bv:.3e}), mean diff {dm:.3e}, gradient diff {dg:.3e} (bound {bg:.3e})")
    assert tuple(ms.shape) == CASES[case][:2] and mean.dim() == 0
    assert dv <= bv and dm <= bv
    assert dg <= bg
    # the [N,C] output has its own gradient path: weight the planes unevenly
    wgt = torch.linspace(0.5, 1.5, ms_ref.numel(), dtype=torch.float64).view_as(ms_ref)
    x2 = xh.double().requires_grad_(True)
    (R.ms_ssim(x2, t.double(), size_average=False) * wgt).sum().backward()
    x3 = xh.cuda().requires_grad_(True)
    (ms_ssim(x3, t.cuda(), size_average=False) * wgt.float().cuda()).sum().backward()
    dg2 = (x3.grad.cpu().double() - x2.grad).abs().max().item() / x2.grad.abs().max().item()
    print(f"{case}: weighted-plane gradient diff {dg2:.3e} (bound {bg:.3e})")
    assert dg2 <= bg


def test_clamp_corner_gives_exact_zero_and_zero_gradient():
    from icm_amd.ops import ms_ssim
    t, xh = clamp_corner_pair()
    ms_ref, g_ref, lv = _ref(t, xh)
    assert (lv.amin(0) <= 0).all(), "input condition: every plane has a non-positive level value"
    assert (ms_ref == 0).all() and (g_ref == 0).all()
    x = xh.cuda().requires_grad_(True)
    ms = ms_ssim(x, t.cuda(), size_average=False)
    ms.sum().backward()
    assert torch.equal(ms.cpu(), torch.zeros(1, 3))
    assert torch.isfinite(x.grad).all() and (x.grad == 0).all()
    # one clamped plane next to healthy ones: only that plane's gradient vanishes
    t2, xh2 = make_pair((1, 3, 192, 192))
    xh2[:, 1] = 1.0 - t2[:, 1]
    x = xh2.cuda().requires_grad_(True)
    ms = ms_ssim(x, t2.cuda(), size_average=False)
    ms.sum().backward()
    assert ms[0, 1].item() == 0.0 and ms[0, 0].item() > 0.5 and ms[0, 2].item() > 0.5
    assert (x.grad[:, 1] == 0).all() and x.grad[:, 0].abs().max().item() > 0 and torch.isfinite(x.grad).all()


def test_two_calls_are_bit_identical():
    from icm_amd.ops import ms_ssim
    t, xh = make_pair(CASES["odd175x201"])
    outs = []
    for _ in range(2):
        x = xh.cuda().requires_grad_(True)
        ms = ms_ssim(x, t.cuda(), size_average=False)
        ms_ssim(x, t.cuda()).backward()
        outs.append((ms.detach().clone(), x.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_error_paths():
    from icm_amd.ops import ms_ssim
    with pytest.raises(ValueError):
        ms_ssim(torch.rand(1, 3, 160, 256, device="cuda"), torch.rand(1, 3, 160, 256, device="cuda"))
    with pytest.raises(ValueError):
        ms_ssim(torch.rand(1, 3, 200, 256, device="cuda"), torch.rand(1, 3, 200, 255, device="cuda"))
    with pytest.raises(ValueError):
        ms_ssim(torch.rand(3, 200, 256, device="cuda"), torch.rand(3, 200, 256, device="cuda"))
    with pytest.raises(ValueError):
        ms_ssim(torch.rand(1, 3, 200, 256), torch.rand(1, 3, 200, 256))
    # the C entry point answers the same geometry with its error code (1 = ICM_ERR_ARG), also for a short workspace
    from icm_amd import _lib as L
    lib = L.lib()
    assert lib.icm_msssim_workspace_floats(1, 3, 160, 256) == 0
    n = lib.icm_msssim_workspace_floats(1, 3, 161, 161)
    assert n > 0
    a = torch.rand(1, 3, 161, 161, device="cuda")
    ms, out, ws = torch.empty(3, device="cuda"), torch.empty(2, device="cuda"), torch.empty(n, device="cuda")
    args = (L.ptr(a), L.ptr(a), 1, 3, 161, 161, 1.0, L.ptr(ms), L.ptr(out), 0.0, 0)
    assert lib.icm_msssim_fwd(*args, L.ptr(ws), n - 1, L.stream()) == 1
    assert lib.icm_msssim_fwd(*args, 0, n, L.stream()) == 1
    assert lib.icm_msssim_fwd(*args, L.ptr(ws), n, L.stream()) == 0
    torch.cuda.synchronize()
    assert ms.min().item() == pytest.approx(1.0, abs=1e-6)     # identical images


def test_rate_distortion_loss_ms_ssim():
    from icm_amd.losses import RateDistortionLoss
    from icm_amd.ops import ms_ssim
    from icm_amd.zoo import models
    net = models["cnn"]()
    net.load_state_dict(W.make_wacnn_state_dict())
    net = net.cuda().eval()
    t, _ = make_pair((1, 3, 256, 256))
    x = t.cuda()
    lmbda = 8.73
    with torch.no_grad():
        out = net(x)
        a = RateDistortionLoss(lmbda, metric="ms-ssim")(out, x)
        b = RateDistortionLoss(0.0067)(out, x)
        ms = ms_ssim(out["x_hat"], x)
    assert set(a) == {"loss", "bpp_loss", "ms_ssim_loss"} and set(b) == {"loss", "bpp_loss", "mse_loss"}
    assert torch.equal(a["bpp_loss"], b["bpp_loss"])
    assert a["ms_ssim_loss"].item() == pytest.approx(1.0 - ms.item(), abs=1e-7)
    want = lmbda * (1.0 - ms.item()) + a["bpp_loss"].item()
    assert a["loss"].item() == pytest.approx(want, rel=4e-7)     # a few f32 roundings of a three-term expression


def test_trainer_ms_ssim_eager_equals_graphed_and_seeds_the_metric_gradient():
    """One trainer: two warm-up steps (step_graphed runs them eagerly), then the third step once as a hipGraph replay
    and once eagerly from the same restored state: bit-identical parameters and scalars.  The dx_hat that seeds the
    backward equals -lmbda * d ms_ssim / d x_hat from ops.ms_ssim alone."""
    from icm_amd import engine as E
    from icm_amd.ops import ms_ssim
    from icm_amd.trainer import Trainer
    from icm_amd.zoo import models
    net = models["cnn"]()
    net.load_state_dict(W.make_wacnn_state_dict())
    lmbda = 8.73
    tr = Trainer(net, device="cuda:0", seed=5, lmbda=lmbda, metric="ms-ssim")
    xs = [make_pair((1, 3, 256, 256), seed=i)[0].cuda() for i in range(3)]
    tr.step_graphed(xs[0])
    tr.step_graphed(xs[1])
    f = tr.flat
    snap = [b.clone() for b in (f.p, f.m, f.v, f.ap, f.am, f.av)]
    gen_state, step_no = tr.gen.get_state(), tr.step_no

    s_graph = tr.step_graphed(xs[2]).clone()
    assert tr._graph is not None
    p_graph = [f.p.clone(), f.ap.clone(), f.m.clone(), f.v.clone()]

    for b, s in zip((f.p, f.m, f.v, f.ap, f.am, f.av), snap):
        b.copy_(s)
    tr.gen.set_state(gen_state)
    tr.step_no = step_no
    E.bump_weight_generation()
    tr.keep_loss_seed = True
    s_eager = tr.step(xs[2]).clone()
    torch.cuda.synchronize()
    assert torch.equal(s_graph, s_eager), (s_graph, s_eager)
    for a, b in zip(p_graph, (f.p, f.ap, f.m, f.v)):
        assert torch.equal(a, b)
    # scalars: loss = lmbda * (1 - ms_ssim) + bpp, [7] = 1 - ms_ssim
    v = s_eager.tolist()
    assert v[2] == pytest.approx(lmbda * v[7] + v[0], rel=1e-6)
    x_hat, dxh = tr.loss_seed
    xr = x_hat.clone().requires_grad_(True)
    m = ms_ssim(xr, xs[2])
    m.backward()
    assert v[7] == pytest.approx(1.0 - m.item(), abs=1e-7)
    want = -lmbda * xr.grad
    assert want.abs().max().item() > 0, "input condition: the metric gradient must not vanish"
    assert (dxh - want).abs().max().item() <= 1e-5 * want.abs().max().item()


def _write(folder, sizes, seed=0):
    os.makedirs(folder, exist_ok=True)
    rng = np.random.default_rng(seed)
    for i, (h, w) in enumerate(sizes):
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([(yy * 3 + xx * 2 + 40 * c) % 256 for c in range(3)], -1)
        a = np.clip(base + rng.integers(-12, 13, size=(h, w, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(a).save(os.path.join(folder, f"im{i:02d}.png"))


def test_eval_cli_reports_ms_ssim(tmp_path, capsys):
    from icm_amd import eval_model as EM
    from icm_amd import utils as U
    from icm_amd.ops import ms_ssim
    from icm_amd.zoo import models
    folder = str(tmp_path / "val")
    _write(folder, [(176, 200), (161, 190)])
    torch.manual_seed(3)
    net = models["cnn"]()
    ck = str(tmp_path / "w.ckpt")
    torch.save({"epoch": 0, "state_dict": net.state_dict()}, ck)
    assert EM.main(["-d", folder, "-a", "cnn", "-p", ck, "--metric", "psnr,ms-ssim"]) == 0
    rep = json.loads(capsys.readouterr().out)
    assert set(rep["results"]) == {"psnr", "ms-ssim", "bpp", "encoding_time", "decoding_time"}
    assert EM.main(["-d", folder, "-a", "cnn", "-p", ck, "--metric", "ms-ssim", "--entropy-estimation"]) == 0
    rep_e = json.loads(capsys.readouterr().out)
    assert set(rep_e["results"]) == {"ms-ssim", "bpp", "encoding_time", "decoding_time"}
    assert EM.main(["-d", folder, "-a", "cnn", "-p", ck]) == 0
    assert set(json.loads(capsys.readouterr().out)["results"]) == {"psnr", "bpp", "encoding_time", "decoding_time"}

    model = EM.load_checkpoint("cnn", ck).to("cuda")
    model.update(force=True)
    direct = []
    for fpath in EM.collect_images(folder):
        x = EM.read_image(fpath).to("cuda").unsqueeze(0)
        kept = []
        rv = U.inference(model, x, recon=kept.append, metrics=["psnr", "ms-ssim"])
        assert rv["ms-ssim"] == ms_ssim(x, kept[0]).item()
        assert set(U.inference(model, x)) == {"psnr", "bpp", "encoding_time", "decoding_time"}
        direct.append(rv["ms-ssim"])
    assert rep["results"]["ms-ssim"][0] == pytest.approx(np.mean(direct), rel=1e-6)

    # an image too small for five levels: a clear failure, not a number
    small = str(tmp_path / "small")
    _write(small, [(96, 200)])
    assert EM.main(["-d", small, "-a", "cnn", "-p", ck, "--metric", "ms-ssim"]) != 0
    cap = capsys.readouterr()
    assert "too small for MS-SSIM" in cap.err and cap.out.strip() == ""
