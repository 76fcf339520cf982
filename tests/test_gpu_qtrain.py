"""MI355X: variable-rate training and estimation on the cnn and stf models.  ``model(x, qstep=K)`` in eval mode is the
codec at that step, bit for bit; the entropy estimate at a step brackets the real stream; the tape of the stepped
Gaussian step carries the float64 gradients; a ``Trainer(qstep_range=...)`` step draws its steps on the device, weighs
the distortion per image, replays from a graph bit for bit, and leaves a trainer without a range exactly as it was."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "image-compression-for-machine_amd"))
import _entropy_ref as R  # noqa: E402
import _qtrain_ref as T  # noqa: E402
from oracle import weights as W  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(2, 3, 64, 64), (2, 3, 128, 64)]
STATE = {"cnn": W.make_wacnn_state_dict, "stf": W.make_stf_state_dict}


def build(name):
    from icm_amd.zoo import models
    m = models[name]()
    m.load_state_dict(STATE[name]())
    return m


@pytest.fixture(scope="module", params=["cnn", "stf"])
def net(request):
    m = build(request.param).to(DEV).eval()
    m.update(force=True)
    m.arch = request.param
    return m


def image(name, shape):
    return W._u(f"qt.{name}.{'x'.join(map(str, shape))}", shape, 0.0, 1.0).to(DEV)


def codec(net, x, k):
    enc = net.compress(x, qstep=k)
    return net.decompress(enc["strings"], enc["shape"], qstep=k)["x_hat"]


# ------------------------------------------------------------------------------------------------ forward == codec
@pytest.mark.parametrize("shape", SHAPES, ids=["64x64", "128x64"])
def test_eval_forward_is_the_codec_at_that_step(net, shape):
    x = image(net.arch, shape)
    with torch.no_grad():
        plain = net(x)
        for k in (-8, 12):
            out = net(x, qstep=k)
            assert torch.equal(out["x_hat"].clamp(0, 1), codec(net, x, k)), f"qstep {k}"
            assert not torch.equal(out["x_hat"], plain["x_hat"])
            assert torch.equal(out["likelihoods"]["z"], plain["likelihoods"]["z"])       # z knows no step
            assert torch.isfinite(out["likelihoods"]["y"]).all() and (out["likelihoods"]["y"] >= 1e-9).all()
        # a larger step is a smaller estimate
        bits = [-torch.log2(net(x, qstep=k)["likelihoods"]["y"]).sum().item() for k in (-8, 0, 12)]
        assert bits[0] > bits[1] > bits[2]
        # a step per image, as a sequence and as an integer tensor: the same result, in the batch's shapes; an image
        # with index 0 in it is that image without a step
        a, b = net(x, qstep=(-8, 12)), net(x, qstep=torch.tensor([-8, 12], dtype=torch.int32))
        assert a["x_hat"].shape == plain["x_hat"].shape
        for name in ("y", "z"):
            assert a["likelihoods"][name].shape == plain["likelihoods"][name].shape
            assert torch.equal(a["likelihoods"][name], b["likelihoods"][name])
        assert torch.equal(a["x_hat"], b["x_hat"])
        c = net(x, qstep=(0, 12))
        assert torch.equal(c["x_hat"][0:1], net(x[0:1])["x_hat"]) and torch.equal(c["x_hat"][1:2], a["x_hat"][1:2])


def test_no_step_is_todays_forward(net):
    x = image(net.arch, SHAPES[0])
    with torch.no_grad():
        a = net(x)
        for q in (0, None, [0, 0]):
            b = net(x, qstep=q)
            assert torch.equal(a["x_hat"], b["x_hat"])
            assert torch.equal(a["likelihoods"]["y"], b["likelihoods"]["y"])
            assert torch.equal(a["likelihoods"]["z"], b["likelihoods"]["z"])
    for bad in (33, -17, 1.5, [4], [1, 2, 3], True, torch.tensor([0.5, 1.0])):
        with pytest.raises(ValueError):
            net(x, qstep=bad)


def test_train_mode_forward_takes_the_step_and_gives_gradients(net):
    name = net.arch
    m = build(name).to(DEV).train()
    B, _, H, Wd = SHAPES[0]
    x = image(name, SHAPES[0])
    noise = {"z": W._u("qt.nz", (B, 192, H // 64, Wd // 64), -0.5, 0.5), "y": W._u("qt.ny", (B, m.M, H // 16, Wd // 16), -0.5, 0.5)}
    drops = None
    if name == "stf":
        torch.manual_seed(3)
        drops = m.draw_drops(B, torch.device(DEV))
        m.inject_noise(noise, drops)
    else:
        m.inject_noise(noise)
    a = m(x)
    b = m(x, qstep=0)
    assert torch.equal(a["x_hat"], b["x_hat"]) and torch.equal(a["likelihoods"]["y"], b["likelihoods"]["y"])
    c = m(x, qstep=[-8, 12])
    assert not torch.equal(a["likelihoods"]["y"], c["likelihoods"]["y"])
    from icm_amd.losses import RateDistortionLoss
    out = RateDistortionLoss(0.0067)(c, x, lmbda_n=[0.0268, 0.0024])
    out["loss"].backward()
    gs = [p.grad for p in m.parameters() if p.grad is not None]
    assert len(gs) > 100 and all(torch.isfinite(g).all() for g in gs)
    assert any(g.abs().max() > 0 for g in gs)


def test_stf6_refuses_a_step():
    from icm_amd.zoo import models
    m = models["stf6"]()
    x = torch.zeros(1, 3, 128, 128)
    for q in (4, [4], torch.tensor([0])):
        with pytest.raises(ValueError):
            m(x, qstep=q)


# ------------------------------------------------------------------------------------------------ estimation
@pytest.mark.parametrize("shape", SHAPES, ids=["64x64", "128x64"])
def test_entropy_estimation_at_a_step_brackets_the_stream(net, shape):
    from icm_amd import utils
    x = image(net.arch, shape)[0]
    for k in (-8, 12):
        r = utils.inference(net, x, qstep=k)
        e = utils.inference_entropy_estimation(net, x, qstep=k)
        print(f"{net.arch} {shape} qstep {k}: stream {r['bpp']:.4f} bpp, estimate {e['bpp']:.4f} bpp, psnr {r['psnr']:.3f} / {e['psnr']:.3f}")
        assert r["bpp"] > 0 and 0.5 * e["bpp"] <= r["bpp"] <= 1.05 * e["bpp"] + 0.05      # test_inference_helpers_pad_and_crop's
        assert abs(r["psnr"] - e["psnr"]) < 1e-3 or e["psnr"] <= r["psnr"]                   # the codec clamps, the estimate does not
    e0 = utils.inference_entropy_estimation(net, x)
    assert e0["bpp"] == utils.inference_entropy_estimation(net, x, qstep=0)["bpp"]
    with pytest.raises(ValueError):
        utils.inference_entropy_estimation(net, x, qstep=40)


def test_eval_model_estimates_at_a_step(net, tmp_path):
    from PIL import Image
    import numpy as np
    from icm_amd import eval_model as EM
    from icm_amd import utils
    img = (image(net.arch, (1, 3, 64, 64))[0].permute(1, 2, 0).cpu().numpy() * 255).astype(np.uint8)
    Image.fromarray(img).save(tmp_path / "a.png")
    got = EM.eval_model(net, [str(tmp_path / "a.png")], entropy_estimation=True, qstep=12)
    want = utils.inference_entropy_estimation(net, EM.read_image(str(tmp_path / "a.png")).to(DEV), qstep=12)
    assert got["bpp"] == want["bpp"] and got["psnr"] == want["psnr"]
    assert got["bpp"] < EM.eval_model(net, [str(tmp_path / "a.png")], entropy_estimation=True)["bpp"]


# ------------------------------------------------------------------------------------------------ tape gradients
@pytest.mark.parametrize("mode", R.MODES)
def test_tape_gradients_of_the_stepped_gaussian_step(mode):
    """E.gc_likelihood_ste(steps=...) as an autograd node, on channel slices like the slice loop's: d lik and d y_hat
    seeds in, the float64 autograd gradients out (limits: tests/_entropy_ref.py's rule)"""
    from icm_amd import engine as E
    from test_gpu_entropy_numerics import check_bands, check_grad, same_bits
    inp = T.stepped_inputs("strided")
    shape = T.shape_of("strided")
    r = T.stepped_raw(inp, mode)
    dlik = R.seed(r, "bits", "qt.tape." + mode)
    _, g64 = T.stepped_oracle(inp, mode, torch.float64, dlik)
    lik32, g32 = T.stepped_oracle(inp, mode, torch.float32, dlik)
    dyh = R.U("qt.tape.dyh", shape, -1.0, 1.0)
    N, Cc, H, Wd = shape
    wide = {k: torch.zeros((N, Cc + 3, H, Wd), device=DEV) for k in ("y", "mu", "scale")}
    for k, buf in wide.items():
        buf[:, 2:2 + Cc] = inp[k].to(DEV)
        buf.requires_grad_(True)
    noise = inp["noise"].to(DEV).contiguous() if mode == "train" else None
    steps = inp["steps"].to(DEV)

    def runner(tape, yw, mw, sw):
        lik, yh = E.new(shape, yw.device), E.new(shape, yw.device)
        ys, ms, ss = (w[:, 2:2 + Cc] for w in (yw, mw, sw))
        # the slice loop's gradient aliasing: a slice's gradient is that slice of the whole buffer's; y accumulates
        # into a defined buffer, mu and scale are first written by this op
        for w, s, ready in ((yw, ys, True), (mw, ms, False), (sw, ss, False)):
            g = E.zeros(w.shape, w.device)
            tape.bind_grad(w, g, True)
            tape.bind_grad(s, g[:, 2:2 + Cc], ready)
        E.gc_likelihood_ste(tape, ys, ms, ss, noise, lik, yh, steps=steps)
        return lik, yh

    lik, yh = E.tape_function(runner, [wide["y"], wide["mu"], wide["scale"]])
    assert same_bits(yh.detach(), T.yhat(inp))
    check_bands(f"tape stepped {mode}", lik.detach().cpu(), lik32, r)
    gy, gmu, gsc = torch.autograd.grad([lik, yh], [wide["y"], wide["mu"], wide["scale"]],
                                       [dlik.to(DEV), dyh.to(DEV)], allow_unused=True)
    live, floor, grey = R.classify(r)
    _, _, sgrey = R.scale_classes(inp["scale"])
    what = f"tape stepped {mode}"
    sel = (slice(None), slice(2, 2 + Cc))
    check_grad(what + " dy", gy[sel], g32[0] + dyh, g64[0] + dyh.double(), r, ~grey)
    check_grad(what + " dmu", gmu[sel], g32[1], g64[1], r, ~grey)
    check_grad(what + " dscale", gsc[sel], g32[2], g64[2], r, ~grey & ~sgrey)
    with pytest.raises(ValueError):
        E.gc_likelihood_ste(E.Tape(need_grad=False), wide["y"].detach()[:, 2:2 + Cc], wide["mu"].detach()[:, 2:2 + Cc],
                            wide["scale"].detach()[:, 2:2 + Cc], None, E.new(shape, DEV), None, steps=steps[:1])


# ------------------------------------------------------------------------------------------------ trainer
def trainer(name, **kw):
    from icm_amd.trainer import Trainer
    return Trainer(build(name), device=DEV, seed=5, **kw)


@pytest.mark.parametrize("name", ["cnn", "stf"])
def test_variable_rate_step(name):
    import _pointwise_ref as P
    from icm_amd.trainer import qstep_tables
    lo, hi = -8, 16
    tr = trainer(name, qstep_range=(lo, hi))
    tr.keep_loss_seed = True
    x = image(name, SHAPES[1])
    B, _, H, Wd = x.shape
    scal = tr.step(x).cpu().double()
    assert torch.isfinite(scal).all() and scal[2] > 0 and scal[5] > 0, scal
    terms = tr.loss_terms
    ks = terms["qstep"].cpu()
    assert ks.shape == (B,) and ((ks >= lo) & (ks <= hi)).all()
    table = qstep_tables((lo, hi), tr.lmbda)[1]
    assert torch.equal(terms["lmbda_n"].cpu(), table[ks - lo])
    # the loss, recomputed in float64 on the host from what the step kept and the steps it drew
    lam = torch.tensor([tr.lmbda * 2.0 ** (-int(k) * 2.0 / 8.0) for k in ks], dtype=torch.float64)
    x64, h64 = x.cpu().double().reshape(B, -1), tr.loss_seed[0].cpu().double().reshape(B, -1)
    ly, lz = terms["y_lik"].cpu().double().reshape(-1), terms["z_lik"].cpu().double().reshape(-1)
    ref = T.rdw_loss(x64, h64, ly, lz, B * H * Wd, lam)
    lim = T.rdw_loss_limit(x64, h64, ly, lz, B * H * Wd, lam) + P.ULP * ref[2].item()      # + lmbda_n rounded to float32
    print(f"{name}: drawn steps {ks.tolist()}, loss {scal[2].item():.6f}, float64 {ref[2].item():.6f}, limit {lim:.3e}")
    assert abs(scal[2].item() - ref[2].item()) <= lim
    assert abs(scal[0].item() - ref[0].item()) <= lim and abs(scal[1].item() - ref[1].item()) <= lim
    # the seed of image n carries its weight
    dxh = tr.loss_seed[1].cpu().double().reshape(B, -1)
    want = (lam * 255.0 ** 2 * 2.0 / x64.numel()).reshape(B, 1) * (h64 - x64)
    assert torch.allclose(dxh, want, rtol=1e-5, atol=1e-12)
    # the draws differ from step to step and between images over a few steps
    seen = set(ks.tolist())
    for _ in range(3):
        tr.step(x)
        seen |= set(tr.loss_terms["qstep"].cpu().tolist())
    assert len(seen) > 2


@pytest.mark.parametrize("name", ["cnn", "stf"])
def test_no_range_is_todays_trainer(name):
    x = image(name, SHAPES[0])
    got = []
    for kw in ({}, {"qstep_range": None}):
        tr = trainer(name, **kw)
        got.append(torch.stack([tr.step(x).clone() for _ in range(2)]).cpu())
    assert torch.equal(got[0], got[1])
    # ... and a range leaves the noise and DropPath draws where they were: the first step's z likelihoods are the same
    tr = trainer(name, qstep_range=(4, 4))
    s = tr.step(x).cpu()
    assert s[4] == got[0][0][4] and s[3] != got[0][0][3]


@pytest.mark.parametrize("name", ["cnn", "stf"])
def test_step_graphed_with_a_range_equals_eager(name):
    xs = [image(f"{name}.g{i}", SHAPES[0]) for i in range(4)]
    outs = []
    for graphed in (False, True):
        tr = trainer(name, qstep_range=(-8, 16))
        losses = [(tr.step_graphed(x) if graphed else tr.step(x)).clone() for x in xs]
        torch.cuda.synchronize()
        outs.append((torch.stack(losses).cpu(), {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}))
        if graphed:
            assert tr.step_no == 4 and tr._graph is not None and tr._graph["qsteps"] is not None
    assert torch.equal(outs[0][0], outs[1][0]), (outs[0][0][:, 2], outs[1][0][:, 2])
    for k, v in outs[0][1].items():
        assert torch.equal(v, outs[1][1][k]), k


def test_trainer_refusals():
    from icm_amd.trainer import Trainer
    from icm_amd.zoo import models
    net = models["cnn"]()
    with pytest.raises(ValueError):
        Trainer(net, device=DEV, metric="ms-ssim", qstep_range=(-8, 16))
    with pytest.raises(ValueError):
        Trainer(models["stf6"](), device=DEV, qstep_range=(-8, 16))
    for bad in ((16, -8), (-17, 0), (0, 33), (0,), (0, 1, 2), (0.5, 2), 4):
        with pytest.raises(ValueError):
            Trainer(net, device=DEV, qstep_range=bad)
    from icm_amd.losses import RateDistortionLoss
    with pytest.raises(ValueError):
        RateDistortionLoss(0.01, metric="ms-ssim")({"x_hat": None, "likelihoods": {"y": None, "z": None}}, None, lmbda_n=[1.0])


def test_train_cli_with_a_range(tmp_path, capsys):
    """``python -m icm_amd.train --qstep-range -8,16``: trains, reports the test loss at K = -8, 0 and 16, records the
    range in the checkpoint, resumes from it"""
    from test_gpu_cli import _write
    from icm_amd import train as TR
    root = str(tmp_path / "data")
    _write(os.path.join(root, "train"), [(80, 72)] * 4, seed=1)
    _write(os.path.join(root, "test"), [(64, 64)] * 2, seed=2)
    save = str(tmp_path / "ck") + os.sep
    common = ["-d", root, "--batch-size", "2", "--test-batch-size", "2", "--patch-size", "64", "64", "-n", "0", "--seed", "7",
              "--save", "--save_path", save, "--test-every", "1", "--qstep-range", "-8,16", "--qstep-lambda-exp", "1.5"]
    assert TR.main(common + ["-e", "1"]) == 0
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("Test epoch 0: qstep")]
    assert [l.split()[4] for l in lines] == ["-8:", "0:", "16:"] and "Average losses" not in out
    bpp = [float(l.split("Bpp loss:")[1]) for l in lines]
    assert bpp[0] > bpp[1] > bpp[2] > 0                                   # a larger step, fewer bits
    ck = torch.load(os.path.join(save, "0.ckpt"), map_location="cpu", weights_only=True)
    assert ck["qstep_range"] == [-8, 16] and ck["qstep_lambda_exp"] == 1.5 and math.isfinite(ck["loss"])
    assert TR.main(common + ["-e", "2", "--checkpoint", os.path.join(save, "0.ckpt")]) == 0
    assert "Train epoch 1:" in capsys.readouterr().out


@pytest.mark.parametrize("shape", SHAPES, ids=["64x64", "128x64"])
def test_per_image_steps_against_single_image_encodes(net, shape):
    """image n of ``model(x, qstep=(-8, 12))`` against ``decompress(compress(x[n:n+1], qstep=K_n))``, a batch of one.

    The convolution plans (Winograd or direct, tile tables) are chosen by the launch's size, batch included, so the
    pipeline without any step differs in the last bits between a batch of two and a batch of one (measured on MI355X,
    max |x_hat difference| of the plain ``model(x)``: cnn 64x64 8.9e-08, cnn 128x64 2.4e-07, stf 128x64 5.5e-07, stf
    64x64 none).  The eval-mode forward therefore runs a call with a step per image one image at a time
    (``CompressionModel._forward_each``); run as one batch of two, this comparison missed by 6.0e-08, 2.1e-07 and
    4.8e-07 in those three cases."""
    x = image(net.arch, shape)
    with torch.no_grad():
        out = net(x, qstep=(-8, 12))["x_hat"].clamp(0, 1)
        for n, k in enumerate((-8, 12)):
            single = codec(net, x[n:n + 1].contiguous(), k)
            print(f"{net.arch} {shape} image {n} qstep {k}: max |batch - single| {(out[n:n + 1] - single).abs().max().item():.3e}")
            assert torch.equal(out[n:n + 1], single), f"image {n} at qstep {k}"
