"""MI355X: quality-map training and estimation on the cnn and stf models.  ``model(x, qmap=M)`` in eval mode is the codec
under that map, bit for bit, a uniform map its scalar step and a map per image the batch-of-one encodes; the entropy
estimate under a map brackets the real stream; the tape of the Gaussian step with a step per position carries the
float64 gradients; a ``Trainer(qmap_rects=R)`` step draws and paints its maps on the device, weighs the distortion per
cell, replays from a graph bit for bit, and ``qmap_rects=0`` leaves the ``qstep_range`` trainer exactly as it was."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "image-compression-for-machine_amd"))
import _entropy_ref as R  # noqa: E402
import _qmtrain_ref as M  # noqa: E402
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
    return W._u(f"qm.{name}.{'x'.join(map(str, shape))}", shape, 0.0, 1.0).to(DEV)


def two_level(h, w, lo=-8, hi=12):
    """background ``hi`` with a rectangle at ``lo`` that touches neither all rows nor all columns"""
    m = np.full((h, w), hi, dtype=np.int8)
    m[1:max(h // 2, 2), 0:max(w - 1, 1)] = lo
    assert len(set(m.reshape(-1).tolist())) == 2
    return m


def codec(net, x, m):
    enc = net.compress(x, qmap=m)
    return enc, net.decompress(enc["strings"], enc["shape"], qmap=m)["x_hat"]


# ------------------------------------------------------------------------------------------------ forward == codec
@pytest.mark.parametrize("shape", SHAPES, ids=["64x64", "128x64"])
def test_eval_forward_is_the_codec_under_that_map(net, shape):
    x = image(net.arch, shape)
    B, _, H, Wd = shape
    m = two_level(H // 16, Wd // 16)
    with torch.no_grad():
        plain = net(x)
        out = net(x, qmap=m)
        assert torch.equal(out["x_hat"].clamp(0, 1), codec(net, x, m)[1])
        assert not torch.equal(out["x_hat"], plain["x_hat"])
        assert torch.equal(out["likelihoods"]["z"], plain["likelihoods"]["z"])       # z knows no step
        assert torch.isfinite(out["likelihoods"]["y"]).all() and (out["likelihoods"]["y"] >= 1e-9).all()
        # a tensor on the device is the same map; between its two uniform levels lies its estimate
        t = net(x, qmap=torch.from_numpy(m).to(DEV).to(torch.int32))
        assert torch.equal(t["x_hat"], out["x_hat"]) and torch.equal(t["likelihoods"]["y"], out["likelihoods"]["y"])
        bits = [-torch.log2(o["likelihoods"]["y"]).sum().item() for o in (net(x, qstep=-8), out, net(x, qstep=12))]
        assert bits[0] > bits[1] > bits[2]
        # a uniform map is its scalar step, bit for bit
        for k in (-8, 0, 12):
            a, b = net(x, qmap=np.full(m.shape, k, dtype=np.int64)), net(x, qstep=k)
            assert torch.equal(a["x_hat"], b["x_hat"]) and torch.equal(a["likelihoods"]["y"], b["likelihoods"]["y"])


@pytest.mark.parametrize("shape", SHAPES, ids=["64x64", "128x64"])
def test_a_map_per_image_is_the_batch_of_one_encodes(net, shape):
    x = image(net.arch, shape)
    B, _, H, Wd = shape
    ms = np.stack([two_level(H // 16, Wd // 16), two_level(H // 16, Wd // 16, 16, -4)])
    with torch.no_grad():
        out = net(x, qmap=ms)
        assert out["x_hat"].shape == x.shape
        for n in range(B):
            single = codec(net, x[n:n + 1].contiguous(), ms[n])[1]
            assert torch.equal(out["x_hat"][n:n + 1].clamp(0, 1), single), f"image {n}"
        again = net(x, qmap=torch.from_numpy(ms))
        assert torch.equal(again["x_hat"], out["x_hat"])


def test_an_unpadded_input_takes_the_padded_latents_map(net):
    x = image(net.arch, (1, 3, 72, 100))
    m = two_level(8, 8)                                    # 72 x 100 pads to 128 x 128
    with torch.no_grad():
        out = net(x, qmap=m)
        assert out["x_hat"].shape == x.shape and out["likelihoods"]["y"].shape[-2:] == (8, 8)
        with pytest.raises(ValueError):
            net(x, qmap=two_level(5, 7))


def test_forward_refusals(net):
    x = image(net.arch, SHAPES[0])
    m = two_level(4, 4)
    bad = [dict(qmap=m, qstep=4), dict(qmap=m, qstep=[4, 4]), dict(qmap=two_level(4, 8)), dict(qmap=m.astype(np.float32)),
           dict(qmap=np.where(m == 12, 33, m)), dict(qmap=np.where(m == 12, -17, m)), dict(qmap=np.stack([m] * 3)),
           dict(qmap=m.reshape(-1)), dict(qmap=np.stack([m, m])[None])]
    for kw in bad:
        with pytest.raises(ValueError):
            net(x, **kw)
    from icm_amd.zoo import models
    with pytest.raises(ValueError):
        models["stf6"]()(torch.zeros(1, 3, 128, 128), qmap=two_level(8, 8))
    from icm_amd.losses import RateDistortionLoss
    none = {"x_hat": None, "likelihoods": {"y": None, "z": None}}
    with pytest.raises(ValueError):
        RateDistortionLoss(0.01, metric="ms-ssim")(none, None, qmap=m)
    with pytest.raises(ValueError):
        RateDistortionLoss(0.01)(none, x, qmap=m, lmbda_n=[1.0, 1.0])
    with pytest.raises(ValueError):
        RateDistortionLoss(0.01)(none, x, qmap=two_level(4, 8))


def test_train_mode_forward_takes_maps_and_gives_gradients(net):
    name = net.arch
    m = build(name).to(DEV).train()
    B, _, H, Wd = SHAPES[0]
    x = image(name, SHAPES[0])
    noise = {"z": W._u("qm.nz", (B, 192, H // 64, Wd // 64), -0.5, 0.5), "y": W._u("qm.ny", (B, m.M, H // 16, Wd // 16), -0.5, 0.5)}
    if name == "stf":
        torch.manual_seed(3)
        m.inject_noise(noise, m.draw_drops(B, torch.device(DEV)))
    else:
        m.inject_noise(noise)
    ms = np.stack([two_level(4, 4), two_level(4, 4, 16, -4)])
    a, b, c = m(x, qmap=ms), m(x, qmap=np.full((4, 4), 12)), m(x, qstep=12)
    assert torch.equal(b["likelihoods"]["y"], c["likelihoods"]["y"]) and torch.equal(b["x_hat"], c["x_hat"])
    assert not torch.equal(a["likelihoods"]["y"], c["likelihoods"]["y"])
    from icm_amd.losses import RateDistortionLoss
    crit = RateDistortionLoss(0.0067)
    out = crit(a, x, qmap=ms, lmbda_exp=1.5)
    # the loss of the library form, in float64 from the same output
    lam = M.pixel_weights(ms, M.lmbda_table(0.0067, 1.5))
    ly, lz = (a["likelihoods"][k].detach().cpu().double().reshape(-1) for k in ("y", "z"))
    x64, h64 = x.cpu().double(), a["x_hat"].detach().cpu().double()
    ref = M.m_loss(x64, h64, ly, lz, B * H * Wd, lam)
    lim = M.m_loss_limit(x64, h64, ly, lz, B * H * Wd, lam)
    print(f"{name}: loss {out['loss'].item():.6f}, float64 {ref[2].item():.6f}, limit {lim:.3e}")
    assert abs(out["loss"].item() - ref[2].item()) <= lim
    # one map for the batch is that map for every image
    one = crit(a, x, qmap=ms[0])
    two = crit(a, x, qmap=np.stack([ms[0], ms[0]]))
    assert torch.equal(one["loss"], two["loss"])
    out["loss"].backward()
    gs = [p.grad for p in m.parameters() if p.grad is not None]
    assert len(gs) > 100 and all(torch.isfinite(g).all() for g in gs)
    assert any(g.abs().max() > 0 for g in gs)


# ------------------------------------------------------------------------------------------------ estimation
@pytest.mark.parametrize("shape", SHAPES, ids=["64x64", "128x64"])
def test_entropy_estimation_under_a_map_brackets_the_stream(net, shape):
    from icm_amd import utils
    x = image(net.arch, shape)[0]
    _, H, Wd = x.shape
    m = two_level(H // 16, Wd // 16)
    enc, x_hat = codec(net, x.unsqueeze(0), m)
    stream = sum(len(s[0]) for s in enc["strings"]) * 8.0 / (H * Wd)
    e = utils.inference_entropy_estimation(net, x, qmap=m)
    print(f"{net.arch} {shape}: stream {stream:.4f} bpp, estimate {e['bpp']:.4f} bpp")
    # the margins of test_entropy_estimation_at_a_step_brackets_the_stream
    assert stream > 0 and 0.5 * e["bpp"] <= stream <= 1.05 * e["bpp"] + 0.05
    lo, hi = (utils.inference_entropy_estimation(net, x, qstep=k)["bpp"] for k in (-8, 12))
    assert lo > e["bpp"] > hi
    with pytest.raises(ValueError):
        utils.inference_entropy_estimation(net, x, qmap=m, qstep=4)


def test_eval_model_estimates_under_a_map(net, tmp_path):
    from PIL import Image
    from icm_amd import eval_model as EM
    from icm_amd import utils
    img = (image(net.arch, (1, 3, 64, 64))[0].permute(1, 2, 0).cpu().numpy() * 255).astype(np.uint8)
    Image.fromarray(img).save(tmp_path / "a.png")
    m = two_level(4, 4)
    got = EM.eval_model(net, [str(tmp_path / "a.png")], entropy_estimation=True, qmap=m)
    want = utils.inference_entropy_estimation(net, EM.read_image(str(tmp_path / "a.png")).to(DEV), qmap=m)
    assert got["bpp"] == want["bpp"] and got["psnr"] == want["psnr"]
    assert got["bpp"] < EM.eval_model(net, [str(tmp_path / "a.png")], entropy_estimation=True)["bpp"]
    with pytest.raises(ValueError):
        EM.eval_model(net, [str(tmp_path / "a.png")], qmap=m)


# ------------------------------------------------------------------------------------------------ tape gradients
@pytest.mark.parametrize("mode", R.MODES)
def test_tape_gradients_of_the_gaussian_step_under_a_map(mode):
    """E.gc_likelihood_ste(qmap=...) as an autograd node, on channel slices like the slice loop's: d lik and d y_hat
    seeds in, the float64 autograd gradients out (limits: tests/_entropy_ref.py's rule)"""
    from icm_amd import engine as E
    from test_gpu_entropy_numerics import check_bands, check_grad, same_bits
    inp = M.inputs("strided")
    shape = M.shape_of("strided")
    r = M.raw(inp, mode)
    dlik = R.seed(r, "bits", "qm.tape." + mode)
    _, g64 = M.oracle(inp, mode, torch.float64, dlik)
    lik32, g32 = M.oracle(inp, mode, torch.float32, dlik)
    dyh = R.U("qm.tape.dyh", shape, -1.0, 1.0)
    N, Cc, H, Wd = shape
    wide = {k: torch.zeros((N, Cc + 3, H, Wd), device=DEV) for k in ("y", "mu", "scale")}
    for k, buf in wide.items():
        buf[:, 2:2 + Cc] = inp[k].to(DEV)
        buf.requires_grad_(True)
    noise = inp["noise"].to(DEV).contiguous() if mode == "train" else None
    qmap = inp["qmap"].to(DEV).contiguous()

    def runner(tape, yw, mw, sw):
        lik, yh = E.new(shape, yw.device), E.new(shape, yw.device)
        ys, ms, ss = (w[:, 2:2 + Cc] for w in (yw, mw, sw))
        for w, s, ready in ((yw, ys, True), (mw, ms, False), (sw, ss, False)):
            g = E.zeros(w.shape, w.device)
            tape.bind_grad(w, g, True)
            tape.bind_grad(s, g[:, 2:2 + Cc], ready)
        E.gc_likelihood_ste(tape, ys, ms, ss, noise, lik, yh, qmap=qmap)
        return lik, yh

    lik, yh = E.tape_function(runner, [wide["y"], wide["mu"], wide["scale"]])
    assert same_bits(yh.detach(), M.yhat(inp))
    what = f"tape map {mode}"
    check_bands(what, lik.detach().cpu(), lik32, r)
    gy, gmu, gsc = torch.autograd.grad([lik, yh], [wide["y"], wide["mu"], wide["scale"]],
                                       [dlik.to(DEV), dyh.to(DEV)], allow_unused=True)
    live, floor, grey = R.classify(r)
    _, _, sgrey = R.scale_classes(inp["scale"])
    sel = (slice(None), slice(2, 2 + Cc))
    check_grad(what + " dy", gy[sel], g32[0] + dyh, g64[0] + dyh.double(), r, ~grey)
    check_grad(what + " dmu", gmu[sel], g32[1], g64[1], r, ~grey)
    check_grad(what + " dscale", gsc[sel], g32[2], g64[2], r, ~grey & ~sgrey)
    # wrong shape, dtype, device; a step and a map together
    ops = [wide[k].detach()[:, 2:2 + Cc] for k in ("y", "mu", "scale")]
    steps = torch.ones((N, 2), device=DEV)
    for kw in (dict(qmap=qmap[:1]), dict(qmap=qmap.to(torch.int32)), dict(qmap=qmap.cpu()), dict(qmap=qmap[:, :, :-1]),
               dict(qmap=qmap.transpose(1, 2)), dict(qmap=qmap, steps=steps)):
        with pytest.raises(ValueError):
            E.gc_likelihood_ste(E.Tape(need_grad=False), *ops, None, E.new(shape, DEV), None, **kw)


# ------------------------------------------------------------------------------------------------ trainer
def trainer(name, **kw):
    from icm_amd.trainer import Trainer
    return Trainer(build(name), device=DEV, seed=5, **kw)


@pytest.mark.parametrize("name", ["cnn", "stf"])
def test_quality_map_step(name):
    from icm_amd.trainer import qmap_rects_of
    lo, hi = -8, 16
    tr = trainer(name, qstep_range=(lo, hi), qmap_rects=2)
    tr.keep_loss_seed = True
    x = image(name, SHAPES[1])
    B, _, H, Wd = x.shape
    h, w = H // 16, Wd // 16
    scal = tr.step(x).cpu().double()
    assert torch.isfinite(scal).all() and scal[2] > 0 and scal[5] > 0, scal
    terms = tr.loss_terms
    ks, rects, qmap = terms["qstep"].cpu(), terms["rects"].cpu(), terms["qmap"].cpu()
    assert ks.shape == (B,) and ((ks >= lo) & (ks <= hi)).all()
    assert rects.shape == (B, 2, 5) and rects.dtype == torch.int32 and qmap.shape == (B, h, w) and qmap.dtype == torch.int8
    # the map the step trained with is the painter's, from the background and the rectangles it kept
    assert np.array_equal(qmap.numpy(), M.paint(ks.numpy(), rects.numpy(), h, w))
    # the same seed's qstep_range run: the same noise (the z likelihoods are the same sum) and the same background K;
    # its generator's NEXT draw is the one the map step turned into rectangles
    ref_tr = trainer(name, qstep_range=(lo, hi))
    ref_tr.keep_loss_seed = True
    ref_scal = ref_tr.step(x).cpu().double()
    assert torch.equal(ref_tr.loss_terms["qstep"].cpu(), ks)
    assert torch.equal(ref_tr.loss_terms["z_lik"], terms["z_lik"]) and ref_scal[4] == scal[4]
    u = torch.rand((B, 2, 5), dtype=torch.float32, device=DEV, generator=ref_tr.gen)
    assert torch.equal(qmap_rects_of(u, h, w, lo, hi).cpu(), rects)
    assert torch.equal(qmap_rects_of(u.cpu(), h, w, lo, hi), rects)
    # the loss, recomputed in float64 on the host from what the step kept
    lam = M.pixel_weights(qmap.numpy(), M.lmbda_table(tr.lmbda, 2.0))
    x64, h64 = x.cpu().double(), tr.loss_seed[0].cpu().double()
    ly, lz = terms["y_lik"].cpu().double().reshape(-1), terms["z_lik"].cpu().double().reshape(-1)
    ref = M.m_loss(x64, h64, ly, lz, B * H * Wd, lam)
    lim = M.m_loss_limit(x64, h64, ly, lz, B * H * Wd, lam)
    print(f"{name}: background {ks.tolist()}, rectangles {rects.tolist()}, loss {scal[2].item():.6f}, "
          f"float64 {ref[2].item():.6f}, limit {lim:.3e}")
    assert abs(scal[2].item() - ref[2].item()) <= lim
    assert abs(scal[0].item() - ref[0].item()) <= lim and abs(scal[1].item() - ref[1].item()) <= lim
    # the seed of a pixel carries its cell's weight
    dxh = tr.loss_seed[1].cpu().double()
    want = lam * (255.0 ** 2 * 2.0 / x64.numel()) * (h64 - x64)
    assert torch.allclose(dxh, want, rtol=1e-5, atol=1e-12)
    # the draws differ from step to step
    seen = {tuple(rects.reshape(-1).tolist())}
    for _ in range(2):
        tr.step(x)
        seen.add(tuple(tr.loss_terms["rects"].cpu().reshape(-1).tolist()))
    assert len(seen) == 3


@pytest.mark.parametrize("name", ["cnn", "stf"])
def test_no_rectangles_is_todays_range_trainer(name):
    x = image(name, SHAPES[0])
    got = []
    for kw in ({}, {"qmap_rects": 0}):
        tr = trainer(name, qstep_range=(-8, 16), **kw)
        got.append(torch.stack([tr.step(x).clone() for _ in range(2)]).cpu())
    assert torch.equal(got[0], got[1])


@pytest.mark.parametrize("name", ["cnn", "stf"])
def test_step_graphed_with_maps_equals_eager(name):
    xs = [image(f"{name}.g{i}", SHAPES[0]) for i in range(4)]
    outs = []
    for graphed in (False, True):
        tr = trainer(name, qstep_range=(-8, 16), qmap_rects=2)
        losses = [(tr.step_graphed(x) if graphed else tr.step(x)).clone() for x in xs]
        torch.cuda.synchronize()
        outs.append((torch.stack(losses).cpu(), {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}))
        if graphed:
            assert tr.step_no == 4 and tr._graph is not None and len(tr._graph["qsteps"]) == 4
            assert tr._graph["qsteps"][3].dtype == torch.int8            # the map buffer the graph paints
    assert torch.equal(outs[0][0], outs[1][0]), (outs[0][0][:, 2], outs[1][0][:, 2])
    for k, v in outs[0][1].items():
        assert torch.equal(v, outs[1][1][k]), k


def test_trainer_refusals():
    from icm_amd.trainer import Trainer
    from icm_amd.zoo import models
    net = models["cnn"]()
    with pytest.raises(ValueError):
        Trainer(net, device=DEV, qmap_rects=1)                                      # no range to draw from
    with pytest.raises(ValueError):
        Trainer(net, device=DEV, metric="ms-ssim", qstep_range=(-8, 16), qmap_rects=1)
    with pytest.raises(ValueError):
        Trainer(models["stf6"](), device=DEV, qstep_range=(-8, 16), qmap_rects=1)
    for bad in (9, -1, 1.5, True, "2", None, (2,)):
        with pytest.raises(ValueError):
            Trainer(net, device=DEV, qstep_range=(-8, 16), qmap_rects=bad)


def test_train_cli_with_maps(tmp_path, capsys):
    """``python -m icm_amd.train --qstep-range -8,16 --qmap-rects 1``, two epochs, the second resumed from the first's
    checkpoint without the flag: trains, prints the ``roi`` line after those of K = -8, 0 and 16 with a rate between
    the two ends', records ``qmap_rects`` in the checkpoint and keeps it"""
    from test_gpu_cli import _write
    from icm_amd import train as TR
    root = str(tmp_path / "data")
    _write(os.path.join(root, "train"), [(80, 72)] * 4, seed=1)
    _write(os.path.join(root, "test"), [(64, 64)] * 2, seed=2)
    save = str(tmp_path / "ck") + os.sep
    common = ["-d", root, "--batch-size", "2", "--test-batch-size", "2", "--patch-size", "64", "64", "-n", "0", "--seed", "7",
              "--save", "--save_path", save, "--test-every", "1", "--qstep-range", "-8,16"]
    assert TR.main(common + ["-e", "1", "--qmap-rects", "1"]) == 0
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("Test epoch 0: qstep")]
    assert [l.split()[4] for l in lines] == ["-8:", "0:", "16:", "roi:"]
    loss, mse, bpp = ([float(l.split(tag)[1].split("|")[0]) for l in lines] for tag in ("Loss:", "MSE loss:", "Bpp loss:"))
    print("\n".join(lines))
    assert bpp[0] > bpp[3] > bpp[2] > 0                                    # strictly between the LO and the HI lines'
    assert math.isfinite(loss[3]) and loss[3] > 0 and mse[3] > 0
    ck = torch.load(os.path.join(save, "0.ckpt"), map_location="cpu", weights_only=True)
    assert ck["qmap_rects"] == 1 and ck["qstep_range"] == [-8, 16] and math.isfinite(ck["loss"])
    assert TR.main(common + ["-e", "2", "--checkpoint", os.path.join(save, "0.ckpt")]) == 0
    out = capsys.readouterr().out
    assert "Train epoch 1:" in out and "Test epoch 1: qstep roi:" in out
    with pytest.raises(SystemExit):
        TR.parse_args(["-d", root, "--qmap-rects", "1"])
    with pytest.raises(SystemExit):
        TR.parse_args(["-d", root, "--qstep-range", "-8,16", "--qmap-rects", "9"])
    assert TR.roi_test_map(4, 6, -8, 16).tolist() == [[16] * 6, [16, -8, -8, -8, 16, 16], [16, -8, -8, -8, 16, 16], [16] * 6]
    assert TR.roi_test_map(1, 1, -8, 16).tolist() == [[-8]]
