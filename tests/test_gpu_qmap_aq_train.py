"""MI355X: AQ-map training and ``eval_model --aq`` on the cnn and stf models.  The map a ``Trainer(qmap_aq=...)`` step
trains with is the map ``codec encode --aq S`` makes for that crop at the step's background index and strength (the
host definition in icm_amd/codec.py and the float64 reference of tests/_aq_ref.py, under the zone rule of
tests/_qmap_aq_inputs.py), rectangles winning; ``step_graphed`` replays it bit for bit; with ``qmap_aq`` off the
``qmap_rects`` trainer is what it was, and with it on every earlier draw keeps its value; ``eval_model(aq=S)`` decodes
what ``codec.encode_image(aq=S)`` writes."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "image-compression-for-machine_amd"))
import _aq_ref as A  # noqa: E402
import _qmap_aq_inputs as I  # noqa: E402
from oracle import weights as W  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPE = (2, 3, 64, 64)                      # the sizes of tests/test_gpu_graph.py
RANGE = (-8, 16)
STATE = {"cnn": W.make_wacnn_state_dict, "stf": W.make_stf_state_dict}
TRAIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "imagefolder", "train")


def build(name):
    from icm_amd.zoo import models
    m = models[name]()
    m.load_state_dict(STATE[name]())
    return m


def trainer(name, **kw):
    from icm_amd.trainer import Trainer
    return Trainer(build(name), device=DEV, seed=5, **kw)


def batch(seed):
    """(u8 uint8 [2, 64, 64, 3] on the host, x f32 [2, 3, 64, 64] on the device through icm_image_u8_to_f32)"""
    from icm_amd import codec
    u8 = I.mixed_images(SHAPE[0], SHAPE[2], SHAPE[3], seed)
    x = torch.cat([codec.image_u8_to_f32(torch.from_numpy(u8[n]).to(DEV), (0, 0, 0, 0)) for n in range(len(u8))])
    assert torch.equal(x.cpu(), torch.from_numpy(I.planar(u8)))
    return u8, x.contiguous()


def image(name):
    return W._u(f"qaq.{name}", SHAPE, 0.0, 1.0).to(DEV)


# ------------------------------------------------------------------------------------------------ train == encode
@pytest.mark.parametrize("rects", [0, 2])
@pytest.mark.parametrize("name", ["cnn", "stf"])
def test_the_step_trains_on_the_encoders_map(name, rects):
    from icm_amd import codec
    u8, x = batch(21)
    tr = trainer(name, qstep_range=RANGE, qmap_aq=(-2.5, 4.0), qmap_rects=rects)
    tr.keep_loss_seed = True
    scal = tr.step(x).cpu().double()
    assert torch.isfinite(scal).all() and scal[2] > 0 and scal[5] > 0, scal
    t = {k: v.cpu() for k, v in tr.loss_terms.items()}
    B, h, w = SHAPE[0], SHAPE[2] // 16, SHAPE[3] // 16
    assert t["qmap"].shape == (B, h, w) and t["qmap"].dtype == torch.int8
    assert t["aq"].shape == (B,) and t["aq"].dtype == torch.float32 and t["aq_ref"].dtype == torch.float64
    assert t["rects"].shape == (B, rects, 5)
    assert ((t["aq"] >= -2.5) & (t["aq"] <= 4.0)).all() and t["aq"][0] != t["aq"][1]
    assert ((t["qstep"] >= RANGE[0]) & (t["qstep"] <= RANGE[1])).all()
    for n in range(B):
        K, S = int(t["qstep"][n]), float(t["aq"][n])
        got = t["qmap"][n].numpy()
        ref = I.image_reference(u8[n], S, K, t["rects"][n].numpy() if rects else None)
        # the encoder's own map: the device statistics of the 8-bit image, the host rule
        stats = codec.cell_stats(torch.from_numpy(u8[n]).to(DEV), (0, 0, 0, 0))
        enc = codec.quality_map(64, 64, (0, 0, 0, 0), K, [], codec.aq_offsets(stats, S, codec.aq_reference(stats)))
        if rects:
            enc = I.paint_over(enc, t["rects"][n].numpy())
            assert (ref["map"] != ref["aq"]).any(), "no rectangle changed a cell"
            assert np.array_equal(got[ref["map"] != ref["aq"]], ref["map"][ref["map"] != ref["aq"]])     # they win
        inside = I.check_maps(got, enc, ref["value"], f"{name} image {n} vs codec")
        I.check_maps(got, ref["map"], ref["value"], f"{name} image {n} vs float64")
        r64, offs, maps = A.image_maps(u8[n], S, base=K)
        I.check_maps(got, maps[0] if not rects else I.paint_over(maps[0], t["rects"][n].numpy()), ref["value"],
                     f"{name} image {n} vs image_maps")
        err = abs(float(t["aq_ref"][n]) - r64)
        print(f"{name} R={rects} image {n}: K {K}, S {S:.4f}, map {got.min()} .. {got.max()}, cells in the zone "
              f"{inside}, mean activity error {err:.2e}")
        assert err <= I.REF_LIMIT
    assert max(len(np.unique(t["qmap"][n].numpy())) for n in range(B)) > 2     # maps that follow the image, not flat ones


@pytest.mark.parametrize("name", ["cnn", "stf"])
def test_step_graphed_equals_eager(name):
    xs = [batch(30 + i)[1] for i in range(4)]
    outs = []
    for graphed in (False, True):
        tr = trainer(name, qstep_range=RANGE, qmap_aq=(-2.5, 4.0), qmap_rects=1)
        tr.keep_loss_seed = not graphed
        losses = [(tr.step_graphed(x) if graphed else tr.step(x)).clone() for x in xs]
        torch.cuda.synchronize()
        if graphed:
            g = tr._graph
            assert tr.step_no == 4 and g is not None and len(g["qsteps"]) == 5
            assert g["qsteps"][3].dtype == torch.float32 and g["qsteps"][4].dtype == torch.int8
            last = (g["qsteps"][3].cpu(), g["qsteps"][4].cpu(), tr._aq_bufs[1].cpu())
        else:
            last = tuple(tr.loss_terms[k].cpu() for k in ("aq", "qmap", "aq_ref"))
        outs.append((torch.stack(losses).cpu(), {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()},
                     last))
    assert torch.equal(outs[0][0], outs[1][0]), (outs[0][0][:, 2], outs[1][0][:, 2])
    for a, b in zip(outs[0][2], outs[1][2]):                  # the strengths, the maps, the mean activities
        assert torch.equal(a, b)
    assert (outs[0][2][0] != 0).all()                         # the capture run's S = 0 was replaced
    for k, v in outs[0][1].items():
        assert torch.equal(v, outs[1][1][k]), k


@pytest.mark.parametrize("name", ["cnn", "stf"])
def test_off_is_the_rectangle_trainer_bit_for_bit(name):
    x = image(name)
    got = []
    for kw in ({}, {"qmap_aq": None}, {"qmap_aq": (0, 0)}):
        tr = trainer(name, qstep_range=RANGE, qmap_rects=1, **kw)
        tr.keep_loss_seed = True
        assert tr.qmap_aq is None
        losses = torch.stack([tr.step(x).clone() for _ in range(2)]).cpu()
        assert "aq" not in tr.loss_terms
        got.append((losses, tr.loss_terms["rects"].cpu(), tr.loss_terms["qmap"].cpu(), tr.loss_terms["qstep"].cpu()))
    for other in got[1:]:
        for a, b in zip(got[0], other):
            assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["cnn", "stf"])
def test_the_strength_is_the_last_draw(name):
    x = image(name)
    s = 1.5
    tr = trainer(name, qstep_range=RANGE, qmap_aq=(s, s))
    ref = trainer(name, qstep_range=RANGE)
    terms = []
    for t in (tr, ref):
        t.keep_loss_seed = True
        t.step(x)
        terms.append(t.loss_terms)
    assert torch.equal(terms[0]["aq"].cpu(), torch.full((SHAPE[0],), s))
    assert terms[0]["rects"].shape == (SHAPE[0], 0, 5)
    # the same noise (z knows no step: its likelihoods are those of the plain run) and the same K
    assert torch.equal(terms[0]["qstep"], terms[1]["qstep"])
    assert torch.equal(terms[0]["z_lik"], terms[1]["z_lik"])
    assert not torch.equal(terms[0]["y_lik"], terms[1]["y_lik"])
    # and after the strengths' draw the generator is one [B] draw further than the plain run's
    torch.rand((SHAPE[0],), dtype=torch.float32, device=DEV, generator=ref.gen)
    assert torch.equal(tr.gen.get_state(), ref.gen.get_state())


# ------------------------------------------------------------------------------------------------ eval_model --aq
@pytest.fixture(scope="module")
def net():
    m = build("cnn").to(DEV).eval()
    m.update(force=True)
    return m


def test_eval_model_decodes_what_encode_image_writes(net, tmp_path):
    from icm_amd import codec
    from icm_amd import eval_model as EM
    files = EM.collect_images(TRAIN)
    assert len(files) == 5
    S, K = 4.0, 4
    recon = str(tmp_path / "recon")
    got = EM.eval_model(net, files, recon_path=recon, aq=S, qstep=K)
    plain = EM.eval_model(net, files, qstep=K)
    assert math.isfinite(got["bpp"]) and got["bpp"] > 0 and math.isfinite(got["psnr"])
    changed = 0
    for f in files:
        img = codec.read_image_u8(f)
        data, info = codec.encode_image_info(net, img, aq=S, qstep=K)
        want, _ = codec.decode_image(net, data)
        name = os.path.basename(f)
        have = np.asarray(Image.open(os.path.join(recon, name)).convert("RGB"))
        assert np.array_equal(have, want.numpy()), name
        m = EM.aq_quality_map(f, torch.device(DEV), S, K)
        assert m.dtype == np.int8 and m.shape == (4, 4) and info["roi_cells"] == int((m != K).sum())
        changed += info["roi_cells"]
    assert changed > 0 and got["bpp"] != plain["bpp"]            # the maps are no uniform ones
    # rdoq rides along on the coder path; a map and aq together are refused
    assert math.isfinite(EM.eval_model(net, files[:1], aq=S, qstep=K, rdoq=50.0)["bpp"])
    with pytest.raises(ValueError):
        EM.eval_model(net, files[:1], entropy_estimation=True, aq=S, qmap=np.zeros((4, 4), dtype=np.int8))
    with pytest.raises(ValueError):
        EM.eval_model(net, files[:1], qmap=np.zeros((4, 4), dtype=np.int8))


def test_eval_model_estimates_under_the_aq_map(net):
    from icm_amd import eval_model as EM
    from icm_amd import utils
    files = EM.collect_images(TRAIN)
    S, K = 4.0, 4
    got = EM.eval_model(net, files, entropy_estimation=True, aq=S, qstep=K)
    assert math.isfinite(got["bpp"]) and got["bpp"] > 0 and math.isfinite(got["psnr"])
    f = files[1]
    want = utils.inference_entropy_estimation(net, EM.read_image(f).to(DEV),
                                              qmap=EM.aq_quality_map(f, torch.device(DEV), S, K))
    one = EM.eval_model(net, [f], entropy_estimation=True, aq=S, qstep=K)
    assert one["bpp"] == want["bpp"] and one["psnr"] == want["psnr"]


def test_the_cli_takes_aq(capsys):
    from icm_amd import eval_model as EM
    assert EM.main(["-d", TRAIN, "-a", "cnn", "--aq", "2", "--qstep", "4", "--limit", "2"]) == 0
    rep = json.loads(capsys.readouterr().out)
    assert math.isfinite(rep["results"]["bpp"][0]) and rep["results"]["bpp"][0] > 0
    assert EM.main(["-d", TRAIN, "-a", "cnn", "--aq", "2", "--qstep", "4", "--limit", "2", "--entropy-estimation"]) == 0
    rep = json.loads(capsys.readouterr().out)
    assert math.isfinite(rep["results"]["bpp"][0])
    assert EM.main(["-d", TRAIN, "-a", "cnn", "--aq", "5"]) == 2
    assert EM.main(["-d", TRAIN, "-a", "cnn", "--qstep", "4", "--entropy-estimation"]) == 2       # as before, without --aq


# ------------------------------------------------------------------------------------------------ train --qmap-aq
def test_train_cli_with_aq_maps(tmp_path, capsys):
    """``python -m icm_amd.train --qstep-range -8,16 --qmap-aq -2,3``, two epochs, the second resumed from the first's
    checkpoint without the flag: trains, prints the ``aq`` line after those of K = -8, 0 and 16, records ``qmap_aq`` in
    the checkpoint and keeps it; ``--qmap-aq 0,0`` on the resumed run drops it"""
    from test_gpu_cli import _write
    from icm_amd import train as TR
    root = str(tmp_path / "data")
    _write(os.path.join(root, "train"), [(80, 72)] * 4, seed=1)
    _write(os.path.join(root, "test"), [(64, 64)] * 2, seed=2)
    save = str(tmp_path / "ck") + os.sep
    common = ["-d", root, "--batch-size", "2", "--test-batch-size", "2", "--patch-size", "64", "64", "-n", "0", "--seed", "7",
              "--save", "--save_path", save, "--test-every", "1", "--qstep-range", "-8,16"]
    assert TR.main(common + ["-e", "1", "--qmap-aq", "-2,3"]) == 0
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("Test epoch 0: qstep")]
    assert [l.split()[4] for l in lines] == ["-8:", "0:", "16:", "aq:"]
    loss, mse, bpp = ([float(l.split(tag)[1].split("|")[0]) for l in lines] for tag in ("Loss:", "MSE loss:", "Bpp loss:"))
    print("\n".join(lines))
    assert all(math.isfinite(v) and v > 0 for v in (loss[3], mse[3], bpp[3]))
    ck = torch.load(os.path.join(save, "0.ckpt"), map_location="cpu", weights_only=True)
    assert ck["qmap_aq"] == [-2.0, 3.0] and "qmap_rects" not in ck and ck["qstep_range"] == [-8, 16]
    assert TR.main(common + ["-e", "2", "--checkpoint", os.path.join(save, "0.ckpt")]) == 0
    out = capsys.readouterr().out
    assert "Train epoch 1:" in out and "Test epoch 1: qstep aq:" in out
