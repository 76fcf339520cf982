"""GPU: image file -> bit-stream file -> image file (icm_amd/codec.py, icm_amd/bitstream.py, csrc/imageio.hip).

The stream is decoded by the encoding process, and by a FRESH process that sees only the file and a checkpoint: every
piece of side information the decoder needs must be in the stream.  The reconstruction must equal, byte for byte, the
8-bit image the host path produces (ToTensor, pad_to_multiple, compress, decompress, crop, to_pil_image).

Weights: the formula state-dicts of oracle/weights.py, the recipe of tests/test_gpu_codec.py."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(HERE, "..", "image-compression-for-machine_amd")
TRAIN = os.path.join(HERE, "golden", "imagefolder", "train")
GOLDEN_IMAGES = ["a_grey.png", "b_rgb.png", "c_rgba.png", "d_palette.png", "e_rgb.bmp"]


def _synthetic(h=192, w=160, seed=4):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(yy * 3 + xx * 2 + 40 * c) % 256 for c in range(3)], -1)
    return np.clip(base + rng.integers(-12, 13, size=(h, w, 3)), 0, 255).astype(np.uint8)


def _inputs():
    out = {n: np.array(Image.open(os.path.join(TRAIN, n)).convert("RGB")) for n in GOLDEN_IMAGES}
    out["synthetic_192x160"] = _synthetic()
    return out


def _build(arch, sd):
    from icm_amd.zoo import models
    m = models[arch]()
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    m.update(force=True)
    return m


@pytest.fixture(scope="module")
def cnn_ckpt(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ckpt") / "cnn_salt0.pt")
    sd = W.make_wacnn_state_dict()
    torch.save(sd, path)
    return path, sd


@pytest.fixture(scope="module")
def net(cnn_ckpt):
    return _build("cnn", cnn_ckpt[1])


def _host_path(model, a):
    """the existing path: to_pil_image(crop(decompress(compress(pad_to_multiple(ToTensor(x)))), pads)) and the strings"""
    from icm_amd import utils as U
    from icm_amd.datasets import ToTensor, to_pil_image
    xp, pads = U.pad_to_multiple(ToTensor()(a)[None].to(DEV), 64)
    enc = model.compress(xp)
    dec = model.decompress(enc["strings"], enc["shape"])
    return np.asarray(to_pil_image(U.crop(dec["x_hat"], pads)[0])), enc, pads


def _psnr_numpy(a, b):
    d = a.astype(np.int64) - b.astype(np.int64)
    return 10.0 * np.log10(255.0 ** 2 / np.mean(d * d))


@pytest.mark.parametrize("name", GOLDEN_IMAGES + ["synthetic_192x160"])
def test_round_trip_equals_the_host_path_byte_for_byte(net, name):
    from icm_amd import bitstream as B
    from icm_amd import codec
    a = _inputs()[name]
    want, enc, pads = _host_path(net, a)
    data = codec.encode_image(net, a)
    header, strings = B.unpack(data)
    assert header == {"arch": "cnn", "height": a.shape[0], "width": a.shape[1], "pads": pads,
                      "shape": tuple(enc["shape"]), "fingerprint": B.fingerprint(net)}
    assert strings == [enc["strings"][0][0], enc["strings"][1][0]]
    assert len(data) == len(strings[0]) + len(strings[1]) + B.HEADER_BYTES_2
    img, info = codec.decode_image(net, data)
    assert img.dtype == torch.uint8 and not img.is_cuda and tuple(img.shape) == a.shape
    assert np.array_equal(img.numpy(), want)
    assert info["bpp"] == 8.0 * len(data) / (a.shape[0] * a.shape[1]) and "psnr" not in info
    # the image may come as a host tensor, a device tensor or a PIL image: same stream
    assert codec.encode_image(net, torch.from_numpy(a).to(DEV)) == data
    assert codec.encode_image(net, Image.fromarray(a)) == data
    # PSNR of the 8-bit images from the integer sum
    img2, info2 = codec.decode_image(net, data, reference=a)
    assert torch.equal(img2, img)
    want_psnr = _psnr_numpy(want, a)
    print(f"{name}: {len(data)} bytes, {info2['bpp']:.3f} bpp, psnr {info2['psnr']:.6f} (numpy {want_psnr:.6f})")
    assert info2["psnr"] == pytest.approx(want_psnr, rel=1e-12)


def test_fresh_process_decodes_the_file(net, cnn_ckpt, tmp_path):
    from icm_amd import bitstream as B
    from icm_amd import codec
    a = _synthetic()
    src = str(tmp_path / "in.png")
    Image.fromarray(a).save(src)
    stream, out = str(tmp_path / "in.icmb"), str(tmp_path / "out.png")
    data = codec.encode_image(net, a)
    with open(stream, "wb") as f:
        f.write(data)
    want, info = codec.decode_image(net, data, reference=a)
    _, enc, _ = _host_path(net, a)
    assert os.path.getsize(stream) == len(enc["strings"][0][0]) + len(enc["strings"][1][0]) + B.HEADER_BYTES_2

    env = {**os.environ, "PYTHONPATH": os.pathsep.join([PKG] + [p for p in [os.environ.get("PYTHONPATH")] if p])}
    r = subprocess.run([sys.executable, "-m", "icm_amd.codec", "decode", stream, "-o", out, "-p", cnn_ckpt[0],
                        "--reference", src], env=env, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert rep["command"] == "decode" and rep["arch"] == "cnn" and (rep["height"], rep["width"]) == (192, 160)
    assert rep["bytes"] == os.path.getsize(stream)
    assert rep["bpp"] == 8.0 * os.path.getsize(stream) / (192 * 160)
    assert rep["psnr"] == pytest.approx(info["psnr"], rel=1e-12) and rep["decode_time"] > 0
    got = np.asarray(Image.open(out))
    assert got.dtype == np.uint8 and np.array_equal(got, want.numpy())


def test_encode_cli_writes_the_library_stream(net, cnn_ckpt, tmp_path, capsys):
    from icm_amd import codec
    a = _inputs()["b_rgb.png"]
    stream = str(tmp_path / "b.icmb")
    assert codec.main(["encode", os.path.join(TRAIN, "b_rgb.png"), "-o", stream, "-a", "cnn", "-p", cnn_ckpt[0]]) == 0
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    data = open(stream, "rb").read()
    assert data == codec.encode_image(net, a)
    assert rep["command"] == "encode" and rep["bytes"] == len(data) and rep["bpp"] == 8.0 * len(data) / (12 * 20)
    assert rep["encode_time"] > 0
    # -a must agree with the stream
    out = str(tmp_path / "b.png")
    assert codec.main(["decode", stream, "-o", out, "-a", "stf", "-p", cnn_ckpt[0]]) == 2
    assert "disagrees" in capsys.readouterr().err and not os.path.exists(out)


def test_wrong_checkpoint_and_corrupt_files_exit_4_and_write_nothing(net, cnn_ckpt, tmp_path, capsys):
    from icm_amd import codec
    data = codec.encode_image(net, _inputs()["e_rgb.bmp"])
    stream, out = str(tmp_path / "e.icmb"), str(tmp_path / "e.png")
    with open(stream, "wb") as f:
        f.write(data)
    other = str(tmp_path / "cnn_salt1.pt")
    torch.save(W.make_wacnn_state_dict(salt=1), other)
    assert codec.main(["decode", stream, "-o", out, "-p", other]) == 4
    err = capsys.readouterr()
    assert "fingerprint" in err.err and err.out == "" and not os.path.exists(out)
    # library: the same refusal as a ValueError
    with pytest.raises(ValueError, match="fingerprint"):
        codec.decode_image(_build("cnn", W.make_wacnn_state_dict(salt=1)), data)

    cut = str(tmp_path / "cut.icmb")
    with open(cut, "wb") as f:
        f.write(data[:len(data) - 7])
    assert codec.main(["decode", cut, "-o", out, "-p", cnn_ckpt[0]]) == 4
    err = capsys.readouterr()
    assert "truncated" in err.err and err.out == "" and not os.path.exists(out)
    flipped = bytearray(data)
    flipped[len(data) // 2] ^= 0x10
    with open(cut, "wb") as f:
        f.write(flipped)
    assert codec.main(["decode", cut, "-o", out, "-p", cnn_ckpt[0]]) == 4
    assert "CRC" in capsys.readouterr().err and not os.path.exists(out)
    assert codec.main(["decode", str(tmp_path / "absent.icmb"), "-o", out, "-p", cnn_ckpt[0]]) == 4
    assert not os.path.exists(out)
    with pytest.raises(ValueError, match="truncated"):
        codec.decode_image(net, data[:20])


def test_stf_round_trip():
    from icm_amd import bitstream as B
    from icm_amd import codec
    m = _build("stf", W.make_stf_state_dict())
    a = _synthetic(100, 70, seed=9)
    want, enc, pads = _host_path(m, a)
    data = codec.encode_image(m, a)
    header, strings = B.unpack(data)
    assert header["arch"] == "stf" and header["pads"] == pads == (29, 29, 14, 14)
    assert len(data) == len(enc["strings"][0][0]) + len(enc["strings"][1][0]) + B.HEADER_BYTES_2
    img, info = codec.decode_image(m, data, reference=a)
    assert np.array_equal(img.numpy(), want)
    assert info["psnr"] == pytest.approx(_psnr_numpy(want, a), rel=1e-12)


def test_stf6_is_refused_before_any_gpu_work(tmp_path, capsys):
    """stf6 has no entropy coder loop.  The library refuses on the class alone -- the instance here was never even
    initialised, so nothing could have been launched -- and the CLI exits 2 before it reads a file."""
    from icm_amd import codec
    from icm_amd.zoo import models
    ghost = models["stf6"].__new__(models["stf6"])
    with pytest.raises(ValueError, match="stf6"):
        codec.encode_image(ghost, _synthetic(64, 64))
    with pytest.raises(ValueError, match="stf6"):
        codec.decode_image(ghost, b"ICMB")
    out = str(tmp_path / "x.icmb")
    assert codec.main(["encode", os.path.join(TRAIN, "b_rgb.png"), "-o", out, "-a", "stf6", "-p", "unused.pt"]) == 2
    assert "stf6" in capsys.readouterr().err and not os.path.exists(out)
    assert codec.main(["decode", out, "-o", str(tmp_path / "x.png"), "-a", "stf6", "-p", "unused.pt"]) == 2
    with pytest.raises(ValueError, match="8-bit"):
        codec._as_u8_image(np.zeros((4, 4, 3), dtype=np.float32), "cpu")


def test_model_must_be_in_eval_mode(net):
    from icm_amd import codec
    net.train()
    try:
        with pytest.raises(ValueError, match="eval"):
            codec.encode_image(net, _synthetic(64, 64))
    finally:
        net.eval()
    assert not math.isnan(codec.decode_image(net, codec.encode_image(net, _synthetic(64, 64)))[1]["bpp"])
