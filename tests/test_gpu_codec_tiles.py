"""GPU: tiled bit-streams (icm_amd/codec.py ``encode_image(tile=, overlap=)`` / ``decode_image(region=)``, the ICMT
container of icm_amd/bitstream.py, ``icm_image_tile_blend`` of csrc/imageio.hip).

One 200x280 image in tiles of 128: 2x3 tiles of at most 128x128 -- the smallest geometry with an interior band, a
four-tile corner and ragged edge tiles.  Every comparison is bit for bit: tile streams against ``encode_image`` of the
crops, the decoded image against the numpy restatement of the blend (tests/_tiles_ref.py) of the per-tile
``decompress`` outputs, regions against crops of the full decode.

Weights: the formula state-dicts of oracle/weights.py, as tests/test_gpu_codec_file.py builds its own."""
import json
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

import _tiles_ref as R
from oracle import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H_IMG, W_IMG, TILE, OVERLAP = 200, 280, 128, 32


def _synthetic(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(yy * 3 + xx * 2 + 40 * c) % 256 for c in range(3)], -1)
    return np.clip(base + rng.integers(-12, 13, size=(h, w, 3)), 0, 255).astype(np.uint8)


def _build(arch, sd):
    from icm_amd.zoo import models
    m = models[arch]()
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    m.update(force=True)
    return m


def _tile_x_hats(model, data):
    """(outer header, plan, the unpadded f32 [3, h, w] ``decompress`` output of every tile)"""
    from icm_amd import bitstream as B
    from icm_amd import codec
    outer, streams = B.unpack_tiled(data)
    rows, cols, plan = codec.plan_tiles(outer["height"], outer["width"], outer["tile"], outer["overlap"])
    tiles = []
    for (y0, x0, h, w), s in zip(plan, streams):
        hd, strings = B.unpack(s)
        left, right, top, bottom = hd["pads"]
        x = model.decompress([[strings[0]], [strings[1]]], hd["shape"])["x_hat"]
        tiles.append(x[0, :, top:top + h, left:left + w].cpu().numpy())
    return outer, (rows, cols, plan), tiles


def _psnr_numpy(a, b):
    d = a.astype(np.int64) - b.astype(np.int64)
    return 10.0 * np.log10(255.0 ** 2 / np.mean(d * d))


@pytest.fixture(scope="module")
def image():
    return _synthetic(H_IMG, W_IMG, seed=21)


@pytest.fixture(scope="module")
def cnn_ckpt(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ckpt") / "cnn_salt0.pt")
    sd = W.make_wacnn_state_dict()
    torch.save(sd, path)
    return path, sd


@pytest.fixture(scope="module")
def net(cnn_ckpt):
    return _build("cnn", cnn_ckpt[1])


@pytest.fixture(scope="module")
def blended(net, image):
    """the overlap-32 stream, its full decode against the original, and the per-tile reconstructions"""
    from icm_amd import codec
    data = codec.encode_image(net, image, tile=TILE, overlap=OVERLAP)
    img, info = codec.decode_image(net, data, reference=image)
    outer, grid, tiles = _tile_x_hats(net, data)
    return {"data": data, "img": img.numpy(), "info": info, "outer": outer, "grid": grid, "tiles": tiles}


def test_every_tile_stream_is_the_stream_of_its_crop(net, image, blended):
    from icm_amd import bitstream as B
    from icm_amd import codec
    data = blended["data"]
    outer, streams = B.unpack_tiled(data)
    assert outer == {"arch": "cnn", "height": H_IMG, "width": W_IMG, "tile": TILE, "overlap": OVERLAP, "rows": 2,
                     "cols": 3, "fingerprint": B.fingerprint(net)}
    rows, cols, plan = blended["grid"]
    assert plan == [(0, 0, 128, 128), (0, 96, 128, 128), (0, 192, 128, 88),
                    (96, 0, 104, 128), (96, 96, 104, 128), (96, 192, 104, 88)]
    for (y0, x0, h, w), s in zip(plan, streams):
        assert s == codec.encode_image(net, image[y0:y0 + h, x0:x0 + w])
    assert len(data) == B.TILED_FIXED_BYTES + 4 * 6 + sum(map(len, streams)) + B.CRC_BYTES


def test_an_image_of_one_tile_is_written_untiled(net):
    from icm_amd import bitstream as B
    from icm_amd import codec
    a = _synthetic(100, 120, seed=22)
    plain = codec.encode_image(net, a)
    assert codec.encode_image(net, a, tile=TILE) == plain
    assert codec.encode_image(net, a, tile=TILE, overlap=OVERLAP) == plain
    assert plain[:4] == B.MAGIC
    with pytest.raises(ValueError):
        codec.encode_image(net, a, tile=100)
    with pytest.raises(ValueError):
        codec.encode_image(net, a, overlap=8)


def test_overlap_zero_pastes_the_tiles(net, image):
    from icm_amd import bitstream as B
    from icm_amd import codec
    data = codec.encode_image(net, image, tile=TILE, overlap=0)
    outer, streams = B.unpack_tiled(data)
    rows, cols, plan = codec.plan_tiles(H_IMG, W_IMG, TILE, 0)
    assert (outer["rows"], outer["cols"]) == (rows, cols) == (2, 3)
    want = np.zeros((H_IMG, W_IMG, 3), np.uint8)
    for (y0, x0, h, w), s in zip(plan, streams):
        want[y0:y0 + h, x0:x0 + w] = codec.decode_image(net, s)[0].numpy()
    img, info = codec.decode_image(net, data)
    assert img.dtype == torch.uint8 and not img.is_cuda and np.array_equal(img.numpy(), want)
    assert info["tiles_decoded"] == 6 and info["bpp"] == 8.0 * len(data) / (H_IMG * W_IMG)


def test_blended_decode_equals_the_reference_blend_of_the_tiles(blended):
    rows, cols, plan = blended["grid"]
    canvas = R.assemble(blended["tiles"], plan, rows, cols, H_IMG, W_IMG, OVERLAP)
    assert np.array_equal(blended["img"], R.quantise(canvas))
    assert blended["info"]["tiles_decoded"] == 6


def test_region_decode_is_a_crop_of_the_full_decode(net, image, blended):
    from icm_amd import codec
    full, data = blended["img"], blended["data"]
    # across the four-tile corner (tiles meet in rows 96..127, columns 96..127 and 192..223)
    y0, x0, h, w = 90, 85, 50, 60
    got, info = codec.decode_image(net, data, region=(y0, x0, h, w))
    assert tuple(got.shape) == (h, w, 3) and np.array_equal(got.numpy(), full[y0:y0 + h, x0:x0 + w])
    assert info["tiles_decoded"] == 4 and info["bpp"] == 8.0 * len(data) / (H_IMG * W_IMG)
    # inside the last tile alone: below row 127 and right of column 223
    y0, x0, h, w = 131, 229, 69, 51
    got, info = codec.decode_image(net, data, reference=image, region=(y0, x0, h, w))
    assert np.array_equal(got.numpy(), full[y0:y0 + h, x0:x0 + w]) and info["tiles_decoded"] == 1
    d = full[y0:y0 + h, x0:x0 + w].astype(np.int64) - image[y0:y0 + h, x0:x0 + w].astype(np.int64)
    assert info["sse"] == int((d * d).sum())
    for bad in [(0, 0, H_IMG + 1, 10), (0, W_IMG - 5, 10, 6), (-1, 0, 10, 10), (0, 0, 0, 10), (H_IMG, 0, 1, 1),
                (0, 0, 10), (1.9, 0, 10, 10)]:
        with pytest.raises(ValueError, match="region"):
            codec.decode_image(net, data, region=bad)


def test_region_of_an_untiled_stream_is_a_crop(net):
    from icm_amd import codec
    a = _synthetic(100, 120, seed=22)
    data = codec.encode_image(net, a)
    full, info0 = codec.decode_image(net, data)
    got, info = codec.decode_image(net, data, region=(13, 17, 40, 33))
    assert np.array_equal(got.numpy(), full.numpy()[13:53, 17:50])
    assert "tiles_decoded" not in info0 and info["bpp"] == info0["bpp"]
    with pytest.raises(ValueError, match="region"):
        codec.decode_image(net, data, region=(90, 0, 20, 10))


def test_sse_and_psnr_are_those_of_the_two_8_bit_images(image, blended):
    d = blended["img"].astype(np.int64) - image.astype(np.int64)
    assert blended["info"]["sse"] == int((d * d).sum())
    assert blended["info"]["psnr"] == pytest.approx(_psnr_numpy(blended["img"], image), rel=1e-12)
    assert blended["info"]["bpp"] == 8.0 * len(blended["data"]) / (H_IMG * W_IMG)


def test_inner_headers_are_checked_before_any_payload(net, blended):
    """a tile stream from another checkpoint, and one of the wrong size, inside a well-formed ICMT stream"""
    from icm_amd import bitstream as B
    from icm_amd import codec
    outer, streams = B.unpack_tiled(blended["data"])
    hd, strings = B.unpack(streams[4])
    forged = list(streams)
    forged[4] = B.pack({**hd, "fingerprint": hd["fingerprint"] ^ 1}, strings)
    with pytest.raises(ValueError, match="tile 4.*fingerprint|fingerprint.*tile 4"):
        codec.decode_image(net, B.pack_tiled(outer, forged))
    forged[4] = streams[5]
    with pytest.raises(ValueError, match="tile 4"):
        codec.decode_image(net, B.pack_tiled(outer, forged))
    with pytest.raises(ValueError, match="fingerprint"):
        codec.decode_image(net, B.pack_tiled({**outer, "fingerprint": outer["fingerprint"] ^ 1}, streams))


def test_cli_round_trip_and_refusals(net, cnn_ckpt, image, blended, tmp_path, capsys):
    from icm_amd import codec
    src, stream = str(tmp_path / "in.png"), str(tmp_path / "in.icmt")
    out, crop = str(tmp_path / "out.png"), str(tmp_path / "crop.png")
    Image.fromarray(image).save(src)
    assert codec.main(["encode", src, "-o", stream, "-p", cnn_ckpt[0], "--tile", "128", "--overlap", "32"]) == 0
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    data = open(stream, "rb").read()
    assert data == blended["data"] and rep["bytes"] == len(data) and rep["bpp"] == 8.0 * len(data) / (H_IMG * W_IMG)
    assert codec.main(["decode", stream, "-o", out, "-p", cnn_ckpt[0], "--reference", src]) == 0
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert np.array_equal(np.asarray(Image.open(out)), blended["img"])
    assert rep["tiles_decoded"] == 6 and rep["psnr"] == pytest.approx(blended["info"]["psnr"], rel=1e-12)
    assert codec.main(["decode", stream, "-o", crop, "-p", cnn_ckpt[0], "--region", "90,85,50,60"]) == 0
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert np.array_equal(np.asarray(Image.open(crop)), blended["img"][90:140, 85:145]) and rep["tiles_decoded"] == 4

    # argument errors: exit 2, nothing written
    none = str(tmp_path / "none.icmt")
    assert codec.main(["encode", src, "-o", none, "-p", cnn_ckpt[0], "--tile", "100"]) == 2
    assert codec.main(["encode", src, "-o", none, "-p", cnn_ckpt[0], "--overlap", "8"]) == 2
    assert codec.main(["encode", src, "-o", none, "-p", cnn_ckpt[0], "--tile", "128", "--overlap", "65"]) == 2
    assert not os.path.exists(none)
    capsys.readouterr()

    # a flipped byte and a second model's checkpoint: exit 4, nothing written
    bad, gone = str(tmp_path / "bad.icmt"), str(tmp_path / "gone.png")
    flipped = bytearray(data)
    flipped[len(data) // 2] ^= 0x10
    with open(bad, "wb") as f:
        f.write(flipped)
    assert codec.main(["decode", bad, "-o", gone, "-p", cnn_ckpt[0]]) == 4
    err = capsys.readouterr()
    assert "CRC" in err.err and err.out == "" and not os.path.exists(gone)
    other = str(tmp_path / "cnn_salt1.pt")
    torch.save(W.make_wacnn_state_dict(salt=1), other)
    assert codec.main(["decode", stream, "-o", gone, "-p", other]) == 4
    err = capsys.readouterr()
    assert "fingerprint" in err.err and err.out == "" and not os.path.exists(gone)
    assert codec.main(["decode", stream, "-o", gone, "-p", cnn_ckpt[0], "--region", "190,0,20,10"]) == 4
    assert "region" in capsys.readouterr().err and not os.path.exists(gone)


def test_stf_tiled_round_trip():
    from icm_amd import codec
    m = _build("stf", W.make_stf_state_dict())
    a = _synthetic(H_IMG, W_IMG, seed=23)
    data = codec.encode_image(m, a, tile=TILE, overlap=OVERLAP)
    outer, (rows, cols, plan), tiles = _tile_x_hats(m, data)
    assert outer["arch"] == "stf" and (rows, cols) == (2, 3)
    img, info = codec.decode_image(m, data, reference=a)
    want = R.quantise(R.assemble(tiles, plan, rows, cols, H_IMG, W_IMG, OVERLAP))
    assert np.array_equal(img.numpy(), want)
    assert info["psnr"] == pytest.approx(_psnr_numpy(want, a), rel=1e-12) and not math.isnan(info["bpp"])
