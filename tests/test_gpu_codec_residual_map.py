"""GPU: error bounds per 16 x 16-pixel cell through the codec (``encode_image(max_error=, error_roi=)``, ``codec encode
--max-error D --error-roi Y0,X0,H,W:D'``, the ICME container): every sample of the decode within its own cell's bound,
the D = 0 cells bit for bit, for both architectures with the deterministic test weights, both coders and their mixtures,
a tiled base with a region decode whose origin is no multiple of four, the quality flags riding along, byte identity
with the scalar ICMR file where the map comes out uniform, a corrupt map string, and the CLI in child processes."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import _residual_map_ref as MR
import _residual_ref as RR
from oracle import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(HERE, "..", "image-compression-for-machine_amd")


def _build(arch):
    from icm_amd.zoo import models
    m = models[arch]()
    m.load_state_dict(W.make_wacnn_state_dict() if arch == "cnn" else W.make_stf_state_dict())
    m = m.to(DEV).eval()
    m.update(force=True)
    return m


@pytest.fixture(scope="module")
def nets():
    return {}


def _net(nets, arch):
    if arch not in nets:
        nets[arch] = _build(arch)
    return nets[arch]


def _textured(h, w, seed):
    """the codec tests' picture: a gradient under noise whose amplitude grows from left to right"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    amp = (1 + (xx * 50) // w + (yy * 12) // h)[..., None]
    base = np.stack([(yy * 2 + xx + 60 * c) % 200 + 20 for c in range(3)], -1)
    noise = rng.integers(-64, 65, size=(h, w, 3)) * amp // 64
    return np.clip(base + noise, 0, 255).astype(np.uint8)


TEX = _textured(100, 150, 5)            # neither side a multiple of 16: partial cells on two edges
TILED = _textured(136, 200, 6)          # tile 64, overlap 16: 3 x 4 tiles
D = 4                                   # the background's bound
# a rectangle at 32 that overlaps the one at 0 and comes earlier, so that it loses there; one at 1 that reaches into
# the partial cells of the last row and column
ROIS = [(10, 20, 50, 60, 32), (30, 50, 40, 45, 0), (85, 130, 15, 20, 1)]
TILED_ROIS = [(20, 30, 60, 70, 32), (40, 61, 50, 50, 0), (120, 180, 16, 20, 1)]


def _abs_err(a, b):
    return np.abs(np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64))


def _check(codec, m, img, data, rois, base_d=D):
    """the decode of ``data`` against the original: every sample against its cell's bound, what the info says, the
    container"""
    from icm_amd import bitstream as B
    H, Wd = img.shape[:2]
    dmap = MR.paint(H, Wd, base_d, rois)
    assert B.is_residual_map(data) and not B.is_residual(data)
    out, info = codec.decode_image(m, data, reference=img)
    err = _abs_err(out.numpy(), img)
    bound = MR.per_pixel(dmap, H, Wd)[..., None]
    assert (err <= bound).all(), int((err > bound).sum())
    zero = np.broadcast_to(bound == 0, err.shape)
    assert zero.any() and np.array_equal(out.numpy()[zero], img[zero])          # the D = 0 cells, bit for bit
    assert info["bound_violations"] == 0 and info["max_abs_error"] == int(err.max())
    assert info["max_error"] == int(dmap.max()) and info["max_error_range"] == [int(dmap.min()), int(dmap.max())]
    assert info["max_error_map"].dtype == np.uint8 and np.array_equal(info["max_error_map"], dmap)
    assert info["sse"] == int((err ** 2).sum())
    assert info["bytes"] == len(data) and info["bpp"] == 8.0 * len(data) / (H * Wd)
    nmap = struct.unpack_from("<I", data, 24)[0]
    assert info["base_bytes"] + nmap + info["residual_bytes"] + B.RESIDUAL_MAP_FIXED_BYTES + B.CRC_BYTES == len(data)
    return out, info, dmap


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("arch", ["cnn", "stf"])
def test_every_sample_is_within_its_cells_bound(nets, arch):
    from icm_amd import bitstream as B
    from icm_amd import codec
    m = _net(nets, arch)
    data, found = codec.encode_image_info(m, TEX, max_error=D, error_roi=ROIS)
    out, info, dmap = _check(codec, m, TEX, data, ROIS)
    assert sorted(set(dmap.reshape(-1).tolist())) == [0, 1, 4, 32]              # the one at 32 lost only where they overlap
    assert dmap[30 // 16, 50 // 16] == 0 and dmap[10 // 16, 20 // 16] == 32
    assert found["max_error"] == D and found["max_error_range"] == [0, 32]
    assert found["error_roi_cells"] == int((dmap != D).sum())
    assert found["base_bytes"] == info["base_bytes"] and found["residual_bytes"] == info["residual_bytes"]
    # the decode is the restatement's: the base's own decode plus the quantised difference under the map
    head, base, m2, _ = B.unpack_residual_map(data)
    assert np.array_equal(m2, dmap) and base == codec.encode_image(m, TEX)
    xhat = codec.decode_image(m, base)[0].numpy()
    q = MR.quantise_map(TEX, xhat, dmap)
    assert np.array_equal(out.numpy(), MR.reconstruct_map(xhat, q, dmap))
    cls = RR.classes(q)
    assert found["residual_class_range"] == [int(cls.min()), int(cls.max())]
    assert head == {"max_error": 32, "coder": "host", "height": 100, "width": 150, "table_crc": codec.ResidualTables().crc}
    # without a reference: the map and its range, no verdict
    info2 = codec.decode_image(m, data)[1]
    assert info2["max_error_range"] == [0, 32] and "bound_violations" not in info2 and "max_abs_error" not in info2
    print(f"{arch}: {len(data)} bytes = base {found['base_bytes']} + residual {found['residual_bytes']}, "
          f"{found['error_roi_cells']} cells off D = {D}")


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("coder", ["host", "lanes"])
def test_both_coders(nets, coder):
    from icm_amd import bitstream as B
    from icm_amd import codec
    m = _net(nets, "cnn")
    data = codec.encode_image(m, TEX, coder=coder, max_error=D, error_roi=ROIS)
    _check(codec, m, TEX, data, ROIS)
    head, base, _, string = B.unpack_residual_map(data)
    assert head["coder"] == coder and B.coder_of(base) == coder
    assert (string[:4] == b"ICML") == (coder == "lanes")


def test_base_and_residual_on_different_coders(nets):
    from icm_amd import bitstream as B
    from icm_amd import codec
    m = _net(nets, "cnn")
    parts = {c: B.unpack_residual_map(codec.encode_image(m, TEX, coder=c, max_error=D, error_roi=ROIS))
             for c in ("host", "lanes")}
    full = codec.decode_image(m, codec.encode_image(m, TEX, max_error=D, error_roi=ROIS))[0]
    for cb, cr in (("host", "lanes"), ("lanes", "host")):
        data = B.pack_residual_map(parts[cr][0], parts[cb][1], parts[cr][2], parts[cr][3])
        out = _check(codec, m, TEX, data, ROIS)[0]
        assert torch.equal(out, full)
        assert B.coder_of(parts[cb][1]) == cb and B.unpack_residual_map(data)[0]["coder"] == cr


# ------------------------------------------------------------------------------------------------ 3
def test_a_tiled_base_and_a_region_decode_off_the_runs_of_four(nets):
    from icm_amd import bitstream as B
    from icm_amd import codec
    m = _net(nets, "cnn")
    data = codec.encode_image(m, TILED, tile=64, overlap=16, coder="lanes", max_error=D, error_roi=TILED_ROIS)
    base = B.unpack_residual_map(data)[1]
    assert B.is_tiled(base) and base == codec.encode_image(m, TILED, tile=64, overlap=16, coder="lanes")
    full, info, dmap = _check(codec, m, TILED, data, TILED_ROIS)
    assert info["tiles"] == 12 and info["tiles_decoded"] == 12
    # the grid is the image's, not a tile's: the tiles start at multiples of 48
    for region in ((37, 53, 40, 61), (33, 30, 50, 83), (0, 0, 1, 1), (120, 150, 16, 50), (47, 63, 3, 3)):
        y0, x0, h, w = region
        part, pinfo = codec.decode_image(m, data, reference=TILED, region=region)
        assert torch.equal(part, full[y0:y0 + h, x0:x0 + w]), region
        err = _abs_err(part.numpy(), TILED[y0:y0 + h, x0:x0 + w])
        assert pinfo["region"] == list(region) and pinfo["max_abs_error"] == int(err.max())
        assert pinfo["bound_violations"] == 0 and (err <= MR.per_pixel(dmap, 136, 200, region)[..., None]).all()
        assert pinfo["max_error_range"] == [0, 32] and np.array_equal(pinfo["max_error_map"], dmap)
    # the first two regions begin off a multiple of four and hold runs across cells of different bounds
    for region in ((37, 53, 40, 61), (33, 30, 50, 83)):
        assert region[1] % 4 and "straddle-differ" in MR.window_paths(136, 200, region, dmap)
    assert codec.decode_image(m, data, region=(0, 0, 1, 1))[1]["tiles_decoded"] == 1


def test_a_violation_is_counted(nets):
    """the count is of the returned samples against the reference given: another reference, another count"""
    from icm_amd import codec
    m = _net(nets, "cnn")
    data = codec.encode_image(m, TEX, max_error=D, error_roi=ROIS)
    out = codec.decode_image(m, data)[0].numpy()
    ref = TEX.copy()
    ref[40, 60, 1] = out[40, 60, 1] ^ 0x01                                       # inside the lossless rectangle: off by 1
    ref[0, 149, 2] = int(out[0, 149, 2]) + (D + 1) * (1 if out[0, 149, 2] < 128 else -1)    # background: off by D + 1
    ref[0, 0, 0] = int(out[0, 0, 0]) + D * (1 if out[0, 0, 0] < 128 else -1)                # background: off by D, fine
    info = codec.decode_image(m, data, reference=ref)[1]
    assert info["bound_violations"] == 2
    assert codec.decode_image(m, data, reference=ref, region=(33, 57, 10, 10))[1]["bound_violations"] == 1


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("kw", [{"qstep": 24}, {"roi": [(20, 30, 40, 60, -12)], "qstep": 16}, {"aq": 1.0},
                                {"rdoq": 2.0, "qstep": 8}], ids=["qstep", "roi", "aq", "rdoq"])
def test_the_quality_flags_ride_along(nets, kw):
    from icm_amd import bitstream as B
    from icm_amd import codec
    m = _net(nets, "cnn")
    data, found = codec.encode_image_info(m, TEX, max_error=D, error_roi=ROIS, **kw)
    out, info, _ = _check(codec, m, TEX, data, ROIS)
    base = B.unpack_residual_map(data)[1]
    plain, plain_found = codec.encode_image_info(m, TEX, **kw)
    assert base == plain                                  # the base is the very stream the flags give without the layer
    for key, v in plain_found.items():
        assert found[key] == v, key
    base_info = codec.decode_image(m, plain)[1]
    for key in ("qstep", "arch", "height", "width"):
        assert info[key] == base_info[key], key
    assert ("qmap" in info) == ("qmap" in base_info)


def test_a_map_that_comes_out_uniform_is_the_scalar_file(nets):
    from icm_amd import bitstream as B
    from icm_amd import codec
    m = _net(nets, "cnn")
    scalar, scalar_found = codec.encode_image_info(m, TEX, max_error=D)
    assert B.is_residual(scalar)
    for rois in ([], [(30, 50, 40, 45, D)], [(0, 0, 1, 1, 0), (0, 0, 16, 16, D)]):
        data, found = codec.encode_image_info(m, TEX, max_error=D, error_roi=rois)
        assert data == scalar, rois                       # no rectangle; one equal to the background; one painted over
        assert found["max_error_range"] == [D, D] and found["error_roi_cells"] == 0
        assert {k: v for k, v in found.items() if k not in ("max_error_range", "error_roi_cells")} == scalar_found
    # a rectangle over every cell: uniform at its own bound, the scalar file of that bound
    data, found = codec.encode_image_info(m, TEX, max_error=D, error_roi=[(0, 0, 100, 150, 0)])
    assert data == codec.encode_image(m, TEX, max_error=0) and found["max_error_range"] == [0, 0]
    assert found["error_roi_cells"] == 7 * 10
    info = codec.decode_image(m, scalar, reference=TEX)[1]                       # scalar files and their info: unchanged
    assert info["max_error"] == D and not {"max_error_range", "max_error_map", "bound_violations"} & set(info)
    assert codec.encode_image(m, TEX, max_error=None, error_roi=None) == codec.encode_image(m, TEX)
    with pytest.raises(ValueError, match="max_error"):
        codec.encode_image(m, TEX, error_roi=ROIS)
    with pytest.raises(ValueError, match="max_error"):
        codec.encode_image(m, TEX, error_roi=[])
    for bad in ([(0, 0, 1, 1, 33)], [(0, 0, 1, 1, -1)], [(90, 0, 11, 1, 0)], [(0, 0, 1, 1)]):
        with pytest.raises(ValueError):
            codec.encode_image(m, TEX, max_error=D, error_roi=bad)
    with pytest.raises(ValueError, match="budget"):
        codec.encode_image(m, TEX, max_error=D, error_roi=ROIS, max_bytes=10 ** 6)


def test_a_flipped_byte_in_the_map_string_is_refused(nets):
    from icm_amd import codec
    m = _net(nets, "cnn")
    data = codec.encode_image(m, TEX, max_error=D, error_roi=ROIS)
    nbase, nmap = struct.unpack_from("<II", data, 20)
    for pos in range(32 + nbase, 32 + nbase + nmap):
        bad = bytearray(data)
        bad[pos] ^= 0x20
        with pytest.raises(ValueError):
            codec.decode_image(m, bytes(bad))


def test_a_reader_with_other_tables_refuses(nets, monkeypatch):
    from icm_amd import codec
    from icm_amd import residual as R
    m = _net(nets, "cnn")
    data = codec.encode_image(m, TEX, max_error=D, error_roi=ROIS)
    monkeypatch.setattr(R.tables(), "crc", R.tables().crc ^ 1)
    with pytest.raises(ValueError, match="table mismatch"):
        codec.decode_image(m, data)


# ------------------------------------------------------------------------------------------------ 5: child processes
@pytest.fixture(scope="module")
def cnn_ckpt(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ckpt") / "cnn_salt0.pt")
    torch.save(W.make_wacnn_state_dict(), path)
    return path


def _cli(*argv):
    env = {**os.environ, "PYTHONPATH": os.pathsep.join([PKG] + [p for p in [os.environ.get("PYTHONPATH")] if p])}
    return subprocess.run([sys.executable, "-m", "icm_amd.codec", *argv], env=env, capture_output=True, text=True,
                          timeout=420)


def _flags(rois):
    return [a for r in rois for a in ("--error-roi", "%d,%d,%d,%d:%d" % r)]


def test_cli_encodes_and_a_fresh_process_decodes(nets, cnn_ckpt, tmp_path):
    from icm_amd import codec
    m = _net(nets, "cnn")
    src, stream, out = str(tmp_path / "in.png"), str(tmp_path / "in.icme"), str(tmp_path / "out.png")
    Image.fromarray(TEX).save(src)
    r = _cli("encode", src, "-o", stream, "-a", "cnn", "-p", cnn_ckpt, "--max-error", str(D), "--coder", "lanes",
             *_flags(ROIS))
    assert r.returncode == 0, r.stderr[-2000:]
    enc = json.loads(r.stdout.strip().splitlines()[-1])
    data = open(stream, "rb").read()
    want_data, found = codec.encode_image_info(m, TEX, coder="lanes", max_error=D, error_roi=ROIS)
    assert data == want_data and enc["bytes"] == len(data)
    for key in ("max_error", "max_error_range", "error_roi_cells", "base_bytes", "residual_bytes", "qstep"):
        assert enc[key] == found[key], key
    r = _cli("decode", stream, "-o", out, "-p", cnn_ckpt, "--reference", src)
    assert r.returncode == 0, r.stderr[-2000:]
    dec = json.loads(r.stdout.strip().splitlines()[-1])
    assert dec["max_error"] == 32 and dec["max_error_range"] == [0, 32] and dec["bound_violations"] == 0
    assert "max_error_map" not in dec and dec["bytes"] == len(data)
    got = np.asarray(Image.open(out))
    dmap = MR.paint(100, 150, D, ROIS)
    err = _abs_err(got, TEX)
    assert (err <= MR.per_pixel(dmap, 100, 150)[..., None]).all() and dec["max_abs_error"] == int(err.max())
    assert np.array_equal(got[32:80, 48:96], TEX[32:80, 48:96])        # the lossless cells, in another process
    assert np.array_equal(got, codec.decode_image(m, data)[0].numpy())
    # a flipped byte in the map string: exit 4, nothing written
    nbase = struct.unpack_from("<I", data, 20)[0]
    bad = bytearray(data)
    bad[32 + nbase + 5] ^= 0x10
    broken, out2 = str(tmp_path / "broken.icme"), str(tmp_path / "out2.png")
    with open(broken, "wb") as f:
        f.write(bytes(bad))
    r = _cli("decode", broken, "-o", out2, "-p", cnn_ckpt)
    assert r.returncode == 4 and "CRC" in r.stderr and not os.path.exists(out2)


def test_cli_refuses_error_roi_without_max_error(cnn_ckpt, tmp_path):
    """the other refusals of the arguments run in-process, without a GPU, in tests/test_residual_map_ref.py"""
    src, stream = str(tmp_path / "in.png"), str(tmp_path / "x.icme")
    Image.fromarray(TEX).save(src)
    r = _cli("encode", src, "-o", stream, "-a", "cnn", "-p", cnn_ckpt, "--error-roi", "0,0,16,16:0")
    assert r.returncode == 2 and "max-error" in r.stderr and not os.path.exists(stream)
