"""GPU: the error-bounded residual layer through the codec (``encode_image(max_error=)``, ``codec encode --max-error``,
the ICMR container): every sample of the decode within D of the original's -- exactly the original at D = 0 -- for both
architectures with the deterministic test weights, both coders and their mixtures, a tiled base, a region decode, the
other quality flags riding along, byte identity with the feature off, and the CLI in child processes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

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


def _max_err(a, b):
    return int(np.abs(np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64)).max())


def _check(codec, m, img, data, d):
    """the decode of ``data`` against the original: the bound, what the info says, the container"""
    from icm_amd import bitstream as B
    assert B.is_residual(data)
    out, info = codec.decode_image(m, data, reference=img)
    err = _max_err(out.numpy(), img)
    assert err <= d, (err, d)
    assert info["max_abs_error"] == err and info["max_error"] == d
    if d == 0:
        assert np.array_equal(out.numpy(), img) and info["sse"] == 0 and info["psnr"] == float("inf")
    else:
        assert info["sse"] == int(((out.numpy().astype(np.int64) - img.astype(np.int64)) ** 2).sum())
    assert info["bytes"] == len(data) and info["bpp"] == 8.0 * len(data) / (img.shape[0] * img.shape[1])
    assert info["base_bytes"] + info["residual_bytes"] + B.RESIDUAL_FIXED_BYTES + B.CRC_BYTES == len(data)
    return out, info


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("d", [0, 1, 4])
@pytest.mark.parametrize("arch", ["cnn", "stf"])
def test_every_sample_is_within_the_bound(nets, arch, d):
    from icm_amd import bitstream as B
    from icm_amd import codec
    m = _net(nets, arch)
    data, found = codec.encode_image_info(m, TEX, max_error=d)
    out, info = _check(codec, m, TEX, data, d)
    assert found["max_error"] == d and found["base_bytes"] == info["base_bytes"]
    assert found["residual_bytes"] == info["residual_bytes"]
    lo, hi = found["residual_class_range"]
    assert 0 <= lo <= hi <= RR.NCLASSES - 1
    # the decode is the restatement's: the base's own decode plus the quantised difference
    head, base, _ = B.unpack_residual(data)
    xhat = codec.decode_image(m, base)[0].numpy()
    q = RR.quantise(TEX, xhat, d)
    assert np.array_equal(out.numpy(), RR.reconstruct(xhat, q, d))
    cls = RR.classes(q)
    assert [lo, hi] == [int(cls.min()), int(cls.max())]
    assert head == {"max_error": d, "coder": "host", "height": 100, "width": 150, "table_crc": codec.ResidualTables().crc}
    print(f"{arch} D={d}: {len(data)} bytes = base {found['base_bytes']} + residual {found['residual_bytes']}, "
          f"classes {lo}..{hi}")


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("coder", ["host", "lanes"])
def test_both_coders_and_the_same_string_content(nets, coder):
    from icm_amd import bitstream as B
    from icm_amd import codec
    m = _net(nets, "cnn")
    data = codec.encode_image(m, TEX, coder=coder, max_error=1)
    _check(codec, m, TEX, data, 1)
    head, base, string = B.unpack_residual(data)
    assert head["coder"] == coder and B.coder_of(base) == coder
    assert (string[:4] == b"ICML") == (coder == "lanes")


def test_base_and_residual_on_different_coders(nets):
    """the container names the residual's coder, the base its own: either mixture decodes"""
    from icm_amd import bitstream as B
    from icm_amd import codec
    m = _net(nets, "cnn")
    parts = {c: B.unpack_residual(codec.encode_image(m, TEX, coder=c, max_error=2)) for c in ("host", "lanes")}
    full = codec.decode_image(m, codec.encode_image(m, TEX, coder="host", max_error=2))[0]
    for cb, cr in (("host", "lanes"), ("lanes", "host")):
        # the two coders' bases decode to the same image, so either residual string fits either base
        data = B.pack_residual(parts[cr][0], parts[cb][1], parts[cr][2])
        out, info = _check(codec, m, TEX, data, 2)
        assert torch.equal(out, full)
        assert B.coder_of(parts[cb][1]) == cb and B.unpack_residual(data)[0]["coder"] == cr


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("coder", ["host", "lanes"])
def test_a_tiled_base_and_a_region_decode(nets, coder):
    from icm_amd import bitstream as B
    from icm_amd import codec
    m = _net(nets, "cnn")
    assert TILED.shape[0] >= 128 and TILED.shape[1] >= 192 and TILED.shape[0] % 16 and TILED.shape[1] % 16
    data, found = codec.encode_image_info(m, TILED, tile=64, overlap=16, coder=coder, max_error=1)
    head, base, _ = B.unpack_residual(data)
    assert B.is_tiled(base) and base == codec.encode_image(m, TILED, tile=64, overlap=16, coder=coder)
    full, info = _check(codec, m, TILED, data, 1)
    assert info["tiles"] == 12 and info["tiles_decoded"] == 12
    for region in ((37, 53, 40, 61), (0, 0, 1, 1), (120, 150, 16, 50)):
        y0, x0, h, w = region
        part, pinfo = codec.decode_image(m, data, reference=TILED, region=region)
        assert torch.equal(part, full[y0:y0 + h, x0:x0 + w]), region
        assert pinfo["region"] == list(region) and pinfo["max_abs_error"] <= 1
        assert pinfo["max_abs_error"] == _max_err(part.numpy(), TILED[y0:y0 + h, x0:x0 + w])
    assert codec.decode_image(m, data, region=(0, 0, 1, 1))[1]["tiles_decoded"] == 1


def test_a_region_of_an_untiled_stream(nets):
    from icm_amd import codec
    m = _net(nets, "stf")
    data = codec.encode_image(m, TEX, max_error=0)
    part = codec.decode_image(m, data, region=(33, 17, 50, 101))[0]
    assert np.array_equal(part.numpy(), TEX[33:83, 17:118])


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("kw", [{"qstep": 24}, {"roi": [(20, 30, 40, 60, -12)], "qstep": 16}, {"aq": 1.0},
                                {"rdoq": 2.0, "qstep": 8}], ids=["qstep", "roi", "aq", "rdoq"])
def test_the_quality_flags_ride_along(nets, kw):
    from icm_amd import bitstream as B
    from icm_amd import codec
    m = _net(nets, "cnn")
    data, found = codec.encode_image_info(m, TEX, max_error=4, **kw)
    out, info = _check(codec, m, TEX, data, 4)
    base = B.unpack_residual(data)[1]
    plain, plain_found = codec.encode_image_info(m, TEX, **kw)
    assert base == plain                                  # the base is the very stream the flags give without the layer
    for key, v in plain_found.items():
        assert found[key] == v, key
    base_info = codec.decode_image(m, plain)[1]
    for key in ("qstep", "arch", "height", "width"):
        assert info[key] == base_info[key], key
    assert ("qmap" in info) == ("qmap" in base_info)


def test_without_the_keyword_the_stream_is_what_it_was(nets):
    from icm_amd import bitstream as B
    from icm_amd import codec
    for arch in ("cnn", "stf"):
        m = _net(nets, arch)
        plain, plain_found = codec.encode_image_info(m, TEX)
        data, found = codec.encode_image_info(m, TEX, max_error=None)
        assert data == plain and found == plain_found and not B.is_residual(plain)
        assert "max_error" not in found and "max_error" not in codec.decode_image(m, plain)[1]
        assert B.unpack_residual(codec.encode_image(m, TEX, max_error=0))[1] == plain
    with pytest.raises(ValueError, match="budget"):
        codec.encode_image(m, TEX, max_error=1, max_bytes=10 ** 6)
    for bad in (-1, 33, 1.5, True):
        with pytest.raises(ValueError, match="max_error"):
            codec.encode_image(m, TEX, max_error=bad)


def test_a_reader_with_other_tables_refuses(nets, monkeypatch):
    from icm_amd import codec
    from icm_amd import residual as R
    m = _net(nets, "cnn")
    data = codec.encode_image(m, TEX, max_error=1)
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


def test_cli_encodes_and_a_fresh_process_decodes(nets, cnn_ckpt, tmp_path):
    from icm_amd import codec
    m = _net(nets, "cnn")
    src, stream, out = str(tmp_path / "in.png"), str(tmp_path / "in.icmr"), str(tmp_path / "out.png")
    Image.fromarray(TEX).save(src)
    r = _cli("encode", src, "-o", stream, "-a", "cnn", "-p", cnn_ckpt, "--max-error", "0", "--coder", "lanes")
    assert r.returncode == 0, r.stderr[-2000:]
    enc = json.loads(r.stdout.strip().splitlines()[-1])
    data = open(stream, "rb").read()
    want_data, found = codec.encode_image_info(m, TEX, coder="lanes", max_error=0)
    assert data == want_data and enc["bytes"] == len(data)
    for key in ("max_error", "base_bytes", "residual_bytes", "residual_class_range", "qstep"):
        assert enc[key] == found[key], key
    r = _cli("decode", stream, "-o", out, "-p", cnn_ckpt, "--reference", src)
    assert r.returncode == 0, r.stderr[-2000:]
    dec = json.loads(r.stdout.strip().splitlines()[-1])
    assert dec["max_error"] == 0 and dec["max_abs_error"] == 0 and dec["bytes"] == len(data)
    assert dec["base_bytes"] == enc["base_bytes"] and dec["residual_bytes"] == enc["residual_bytes"]
    assert np.array_equal(np.asarray(Image.open(out)), TEX)            # the original, bit for bit, in another process
    # a corrupt file: exit 4, nothing written
    bad = bytearray(data)
    bad[len(bad) // 2] ^= 0x10
    broken, out2 = str(tmp_path / "broken.icmr"), str(tmp_path / "out2.png")
    with open(broken, "wb") as f:
        f.write(bytes(bad))
    r = _cli("decode", broken, "-o", out2, "-p", cnn_ckpt)
    assert r.returncode == 4 and "CRC" in r.stderr and not os.path.exists(out2)


def test_cli_refuses_a_bound_with_a_budget(cnn_ckpt, tmp_path):
    src, stream = str(tmp_path / "in.png"), str(tmp_path / "x.icmr")
    Image.fromarray(TEX).save(src)
    for extra in (["--target-bytes", "5000"], ["--target-bpp", "1.0"]):
        r = _cli("encode", src, "-o", stream, "-a", "cnn", "-p", cnn_ckpt, "--max-error", "2", *extra)
        assert r.returncode == 2 and "max-error" in r.stderr and not os.path.exists(stream)
