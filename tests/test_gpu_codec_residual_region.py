"""GPU: region decode of error-bounded files (ICMR / ICME) reads only the wave bodies of the residual string that the
window needs (``icm_amd.residual.region_plan`` / ``decode_residual(window=)`` / ``codec.decode_image(region=)``): with the
deterministic test weights, a 150 x 200 image and ``symbols_per_wave=1024`` (G = 30 residual waves, the classes in
waves 0 .. 2), every region is bit for bit the crop of the full decode, ``info["residual_waves"]`` says how few waves
were decoded, and the verdicts against a reference are those of the full decode's crop."""
import numpy as np
import pytest
import torch

import _residual_map_ref as MR
from oracle import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, WD, SPW, G = 150, 200, 1024, 30
ROIS = [(20, 30, 60, 70, 8), (40, 61, 50, 50, 0), (130, 180, 20, 20, 1)]
# the first pixel, the last, a full-width strip, a window inside one row of cells, one in the bottom rows (class waves
# 0 .. 2 or so, plane waves 27 ..: disjoint), and the whole image
REGIONS = [(0, 0, 1, 1), (149, 199, 1, 1), (70, 0, 10, 200), (34, 50, 8, 40), (140, 10, 8, 30), (0, 0, 150, 200)]
ENCODINGS = {"D0": dict(max_error=0), "D2": dict(max_error=2), "roi": dict(max_error=2, error_roi=ROIS),
             "D2-tiled": dict(max_error=2, tile=64, overlap=16)}


def _textured(h, w, seed):
    """the codec tests' picture: a gradient under noise whose amplitude grows from left to right"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    amp = (1 + (xx * 50) // w + (yy * 12) // h)[..., None]
    base = np.stack([(yy * 2 + xx + 60 * c) % 200 + 20 for c in range(3)], -1)
    noise = rng.integers(-64, 65, size=(h, w, 3)) * amp // 64
    return np.clip(base + noise, 0, 255).astype(np.uint8)


IMG = _textured(H, WD, 9)


@pytest.fixture(scope="module")
def net():
    from icm_amd.zoo import models
    m = models["cnn"]()
    m.load_state_dict(W.make_wacnn_state_dict())
    m = m.to(DEV).eval()
    m.update(force=True)
    return m


@pytest.fixture(scope="module")
def files(net):
    """name -> (the file, its full decode and info against the original), made once"""
    from icm_amd import codec
    out = {}
    for name, kw in ENCODINGS.items():
        data = codec.encode_image(net, IMG, coder="lanes", symbols_per_wave=SPW, **kw)
        out[name] = (data,) + codec.decode_image(net, data, reference=IMG)
    return out


def _abs_err(a, b):
    return np.abs(np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64))


@pytest.mark.parametrize("name", list(ENCODINGS))
def test_every_region_is_the_crop_of_the_full_decode(net, files, name):
    from icm_amd import bitstream as B
    from icm_amd import codec
    from icm_amd import residual as R
    data, full, finfo = files[name]
    assert (B.is_residual_map(data) if name == "roi" else B.is_residual(data))
    assert finfo["residual_waves"] == [G, G] and finfo["max_abs_error"] <= finfo["max_error"]
    assert (name != "D0" or np.array_equal(full.numpy(), IMG)) and finfo.get("bound_violations", 0) == 0
    assert (finfo.get("tiles", 1) > 1) == (name == "D2-tiled")
    for region in REGIONS:
        y0, x0, h, w = region
        part, info = codec.decode_image(net, data, reference=IMG, region=region)
        assert torch.equal(part, full[y0:y0 + h, x0:x0 + w]), region
        plan = R.region_plan(H, WD, G, region)
        waves = set(range(*plan.plane_waves)) | set(range(*plan.class_waves))
        assert info["residual_waves"] == [len(waves), G], (region, info["residual_waves"])
        assert (info["residual_waves"][0] < G) == (region != (0, 0, H, WD)), region
        err = _abs_err(part.numpy(), IMG[y0:y0 + h, x0:x0 + w])
        assert info["region"] == list(region) and info["max_abs_error"] == int(err.max())
        assert info["max_abs_error"] == int(_abs_err(full.numpy(), IMG)[y0:y0 + h, x0:x0 + w].max())
        assert info["sse"] == int((err ** 2).sum()) and info["max_error"] == finfo["max_error"]
        if name == "roi":
            dmap = finfo["max_error_map"]
            assert info["bound_violations"] == 0 and np.array_equal(info["max_error_map"], dmap)
            assert (err <= MR.per_pixel(dmap, H, WD, region)[..., None]).all()
        else:
            assert "bound_violations" not in info and int(err.max()) <= finfo["max_error"]
        if name == "D2-tiled":
            assert (info["tiles_decoded"] < info["tiles"]) == (region != (0, 0, H, WD))
        # without a reference: the same pixels, no verdict
        part2, info2 = codec.decode_image(net, data, region=region)
        assert torch.equal(part2, part) and "max_abs_error" not in info2
        assert info2["residual_waves"] == info["residual_waves"]


def test_the_regions_reach_what_they_are_there_for():
    from icm_amd import residual as R
    assert R.region_plan(H, WD, G, (0, 0, H, WD)).class_waves == (0, 3)             # 130 cells in steps of 64
    p = R.region_plan(H, WD, G, (140, 10, 8, 30))
    assert p.plane_waves[0] >= p.class_waves[1]                                     # disjoint ranges
    p = R.region_plan(H, WD, G, (0, 0, 1, 1))
    assert p.plane_waves == (0, 1) and p.class_waves == (0, 1)                      # one wave serves both
    p = R.region_plan(H, WD, G, (34, 50, 8, 40))
    assert p.cell_rows[0] <= 2 < p.cell_rows[1] and p.band[0] % WD and p.band[1] % WD   # the band cuts rows


def test_a_violation_in_a_region_is_counted_as_in_the_full_decode(net, files):
    from icm_amd import codec
    data, full, _ = files["roi"]
    ref = IMG.copy()
    v = int(full[45, 70, 1])
    ref[45, 70, 1] = v ^ 0x01                                # inside the lossless rectangle: off by 1
    whole = codec.decode_image(net, data, reference=ref)[1]
    part = codec.decode_image(net, data, reference=ref, region=(44, 60, 4, 20))[1]
    assert whole["bound_violations"] == 1 == part["bound_violations"] and part["residual_waves"][0] < G


def test_decode_residual_with_a_window(net, files):
    """the layer's own surface: a band with the window's symbols, equal to that part of the whole decode"""
    from icm_amd import bitstream as B
    from icm_amd import residual as R
    from icm_amd.ans import coder_for
    head, _, string = B.unpack_residual(files["D2"][0], R.tables().crc)
    whole = R.decode_residual(string, H, WD, coder_for(head["coder"]), DEV)
    assert whole.shape == (3, H, WD)
    for window in ((140, 10, 8, 30), (34, 50, 8, 40), (0, 0, H, WD)):
        res = R.decode_residual(string, H, WD, coder_for(head["coder"]), DEV, window=window)
        e_lo, e_hi = res.band
        assert res.band == R.region_plan(H, WD, G, window).band and res.waves[1] == G
        assert torch.equal(res.symbols, whole.reshape(3, -1)[:, e_lo:e_hi])
    # a damaged body the window does not need: the region decodes, the whole file is refused
    from _lanes_waves_cases import corrupt_word
    bad = corrupt_word(string, 10)
    res = R.decode_residual(bad, H, WD, coder_for("lanes"), DEV, window=(140, 10, 8, 30))
    assert torch.equal(res.symbols, whole.reshape(3, -1)[:, res.band[0]:res.band[1]])
    with pytest.raises(ValueError, match="lane stream decode"):
        R.decode_residual(bad, H, WD, coder_for("lanes"), DEV)
    with pytest.raises(ValueError, match="lane stream decode"):
        R.decode_residual(corrupt_word(string, 28), H, WD, coder_for("lanes"), DEV, window=(140, 10, 8, 30))


def test_a_host_coded_file_decodes_its_region_as_before(net):
    from icm_amd import codec
    data = codec.encode_image(net, IMG, max_error=2)
    full, finfo = codec.decode_image(net, data, reference=IMG)
    assert finfo["residual_waves"] is None
    for region in ((140, 10, 8, 30), (0, 0, 1, 1)):
        y0, x0, h, w = region
        part, info = codec.decode_image(net, data, reference=IMG, region=region)
        assert torch.equal(part, full[y0:y0 + h, x0:x0 + w]) and info["residual_waves"] is None
        assert info["max_abs_error"] <= 2
    # a lanes base under a host-coded residual string, and the reverse: the residual's coder decides
    from icm_amd import bitstream as B
    lanes = codec.encode_image(net, IMG, coder="lanes", symbols_per_wave=SPW, max_error=2)
    hl, bl, sl = B.unpack_residual(lanes)
    hh, bh, sh = B.unpack_residual(data)
    mixed = B.pack_residual(hl, bh, sl)
    part, info = codec.decode_image(net, mixed, region=(140, 10, 8, 30))
    assert torch.equal(part, full[140:148, 10:40]) and info["residual_waves"][0] < G
    assert codec.decode_image(net, B.pack_residual(hh, bl, sh), region=(140, 10, 8, 30))[1]["residual_waves"] is None
