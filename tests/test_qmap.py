"""CPU: the host side of the codec's quality maps -- the run-length string a map travels in against an independent
writer (tests/_qmap_ref.py) and every malformed form of it, the (step, inv) table the kernels index, the one check of
a map, ``codec.roi_map`` against a per-pixel restatement, and the packing of a uniform map, which is the scalar
stream byte for byte."""
import struct

import numpy as np
import pytest
import torch

import _qmap_ref as R
import _qstep_ref as Q
from icm_amd import bitstream as B

HDR = {"arch": "cnn", "height": 100, "width": 150, "pads": (21, 21, 14, 14), "shape": (2, 3), "fingerprint": 0xDEADBEEF}
ALL_K = list(range(B.QSTEP_MIN, B.QSTEP_MAX + 1))


def _maps():
    rng = np.random.default_rng(7)
    m48 = rng.integers(-16, 33, size=(4, 8)).astype(np.int8)
    m48[1, 2:6] = 5                                              # a run inside a row
    m48[2, 6:], m48[3, :3] = -3, -3                              # a run across a row end
    long_run = np.zeros((300, 300), dtype=np.int8)               # 89 999 zeros: 65535 + 24 464, then one odd cell
    long_run[-1, -1] = 7
    exact = np.full((4, 65536 // 4 + 4), 3, dtype=np.int8)       # a run of exactly 65535, then another k
    exact.reshape(-1)[65535:] = -2
    all49 = np.array(ALL_K + ALL_K[::-1][:15], dtype=np.int8).reshape(8, 8)
    return {"4x8": m48, "1x2": np.array([[-16, 32]], dtype=np.int8), "long_run": long_run, "exact_65535": exact,
            "all_49_values": all49}


MAPS = _maps()


def _z(m):
    return m.shape[0] // 4, m.shape[1] // 4


# ------------------------------------------------------------------------------------------------ the map string
@pytest.mark.parametrize("name", [n for n in MAPS if n != "1x2"])
def test_map_string_round_trip_equals_the_reference_writer(name):
    m = MAPS[name]
    s = B.qmap_string(m)
    assert isinstance(s, bytes) and s == R.write_map(m) and len(s) >= B.QMAP_STRING_MIN == 10
    back = B.qmap_from_string(s, _z(m))
    assert back.dtype == np.int8 and back.shape == m.shape and np.array_equal(back, m)
    assert np.array_equal(R.read_map(s), m)
    k, got = B.quality_from_strings([b"y", b"z", s], _z(m))
    assert k is None and np.array_equal(got, m)
    if name == "all_49_values":
        assert len(set(m.reshape(-1).tolist())) == 49
    if name == "long_run":
        assert s == struct.pack("<HH", 300, 300) + struct.pack("<Hb", 65535, 0) + struct.pack("<Hb", 24464, 0) + \
            struct.pack("<Hb", 1, 7)
    if name == "exact_65535":
        assert s[4:] == struct.pack("<Hb", 65535, 3) + struct.pack("<Hb", m.size - 65535, -2)


def test_the_shortest_map_string():
    m = MAPS["1x2"]
    s = B.qmap_string(m)
    assert s == R.write_map(m) == struct.pack("<HHHbHb", 1, 2, 1, -16, 1, 32) and len(s) == 10
    # 1 x 2 is no multiple of a z shape: the reader is asked for the size the header implies, and refuses
    with pytest.raises(ValueError, match="header"):
        B.qmap_from_string(s, (1, 1))
    m44 = np.zeros((4, 4), dtype=np.int8)
    m44[2:] = 9
    s = B.qmap_string(m44)
    assert len(s) == 10 and np.array_equal(B.qmap_from_string(s, (1, 1)), m44)
    assert B.quality_from_strings([b"y", b"z"], (1, 1)) == (0, None)
    assert B.quality_from_strings([b"y", b"z", B.qstep_string(-7)], (1, 1)) == (-7, None)


def _runs(h, w, *runs):
    return struct.pack("<HH", h, w) + b"".join(struct.pack("<Hb", c, k) for c, k in runs)


MALFORMED = {
    "wrong size against the header": (_runs(4, 8, (16, 1), (16, 2)), (1, 1), "header"),
    "transposed size": (_runs(8, 4, (16, 1), (16, 2)), (1, 2), "header"),
    "a count of 0": (_runs(4, 4, (8, 1), (0, 2), (8, 3)), (1, 1), "count of 0"),
    "runs short of h w": (_runs(4, 4, (8, 1), (7, 2)), (1, 1), "cover 15 of"),
    "runs past h w": (_runs(4, 4, (8, 1), (9, 2)), (1, 1), "past"),
    "a whole run after the end": (_runs(4, 4, (8, 1), (8, 2), (1, 3)), (1, 1), "trailing"),
    "trailing bytes": (_runs(4, 4, (8, 1), (8, 2)) + b"\x00", (1, 1), "trailing"),
    "a non-maximal run": (_runs(4, 4, (4, 1), (4, 1), (8, 2)), (1, 1), "not maximal"),
    "k above the range": (_runs(4, 4, (8, 1), (8, 33)), (1, 1), "outside"),
    "k below the range": (_runs(4, 4, (8, -17), (8, 2)), (1, 1), "outside"),
    "a single distinct k": (_runs(256, 260, (65535, 4), (1025, 4)), (64, 65), "single"),
    "shorter than two runs": (_runs(4, 4, (16, 1)), (1, 1), "at least 10"),
}


@pytest.mark.parametrize("name", list(MALFORMED))
def test_malformed_map_strings_are_refused(name):
    data, shape, word = MALFORMED[name]
    with pytest.raises(ValueError, match=word):
        B.qmap_from_string(data, shape)
    if len(data) >= B.QMAP_STRING_MIN:
        with pytest.raises(ValueError, match=word):
            B.quality_from_strings([b"y", b"z", data], shape)


def test_a_full_count_may_be_followed_by_the_same_k_and_nothing_shorter_may():
    ok = _runs(256, 260, (65535, 4), (1024, 4), (1, 5))
    m = B.qmap_from_string(ok, (64, 65))
    assert m.shape == (256, 260) and B.qmap_string(m) == ok
    with pytest.raises(ValueError, match="not maximal"):
        B.qmap_from_string(_runs(256, 260, (65534, 4), (1025, 4), (1, 5)), (64, 65))


def test_uniform_and_invalid_maps_have_no_string():
    for k in (-16, 0, 5, 32):
        with pytest.raises(ValueError, match="uniform"):
            B.qmap_string(np.full((4, 8), k, dtype=np.int8))
    bad = np.zeros((4, 8), dtype=np.int64)
    bad[0, 0] = 33
    for m in (bad, np.zeros((4, 8), dtype=np.float32), np.zeros(8, dtype=np.int8), np.zeros((2, 2, 2), dtype=np.int8)):
        with pytest.raises(ValueError):
            B.qmap_string(m)


def test_a_reader_from_before_the_map_refuses_a_mapped_stream():
    s = B.qmap_string(MAPS["4x8"])
    with pytest.raises(ValueError, match="must be one byte"):
        B.qstep_from_strings([b"y", b"z", s])
    from icm_amd import codec
    with pytest.raises(ValueError, match="must be one byte"):
        codec._check_strings("cnn", [b"y", b"z", s])
    # the container itself is indifferent: the map string is a third string like the step's byte
    h, strings = B.unpack(B.pack(HDR, [b"yyyy", b"zz", s], coder="lanes"))
    assert h == HDR and strings == [b"yyyy", b"zz", s]


# ------------------------------------------------------------------------------------------------ table and check
def test_step_table():
    t = B.step_table()
    assert t.dtype == np.float32 and t.shape == (256, 2)
    assert np.array_equal(t.view(np.int32), R.step_table().view(np.int32))
    for k in ALL_K:
        assert tuple(float(v) for v in t[k & 0xFF]) == B.step_of(k)
    invalid = [b for b in range(256) if not B.QSTEP_MIN <= (b if b < 128 else b - 256) <= B.QSTEP_MAX]
    assert len(invalid) == 256 - 49 and np.array_equal(t[invalid], np.ones((len(invalid), 2), dtype=np.float32))
    step, inv = R.steps_of_map(np.array([[-16, 0], [5, 32]], dtype=np.int8))
    assert [float(v) for v in step] == [B.step_of(k)[0] for k in (-16, 0, 5, 32)]
    assert [float(v) for v in inv] == [B.step_of(k)[1] for k in (-16, 0, 5, 32)]


def test_check_qmap():
    m = MAPS["4x8"]
    for given in (m, m.astype(np.int64), m.astype(np.int16).tolist(), torch.from_numpy(m.copy()),
                  torch.from_numpy(m.astype(np.int32)), m.T.copy().T):
        out = B.check_qmap(given, (4, 8))
        assert out.dtype == np.int8 and out.flags.c_contiguous and np.array_equal(out, m)
    assert B.uniform_qmap(m) is None and B.uniform_qmap(np.full((4, 8), -3, dtype=np.int8)) == -3
    over, under = m.astype(np.int64), m.astype(np.int64)
    over[3, 7], under[0, 0] = 33, -17
    for bad, word in ((m, None), (m.T, "size"), (m.reshape(-1), "size"), (m[None], "size"), (over, "outside"),
                      (under, "outside"), (m.astype(np.float32), "integers"), (m != 0, "integers"),
                      (torch.from_numpy(m.astype(np.float32)), "integers"), (m.astype(np.uint8), "outside")):
        if word is None:
            with pytest.raises(ValueError, match="size"):
                B.check_qmap(bad, (8, 4))
            with pytest.raises(ValueError, match="not both"):
                B.check_qmap(bad, (4, 8), 5)
            continue
        with pytest.raises(ValueError, match=word):
            B.check_qmap(bad, (4, 8))


def test_models_refuse_a_bad_map_before_any_work():
    from icm_amd.zoo import models
    net = models["cnn"]().eval()
    x = torch.zeros(1, 3, 64, 128)                     # on the host: nothing below may reach a kernel
    m = MAPS["4x8"]
    over = m.astype(np.int64)
    over[0, 0] = 40
    for bad in (m.T, m[:, :4], over, m.astype(np.float32), m.reshape(-1)):
        with pytest.raises(ValueError, match="qmap"):
            net.compress(x, qmap=bad)
        with pytest.raises(ValueError, match="qmap"):
            net.compress_latent(torch.zeros(1, 320, 4, 8), qmap=bad)
        with pytest.raises(ValueError, match="qmap"):
            net.decompress([[b""], [b""]], (1, 2), qmap=bad)
    with pytest.raises(ValueError, match="not both"):
        net.compress(x, qstep=3, qmap=m)
    with pytest.raises(ValueError, match="not both"):
        net.decompress([[b""], [b""]], (1, 2), qstep=3, qmap=m)
    stf6 = models["stf6"]().eval()
    with pytest.raises(NotImplementedError):
        stf6.compress(x, qmap=m)
    with pytest.raises(NotImplementedError):
        stf6.decompress([[b""], [b""]], (1, 2), qmap=m)


# ------------------------------------------------------------------------------------------------ roi_map
ROI_CASES = {
    "one rectangle": [(30, 40, 40, 60, -24)],
    "one pixel": [(57, 83, 1, 1, -5)],
    "the first and the last pixel": [(0, 0, 1, 1, 4), (-1, -1, 1, 1, -4)],
    "overlapping, a then b": [(10, 10, 50, 50, -8), (40, 30, 30, 90, 6)],
    "overlapping, b then a": [(40, 30, 30, 90, 6), (10, 10, 50, 50, -8)],
    "offsets that clamp at both ends": [(0, 0, 20, 20, -100), (30, 30, 20, 20, 100)],
    "the whole image": [(0, 0, None, None, -3)],
    "an offset of 0": [(5, 5, 30, 30, 0)],
    "none": [],
}


def _rects(rois, H, W):
    """the case's rectangles for an H x W image: negative origins count from the end, extents are cut at the image,
    a rectangle that begins outside it is left out"""
    out = []
    for y0, x0, h, w, d in rois:
        y0, x0 = (H + y0 if y0 < 0 else y0), (W + x0 if x0 < 0 else x0)
        if y0 >= H or x0 >= W:
            continue
        out.append((y0, x0, min(H - y0, H if h is None else h), min(W - x0, W if w is None else w), d))
    return out


@pytest.mark.parametrize("size", [(100, 150), (64, 64)], ids=["100x150", "64x64"])
@pytest.mark.parametrize("case", list(ROI_CASES))
@pytest.mark.parametrize("base", [16, 0, -14])
def test_roi_map_equals_the_restatement(size, case, base):
    from icm_amd import codec
    H, W = size
    rois = _rects(ROI_CASES[case], H, W)
    pads = codec.center_pads(H, W)
    assert pads == R.center_pads(H, W)
    if size == (100, 150):
        assert min(pads) > 0 and pads[0] % 16 and pads[2] % 16          # both axes padded, cells not aligned to the image
    got = codec.roi_map(H, W, pads, base, rois)
    want = R.roi_map(H, W, pads, base, rois)
    assert got.dtype == np.int8 and got.shape == ((H + pads[2] + pads[3]) // 16, (W + pads[0] + pads[1]) // 16)
    assert np.array_equal(got, want)
    if case == "offsets that clamp at both ends" and H >= 50:
        assert got.min() == B.QSTEP_MIN and got.max() == B.QSTEP_MAX
    if case in ("none", "an offset of 0"):
        assert B.uniform_qmap(got) == base


def test_a_rectangle_ending_on_a_cell_boundary_does_not_paint_the_next_cell():
    from icm_amd import codec
    H = W = 64                                           # no padding: cell c holds pixels 16 c .. 16 c + 15
    m = codec.roi_map(H, W, (0, 0, 0, 0), 8, [(16, 16, 16, 32, -8)])
    want = np.full((4, 4), 8, dtype=np.int8)
    want[1, 1:3] = 0
    assert np.array_equal(m, want) and np.array_equal(m, R.roi_map(H, W, (0, 0, 0, 0), 8, [(16, 16, 16, 32, -8)]))
    m = codec.roi_map(H, W, (0, 0, 0, 0), 8, [(16, 16, 17, 33, -8)])      # one pixel more: the next row and column
    want[1:3, 1:4] = 0
    assert np.array_equal(m, want)
    # with pads the boundary moves with them: 100 x 150 has top = 14, left = 21
    pads = codec.center_pads(100, 150)
    m = codec.roi_map(100, 150, pads, 0, [(2, 11, 16, 16, 3)])              # padded rows 16..31, columns 32..47
    assert int((m != 0).sum()) == 1 and m[1, 2] == 3
    assert np.array_equal(m, R.roi_map(100, 150, pads, 0, [(2, 11, 16, 16, 3)]))


def test_cells_wholly_in_the_padding_keep_the_base():
    from icm_amd import codec
    pads = codec.center_pads(100, 150)                   # (21, 21, 14, 14): column 0 and column 11 hold no image pixel
    m = codec.roi_map(100, 150, pads, 4, [(0, 0, 100, 150, -4)])
    assert (m[:, 0] == 4).all() and (m[:, -1] == 4).all() and (m[:, 1:-1] == 0).all()


@pytest.mark.parametrize("bad", [[(0, 0, 200, 10, -8)], [(0, 0, 100, 151, 1)], [(-1, 0, 5, 5, 1)], [(0, 0, 0, 5, 1)],
                                 [(99, 149, 2, 1, 1)], [(0, 0, 5, 5)], [(0, 0, 5, 5, 1.5)], [(0, 0, 5.0, 5, 1)],
                                 [(0, 0, 5, 5, True)], 5, [7]], ids=repr)
def test_rectangles_outside_the_image_and_malformed_ones_are_refused(bad):
    from icm_amd import codec
    with pytest.raises(ValueError):
        codec.roi_map(100, 150, codec.center_pads(100, 150), 0, bad)
    with pytest.raises(ValueError):
        codec.check_rois(bad, 100, 150)


def test_roi_map_refuses_a_bad_base():
    from icm_amd import codec
    for base in (33, -17, 1.5):
        with pytest.raises(ValueError):
            codec.roi_map(64, 64, (0, 0, 0, 0), base, [])


def test_clip_rois_gives_each_tile_its_part():
    from icm_amd import codec
    H, W = 200, 300
    rois = [(30, 40, 40, 60, -24), (100, 100, 90, 150, 5)]
    rows, cols, plan = codec.plan_tiles(H, W, 128, 16)
    assert (rows, cols) == (2, 3)
    paint = np.zeros((H, W), dtype=np.int64)
    for y0, x0, h, w, d in rois:
        paint[y0:y0 + h, x0:x0 + w] = d
    for ty, tx, th, tw in plan:
        part = codec.clip_rois(rois, ty, tx, th, tw)
        got = np.zeros((th, tw), dtype=np.int64)
        for y0, x0, h, w, d in codec.check_rois(part, th, tw):              # every part lies inside its tile
            got[y0:y0 + h, x0:x0 + w] = d
        assert np.array_equal(got, paint[ty:ty + th, tx:tx + tw])
    assert codec.clip_rois(rois[:1], 0, 224, 128, 76) == []                  # the first never reaches the top right tile
    assert codec.clip_rois(rois, 0, 224, 128, 76) == [(100, 0, 28, 26, 5)]


# ------------------------------------------------------------------------------------------------ uniform maps
def test_a_uniform_map_packs_to_the_scalar_stream_byte_for_byte():
    from icm_amd import codec
    from icm_amd import models as M_
    for k in (0, 5, -16):
        m = np.full((8, 12), k, dtype=np.int8)
        qstep, qmap = M_._quality(0, m, (8, 12), "compress: ")              # what compress() does with the map
        assert (qstep, qmap) == (k, None)
        enc_map = {"strings": [[b"yyyy"], [b"zz"]], "shape": (2, 3), "qstep": qstep}
        enc_k = {"strings": [[b"yyyy"], [b"zz"]], "shape": (2, 3), "qstep": k}
        a = codec._pack_one("cnn", 0xDEADBEEF, 100, 150, (21, 21, 14, 14), enc_map, "host")
        b = codec._pack_one("cnn", 0xDEADBEEF, 100, 150, (21, 21, 14, 14), enc_k, "host")
        assert a == b == B.pack(HDR, [b"yyyy", b"zz"] + ([B.qstep_string(k)] if k else []))
        h, strings = B.unpack(a)
        assert B.quality_from_strings(strings, h["shape"]) == (k, None)
        assert codec._check_quality("cnn", h, strings) == (k, None)
    # a non-uniform map: the third string is the map's, and the codec's reader returns the map
    m = codec.roi_map(100, 150, (21, 21, 14, 14), 16, [(30, 40, 40, 60, -24)])
    qstep, qmap = M_._quality(0, m, (8, 12), "compress: ")
    assert qstep == 0 and np.array_equal(qmap, m)
    enc = {"strings": [[b"yyyy"], [b"zz"]], "shape": (2, 3), "qstep": None, "qmap": qmap}
    data = codec._pack_one("cnn", 0xDEADBEEF, 100, 150, (21, 21, 14, 14), enc, "lanes")
    h, strings = B.unpack(data)
    assert strings[2] == R.write_map(m) and B.coder_of(data) == "lanes"
    k, got = codec._check_quality("cnn", h, strings)
    assert k is None and np.array_equal(got, m)
    corrupt = strings[:2] + [strings[2][:-1] + b"\x7f"]
    with pytest.raises(ValueError, match="tile 3.*outside"):
        codec._check_quality("cnn", h, corrupt, "tile 3")


# ------------------------------------------------------------------------------------------------ CLI argument errors
@pytest.mark.parametrize("flags", [["--roi", "1,2,3,4"], ["--roi", "1,2,3:4"], ["--roi", "1,2,3,4:x"],
                                   ["--roi", "1,2,3,4,5"], ["--roi", "a,2,3,4:5"], ["--roi", ""]],
                         ids=lambda f: " ".join(f))
def test_codec_cli_refuses_a_malformed_roi_before_any_gpu_check(flags, tmp_path, capsys, monkeypatch):
    from icm_amd import codec

    def no_gpu_check():
        raise AssertionError("the GPU was asked for")
    monkeypatch.setattr(torch.cuda, "is_available", no_gpu_check)
    out = str(tmp_path / "o.icmb")
    with pytest.raises(SystemExit) as e:
        codec.main(["encode", str(tmp_path / "missing.png"), "-o", out, "-p", "none.pt", *flags])
    assert e.value.code == 2
    assert "Y0,X0,H,W:D" in capsys.readouterr().err
    assert not (tmp_path / "o.icmb").exists()


def test_codec_cli_refuses_a_roi_outside_the_image_before_any_gpu_check(tmp_path, capsys, monkeypatch):
    from PIL import Image
    from icm_amd import codec

    def no_gpu_check():
        raise AssertionError("the GPU was asked for")
    monkeypatch.setattr(torch.cuda, "is_available", no_gpu_check)
    src, out = str(tmp_path / "in.png"), str(tmp_path / "o.icmb")
    Image.fromarray(np.zeros((100, 150, 3), dtype=np.uint8)).save(src)
    assert codec.main(["encode", src, "-o", out, "-p", "none.pt", "--qstep", "16", "--roi", "0,0,200,10:-8"]) == 2
    assert "not inside the 100x150 image" in capsys.readouterr().err
    assert not (tmp_path / "o.icmb").exists()
