"""CPU: the host side of variance-adaptive quantisation (``codec encode --aq``) -- the numpy restatement of the cell
statistics (tests/_aq_ref.py) against a triple Python loop, ``codec.aq_offsets`` on hand-made statistics (empty cells,
clipping, ties, sign), ``codec.quality_map`` against ``codec.roi_map`` and the restatement, ``codec.check_aq``, and
the CLI's argument errors."""
import math

import numpy as np
import pytest
import torch

import _aq_ref as A
from icm_amd import bitstream as B
from icm_amd import codec
from test_qmap import ROI_CASES, _rects


# ------------------------------------------------------------------------------------------------ the restatement
def _loop_stats(img, top, left, gh, gw):
    out = [[[0, 0, 0] for _ in range(gw)] for _ in range(gh)]
    for y in range(img.shape[0]):
        for x in range(img.shape[1]):
            r, g, b = (int(v) for v in img[y, x])
            Y = (77 * r + 150 * g + 29 * b + 128) // 256
            cell = out[(top + y) // 16][(left + x) // 16]
            cell[0] += 1
            cell[1] += Y
            cell[2] += Y * Y
    return np.array(out, dtype=np.int32)


@pytest.mark.parametrize("case", [(1, 1, 31, 31, 4, 4), (17, 33, 0, 0, 2, 3), (20, 37, 7, 29, 2, 5),
                                  (16, 16, 0, 0, 1, 1)], ids=lambda c: "x".join(map(str, c)))
def test_restatement_equals_a_loop_over_pixels(case):
    H, W, top, left, gh, gw = case
    img = np.random.default_rng(H * 100 + W).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    got = A.cell_stats_ref(img, top, left, gh, gw)
    assert got.dtype == np.int32 and got.shape == (gh, gw, 3)
    assert np.array_equal(got, _loop_stats(img, top, left, gh, gw))
    assert int(got[..., 0].sum()) == H * W


def test_luma_weights_and_extremes():
    assert A.luma(np.array([[[255, 255, 255]]], dtype=np.uint8))[0, 0] == 255
    assert A.luma(np.array([[[0, 0, 0]]], dtype=np.uint8))[0, 0] == 0
    assert [int(A.luma(np.array([[c]], dtype=np.uint8))[0, 0]) for c in ([255, 0, 0], [0, 255, 0], [0, 0, 255])] == \
        [(77 * 255 + 128) >> 8, (150 * 255 + 128) >> 8, (29 * 255 + 128) >> 8] == [77, 149, 29]
    full = A.cell_stats_ref(np.full((16, 16, 3), 255, dtype=np.uint8), 0, 0, 1, 1)
    assert full.tolist() == [[[256, 65280, 16646400]]]


# ------------------------------------------------------------------------------------------------ the rule
def _stats(cells):
    """[1, len(cells), 3] statistics of cells given as lists of luma values"""
    return np.array([[[len(c), sum(c), sum(v * v for v in c)] for c in cells]], dtype=np.int32)


VAR0, VAR1, VAR3, VAR63 = [7, 7, 7], [0, 2], [0, 0, 0, 4], [64] + [0] * 63  # variances 0, 1, 3, 63: L = 0, 1, 2, 6


def test_activity_and_reference():
    st = _stats([VAR0, VAR1, [], VAR3, VAR63])
    act = codec.aq_activity(st)
    assert act.dtype == np.float64 and act.shape == (1, 5)
    assert act[0, [0, 1, 3, 4]].tolist() == [0.0, 1.0, 2.0, 6.0] and math.isnan(act[0, 2])
    assert np.array_equal(act, A.activity(st), equal_nan=True)
    assert codec.aq_reference(st) == A.reference(st) == 9.0 / 4.0            # the empty cell is not averaged
    big = A.cell_stats_ref(np.random.default_rng(3).integers(0, 256, size=(40, 70, 3), dtype=np.uint8), 0, 0, 3, 5)
    assert np.array_equal(codec.aq_activity(big), A.activity(big))
    assert codec.aq_reference(big) == pytest.approx(A.reference(big), rel=1e-14)


def test_offsets_on_hand_made_statistics():
    st = _stats([VAR0, VAR1, [], VAR3, VAR63])
    d = codec.aq_offsets(st, 1.0, 1.0)
    assert d.dtype == np.int8 and d.shape == (1, 5)
    assert d.tolist() == [[-4, 0, 0, 4, 16]]                                  # n = 0 gives 0; 4 (6 - 1) = 20 clips at 16
    assert codec.aq_offsets(st, -1.0, 1.0).tolist() == [[4, 0, 0, -4, -16]]   # the sign flips with the strength
    assert codec.aq_offsets(st, 4.0, 3.0).tolist() == [[-16, -16, 0, -16, 16]]
    assert codec.AQ_MAX_OFFSET == 16 and codec.AQ_STRENGTH_MAX == 4.0
    # ties go to the even integer: 4 (1 - ref) = 0.5, 1.5, 2.5, -0.5, -1.5 for the cell of variance 1
    one = _stats([VAR1])
    for ref, want in ((0.875, 0), (0.625, 2), (0.375, 2), (1.125, 0), (1.375, -2), (0.125, 4)):
        assert codec.aq_offsets(one, 1.0, ref).tolist() == [[want]], ref
        assert codec.aq_offsets(one, -1.0, ref).tolist() == [[-want]], ref
        assert A.offsets(one, 1.0, ref).tolist() == [[want]], ref
    for s in (1.0, -1.0, 0.3, 4.0):
        for ref in (0.0, 1.0, 2.25):
            assert np.array_equal(codec.aq_offsets(st, s, ref), A.offsets(st, s, ref))
    # a strength so small that everything rounds to 0
    assert not codec.aq_offsets(st, 0.01, 2.25).any()


def test_a_flat_image_gives_all_zeros():
    img = np.full((50, 70, 3), (200, 30, 90), dtype=np.uint8)
    for pads in ((0, 0, 0, 0), A.center_pads(50, 70)):
        st = A.stats_of(img, pads)
        ref = codec.aq_reference(A.stats_of(img, (0, 0, 0, 0)))
        assert ref == 0.0
        for s in (1.0, -4.0):
            d = codec.aq_offsets(st, s, ref)
            assert d.shape == st.shape[:2] and not d.any()


# ------------------------------------------------------------------------------------------------ quality_map
@pytest.mark.parametrize("size", [(100, 150), (64, 64)], ids=["100x150", "64x64"])
@pytest.mark.parametrize("case", list(ROI_CASES))
@pytest.mark.parametrize("base", [16, 0, -14])
def test_quality_map_without_offsets_is_roi_map(size, case, base):
    H, W = size
    rois = _rects(ROI_CASES[case], H, W)
    pads = codec.center_pads(H, W)
    got = codec.quality_map(H, W, pads, base, rois, None)
    assert got.dtype == np.int8 and np.array_equal(got, codec.roi_map(H, W, pads, base, rois))
    assert np.array_equal(got, codec.quality_map(H, W, pads, base, rois))
    assert np.array_equal(got, A.quality_map(H, W, pads, base, rois, None))
    # and with offsets: the restatement, per pixel
    offs = np.random.default_rng(100 + len(case) + base).integers(-16, 17, size=got.shape).astype(np.int8)
    with_offs = codec.quality_map(H, W, pads, base, rois, offs)
    assert with_offs.dtype == np.int8 and np.array_equal(with_offs, A.quality_map(H, W, pads, base, rois, offs))


def test_rectangles_win_over_offsets_and_both_clamp():
    H = W = 64
    pads = (0, 0, 0, 0)
    offs = np.array([[-16, -8, 0, 16]] * 4, dtype=np.int8)
    m = codec.quality_map(H, W, pads, 4, [(16, 0, 16, 64, -3)], offs)
    want = np.array([[-12, -4, 4, 20]] * 4, dtype=np.int8)
    want[1] = 1                                                               # the rectangle's row: base + d, no offset
    assert np.array_equal(m, want)
    # a rectangle with d = 0 still wins: its cells hold the base
    assert np.array_equal(codec.quality_map(H, W, pads, 4, [(16, 0, 16, 64, 0)], offs)[1], np.full(4, 4))
    low = codec.quality_map(H, W, pads, B.QSTEP_MIN + 2, [], offs)
    assert low[0].tolist() == [B.QSTEP_MIN, B.QSTEP_MIN, B.QSTEP_MIN + 2, 2]
    high = codec.quality_map(H, W, pads, B.QSTEP_MAX - 2, [(0, 0, 1, 1, 100)], offs)
    assert high[1].tolist() == [14, 22, 30, B.QSTEP_MAX] and high[0, 0] == B.QSTEP_MAX
    assert B.uniform_qmap(codec.quality_map(H, W, pads, 7, [], np.zeros((4, 4), dtype=np.int8))) == 7
    for bad in (offs[:3], offs.astype(np.float32), offs.reshape(-1)):
        with pytest.raises(ValueError, match="offsets"):
            codec.quality_map(H, W, pads, 4, [], bad)
    with pytest.raises(ValueError):
        codec.quality_map(H, W, pads, 40, [], offs)


# ------------------------------------------------------------------------------------------------ check_aq
def test_check_aq():
    assert codec.check_aq(None) is None and codec.check_aq(0) is None and codec.check_aq(0.0) is None
    assert codec.check_aq(-0.0) is None
    for s in (1, 1.0, -1.0, 0.25, 4.0, -4.0, np.float32(0.5), np.int64(2), 1e-9):
        got = codec.check_aq(s, "codec: ")
        assert type(got) is float and got == float(s) and 0 < abs(got) <= codec.AQ_STRENGTH_MAX
    for bad in (True, False, "1", "x", math.nan, math.inf, -math.inf, 4.000001, -5, 9, [1.0], np.array([1.0])):
        with pytest.raises(ValueError, match="aq"):
            codec.check_aq(bad, "codec: ")


def test_the_library_refuses_a_bad_strength_before_any_work():
    from icm_amd.zoo import models
    net = models["cnn"]().eval()
    img = np.zeros((64, 64, 3), dtype=np.uint8)
    for bad in (9, math.nan, "1", True):
        with pytest.raises(ValueError, match="aq"):
            codec.encode_image(net, img, aq=bad)
        with pytest.raises(ValueError, match="aq"):
            codec.encode_image_info(net, img, aq=bad)


# ------------------------------------------------------------------------------------------------ CLI argument errors
@pytest.mark.parametrize("value", ["nan", "9", "x", "inf", "-4.5"])
def test_codec_cli_refuses_a_bad_strength_before_any_gpu_check(value, tmp_path, capsys, monkeypatch):
    from PIL import Image

    def no_gpu_check():
        raise AssertionError("the GPU was asked for")
    monkeypatch.setattr(torch.cuda, "is_available", no_gpu_check)
    src, out = str(tmp_path / "in.png"), str(tmp_path / "o.icmb")
    Image.fromarray(np.zeros((64, 64, 3), dtype=np.uint8)).save(src)
    try:
        code = codec.main(["encode", src, "-o", out, "-p", "none.pt", "--aq", value])
    except SystemExit as e:                                                   # argparse's own refusal of a non-number
        code = e.code
    assert code == 2
    assert "aq" in capsys.readouterr().err
    assert not (tmp_path / "o.icmb").exists()
