"""GPU: ``icm_image_cell_stats`` (csrc/imageio.hip), the per-cell luma statistics behind the encoder's
variance-adaptive quality maps, against the integer restatement (tests/_aq_ref.py) bit for bit: the output is prefilled
with a sentinel, so an entry the kernel skips or writes twice with another value shows."""
import numpy as np
import pytest
import torch

import _aq_ref as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -12345
ERR_ARG = 1


def _lib():
    from icm_amd import _lib as L
    return L


def _run(img, top, left, gh, gw, offset=0):
    """the kernel on ``img`` placed ``offset`` bytes into a device buffer (offset 1: a pointer of no alignment at all)"""
    L = _lib()
    H, W = img.shape[:2]
    buf = torch.zeros(img.size + offset + 16, dtype=torch.uint8, device=DEV)
    buf[offset:offset + img.size] = torch.from_numpy(np.ascontiguousarray(img).reshape(-1)).to(DEV)
    out = torch.full((gh + 1, gw, 3), SENT, dtype=torch.int32, device=DEV)       # one row of cells more: a guard
    rc = L.lib().icm_image_cell_stats(buf.data_ptr() + offset, H, W, top, left, gh, gw, out.data_ptr(), L.stream())
    torch.cuda.synchronize()
    assert bool((out[gh] == SENT).all())
    return rc, out[:gh].cpu().numpy()


def _random(H, W):
    return np.random.default_rng(1000 * H + W).integers(0, 256, size=(H, W, 3), dtype=np.uint8)


def _checker(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)


def _channels(H, W):
    """three channels that differ from each other and across the image, 0 and 255 among them"""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([(yy * 4) % 256, (xx * 4 + 3) % 256, ((yy + 2 * xx) * 5) % 256], -1).astype(np.uint8)


CASES = {
    "1x1 at (31, 31) of a 4x4 grid": (_random(1, 1), 31, 31, 4, 4),
    "16x16, one full cell": (_random(16, 16), 0, 0, 1, 1),
    "17x33, ragged last row and column": (_random(17, 33), 0, 0, 2, 3),
    "50x70 at (7, 29), partial cells on four sides": (_random(50, 70), 7, 29, 4, 8),
    "16x1040, 65 cells wide": (_random(16, 1040), 0, 0, 1, 65),
    "272x16, 17 cells tall": (_random(272, 16), 0, 0, 17, 1),
    "64x64 all 255": (np.full((64, 64, 3), 255, dtype=np.uint8), 0, 0, 4, 4),
    "64x64 all 0": (np.zeros((64, 64, 3), dtype=np.uint8), 0, 0, 4, 4),
    "64x64 checkerboard of 0 and 255": (_checker(64, 64), 0, 0, 4, 4),
    "64x64 channels that differ": (_channels(64, 64), 0, 0, 4, 4),
}


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "odd_pointer"])
@pytest.mark.parametrize("name", list(CASES))
def test_cell_stats_equal_the_restatement_bit_for_bit(name, offset):
    img, top, left, gh, gw = CASES[name]
    H, W = img.shape[:2]
    want = A.cell_stats_ref(img, top, left, gh, gw)
    rc, got = _run(img, top, left, gh, gw, offset)
    assert rc == 0
    assert got.dtype == np.int32 and np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert int(got[..., 0].sum()) == H * W and SENT not in got
    if name.startswith("1x1"):
        assert int((got[..., 0] == 1).sum()) == 1 and int((got[..., 0] == 0).sum()) == 15 and got[1, 1, 0] == 1
        assert not got[got[..., 0] == 0].any()                                  # a cell in the padding: 0, 0, 0
    if name.endswith("all 255"):
        assert (got == np.array([256, 65280, 16646400])).all()
    if name.endswith("all 0"):
        assert (got == np.array([256, 0, 0])).all()
    if "checkerboard" in name:
        assert (got == np.array([256, 128 * 255, 128 * 255 * 255])).all()
    if "channels" in name:                                                       # another weighting gives other sums
        grey = np.repeat(img.astype(np.int64).sum(-1, keepdims=True) // 3, 3, axis=2).astype(np.uint8)
        assert not np.array_equal(A.cell_stats_ref(grey, top, left, gh, gw)[..., 1], want[..., 1])
        swapped = A.cell_stats_ref(img[..., ::-1], top, left, gh, gw)
        assert not np.array_equal(swapped[..., 1], want[..., 1])


def test_a_grid_larger_than_the_image_and_the_codecs_pads():
    """the grid the codec asks for: centre pads of a 100 x 150 image (top 14, left 21), cells of padding all around"""
    img = _random(100, 150)
    left, right, top, bottom = A.center_pads(100, 150)
    gh, gw = (top + 100 + bottom) // 16, (left + 150 + right) // 16
    rc, got = _run(img, top, left, gh, gw)
    assert rc == 0 and (gh, gw) == (8, 12) and np.array_equal(got, A.cell_stats_ref(img, top, left, gh, gw))
    assert not got[:, 0].any() and not got[:, -1].any()                          # columns wholly in the padding
    from icm_amd import codec
    u8 = torch.from_numpy(img).to(DEV)
    st = codec.cell_stats(u8, (left, right, top, bottom))
    assert st.dtype == np.int32 and np.array_equal(st, got)
    anchored = codec.cell_stats(u8, (0, 0, 0, 0))
    assert anchored.shape == (7, 10, 3) and np.array_equal(anchored, A.cell_stats_ref(img, 0, 0, 7, 10))


def test_argument_errors_leave_the_output_alone():
    L = _lib()
    img = torch.from_numpy(_random(50, 70)).to(DEV)
    out = torch.full((4, 8, 3), SENT, dtype=torch.int32, device=DEV)
    good = dict(img=img.data_ptr(), H=50, W=70, top=7, left=29, gh=4, gw=8, stats=out.data_ptr())

    def call(**kw):
        a = {**good, **kw}
        return L.lib().icm_image_cell_stats(a["img"], a["H"], a["W"], a["top"], a["left"], a["gh"], a["gw"], a["stats"],
                                            L.stream())

    bad = [{"img": 0}, {"stats": 0}, {"H": 0}, {"H": -1}, {"W": 0}, {"W": -5}, {"gh": 0}, {"gh": -1}, {"gw": 0},
           {"gw": -1}, {"top": -1}, {"left": -1},
           {"top": 15}, {"gh": 3}, {"H": 58},                                    # top + H > 16 gh
           {"left": 59}, {"gw": 6}, {"W": 100}]                                  # left + W > 16 gw
    for kw in bad:
        assert call(**kw) == ERR_ARG, kw
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
    assert call(top=14, left=58) == 0                                            # the image just fits the grid
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), A.cell_stats_ref(img.cpu().numpy(), 14, 58, 4, 8))
