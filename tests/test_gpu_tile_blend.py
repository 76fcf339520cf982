"""GPU: ``icm_image_tile_blend`` (csrc/imageio.hip) against the numpy float32 restatement of its formula
(tests/_tiles_ref.py), bit for bit: two products and one sum per element, each rounded once, in a fixed association, so
there is no tolerance.  Kernel only, milliseconds each.

Every case runs on a canvas prefilled with random values inside the window (the accumulation shows) and NaN everywhere
else, from a source that is NaN outside its window: an element outside the window must keep its bits, and a read
outside the source window would poison the result."""
import numpy as np
import pytest
import torch

import _tiles_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = 1

# (PH, PW, top, left, h, w, H, W, y0, x0)
ODD = (32, 48, 3, 5, 24, 40, 50, 70, 7, 9)            # nothing aligned: the float-by-float path on both sides
VEC = (32, 48, 4, 8, 24, 40, 52, 72, 8, 12)           # all multiples of four: 16-byte accesses on both sides
SRC_VEC = (100, 152, 4, 8, 70, 131, 129, 203, 5, 7)   # ten workgroups, a ragged last run; only the source side aligned
DST_VEC = (101, 151, 3, 5, 70, 131, 128, 200, 8, 12)  # ... only the canvas side (and not in every plane / row)
GEOMS = {"odd": ODD, "vec": VEC, "src_vec": SRC_VEC, "dst_vec": DST_VEC}


def _case(geom, seed):
    PH, PW, top, left, h, w, H, W, y0, x0 = geom
    rng = np.random.default_rng(seed)
    src = np.full((3, PH, PW), np.nan, np.float32)
    src[:, top:top + h, left:left + w] = rng.uniform(-2, 2, (3, h, w)).astype(np.float32)
    canvas = np.full((3, H, W), np.nan, np.float32)
    canvas[:, y0:y0 + h, x0:x0 + w] = rng.uniform(-2, 2, (3, h, w)).astype(np.float32)
    return src, canvas


def _run(geom, src, canvas, m, edges):
    from icm_amd import _lib as L
    from icm_amd import codec
    PH, PW, top, left, h, w, H, W, y0, x0 = geom
    s, c = torch.from_numpy(src).to(DEV), torch.from_numpy(canvas).to(DEV)
    ramp = torch.from_numpy(codec.blend_ramp(m)).to(DEV) if m else None
    rc = L.lib().icm_image_tile_blend(s.data_ptr(), PH, PW, top, left, h, w, c.data_ptr(), H, W, y0, x0, L.ptr(ramp), m,
                                      edges, L.stream())
    torch.cuda.synchronize()
    return rc, c.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("m", [0, 1, 8])
@pytest.mark.parametrize("name", list(GEOMS))
def test_blend_equals_the_formula_bit_for_bit(name, m):
    geom = GEOMS[name]
    src, canvas = _case(geom, seed=11 + m)
    rc, got = _run(geom, src, canvas, m, 15)
    assert rc == 0
    want = R.blend(canvas, src, *geom[2:6], *geom[8:10], m, 15)
    assert not np.isnan(want[:, geom[8]:geom[8] + geom[4], geom[9]:geom[9] + geom[5]]).any()
    assert _same_bits(got, want)                      # the window, and every NaN around it with its bits
    assert not _same_bits(got, canvas)


@pytest.mark.parametrize("edges", range(16))
def test_every_edge_mask(edges):
    src, canvas = _case(ODD, seed=100 + edges)
    rc, got = _run(ODD, src, canvas, 8, edges)
    assert rc == 0
    assert _same_bits(got, R.blend(canvas, src, *ODD[2:6], *ODD[8:10], 8, edges))


def test_a_pixel_under_one_tile_keeps_its_value_and_two_runs_agree():
    """zero canvas, no neighbours: 0 + 1 * v = v exactly; with bands, two runs give the same bits"""
    PH, PW, top, left, h, w, H, W, y0, x0 = ODD
    src, canvas = _case(ODD, seed=5)
    canvas[:] = 0.0
    rc, got = _run(ODD, src, canvas, 8, 0)
    assert rc == 0
    assert _same_bits(got[:, y0:y0 + h, x0:x0 + w], src[:, top:top + h, left:left + w])
    a, b = _run(ODD, src, canvas, 8, 15)[1], _run(ODD, src, canvas, 8, 15)[1]
    assert _same_bits(a, b)


def test_band_as_wide_as_the_window_and_both_bands_over_one_pixel():
    """m == w is accepted; where the near and the far band both reach a pixel the near side decides"""
    geom = (16, 16, 2, 3, 8, 8, 20, 20, 5, 6)
    src, canvas = _case(geom, seed=8)
    rc, got = _run(geom, src, canvas, 8, 15)
    assert rc == 0
    assert _same_bits(got, R.blend(canvas, src, 2, 3, 8, 8, 5, 6, 8, 15))


def test_two_tiles_over_a_band_sum_to_the_value():
    """a constant image cut into two overlapping tiles comes back to within one rounding of the constant"""
    from icm_amd import _lib as L
    from icm_amd import codec
    m, H, W = 8, 12, 40
    v = np.float32(0.7)
    tile = torch.full((3, H, 24), float(v), dtype=torch.float32, device=DEV)
    canvas = torch.zeros((3, H, W), dtype=torch.float32, device=DEV)
    ramp = torch.from_numpy(codec.blend_ramp(m)).to(DEV)
    for x0, e in ((0, R.EDGE_RIGHT), (16, R.EDGE_LEFT)):
        assert L.lib().icm_image_tile_blend(tile.data_ptr(), H, 24, 0, 0, H, 24, canvas.data_ptr(), H, W, 0, x0,
                                            ramp.data_ptr(), m, e, L.stream()) == 0
    got = canvas.cpu().numpy()
    want = R.blend(R.blend(np.zeros((3, H, W), np.float32), np.full((3, H, 24), v), 0, 0, H, 24, 0, 0, m, R.EDGE_RIGHT),
                   np.full((3, H, 24), v), 0, 0, H, 24, 0, 16, m, R.EDGE_LEFT)
    assert _same_bits(got, want)
    assert np.abs(got - v).max() <= 2 * np.spacing(v) and (got[:, :, :16] == v).all() and (got[:, :, 24:] == v).all()


def test_refused_arguments_leave_the_canvas_untouched():
    from icm_amd import _lib as L
    PH, PW, top, left, h, w, H, W, y0, x0 = ODD
    src, canvas = _case(ODD, seed=3)
    s, c = torch.from_numpy(src).to(DEV), torch.from_numpy(canvas).to(DEV)
    ramp = torch.full((64,), 0.5, dtype=torch.float32, device=DEV)
    S, C, RP, st = s.data_ptr(), c.data_ptr(), ramp.data_ptr(), L.stream()
    good = (S, PH, PW, top, left, h, w, C, H, W, y0, x0, RP, 8, 15)
    bad = [
        (0,) + good[1:],                                               # null source
        good[:7] + (0,) + good[8:],                                    # null canvas
        good[:12] + (0, 8, 15),                                        # m > 0 without a ramp
        good[:13] + (-1, 15),                                          # m < 0
        good[:14] + (16,), good[:14] + (-1,),                          # edges outside the mask
        (S, 0, PW) + good[3:], (S, PH, -1) + good[3:], (S, 32769, PW) + good[3:],
        good[:5] + (0, w) + good[7:], good[:5] + (h, 0) + good[7:], good[:5] + (-3, w) + good[7:],
        good[:8] + (0, W) + good[10:], good[:8] + (H, 32769) + good[10:],
        good[:3] + (-1, left) + good[5:], good[:3] + (top, -1) + good[5:],
        good[:3] + (PH - h + 1, left) + good[5:], good[:3] + (top, PW - w + 1) + good[5:],      # window outside src
        good[:10] + (-1, x0) + good[12:], good[:10] + (y0, -1) + good[12:],
        good[:10] + (H - h + 1, x0) + good[12:], good[:10] + (y0, W - w + 1) + good[12:],       # ... outside the canvas
        good[:13] + (w + 1, 1), good[:13] + (w + 1, 2), good[:13] + (h + 1, 4), good[:13] + (h + 1, 8),  # band > window
    ]
    for a in bad:
        assert L.lib().icm_image_tile_blend(*a, st) == ERR_ARG, a
    torch.cuda.synchronize()
    assert _same_bits(c.cpu().numpy(), canvas)
    # a band wider than the window is no matter on a side without a neighbour, and the good call does write
    assert L.lib().icm_image_tile_blend(*good[:13], h + 1, 3, st) == 0      # left + right only: h is not looked at
    assert L.lib().icm_image_tile_blend(*good, st) == 0
    torch.cuda.synchronize()
    assert not _same_bits(c.cpu().numpy(), canvas)
