"""CPU: ``icm_amd.residual.region_plan`` -- which waves of a residual string a window needs -- against a brute-force
restatement that asks, element by element, which wave owns it (wave g owns [g c, (g + 1) c) of a run, c = the per-wave
share rounded up to whole steps of 64: icm_amd/bitstream.py)."""
import numpy as np
import pytest

CELL = 16


def _owner(n, G):
    """int array [n]: the wave that owns each element of a run of n"""
    c = (-(-n // G) + 63) // 64 * 64
    return np.arange(n) // c, c


def _brute(H, W, G, window):
    y0, x0, h, w = window
    n = H * W
    own, c = _owner(n, G)
    rows = np.arange(n) // W
    waves = np.unique(own[(rows >= y0) & (rows < y0 + h)])              # the window's rows, at full width
    assert np.array_equal(waves, np.arange(waves[0], waves[-1] + 1))
    band = np.flatnonzero(np.isin(own, waves))                          # every element those waves own
    assert np.array_equal(band, np.arange(band[0], band[-1] + 1))
    cell_rows = np.unique(rows[band] // CELL)
    gh, gw = -(-H // CELL), -(-W // CELL)
    cown, _ = _owner(gh * gw, G)
    cells = np.arange(gh * gw)
    kwaves = np.unique(cown[np.isin(cells // gw, cell_rows)])
    assert np.array_equal(kwaves, np.arange(kwaves[0], kwaves[-1] + 1))
    return ((int(waves[0]), int(waves[-1]) + 1), (int(band[0]), int(band[-1]) + 1),
            (int(cell_rows[0]), int(cell_rows[-1]) + 1), (int(kwaves[0]), int(kwaves[-1]) + 1)), c


def _windows(H, W):
    out = [(0, 0, 1, 1), (H - 1, W - 1, 1, 1), (H // 2, 0, 1, W), (0, 0, H, W)]
    if H > 20 and W > 8:
        out += [(H - 3, 2, 3, 5), (17, 3, 2, 4)]
    return out


# W no multiple of 4 or 16; G = 1; a last wave that owns nothing (64 x 48 = 3072 elements in 9 waves of 384 and 100 x 64
# = 6400 in 51 waves of 128: the waves before the last hold them all); gh gw < 64: all classes in wave 0, the class range
# disjoint from the plane range of a window further down
SHAPES = [(40, 50, 16), (37, 67, 20), (150, 200, 30), (33, 47, 1), (64, 48, 9), (100, 64, 51), (16, 16, 3), (1, 1, 1),
          (5, 301, 4)]


@pytest.mark.parametrize("H,W,G", SHAPES)
def test_the_plan_is_the_brute_force_answer(H, W, G):
    from icm_amd import residual as R
    for window in _windows(H, W):
        want, c = _brute(H, W, G, window)
        got = R.region_plan(H, W, G, window)
        assert tuple(got) == want, (window, tuple(got), want)
        assert got.plane_waves == want[0] and got.band == want[1] and got.cell_rows == want[2] and got.class_waves == want[3]
        assert got.band == (got.plane_waves[0] * c, min(H * W, got.plane_waves[1] * c))


def test_the_shapes_hold_what_they_are_there_for():
    from icm_amd import residual as R
    assert [s for s in SHAPES if s[1] % 4] and [s for s in SHAPES if s[1] % 16 and not s[1] % 4] and (33, 47, 1) in SHAPES
    for H, W, G in ((64, 48, 9), (100, 64, 51)):                       # the last wave owns nothing
        own, c = _owner(H * W, G)
        assert own.max() < G - 1 and (G - 1) * c >= H * W
        assert R.region_plan(H, W, G, (H - 1, W - 1, 1, 1)).plane_waves[1] == own.max() + 1 < G
    # fewer than 64 cells: the classes sit in wave 0, and a window in the bottom rows needs plane waves far from it
    p = R.region_plan(40, 50, 16, (38, 0, 2, 50))
    assert p.class_waves == (0, 1) and p.plane_waves[0] > 1 and p.cell_rows[1] == 3
    p = R.region_plan(150, 200, 30, (140, 10, 5, 20))
    assert p.class_waves == (1, 3) and p.plane_waves == (27, 29)      # 28000 .. 28999 in waves of 1024
    # the whole image: every wave that owns anything, the band the planes
    p = R.region_plan(150, 200, 30, (0, 0, 150, 200))
    assert p.plane_waves == (0, 30) and p.band == (0, 30000) and p.class_waves == (0, 3)
    # one row of a wide image is not one wave's: a window costs whole waves
    p = R.region_plan(5, 301, 4, (2, 100, 1, 10))
    assert p.band[0] <= 2 * 301 and p.band[1] >= 3 * 301 and (p.band[1] - p.band[0]) % 64 in (0, (5 * 301) % 64)


def test_the_clamp_of_4096_waves():
    """plan only: a 12-megapixel image at symbols_per_wave = 1 has G = 4096 and c = 3008"""
    from icm_amd import ans
    from icm_amd import residual as R
    H, W = 3008, 4032
    G = ans.lanes_waves([H * W], 1)
    assert G == 4096
    c = ans.lanes_chunk(H * W, G)
    assert c == 3008 and -(-H * W // c) == 4032 < G           # 2961 per wave, rounded up to steps of 64: 64 waves idle
    for window in ((0, 0, 1, 1), (H - 1, W - 1, 1, 1), (1500, 0, 1, W), (1248, 1760, 512, 512), (0, 0, H, W)):
        y0, x0, h, w = window
        p = R.region_plan(H, W, G, window)
        (pa, pb), (e_lo, e_hi), (cr0, cr1), (ka, kb) = p
        assert 0 <= pa < pb <= G and (e_lo, e_hi) == (pa * c, min(H * W, pb * c))
        assert e_lo <= y0 * W and (y0 + h) * W <= e_hi        # the rows lie in the band
        assert e_lo > y0 * W - c and e_hi < (y0 + h) * W + c   # and no wave is there for nothing
        assert cr0 == (e_lo // W) // 16 and cr1 == ((e_hi - 1) // W) // 16 + 1
        gw, kc = 252, ans.lanes_chunk(188 * 252, G)
        assert kc == 64 and (ka, kb) == (cr0 * gw // kc, (cr1 * gw - 1) // kc + 1)
    assert R.region_plan(H, W, G, (0, 0, H, W)).plane_waves == (0, -(-H * W // c))


def test_refusals():
    from icm_amd import residual as R
    for window in ((0, 0, 0, 1), (0, 0, 1, 0), (-1, 0, 1, 1), (0, 0, 41, 1), (0, 49, 1, 2)):
        with pytest.raises(ValueError):
            R.region_plan(40, 50, 16, window)
    with pytest.raises(ValueError):
        R.region_plan(40, 50, 0, (0, 0, 1, 1))
