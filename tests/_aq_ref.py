"""Variance-adaptive quantisation restated in numpy, independently of the package: the per-cell luma statistics of an
8-bit image in integer arithmetic (what ``icm_image_cell_stats`` computes), and the host rule that turns them into
offsets to the background step index and into a quality map (``icm_amd.codec``: ``aq_activity``, ``aq_reference``,
``aq_offsets``, ``quality_map``), cell by cell in Python numbers."""
import math

import numpy as np

import _qmap_ref as QM

CELL = 16
AQ_STRENGTH_MAX = 4.0
AQ_MAX_OFFSET = 16
QSTEP_MIN, QSTEP_MAX = QM.QSTEP_MIN, QM.QSTEP_MAX
center_pads = QM.center_pads


def luma(img):
    """int64 [H, W]: (77 R + 150 G + 29 B + 128) >> 8 of an 8-bit [H, W, 3] image"""
    a = np.asarray(img).astype(np.int64)
    return (77 * a[..., 0] + 150 * a[..., 1] + 29 * a[..., 2] + 128) >> 8


def cell_stats_ref(img, top, left, gh, gw):
    """int32 [gh, gw, 3] = (n, sum Y, sum Y^2) over the image pixels of each cell of the grid of the image padded by
    ``top`` rows and ``left`` columns; integers only.  The image is laid into a canvas of whole cells next to a mask of
    where it lies, and every cell is summed."""
    Y = luma(img)
    H, W = Y.shape
    assert top >= 0 and left >= 0 and top + H <= CELL * gh and left + W <= CELL * gw
    canvas = np.zeros((3, CELL * gh, CELL * gw), dtype=np.int64)
    canvas[0, top:top + H, left:left + W] = 1
    canvas[1, top:top + H, left:left + W] = Y
    canvas[2, top:top + H, left:left + W] = Y * Y
    s = canvas.reshape(3, gh, CELL, gw, CELL).sum(axis=(2, 4))
    assert s.max() < 2 ** 31
    return np.ascontiguousarray(np.moveaxis(s, 0, -1)).astype(np.int32)


def grid_of(H, W, pads):
    """(top, left, gh, gw) of the grid of an H x W image padded by ``pads`` = (left, right, top, bottom)"""
    left, right, top, bottom = pads
    return top, left, -(-(top + H + bottom) // CELL), -(-(left + W + right) // CELL)


def stats_of(img, pads):
    return cell_stats_ref(img, *grid_of(img.shape[0], img.shape[1], pads))


def activity(stats):
    """float64 [gh, gw]: log2(1 + (n s2 - s1^2) / n^2), the numerator and the denominator formed as Python integers and
    divided once; nan where n = 0"""
    st = np.asarray(stats)
    v = np.full(st.shape[:2], np.nan)
    for i in range(st.shape[0]):
        for j in range(st.shape[1]):
            n, s1, s2 = (int(t) for t in st[i, j])
            if n:
                v[i, j] = (n * s2 - s1 * s1) / (n * n)
    with np.errstate(invalid="ignore"):
        return np.log2(1.0 + v)


def reference(stats_anchored):
    """the mean activity over the cells that hold a pixel, summed without rounding error"""
    a = activity(stats_anchored)
    vals = [float(t) for t in a.reshape(-1) if not math.isnan(t)]
    return math.fsum(vals) / len(vals)


def offsets(stats, strength, ref):
    """int8 [gh, gw]: clip(round-half-even(4 strength (L - ref)), -16, 16), 0 where n = 0"""
    a = activity(stats)
    out = np.zeros(a.shape, dtype=np.int8)
    for i in range(a.shape[0]):
        for j in range(a.shape[1]):
            if not math.isnan(a[i, j]):
                d = round(4.0 * strength * (float(a[i, j]) - ref))          # Python's round: ties to even
                out[i, j] = max(-AQ_MAX_OFFSET, min(AQ_MAX_OFFSET, d))
    return out


def quality_map(H, W, pads, base, rois, offs):
    """every cell clamp(base + its offset), then per pixel of every rectangle, in list order, clamp(base + d)"""
    left, right, top, bottom = pads
    gh, gw = (top + H + bottom) // CELL, (left + W + right) // CELL
    m = np.full((gh, gw), base, dtype=np.int64)
    if offs is not None:
        assert offs.shape == (gh, gw)
        m = np.clip(base + offs.astype(np.int64), QSTEP_MIN, QSTEP_MAX)
    for y0, x0, h, w, d in rois:
        k = max(QSTEP_MIN, min(QSTEP_MAX, base + d))
        for y in range(y0, y0 + h):
            for x in range(x0, x0 + w):
                m[(top + y) // CELL, (left + x) // CELL] = k
    return m.astype(np.int8)


def image_maps(img, strength, base=0, tiles=None, rois_per_tile=None):
    """(reference, [offsets per tile], [quality map per tile]) of an encode of ``img``: the reference from the grid
    anchored at the whole image's first pixel, each tile (y0, x0, h, w) with its own centre pads.  ``tiles`` None: the
    image as one tile."""
    H, W = img.shape[:2]
    tiles = [(0, 0, H, W)] if tiles is None else tiles
    ref = reference(stats_of(img, (0, 0, 0, 0)))
    offs, maps = [], []
    for t, (y0, x0, h, w) in enumerate(tiles):
        pads = center_pads(h, w)
        o = offsets(stats_of(img[y0:y0 + h, x0:x0 + w], pads), strength, ref)
        offs.append(o)
        maps.append(quality_map(h, w, pads, base, [] if rois_per_tile is None else rois_per_tile[t], o))
    return ref, offs, maps
