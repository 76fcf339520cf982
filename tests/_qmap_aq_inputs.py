"""Inputs and float64 references of the AQ-map tests (``icm_qmap_aq``, ``Trainer(qmap_aq=...)``): the image generators,
the cases the GPU file runs, and for each case the maps and mean activities of ``tests/_aq_ref.py`` (Python integers and
float64, an ``fsum`` mean).  CPU only and deterministic, so that tests/test_qmap_aq_ref.py can check on any machine what
tests/test_gpu_qmap_aq_numerics.py relies on: that no cell of a case lies in the zone where device and reference may
round differently, and that every case reaches what it is named for.

The zone (derived in the numerics file's docstring): device and reference differ only through the last bits of log2
and of the mean, below 2e-11 on the value 4 S (L - mean) that is rounded, so a map must equal the reference on every
cell whose value lies more than ZONE = 1e-9 from a half-integer; a cell inside may be either neighbour."""
import functools

import numpy as np

import _aq_ref as A

F = np.float32
CELL = 16
ZONE = 1e-9
REF_LIMIT = 1e-12
AMPLITUDES = (0, 1, 2, 4, 8, 16, 32, 64, 127)


# ------------------------------------------------------------------------------------------------ images
def noise_images(N, H, W, seed):
    """uint8 [N, H, W, 3]: uniform 8-bit noise"""
    return np.random.default_rng(seed).integers(0, 256, (N, H, W, 3)).astype(np.uint8)


def mixed_images(N, H, W, seed):
    """uint8 [N, H, W, 3]: every 16 x 16 cell is noise of an amplitude drawn from AMPLITUDES around a mean of its own,
    so an image holds flat cells (activity 0) next to cells busy enough to saturate the offset; cell (0, 0) of every
    image is flat and cell (0, 1) has the largest amplitude"""
    rng = np.random.default_rng(seed)
    h, w = H // CELL, W // CELL
    amp = rng.choice(AMPLITUDES, (N, h, w))
    amp[:, 0, 0], amp[:, 0, 1] = 0, 127
    mean = rng.integers(0, 256, (N, h, w))
    up = lambda a: np.repeat(np.repeat(a, CELL, axis=1), CELL, axis=2)[..., None]   # noqa: E731
    a = up(amp)
    d = np.floor(rng.random((N, H, W, 3)) * (2 * a + 1)).astype(np.int64) - a
    return np.clip(up(mean) + d, 0, 255).astype(np.uint8)


def float_images(N, H, W, seed):
    """float32 [N, 3, H, W]: arbitrary values, a fifth of them below 0 or above 1, smooth enough per cell to give
    different activities (a per-cell scale times uniform noise around a per-cell level)"""
    rng = np.random.default_rng(seed)
    h, w = H // CELL, W // CELL
    up = lambda a: np.repeat(np.repeat(a, CELL, axis=2), CELL, axis=3)   # noqa: E731
    level = up(rng.uniform(-0.2, 1.2, (N, 1, h, w)))
    scale = up(rng.choice([0.0, 0.01, 0.05, 0.2, 0.6], (N, 1, h, w)))
    return (level + scale * rng.uniform(-1.0, 1.0, (N, 3, H, W))).astype(F)


def planar(u8):
    """uint8 [N, H, W, 3] -> float32 [N, 3, H, W] = fl32(k / 255), what ToTensor and icm_image_u8_to_f32 make"""
    return np.ascontiguousarray(np.moveaxis(u8.astype(F) / F(255.0), -1, 1))


def to_u8(x):
    """float32 [N, 3, H, W] -> uint8 [N, H, W, 3] by the rule of icm_image_f32_to_u8, in numpy float32: clamp to
    [0, 1], one multiplication by 255 rounded to float32, truncation"""
    x = np.asarray(x)
    assert x.dtype == F
    v = np.minimum(np.maximum(x, F(0.0)), F(1.0)) * F(255.0)
    assert v.dtype == F
    return np.ascontiguousarray(np.moveaxis(v.astype(np.int64), 1, -1)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ cases
def _rects(h, w):
    """[2, 2, 5] (y0, x0, y1, x1, k) in cells: image 0 an empty rectangle and one the map's edge clips, image 1 two
    that overlap, the second clipped at the top left corner and winning where they meet"""
    return np.array([[(1, 1, 1, 3, -5), (h - 1, w - 2, h + 3, w + 4, 20)],
                     [(0, 0, 2, 2, 7), (-1, -1, 1, 1, -9)]], dtype=np.int32)


# name -> (generator, (N, H, W), seed, strength [N], base [N], rects or None, what the case must reach)
CASES = {
    "mixed-48x80": ("mixed", (3, 48, 80), 11, [4.0, -2.5, 1.0], [-16, 8, 32], None,
                    {"saturated", "clamp_lo", "clamp_hi", "flat"}),
    "noise-48x80": ("noise", (3, 48, 80), 12, [0.37, 4.0, -4.0], [0, -3, 17], None, set()),
    "mixed-64x64": ("mixed", (2, 64, 64), 13, [0.0, -4.0], [5, -16], _rects(4, 4),
                    {"saturated", "clamp_lo", "flat", "rect_wins"}),
    "noise-64x64": ("noise", (2, 64, 64), 14, [1.0, -2.5], [32, -16], _rects(4, 4), {"rect_wins"}),
    "mixed-128x192": ("mixed", (2, 128, 192), 15, [0.37, 4.0], [32, 0], _rects(8, 12),
                      {"saturated", "clamp_hi", "flat", "rect_wins"}),
    "floats-48x80": ("floats", (3, 48, 80), 16, [1.0, 4.0, -1.0], [5, -16, 32], None, {"clamp_lo", "flat"}),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(x float32 [N, 3, H, W], u8 uint8 [N, H, W, 3], strength float32 [N], base int8 [N], rects int32 [N, R, 5] or
    None) of a case; u8 is what the codec would see of x"""
    kind, (N, H, W), seed, strength, base, rects, _ = CASES[name]
    if kind == "floats":
        x = float_images(N, H, W, seed)
        u8 = to_u8(x)
    else:
        u8 = (mixed_images if kind == "mixed" else noise_images)(N, H, W, seed)
        x = planar(u8)
    return x, u8, np.array(strength, dtype=F), np.array(base, dtype=np.int8), rects


# ------------------------------------------------------------------------------------------------ reference
def paint_over(m, rects):
    """the rectangles (y0, x0, y1, x1, k) of one image over its map, as icm_qmap_paint paints them: cells, half open,
    clipped to the map, in order, k as given"""
    m = m.copy()
    h, w = m.shape
    for y0, x0, y1, x1, k in np.asarray(rects).reshape(-1, 5).tolist():
        y0, x0, y1, x1 = max(y0, 0), max(x0, 0), min(y1, h), min(x1, w)
        if y1 > y0 and x1 > x0:
            m[y0:y1, x0:x1] = k
    return m


def image_reference(u8, strength, base, rects=None):
    """one image -> dict: "ref" the mean activity (fsum), "value" float64 [h, w] = 4 S (L - ref), the number that is
    rounded, "offsets" int8, "aq" the map before the rectangles, "map" int8 [h, w] after them.  ``strength`` is taken
    as the float32 the device reads."""
    H, W = u8.shape[:2]
    S = float(F(strength))
    stats = A.stats_of(u8, (0, 0, 0, 0))
    act, ref = A.activity(stats), A.reference(stats)
    offs = A.offsets(stats, S, ref)
    aq = A.quality_map(H, W, (0, 0, 0, 0), int(base), [], offs)
    return {"ref": ref, "activity": act, "value": 4.0 * S * (act - ref), "offsets": offs, "aq": aq,
            "map": aq if rects is None else paint_over(aq, rects)}


@functools.lru_cache(maxsize=None)
def reference(name):
    """the per-image references of a case, stacked: dict of arrays with a leading N"""
    _, u8, strength, base, rects = case(name)
    per = [image_reference(u8[n], strength[n], base[n], None if rects is None else rects[n]) for n in range(len(u8))]
    return {k: np.stack([np.asarray(p[k]) for p in per]) for k in per[0]}


def zone_distance(value):
    """distance of every value to the nearest half-integer"""
    v = np.asarray(value, dtype=np.float64)
    return np.abs(v - (np.floor(v) + 0.5))


def check_maps(got, want, value, what=""):
    """the zone rule: ``got`` equals ``want`` on every cell outside the zone; a cell inside it (and not painted by a
    rectangle: there both hold the rectangle's k) may hold either neighbour's step.  Returns the number of cells
    inside the zone."""
    got, want = np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    inside = zone_distance(value) <= ZONE
    bad = (got != want) & ~inside
    assert not bad.any(), f"{what}: {int(bad.sum())} cells differ outside the zone, first at {np.argwhere(bad)[0]}: " \
                          f"{got[bad][0]} != {want[bad][0]}"
    assert (np.abs(got - want)[inside] <= 1).all(), f"{what}: a cell inside the zone is no neighbour"
    return int(inside.sum())


def reached(name):
    """what a case's reference reaches, as the set of names CASES uses"""
    _, _, strength, base, rects = case(name)
    r = reference(name)
    b = base.astype(np.int64).reshape(-1, 1, 1)
    out = set()
    if (np.abs(r["offsets"]) == A.AQ_MAX_OFFSET).any() and (np.abs(r["value"]) > A.AQ_MAX_OFFSET + 0.5).any():
        out.add("saturated")
    if ((b + r["offsets"]) < A.QSTEP_MIN).any():
        out.add("clamp_lo")
    if ((b + r["offsets"]) > A.QSTEP_MAX).any():
        out.add("clamp_hi")
    if (r["activity"] == 0.0).any():
        out.add("flat")
    if rects is not None and (r["map"] != r["aq"]).any():
        out.add("rect_wins")
    return out
