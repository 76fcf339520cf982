"""Host restatement, in numpy and Python integers, of the residual layer under a bound per 16 x 16-pixel cell
(icm_amd/residual.py, csrc/residual.hip ``icm_residual_code_map`` / ``icm_residual_apply_map``, the ICME container of
icm_amd/bitstream.py, ``codec.error_map``): the quantiser and the reconstruction with a map, the painter of the
rectangles pixel by pixel, the map string, and the cases the GPU kernel test runs, with the path each of them is named
for, so that a CPU test can check that it gets there.  Nothing here imports the package."""
import struct

import numpy as np

CELL = 16
MAX_ERROR = 32
RUN = 4                 # window pixels per thread of the apply kernel


def grid(H, W):
    return -(-H // CELL), -(-W // CELL)


def per_pixel(dmap, H, W, window=None):
    """int64 [h, w]: the bound of every pixel of the window (y0, x0, h, w) of the H x W image, that of the cell of its
    image position; a map byte above 32 counts as 32, as in the kernels"""
    d = np.minimum(np.asarray(dmap).reshape(grid(H, W)).astype(np.int64), MAX_ERROR)
    y0, x0, h, w = (0, 0, H, W) if window is None else window
    ys, xs = (np.arange(y0, y0 + h) // CELL)[:, None], (np.arange(x0, x0 + w) // CELL)[None, :]
    return d[ys, xs]


# ------------------------------------------------------------------------------------------------- arithmetic
def quantise_map(x, xhat, dmap):
    """8-bit [H, W, 3] original and reconstruction, bounds [gh, gw] -> q, int32 in plane order [3, H, W]:
    q = sign(r) ((|r| + D) div (2 D + 1)) with D the bound of the sample's cell"""
    x = np.asarray(x)
    r = x.astype(np.int64) - np.asarray(xhat).astype(np.int64)
    d = per_pixel(dmap, x.shape[0], x.shape[1])[..., None]
    q = np.sign(r) * ((np.abs(r) + d) // (2 * d + 1))
    return np.ascontiguousarray(q.transpose(2, 0, 1)).astype(np.int32)


def reconstruct_map(xhat_window, q, dmap, window=None):
    """8-bit [h, w, 3] reconstruction of the window (y0, x0, h, w), the image's q [3, H, W] and its bounds [gh, gw]
    -> 8-bit [h, w, 3]: clamp(xhat + q (2 D + 1), 0, 255), D that of the cell of the pixel's image position"""
    H, W = q.shape[1:]
    y0, x0, h, w = (0, 0, H, W) if window is None else window
    qq = q[:, y0:y0 + h, x0:x0 + w].astype(np.int64).transpose(1, 2, 0)
    s = 2 * per_pixel(dmap, H, W, (y0, x0, h, w))[..., None] + 1
    return np.clip(np.asarray(xhat_window).astype(np.int64) + qq * s, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------- painter
def paint(H, W, base, rois):
    """uint8 [gh, gw], pixel by pixel: every pixel starts at ``base``, the rectangles (y0, x0, h, w, d) are laid over
    the pixels in list order, and a cell takes the d of the last rectangle that holds one of its pixels"""
    gh, gw = grid(H, W)
    m = np.full((gh, gw), base, np.uint8)
    for y0, x0, h, w, d in rois:
        touched = np.zeros((gh, gw), bool)
        for y in range(y0, y0 + h):
            for x in range(x0, x0 + w):
                touched[y // CELL, x // CELL] = True
        m[touched] = d
    return m


# ------------------------------------------------------------------------------------------------- map string
def map_string(dmap):
    """u16 gh, u16 gw, then maximal runs (u16 count, u8 d) in row-major order, a run longer than 65535 split into
    full counts first"""
    dmap = np.asarray(dmap)
    out = bytearray(struct.pack("<HH", *dmap.shape))
    flat = [int(v) for v in dmap.reshape(-1)]
    i = 0
    while i < len(flat):
        j = i
        while j < len(flat) and flat[j] == flat[i]:
            j += 1
        n = j - i
        while n > 0:
            c = min(n, 65535)
            out += struct.pack("<HB", c, flat[i])
            n -= c
        i = j
    return bytes(out)


def map_from_string(data):
    gh, gw = struct.unpack_from("<HH", data, 0)
    flat = []
    for off in range(4, len(data), 3):
        c, d = struct.unpack_from("<HB", data, off)
        flat += [d] * c
    return np.asarray(flat, np.uint8).reshape(gh, gw)


# ------------------------------------------------------------------------------------------------- kernel cases
SHAPES = [(1, 1), (16, 16), (17, 33), (37, 53), (64, 48)]


def random_map(H, W, seed):
    """bounds over 0..32 with the two extremes side by side wherever the grid has two cells in a row or a column: cell
    (0, 0) lossless, its right and lower neighbours at 32"""
    rng = np.random.default_rng(1000 + seed)
    gh, gw = grid(H, W)
    m = rng.integers(0, MAX_ERROR + 1, size=(gh, gw)).astype(np.uint8)
    m[0, 0] = 0
    if gw > 1:
        m[0, 1] = 32
    if gh > 1:
        m[1, 0] = 32
    if gh > 1 and gw > 1:
        m[1, 1] = 0
    return m


def random_pair(H, W, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    # half of the image close to x (small classes), half independent (large ones)
    near = np.clip(x.astype(np.int64) + rng.integers(-6, 7, size=x.shape), 0, 255).astype(np.uint8)
    far = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    return x, np.where((np.arange(W) < (W + 1) // 2)[None, :, None], near, far).astype(np.uint8)


def extreme_pair(H, W, reverse):
    a, b = np.full((H, W, 3), 255, np.uint8), np.zeros((H, W, 3), np.uint8)
    return (b, a) if reverse else (a, b)


def run_paths(H, W, byte_offset=0, elem_offset=0):
    """as ``_residual_ref.run_paths``: "dword" / "byte" for the interleaved side of the runs of four pixels of an
    H x W image, "vec" / "scalar" for the planar side, "full" / "partial" for the cells"""
    seen = set()
    for y in range(H):
        for x0 in range(0, W, RUN):
            n = min(RUN, W - x0)
            seen.add("dword" if n == RUN and (byte_offset + (y * W + x0) * 3) % 4 == 0 else "byte")
            for c in range(3):
                seen.add("vec" if n == RUN and (elem_offset + c * H * W + y * W + x0) % 4 == 0 else "scalar")
    gh, gw = grid(H, W)
    for cy in range(gh):
        for cx in range(gw):
            seen.add("full" if min(CELL, H - cy * CELL) == CELL and min(CELL, W - cx * CELL) == CELL else "partial")
    return seen


def map_paths(dmap):
    """what a map puts next to what: "0|32" where a lossless cell and one at the largest bound are neighbours in a row
    or a column, "uniform" for a map of one value, "over" where a byte is above 32"""
    m = np.asarray(dmap).astype(np.int64)
    seen = set()
    pairs = list(zip(m[:, :-1].reshape(-1), m[:, 1:].reshape(-1))) + list(zip(m[:-1].reshape(-1), m[1:].reshape(-1)))
    if any({int(a), int(b)} == {0, 32} for a, b in pairs):
        seen.add("0|32")
    if (m == m.flat[0]).all():
        seen.add("uniform")
    if (m > MAX_ERROR).any():
        seen.add("over")
    return seen


def window_paths(H, W, window, dmap):
    """what the apply kernel's runs of four window pixels do with the map: "one-cell" for a run inside one cell,
    "straddle" for a run that crosses a cell boundary of the image, "straddle-differ" where the two cells' bounds
    differ, "straddle-0|32" where they are 0 and 32, "partial-run" for a run cut by the window's right edge,
    "partial-straddle" for such a run that still crosses a boundary, "row-boundary" where the window's rows cross a
    boundary between cells of different bounds"""
    d = per_pixel(dmap, H, W)
    y0, x0, h, w = window
    seen = set()
    for y in range(h):
        for x in range(0, w, RUN):
            n = min(RUN, w - x)
            px = [x0 + x + j for j in range(n)]
            cells = {p // CELL for p in px}
            if n < RUN:
                seen.add("partial-run")
            if len(cells) == 1:
                seen.add("one-cell")
                continue
            seen.add("straddle")
            if n < RUN:
                seen.add("partial-straddle")
            b = {int(d[y0 + y, p]) for p in px}
            if len(b) == 2:
                seen.add("straddle-differ")
            if b == {0, 32}:
                seen.add("straddle-0|32")
    for y in range(h - 1):
        if (y0 + y) // CELL != (y0 + y + 1) // CELL and (d[y0 + y, x0:x0 + w] != d[y0 + y + 1, x0:x0 + w]).any():
            seen.add("row-boundary")
    return seen


def kernel_cases():
    """every case of the GPU kernel test of the two map entries: dicts with name, x, xhat (8-bit [H, W, 3]), dmap
    (uint8 [gh, gw]), byte_offset / elem_offset of the buffers, ``paths``: what of ``run_paths`` the case is there for,
    and ``map_paths``: what of ``map_paths``"""
    full = {(1, 1): {"byte", "scalar", "partial"}, (16, 16): {"dword", "vec", "full"},
            (17, 33): {"dword", "byte", "vec", "scalar", "full", "partial"},
            (37, 53): {"dword", "byte", "vec", "scalar", "full", "partial"}, (64, 48): {"dword", "vec", "full"}}
    cases = []
    for k, (H, W) in enumerate(SHAPES):
        x, xhat = random_pair(H, W, 200 + k)
        cases.append(dict(name=f"random-{H}x{W}", x=x, xhat=xhat, dmap=random_map(H, W, k), byte_offset=0, elem_offset=0,
                          paths=full[(H, W)], map_paths={"0|32"} if max(H, W) > CELL else set()))
        for reverse in (False, True):
            x, xhat = extreme_pair(H, W, reverse)
            cases.append(dict(name=f"extreme{'-rev' if reverse else ''}-{H}x{W}", x=x, xhat=xhat,
                              dmap=random_map(H, W, 10 + k), byte_offset=0, elem_offset=0, paths=set(),
                              map_paths={"0|32"} if max(H, W) > CELL else set()))
    # buffers off their natural 16-byte boundary: the full runs of the aligned shapes take the slow paths
    x, xhat = random_pair(64, 48, 7)
    cases.append(dict(name="random-64x48-odd-pointers", x=x, xhat=xhat, dmap=random_map(64, 48, 20), byte_offset=1,
                      elem_offset=1, paths={"byte", "scalar", "full"}, map_paths={"0|32"}))
    x, xhat = random_pair(16, 16, 8)
    cases.append(dict(name="random-16x16-odd-pointers", x=x, xhat=xhat, dmap=np.full((1, 1), 3, np.uint8),
                      byte_offset=3, elem_offset=3, paths={"byte", "scalar", "full"}, map_paths={"uniform"}))
    return cases


WINDOW_SHAPES = [(37, 53), (64, 48)]
WINDOW_X0 = [13, 14, 15, 16, 17]
WINDOW_Y0 = [0, 15, 16]


def window_map(H, W):
    """columns of cells alternate 0, 32, 0, ... in the first row of cells and 32, 0, 32, ... in the next, and so on: the
    boundaries at x = 16 and x = 32 and at y = 16 all separate the two extremes"""
    gh, gw = grid(H, W)
    cy, cx = np.mgrid[0:gh, 0:gw]
    return np.where((cy + cx) % 2 == 0, 0, 32).astype(np.uint8)


def window_cases():
    """the windows of ``icm_residual_apply_map``: on both shapes every x0 in 13..17 with every y0 in {0, 15, 16}, wide
    enough to reach past x = 32 and of a width that is no multiple of four, under ``window_map``; and a window of one
    pixel.  dicts with name, shape, window, dmap, off (the buffers' odd offset), ``paths`` of ``window_paths``"""
    cases = []
    for H, W in WINDOW_SHAPES:
        dmap = window_map(H, W)
        for y0 in WINDOW_Y0:
            for x0 in WINDOW_X0:
                h, w = min(19, H - y0), min(22, W - x0)
                paths = {"one-cell", "partial-run"}
                if x0 % RUN:                             # runs from a multiple of four never cross: 16 and 32 are such
                    paths = paths | {"straddle", "straddle-differ", "straddle-0|32"}
                if y0 + h > 16 and y0 < 16:
                    paths = paths | {"row-boundary"}
                cases.append(dict(name=f"{H}x{W}-y{y0}-x{x0}", shape=(H, W), window=(y0, x0, h, w), dmap=dmap,
                                  off=(x0 + y0) % 4, paths=paths))
    cases.append(dict(name="37x53-one-pixel", shape=(37, 53), window=(16, 31, 1, 1), dmap=window_map(37, 53), off=0,
                      paths={"partial-run", "one-cell"}))
    # a run cut by the window's edge that still crosses the boundary at x = 16: pixels 14, 15, 16
    cases.append(dict(name="37x53-cut-run-crosses", shape=(37, 53), window=(3, 14, 5, 3), dmap=window_map(37, 53), off=1,
                      paths={"partial-run", "partial-straddle", "straddle-0|32"}))
    return cases
