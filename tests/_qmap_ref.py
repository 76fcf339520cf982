"""The quality map (a quantiser step per latent position) restated in numpy, independently of the package: the
kernels' arithmetic with step and inverse arrays broadcast over [N, C, HW] (the operations are those of
tests/_qstep_ref.py, which numpy applies elementwise with one rounding each), the 256-entry (step, inv) table the
kernels index with a map byte, the run-length string a map travels in, and the map of a list of rectangles."""
import struct

import numpy as np

import _qstep_ref as Q

F = np.float32
QSTEP_MIN, QSTEP_MAX = Q.QSTEP_MIN, Q.QSTEP_MAX
CELL = 16
RUN_MAX = 65535


def step_table():
    """float32 [256, 2]: row b = step_of(k) for the byte b of k as a signed byte, (1, 1) for every other byte"""
    t = np.ones((256, 2), dtype=F)
    for k in range(QSTEP_MIN, QSTEP_MAX + 1):
        t[np.array(k, dtype=np.int8).view(np.uint8)] = Q.step_of(k)
    return t


def steps_of_map(qmap):
    """(step, inv) float32 arrays of the flat map's shape, through the table as the kernels read it"""
    t = step_table()
    b = np.ascontiguousarray(qmap, dtype=np.int8).reshape(-1).view(np.uint8)
    return t[b, 0], t[b, 1]


def _bc(a, like):
    """a per-position array [HW] broadcast over [N, C, HW]"""
    return np.broadcast_to(np.asarray(a, dtype=F), np.asarray(like).shape)


def symbols(y, mu, inv):
    return Q.symbols(y, mu, _bc(inv, y))


def dequantize(sym, mu, step):
    return Q.dequantize(sym, mu, _bc(step, mu))


def indexes(scale, table, bound, inv):
    return Q.indexes(scale, table, bound, _bc(inv, scale))


def code(y, mu, scale, table, bound, qmap):
    """the encoder's fused kernel with a map over HW: (symbols, indexes, y_hat)"""
    step, inv = steps_of_map(qmap)
    sym = symbols(y, mu, inv)
    return sym, indexes(scale, table, bound, inv), dequantize(sym, mu, step)


# ------------------------------------------------------------------------------------------------ the map's string
def write_map(qmap):
    """u16 h, u16 w, then maximal runs (u16 count, i8 k) in row-major order, a run longer than 65535 as full counts
    followed by the rest"""
    a = np.asarray(qmap)
    h, w = a.shape
    out = [struct.pack("<HH", h, w)]
    flat = [int(v) for v in a.reshape(-1)]
    i = 0
    while i < len(flat):
        j = i
        while j < len(flat) and flat[j] == flat[i]:
            j += 1
        n = j - i
        while n:
            c = min(n, RUN_MAX)
            out.append(struct.pack("<Hb", c, flat[i]))
            n -= c
        i = j
    return b"".join(out)


def read_map(data):
    """the map of a well-formed string (no checks: the package's reader is what the tests check)"""
    h, w = struct.unpack_from("<HH", data, 0)
    flat = []
    for off in range(4, len(data), 3):
        c, k = struct.unpack_from("<Hb", data, off)
        flat += [k] * c
    return np.array(flat, dtype=np.int8).reshape(h, w)


# ------------------------------------------------------------------------------------------------ rectangles
def center_pads(h, w, p=64):
    nh, nw = -(-h // p) * p, -(-w // p) * p
    left, top = (nw - w) // 2, (nh - h) // 2
    return left, nw - w - left, top, nh - h - top


def roi_map(H, W, pads, base, rois):
    """per pixel, not per rectangle edge: every pixel of every rectangle, in list order, sets the cell it lies in"""
    left, right, top, bottom = pads
    m = np.full(((top + H + bottom) // CELL, (left + W + right) // CELL), base, dtype=np.int64)
    for y0, x0, h, w, d in rois:
        assert 0 <= y0 and 0 <= x0 and h >= 1 and w >= 1 and y0 + h <= H and x0 + w <= W
        k = max(QSTEP_MIN, min(QSTEP_MAX, base + d))
        for y in range(y0, y0 + h):
            for x in range(x0, x0 + w):
                m[(top + y) // CELL, (left + x) // CELL] = k
    return m.astype(np.int8)
