"""Host restatement of the tile assembly of a tiled image (``icm_image_tile_blend``, include/icm_hip.h), in numpy.

    canvas[c][y0 + y][x0 + x] = canvas[c][y0 + y][x0 + x] + (wy(y) * wx(x)) * src[c][top + y][left + x]

Every numpy elementwise operation on float32 arrays is one IEEE operation rounded once (no fused multiply-add), and the
three operations are made in the association above, so the result is the kernel's bit for bit.  Written from the
formula, not from the kernel: it shares no code with icm_amd."""
import numpy as np

EDGE_LEFT, EDGE_RIGHT, EDGE_TOP, EDGE_BOTTOM = 1, 2, 4, 8     # ICM_TILE_EDGE_*


def ramp(m, dtype=np.float32):
    """(i + 0.5) / m, i < m, in ``dtype``"""
    return (np.arange(m, dtype=dtype) + dtype(0.5)) / dtype(m) if m else np.zeros(0, dtype)


def weights(n, m, near, far, dtype=np.float32):
    """the n weights along one axis of a window: ramp[i] within m of a side that has a neighbour (the near side decides
    where both bands reach), 1 elsewhere"""
    r = ramp(m, dtype)
    w = np.ones(n, dtype)
    for i in range(n):
        if near and i < m:
            w[i] = r[i]
        elif far and n - 1 - i < m:
            w[i] = r[n - 1 - i]
    return w


def blend(canvas, src, top, left, h, w, y0, x0, m, edges):
    """a copy of ``canvas`` [3, H, W] with the h x w window of ``src`` [3, PH, PW] at (top, left) added at (y0, x0)"""
    assert canvas.dtype == np.float32 and src.dtype == np.float32
    wy = weights(h, m, edges & EDGE_TOP, edges & EDGE_BOTTOM)
    wx = weights(w, m, edges & EDGE_LEFT, edges & EDGE_RIGHT)
    k = wy[:, None] * wx[None, :]                                   # rounded once
    t = k[None] * src[:, top:top + h, left:left + w]                # rounded once
    out = canvas.copy()
    out[:, y0:y0 + h, x0:x0 + w] = out[:, y0:y0 + h, x0:x0 + w] + t  # rounded once
    assert k.dtype == t.dtype == out.dtype == np.float32
    return out


def edges_of(r, c, rows, cols):
    return ((EDGE_LEFT if c > 0 else 0) | (EDGE_RIGHT if c < cols - 1 else 0) |
            (EDGE_TOP if r > 0 else 0) | (EDGE_BOTTOM if r < rows - 1 else 0))


def assemble(tiles, plan, rows, cols, H, W, m):
    """zero canvas [3, H, W] + every tile [3, h, w] of the row-major ``plan`` in order"""
    canvas = np.zeros((3, H, W), np.float32)
    for k, ((y0, x0, h, w), t) in enumerate(zip(plan, tiles)):
        assert t.shape == (3, h, w)
        canvas = blend(canvas, t, 0, 0, h, w, y0, x0, m, edges_of(k // cols, k % cols, rows, cols))
    return canvas


def quantise(canvas):
    """planar f32 [3, H, W] -> interleaved 8-bit [H, W, 3]: clamp to [0, 1], one f32 product by 255, truncation"""
    q = np.minimum(np.maximum(canvas, np.float32(0)), np.float32(1)) * np.float32(255)
    return np.ascontiguousarray(q.astype(np.uint8).transpose(1, 2, 0))
