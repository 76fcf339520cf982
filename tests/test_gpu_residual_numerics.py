"""GPU: the three kernels of the residual layer (csrc/residual.hip) through the C ABI, bit for bit against the numpy
restatement of tests/_residual_ref.py.  The cases and the paths they are there for come from ``_residual_ref.kernel_cases``
(tests/test_residual_ref.py checks on the CPU that each reaches its path): every shape x bound on random byte pairs,
x = 255 against xhat = 0 and the reverse, buffers off their natural alignment, and cells that sit on every class
threshold the bound can reach -- 16 S = N T_j exactly, the next sum above it, and, where a partial cell allows it (odd
T_j: 16 S is a multiple of 16), 16 S = N T_j + 1 exactly.  Outputs are pre-filled with a sentinel and carry guard
elements on both sides."""
import numpy as np
import pytest
import torch

import _residual_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = 1
SENT32, SENT8, GUARD = 0x5A5A5A5A, 0xA5, 8
CASES = RR.kernel_cases()


def _lib():
    from icm_amd import _lib as L
    return L.lib(), L.stream()


class Buf:
    """``n`` elements of a device buffer that begin ``offset`` elements past a 16-byte boundary, with guards around
    them, everything pre-filled with the sentinel (or with ``data``)"""

    def __init__(self, n, dtype, offset=0, data=None):
        sent = SENT32 if dtype == torch.int32 else SENT8
        self.whole = torch.full((16 + offset + n + GUARD,), sent, dtype=dtype, device=DEV)
        assert self.whole.data_ptr() % 16 == 0
        self.lo, self.n, self.sent = 16 + offset, n, sent
        if data is not None:
            self.whole[self.lo:self.lo + n] = torch.from_numpy(np.ascontiguousarray(data).reshape(-1)).to(DEV)
        self.ptr = self.whole.data_ptr() + self.lo * self.whole.element_size()

    def get(self, shape):
        w = self.whole.cpu().numpy()
        assert (w[:self.lo] == self.sent).all() and (w[self.lo + self.n:] == self.sent).all(), "a guard was written"
        return w[self.lo:self.lo + self.n].reshape(shape)


def _code(c):
    lib, st = _lib()
    H, W = c["x"].shape[:2]
    gh, gw = RR.grid(H, W)
    x = Buf(H * W * 3, torch.uint8, c["byte_offset"], c["x"])
    xhat = Buf(H * W * 3, torch.uint8, c["byte_offset"], c["xhat"])
    sym, idx = (Buf(3 * H * W, torch.int32, c["elem_offset"]) for _ in range(2))
    cls = Buf(gh * gw, torch.int32)
    assert lib.icm_residual_code(x.ptr, xhat.ptr, H, W, c["d"], sym.ptr, idx.ptr, cls.ptr, st) == 0
    torch.cuda.synchronize()
    return sym, idx, cls, xhat


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_code_indexes_and_apply_match_the_restatement(c):
    lib, st = _lib()
    H, W = c["x"].shape[:2]
    d = c["d"]
    q = RR.quantise(c["x"], c["xhat"], d)
    want_cls = RR.classes(q)
    sym, idx, cls, xhat = _code(c)
    got_cls = cls.get(want_cls.shape)
    assert np.array_equal(got_cls, want_cls), (got_cls, want_cls)
    got_sym = sym.get((3, H, W))
    assert np.array_equal(got_sym, q)                    # every element written: none is the sentinel, no |q| reaches it
    assert np.array_equal(idx.get((3, H, W)), RR.indexes(want_cls, H, W))
    # the decoder's expansion of the same classes
    idx2 = Buf(3 * H * W, torch.int32, c["elem_offset"])
    assert lib.icm_residual_indexes(cls.ptr, H, W, idx2.ptr, st) == 0
    assert np.array_equal(idx2.get((3, H, W)), RR.indexes(want_cls, H, W))
    # the reconstruction of the full image, and the bound
    out = Buf(H * W * 3, torch.uint8, c["byte_offset"])
    assert lib.icm_residual_apply(xhat.ptr, sym.ptr, H, W, 0, 0, H, W, d, out.ptr, st) == 0
    got = out.get((H, W, 3))
    assert np.array_equal(got, RR.reconstruct(c["xhat"], q, d))
    err = int(np.abs(got.astype(np.int64) - c["x"].astype(np.int64)).max())
    assert err <= d and (d != 0 or np.array_equal(got, c["x"]))


@pytest.mark.parametrize("d", RR.BOUNDS)
def test_cells_on_a_threshold_get_the_class_of_their_side(d):
    x, xhat, want = RR.threshold_image(d)
    c = dict(x=x, xhat=xhat, d=d, byte_offset=0, elem_offset=0)
    got = _code(c)[2].get(RR.grid(*x.shape[:2]))
    for cy, cx, j, k in want:
        assert got[cy, cx] == k, (j, k, got[cy, cx])
    for j, sx, sxhat in RR.odd_threshold_strips(d):
        got = _code(dict(x=sx, xhat=sxhat, d=d, byte_offset=0, elem_offset=0))[2].get((1, 1))
        assert got[0, 0] == j + 1, j


WINDOWS = [((37, 53), (3, 5, 21, 31), 0), ((37, 53), (36, 52, 1, 1), 0), ((64, 48), (16, 4, 32, 40), 0),
           ((64, 48), (1, 3, 63, 45), 1), ((17, 33), (0, 0, 17, 33), 3)]


@pytest.mark.parametrize("shape,window,off", WINDOWS, ids=[f"{s[0]}x{s[1]}-{'_'.join(map(str, w))}-off{o}"
                                                           for s, w, o in WINDOWS])
@pytest.mark.parametrize("d", [0, 3, 32])
def test_apply_on_a_window(shape, window, off, d):
    lib, st = _lib()
    H, W = shape
    y0, x0, h, w = window
    x, xhat = RR.random_pair(H, W, 31 + d)
    q = RR.quantise(x, xhat, d)
    q[:, y0, x0] = [2 ** 31 - 1, -2 ** 31, 300]          # symbols no valid stream holds: saturate, do not overflow
    crop = np.ascontiguousarray(xhat[y0:y0 + h, x0:x0 + w])
    xb = Buf(h * w * 3, torch.uint8, off, crop)
    sb = Buf(3 * H * W, torch.int32, off, q)
    out = Buf(h * w * 3, torch.uint8, off)
    assert lib.icm_residual_apply(xb.ptr, sb.ptr, H, W, y0, x0, h, w, d, out.ptr, st) == 0
    torch.cuda.synchronize()
    want = RR.reconstruct(crop, q, d, window)
    assert np.array_equal(out.get((h, w, 3)), want)
    assert tuple(want[0, 0]) == (255, 0, 255)
    # a window of the full reconstruction is the reconstruction of the window
    full = RR.reconstruct(xhat, q, d)
    assert np.array_equal(want, full[y0:y0 + h, x0:x0 + w])


def test_indexes_pass_a_class_outside_the_tables_through():
    lib, st = _lib()
    H, W = 37, 53
    gh, gw = RR.grid(H, W)
    cls = np.arange(gh * gw, dtype=np.int32).reshape(gh, gw) % RR.NCLASSES
    cls[0, 1], cls[2, 3], cls[1, 0] = 19, -7, 2 ** 31 - 1
    cb = Buf(gh * gw, torch.int32, 1, cls)
    idx = Buf(3 * H * W, torch.int32)
    assert lib.icm_residual_indexes(cb.ptr, H, W, idx.ptr, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(idx.get((3, H, W)), RR.indexes(cls, H, W))


def test_argument_errors_come_back_before_any_launch():
    lib, st = _lib()
    H, W = 16, 16
    u8 = Buf(H * W * 3, torch.uint8, 0, np.zeros((H, W, 3), np.uint8))
    i32 = [Buf(3 * H * W, torch.int32) for _ in range(3)]
    good = [u8.ptr, u8.ptr, H, W, 1, i32[0].ptr, i32[1].ptr, i32[2].ptr]
    assert lib.icm_residual_code(*good, st) == 0
    for pos, bad in [(0, 0), (1, 0), (5, 0), (6, 0), (7, 0), (2, 0), (2, -1), (2, 32769), (3, 0), (3, 32769), (4, -1),
                     (4, 33)]:
        a = list(good)
        a[pos] = bad
        assert lib.icm_residual_code(*a, st) == ERR_ARG, (pos, bad)
    good = [i32[2].ptr, H, W, i32[1].ptr]
    assert lib.icm_residual_indexes(*good, st) == 0
    for pos, bad in [(0, 0), (3, 0), (1, 0), (1, 32769), (2, 0), (2, -5), (2, 32769)]:
        a = list(good)
        a[pos] = bad
        assert lib.icm_residual_indexes(*a, st) == ERR_ARG, (pos, bad)
    out = Buf(H * W * 3, torch.uint8)
    good = [u8.ptr, i32[0].ptr, H, W, 0, 0, H, W, 1, out.ptr]
    assert lib.icm_residual_apply(*good, st) == 0
    for pos, bad in [(0, 0), (1, 0), (9, 0), (2, 0), (2, 32769), (3, 0), (3, 32769), (4, -1), (5, -1), (4, 1), (5, 1),
                     (6, 0), (7, 0), (6, 17), (7, 17), (6, 32769), (8, -1), (8, 33)]:
        a = list(good)
        a[pos] = bad
        assert lib.icm_residual_apply(*a, st) == ERR_ARG, (pos, bad)
    # the largest sides pass the check (a one-row image: nothing large is allocated)
    n = 32768
    row = Buf(n * 3, torch.uint8, 0, np.zeros(n * 3, np.uint8))
    big = [Buf(3 * n, torch.int32) for _ in range(2)]
    cl = Buf(n // 16, torch.int32)
    assert lib.icm_residual_code(row.ptr, row.ptr, 1, n, 32, big[0].ptr, big[1].ptr, cl.ptr, st) == 0
    assert lib.icm_residual_code(row.ptr, row.ptr, n, 1, 32, big[0].ptr, big[1].ptr, Buf(n // 16, torch.int32).ptr, st) == 0
    torch.cuda.synchronize()
    assert (big[0].get((3 * n,)) == 0).all() and (cl.get((n // 16,)) == 0).all()
