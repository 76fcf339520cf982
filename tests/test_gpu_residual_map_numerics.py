"""GPU: the two map kernels of the residual layer (csrc/residual.hip, ``icm_residual_code_map`` /
``icm_residual_apply_map``) through the C ABI, bit for bit against the numpy restatement of tests/_residual_map_ref.py.
The cases and the paths they are there for come from ``_residual_map_ref.kernel_cases`` / ``window_cases``
(tests/test_residual_map_ref.py checks on the CPU that each reaches its path): every shape on random byte pairs under
random maps that hold 0 and 32 side by side, x = 255 against xhat = 0 and the reverse, buffers off their natural
alignment, a uniform map against the scalar entries, windows whose runs of four straddle the cell boundaries at x = 16
and x = 32 under differing bounds, a one-pixel window, a map byte above 32, and the argument errors.  Outputs are
pre-filled with a sentinel and carry guard elements on both sides."""
import numpy as np
import pytest
import torch

import _residual_map_ref as MR
import _residual_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = 1
SENT32, SENT8, GUARD = 0x5A5A5A5A, 0xA5, 8
CASES = MR.kernel_cases()
WINDOWS = MR.window_cases()


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

    def untouched(self):
        return bool((self.whole.cpu().numpy() == self.sent).all())


def _code_map(x, xhat, dmap, byte_offset=0, elem_offset=0):
    lib, st = _lib()
    H, W = x.shape[:2]
    gh, gw = MR.grid(H, W)
    xb = Buf(H * W * 3, torch.uint8, byte_offset, x)
    eb = Buf(H * W * 3, torch.uint8, byte_offset, xhat)
    mb = Buf(gh * gw, torch.uint8, byte_offset, dmap)
    sym, idx = (Buf(3 * H * W, torch.int32, elem_offset) for _ in range(2))
    cls = Buf(gh * gw, torch.int32)
    assert lib.icm_residual_code_map(xb.ptr, eb.ptr, H, W, mb.ptr, sym.ptr, idx.ptr, cls.ptr, st) == 0
    torch.cuda.synchronize()
    return sym, idx, cls, eb, mb


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_code_map_and_apply_map_match_the_restatement(c):
    lib, st = _lib()
    H, W = c["x"].shape[:2]
    dmap = c["dmap"]
    q = MR.quantise_map(c["x"], c["xhat"], dmap)
    want_cls = RR.classes(q)                             # the class rule is unchanged: a cell's class from its own q
    sym, idx, cls, xhat, mb = _code_map(c["x"], c["xhat"], dmap, c["byte_offset"], c["elem_offset"])
    assert np.array_equal(cls.get(want_cls.shape), want_cls)
    assert np.array_equal(sym.get((3, H, W)), q)         # every element written: none is the sentinel
    assert np.array_equal(idx.get((3, H, W)), RR.indexes(want_cls, H, W))
    out = Buf(H * W * 3, torch.uint8, c["byte_offset"])
    assert lib.icm_residual_apply_map(xhat.ptr, sym.ptr, H, W, 0, 0, H, W, mb.ptr, out.ptr, st) == 0
    torch.cuda.synchronize()
    got = out.get((H, W, 3))
    assert np.array_equal(got, MR.reconstruct_map(c["xhat"], q, dmap))
    # the bound, on every sample, under its own cell's D; the lossless cells bit for bit
    err = np.abs(got.astype(np.int64) - c["x"].astype(np.int64))
    bound = MR.per_pixel(dmap, H, W)[..., None]
    assert (err <= bound).all()
    zero = np.broadcast_to(bound == 0, err.shape)
    assert np.array_equal(got[zero], c["x"][zero])


@pytest.mark.parametrize("shape", MR.SHAPES, ids=[f"{h}x{w}" for h, w in MR.SHAPES])
@pytest.mark.parametrize("d", [0, 3, 32])
def test_a_uniform_map_gives_the_scalar_entries_outputs(shape, d):
    lib, st = _lib()
    H, W = shape
    gh, gw = MR.grid(H, W)
    x, xhat = MR.random_pair(H, W, 50 + d)
    sym, idx, cls, eb, mb = _code_map(x, xhat, np.full((gh, gw), d, np.uint8))
    xb = Buf(H * W * 3, torch.uint8, 0, x)
    sym2, idx2 = (Buf(3 * H * W, torch.int32) for _ in range(2))
    cls2 = Buf(gh * gw, torch.int32)
    assert lib.icm_residual_code(xb.ptr, eb.ptr, H, W, d, sym2.ptr, idx2.ptr, cls2.ptr, st) == 0
    out, out2 = (Buf(H * W * 3, torch.uint8) for _ in range(2))
    assert lib.icm_residual_apply_map(eb.ptr, sym.ptr, H, W, 0, 0, H, W, mb.ptr, out.ptr, st) == 0
    assert lib.icm_residual_apply(eb.ptr, sym2.ptr, H, W, 0, 0, H, W, d, out2.ptr, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(sym.get((3, H, W)), sym2.get((3, H, W)))
    assert np.array_equal(idx.get((3, H, W)), idx2.get((3, H, W)))
    assert np.array_equal(cls.get((gh, gw)), cls2.get((gh, gw)))
    assert np.array_equal(out.get((H, W, 3)), out2.get((H, W, 3)))
    assert np.array_equal(sym2.get((3, H, W)), RR.quantise(x, xhat, d))


@pytest.mark.parametrize("c", WINDOWS, ids=[c["name"] for c in WINDOWS])
def test_apply_map_on_a_window(c):
    lib, st = _lib()
    H, W = c["shape"]
    y0, x0, h, w = c["window"]
    dmap, off = c["dmap"], c["off"]
    x, xhat = MR.random_pair(H, W, 77)
    q = MR.quantise_map(x, xhat, dmap)
    crop = np.ascontiguousarray(xhat[y0:y0 + h, x0:x0 + w])
    xb = Buf(h * w * 3, torch.uint8, off, crop)
    sb = Buf(3 * H * W, torch.int32, off, q)
    mb = Buf(dmap.size, torch.uint8, off, dmap)
    out = Buf(h * w * 3, torch.uint8, off)
    assert lib.icm_residual_apply_map(xb.ptr, sb.ptr, H, W, y0, x0, h, w, mb.ptr, out.ptr, st) == 0
    torch.cuda.synchronize()
    got = out.get((h, w, 3))
    want = MR.reconstruct_map(crop, q, dmap, c["window"])
    assert np.array_equal(got, want)
    # a window of the full reconstruction is the reconstruction of the window, and the bound holds per cell
    full = MR.reconstruct_map(xhat, q, dmap)
    assert np.array_equal(want, full[y0:y0 + h, x0:x0 + w])
    err = np.abs(got.astype(np.int64) - x[y0:y0 + h, x0:x0 + w].astype(np.int64))
    assert (err <= MR.per_pixel(dmap, H, W, c["window"])[..., None]).all()
    # the map matters here: one bound for the whole run, the first pixel's or the last one's, gives another window
    if "straddle-differ" in c["paths"]:
        for wrong in (0, 32):
            assert not np.array_equal(want, RR.reconstruct(crop, q, wrong, c["window"]))


def test_a_map_byte_above_32_behaves_as_32():
    lib, st = _lib()
    H, W = 37, 53
    x, xhat = MR.random_pair(H, W, 9)
    dmap = MR.random_map(H, W, 3)
    over = dmap.copy()
    over[dmap == 32] = 200
    over[2, 3] = 255
    dmap[2, 3] = 32
    assert (over > 32).sum() >= 3 and "over" in MR.map_paths(over)
    sym, idx, cls, eb, mb = _code_map(x, xhat, over)
    q = MR.quantise_map(x, xhat, dmap)
    assert np.array_equal(sym.get((3, H, W)), q) and np.array_equal(cls.get(MR.grid(H, W)), RR.classes(q))
    for win in ((0, 0, H, W), (15, 13, 20, 30)):
        y0, x0, h, w = win
        crop = np.ascontiguousarray(xhat[y0:y0 + h, x0:x0 + w])
        xb = Buf(h * w * 3, torch.uint8, 0, crop)
        out = Buf(h * w * 3, torch.uint8)
        assert lib.icm_residual_apply_map(xb.ptr, sym.ptr, H, W, y0, x0, h, w, mb.ptr, out.ptr, st) == 0
        torch.cuda.synchronize()
        assert np.array_equal(out.get((h, w, 3)), MR.reconstruct_map(crop, q, dmap, win))


def test_apply_map_saturates_like_the_exact_integers():
    """symbols no valid stream holds, next to a cell boundary"""
    lib, st = _lib()
    H, W = 37, 53
    dmap = MR.window_map(H, W)
    x, xhat = MR.random_pair(H, W, 5)
    q = MR.quantise_map(x, xhat, dmap)
    q[:, 16, 15] = [2 ** 31 - 1, -2 ** 31, 300]
    q[:, 16, 16] = [-2 ** 31, 2 ** 31 - 1, -300]
    win = (16, 14, 2, 7)
    crop = np.ascontiguousarray(xhat[16:18, 14:21])
    xb, sb = Buf(crop.size, torch.uint8, 0, crop), Buf(q.size, torch.int32, 0, q)
    mb, out = Buf(dmap.size, torch.uint8, 0, dmap), Buf(crop.size, torch.uint8)
    assert lib.icm_residual_apply_map(xb.ptr, sb.ptr, H, W, *win, mb.ptr, out.ptr, st) == 0
    torch.cuda.synchronize()
    got = out.get(crop.shape)
    assert np.array_equal(got, MR.reconstruct_map(crop, q, dmap, win))
    assert tuple(got[0, 1]) == (255, 0, 255) and tuple(got[0, 2]) == (0, 255, 0)


def test_argument_errors_come_back_before_any_launch():
    lib, st = _lib()
    H, W = 16, 16
    u8 = Buf(H * W * 3, torch.uint8, 0, np.zeros((H, W, 3), np.uint8))
    dm = Buf(1, torch.uint8, 0, np.zeros(1, np.uint8))
    i32 = [Buf(3 * H * W, torch.int32) for _ in range(3)]
    good = [u8.ptr, u8.ptr, H, W, dm.ptr, i32[0].ptr, i32[1].ptr, i32[2].ptr]
    for pos, bad in [(0, 0), (1, 0), (4, 0), (5, 0), (6, 0), (7, 0), (2, 0), (2, -1), (2, 32769), (3, 0), (3, 32769)]:
        a = list(good)
        a[pos] = bad
        assert lib.icm_residual_code_map(*a, st) == ERR_ARG, (pos, bad)
    torch.cuda.synchronize()
    assert all(b.untouched() for b in i32)               # nothing was launched: guards and body hold the sentinel
    assert lib.icm_residual_code_map(*good, st) == 0
    torch.cuda.synchronize()
    assert (i32[0].get((3 * H * W,)) == 0).all()
    out = Buf(H * W * 3, torch.uint8)
    good = [u8.ptr, i32[0].ptr, H, W, 0, 0, H, W, dm.ptr, out.ptr]
    for pos, bad in [(0, 0), (1, 0), (8, 0), (9, 0), (2, 0), (2, 32769), (3, 0), (3, 32769), (4, -1), (5, -1), (4, 1),
                     (5, 1), (6, 0), (7, 0), (6, 17), (7, 17), (6, 32769), (7, -3)]:
        a = list(good)
        a[pos] = bad
        assert lib.icm_residual_apply_map(*a, st) == ERR_ARG, (pos, bad)
    torch.cuda.synchronize()
    assert out.untouched()
    assert lib.icm_residual_apply_map(*good, st) == 0
    torch.cuda.synchronize()
    assert (out.get((H * W * 3,)) == 0).all()
    # the largest sides pass the check (a one-row image: nothing large is allocated)
    n = 32768
    row = Buf(n * 3, torch.uint8, 0, np.zeros(n * 3, np.uint8))
    big = [Buf(3 * n, torch.int32) for _ in range(2)]
    cl = Buf(n // 16, torch.int32)
    dmr = Buf(n // 16, torch.uint8, 0, np.full(n // 16, 32, np.uint8))
    assert lib.icm_residual_code_map(row.ptr, row.ptr, 1, n, dmr.ptr, big[0].ptr, big[1].ptr, cl.ptr, st) == 0
    assert lib.icm_residual_code_map(row.ptr, row.ptr, n, 1, dmr.ptr, big[0].ptr, big[1].ptr,
                                     Buf(n // 16, torch.int32).ptr, st) == 0
    torch.cuda.synchronize()
    assert (big[0].get((3 * n,)) == 0).all() and (cl.get((n // 16,)) == 0).all()


def test_the_python_wrappers_take_an_int_or_a_host_map():
    from icm_amd import residual as R
    H, W = 37, 53
    x, xhat = MR.random_pair(H, W, 11)
    dmap = MR.random_map(H, W, 4)
    xd, ed = torch.from_numpy(x).to(DEV), torch.from_numpy(xhat).to(DEV)
    sym, idx, cls = R.residual_code(xd, ed, dmap)
    q = MR.quantise_map(x, xhat, dmap)
    assert np.array_equal(sym.cpu().numpy(), q) and np.array_equal(cls.cpu().numpy(), RR.classes(q))
    win = (15, 13, 20, 30)
    out = R.residual_apply(ed[15:35, 13:43].contiguous(), sym, win, dmap)
    assert np.array_equal(out.cpu().numpy(), MR.reconstruct_map(xhat[15:35, 13:43], q, dmap, win))
    sym3 = R.residual_code(xd, ed, 3)[0]
    assert np.array_equal(sym3.cpu().numpy(), RR.quantise(x, xhat, 3))
    for bad in (dmap.astype(np.int64), dmap[:-1], np.full_like(dmap, 33), torch.from_numpy(dmap).to(DEV)):
        with pytest.raises(ValueError):
            R.residual_code(xd, ed, bad)
        with pytest.raises(ValueError):
            R.residual_apply(ed, sym, (0, 0, H, W), bad)
