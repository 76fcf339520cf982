"""GPU: the band forms of the residual decoder's kernels (csrc/residual.hip ``icm_residual_indexes_band`` /
``icm_residual_apply_band`` / ``icm_residual_apply_map_band``) through the C ABI, bit for bit against the numpy rules of
tests/_residual_ref.py and tests/_residual_map_ref.py: buffers that hold the elements [e_lo, e_hi) of every plane, a
band that starts and ends in the middle of a row, windows on the band's first and last row, widths that are no multiple
of four, buffers off their 16-byte alignment, and -- for the map form -- runs of four pixels across a cell boundary
whose two cells have different bounds.  Outputs are pre-filled with a sentinel and carry guards."""
import numpy as np
import pytest
import torch

import _residual_map_ref as MR
import _residual_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = 1
SENT32, SENT8, GUARD = 0x5A5A5A5A, 0xA5, 8


def _lib():
    from icm_amd import _lib as L
    return L.lib(), L.stream()


class Buf:
    """``n`` elements of a device buffer that begin ``offset`` elements past a 16-byte boundary, guards around them,
    pre-filled with the sentinel (or with ``data``)"""

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


# (H, W), (e_lo, e_hi): bands as a region decode makes them (multiples of 64, the last one cut by the plane's end) and
# bands that begin and end anywhere; every one starts or ends inside a row
BANDS = [((40, 50), (384, 1152)), ((40, 50), (1920, 2000)), ((40, 50), (0, 128)), ((40, 50), (70, 90)),
         ((37, 67), (640, 1920)), ((37, 67), (641, 1919)), ((37, 67), (2432, 2479)), ((37, 67), (0, 2479))]


def _rowcol(e, W):
    return divmod(e, W)


@pytest.mark.parametrize("shape,band", BANDS, ids=[f"{s[0]}x{s[1]}-{b[0]}_{b[1]}" for s, b in BANDS])
@pytest.mark.parametrize("off", [0, 1])
def test_indexes_of_a_band(shape, band, off):
    lib, st = _lib()
    H, W = shape
    e_lo, e_hi = band
    gh, gw = RR.grid(H, W)
    cls = np.random.default_rng(H + e_lo).integers(0, 19, size=(gh, gw)).astype(np.int32)
    want = RR.indexes(cls, H, W).reshape(3, -1)[:, e_lo:e_hi]
    cbuf = Buf(gh * gw, torch.int32, 0, cls)
    out = Buf(3 * (e_hi - e_lo), torch.int32, off)
    assert lib.icm_residual_indexes_band(cbuf.ptr, H, W, e_lo, e_hi, out.ptr, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.get(want.shape), want)       # every element of the band, nothing outside it


def _windows(shape, band):
    """windows inside the band: its first (partial) row from the band's first element, its last row up to the band's
    last element, rows in between at widths that are no multiple of four and origins off the runs of four"""
    H, W = shape
    e_lo, e_hi = band
    (ya, xa), (yb, xb) = _rowcol(e_lo, W), _rowcol(e_hi - 1, W)
    out = []
    if ya == yb:
        return [(ya, xa, 1, xb - xa + 1), (ya, xa + 1, 1, min(7, xb - xa))]
    out.append((ya, xa, 1, W - xa))                         # the first row, from the band's first element
    out.append((yb, 0, 1, xb + 1))                          # the last row, to the band's last element
    if yb - ya >= 2:
        out.append((ya + 1, 0, yb - ya - 1, W))             # every full row
        out.append((ya + 1, 13, min(yb - ya - 1, 18), min(W - 13, 23)))
        out.append((yb - 1, W - 7, 1, 7))
        if xa < W - 1:
            out.append((ya, xa + 1, yb - ya, W - xa - 1))   # from the first row down, right of the band's start
    return out


@pytest.mark.parametrize("shape,band", BANDS, ids=[f"{s[0]}x{s[1]}-{b[0]}_{b[1]}" for s, b in BANDS])
@pytest.mark.parametrize("d,off", [(0, 0), (3, 1), (32, 3)])
def test_apply_from_a_band(shape, band, d, off):
    lib, st = _lib()
    H, W = shape
    e_lo, e_hi = band
    x, xhat = RR.random_pair(H, W, 17 + d)
    q = RR.quantise(x, xhat, d)
    ya, xa = _rowcol(e_lo, W)
    q[:, ya, xa] = [2 ** 31 - 1, -2 ** 31, 300]             # the band's first element: saturates, does not overflow
    sym = Buf(3 * (e_hi - e_lo), torch.int32, off, q.reshape(3, -1)[:, e_lo:e_hi])
    for window in _windows(shape, band):
        y0, x0, h, w = window
        crop = np.ascontiguousarray(xhat[y0:y0 + h, x0:x0 + w])
        xb, out = Buf(h * w * 3, torch.uint8, off, crop), Buf(h * w * 3, torch.uint8, off)
        assert lib.icm_residual_apply_band(xb.ptr, sym.ptr, H, W, e_lo, e_hi, y0, x0, h, w, d, out.ptr, st) == 0, window
        torch.cuda.synchronize()
        got = out.get((h, w, 3))
        assert np.array_equal(got, RR.reconstruct(crop, q, d, window)), window
        # and it is what the whole planes give
        full, out2 = Buf(3 * H * W, torch.int32, 0, q), Buf(h * w * 3, torch.uint8, 0)
        xb2 = Buf(h * w * 3, torch.uint8, 0, crop)
        assert lib.icm_residual_apply(xb2.ptr, full.ptr, H, W, y0, x0, h, w, d, out2.ptr, st) == 0
        torch.cuda.synchronize()
        assert np.array_equal(out2.get((h, w, 3)), got), window


MAP_CASES = [((40, 50), (384, 1152), (8, 13, 14, 23)), ((40, 50), (384, 1152), (7, 45, 16, 5)),
             ((37, 67), (640, 1920), (14, 29, 5, 11)), ((37, 67), (641, 1919), (10, 15, 18, 50)),
             ((37, 67), (640, 1920), (9, 37, 1, 30))]


@pytest.mark.parametrize("shape,band,window", MAP_CASES, ids=[f"{s[0]}x{s[1]}-{'_'.join(map(str, w))}"
                                                              for s, b, w in MAP_CASES])
@pytest.mark.parametrize("off", [0, 1])
def test_apply_map_from_a_band(shape, band, window, off):
    lib, st = _lib()
    H, W = shape
    e_lo, e_hi = band
    y0, x0, h, w = window
    dmap = MR.window_map(H, W)                              # 0 and 32 on either side of every cell boundary
    paths = MR.window_paths(H, W, window, dmap)
    assert "straddle-differ" in paths, paths                # a run of four pixels over two cells of different bounds
    x, xhat = MR.random_pair(H, W, 23)
    q = MR.quantise_map(x, xhat, dmap)
    sym = Buf(3 * (e_hi - e_lo), torch.int32, off, q.reshape(3, -1)[:, e_lo:e_hi])
    crop = np.ascontiguousarray(xhat[y0:y0 + h, x0:x0 + w])
    xb, out = Buf(h * w * 3, torch.uint8, off, crop), Buf(h * w * 3, torch.uint8, off)
    dm = Buf(dmap.size, torch.uint8, 0, dmap)
    assert lib.icm_residual_apply_map_band(xb.ptr, sym.ptr, H, W, e_lo, e_hi, y0, x0, h, w, dm.ptr, out.ptr, st) == 0
    torch.cuda.synchronize()
    got = out.get((h, w, 3))
    assert np.array_equal(got, MR.reconstruct_map(crop, q, dmap, window))
    err = np.abs(got.astype(np.int64) - x[y0:y0 + h, x0:x0 + w].astype(np.int64))
    assert (err <= MR.per_pixel(dmap, H, W, window)[..., None]).all()


def test_refusals():
    lib, st = _lib()
    H, W, e_lo, e_hi = 40, 50, 384, 1152                    # rows 7 (from column 34) .. 23 (to column 1)
    b32, b8 = Buf(3 * (e_hi - e_lo), torch.int32), Buf(40 * 50 * 3, torch.uint8)
    out = Buf(40 * 50 * 3, torch.uint8)
    for lo, hi in ((-1, 10), (10, 10), (20, 10), (0, H * W + 1)):
        assert lib.icm_residual_indexes_band(b32.ptr, H, W, lo, hi, b32.ptr, st) == ERR_ARG
        assert lib.icm_residual_apply_band(b8.ptr, b32.ptr, H, W, lo, hi, 0, 0, 1, 1, 0, out.ptr, st) == ERR_ARG
    # a window with a sample outside the band: before its first element, after its last, a row above, a row below
    for window in ((7, 33, 1, 4), (23, 0, 1, 3), (6, 40, 2, 4), (23, 0, 2, 1), (8, 0, 16, 50), (0, 0, 40, 50)):
        assert lib.icm_residual_apply_band(b8.ptr, b32.ptr, H, W, e_lo, e_hi, *window, 0, out.ptr, st) == ERR_ARG, window
        assert lib.icm_residual_apply_map_band(b8.ptr, b32.ptr, H, W, e_lo, e_hi, *window, b8.ptr, out.ptr,
                                               st) == ERR_ARG, window
    assert lib.icm_residual_apply_band(b8.ptr, b32.ptr, H, W, e_lo, e_hi, 7, 34, 1, 16, 0, out.ptr, st) == 0
    assert lib.icm_residual_apply_band(b8.ptr, b32.ptr, H, W, e_lo, e_hi, 23, 0, 1, 2, 0, out.ptr, st) == 0
    assert lib.icm_residual_apply_band(b8.ptr, None, H, W, e_lo, e_hi, 8, 0, 1, 1, 0, out.ptr, st) == ERR_ARG
    assert lib.icm_residual_apply_band(b8.ptr, b32.ptr, H, W, e_lo, e_hi, 8, 0, 1, 1, 33, out.ptr, st) == ERR_ARG
    torch.cuda.synchronize()
    from icm_amd import residual as R
    sym = torch.zeros((3, e_hi - e_lo), dtype=torch.int32, device=DEV)
    xhat = torch.zeros((1, 4, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="inside the band"):
        R.residual_apply(xhat, sym, (7, 33, 1, 4), 0, band=(e_lo, e_hi), size=(H, W))
    with pytest.raises(ValueError, match="not a band"):
        R.residual_indexes(torch.zeros((3, 4), dtype=torch.int32, device=DEV), H, W, band=(5, 5))
    assert R.residual_apply(xhat, sym, (7, 34, 1, 4), 0, band=(e_lo, e_hi), size=(H, W)).shape == (1, 4, 3)
