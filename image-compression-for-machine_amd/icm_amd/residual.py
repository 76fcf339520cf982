"""The error-bounded residual layer of the codec: quantiser, context classes, static tables, and the kernels' wrappers.

Parity unpinned: no counterpart in the reference.  A second layer over any base stream, as in JPEG-LS near-lossless
coding or the residual layers of learned lossless coders: it codes the quantised difference between the original 8-bit
image x and the decoder's 8-bit reconstruction xhat of the base stream, so that the decode differs from the original by
at most D in every sample (D = 0: not at all).  Integers only, one definition for encoder, decoder and tests
(tests/_residual_ref.py restates it in numpy):

    s = 2 D + 1,  r = x - xhat,  q = sign(r) ((|r| + D) div s),  xtilde = min(max(xhat + q s, 0), 255)

|x - xtilde| <= D for every (x, xhat, D), the clamp included (x itself lies in 0..255, so clamping moves xtilde toward
it).  Symbols are coded in plane order [3][H][W], row-major, image pixels only.

Context model -- one class per 16 x 16-pixel cell of the image (``CELL``; the grid is anchored at pixel (0, 0), edge
cells are partial), shared by the three channels: with N the coded samples of the cell and S the sum of |q| over them,
the class is the number of ``THRESHOLDS`` T_j with 16 S > N T_j, an integer comparison.  T_j = round(2^(1 + j/2)),
j = 0..17: 19 classes that cover a mean |q| from 1/8 to 45 in half octaves.  The classes travel in the stream, so the
thresholds are the encoder's business and affect the rate alone.

Tables -- per class k a two-sided geometric law in integers: w(0) = 2^24, w(n + 1) = (w(n) R_k) >> 16 with the Q16 ratio
``RATIOS[k]``, chosen so that E|q| = 2 r / (1 - r^2) of the law is the geometric mean of the class's bounds T_(k-1) / 16
and T_k / 16 (class 0: its upper bound and a quarter of it; class 18: 724 / 16 and 1024 / 16).  The support is |v| <= L_k,
the last n with w(n) > 0, capped at 255 (``SUPPORTS``: 4 .. 255); anything outside takes the coder's escape path, whose
bin has the weight 1.  The weights go through ``ans.pmf_to_quantized_cdf`` as w 2^-24 -- exact in float32, and inside
the range that function's 32-bit counts hold -- and come out as the usual (cdf, sizes, offsets) triple with offsets
-L_k.  Row ``NCLASSES`` (19) is uniform over the classes and codes the class map.  ``ResidualTables`` holds the triple
and answers ``_tables()`` / ``_device_tables()``, which is all ``ans.HostCoder`` / ``ans.LanesCoder`` ask of an entropy
model.

Bound map -- the bound may also be one byte per cell of the same grid (``check_error_map``; ICME streams): a sample of
cell (cy, cx) is coded by the rule above under D[cy, cx], and the class of a cell is taken from its own q, so classes,
thresholds and tables are untouched.  ``residual_code``, ``residual_apply`` and ``encode_residual`` take either the int
or a host map, which is checked here and then uploaded (``icm_residual_code_map`` / ``icm_residual_apply_map``); the
decode is within D[cy, cx] of the original in every sample of the cell, bit-exact where the byte is 0.

String -- one string of four runs: the class map (gh gw symbols, all with index 19), then the R, G and B planes (H W
symbols each, the index of a sample being the class of its cell).

Region decode -- a lane stream is G independent wave bodies, and wave g owns the elements [g c, min(n, (g + 1) c)) of
every run of n (c = ``ans.lanes_chunk(n, G)``).  The rows of a window are therefore a contiguous range of waves, the
same for the three planes, and the classes those waves need are a (small) range of waves of the class run:
``region_plan`` works both out, and ``decode_residual(..., window=...)`` decodes those waves alone into a band
[3, e_hi - e_lo] of the planes (``ResidualBand``), which ``residual_indexes`` and ``residual_apply`` take through their
``band`` argument.  What a window costs is whole waves: every row of the waves that hold its rows, at full width (rows,
not columns).  A host-coded string is one chain and is decoded whole."""
from __future__ import annotations

import zlib
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from ._lib import check
from .bitstream import MAX_ERROR        # the largest D, defined with the container that stores it
from .bitstream import check_error_map as _check_error_map

CELL = 16
THRESHOLDS = (2, 3, 4, 6, 8, 11, 16, 23, 32, 45, 64, 91, 128, 181, 256, 362, 512, 724)
NCLASSES = len(THRESHOLDS) + 1          # 19; also the index of the class map's own table
RATIOS = (2046, 4988, 7013, 9808, 13580, 17795, 23636, 30678, 37434, 43491, 48848, 53221, 56537, 59008, 60846, 62182,
          63146, 63836, 64330)
MAX_SUPPORT = 255
assert len(RATIOS) == NCLASSES


def check_max_error(d, who: str = ""):
    """``d`` as an int if it is an integer in 0 .. MAX_ERROR, None for None (off); ValueError otherwise"""
    if d is None:
        return None
    if isinstance(d, bool) or not hasattr(d, "__index__"):
        raise ValueError(f"{who}max_error must be an integer, got {d!r}")
    d = int(d)
    if not 0 <= d <= MAX_ERROR:
        raise ValueError(f"{who}max_error = {d} outside [0, {MAX_ERROR}]")
    return d


def grid(H: int, W: int) -> Tuple[int, int]:
    """(gh, gw): the cells of an H x W image"""
    return -(-H // CELL), -(-W // CELL)


def check_error_map(dmap, H: int, W: int, who: str = "") -> np.ndarray:
    """``dmap`` as a contiguous host uint8 [gh, gw] array: the bounds of the cells of an H x W image, each in
    0 .. MAX_ERROR (``bitstream.check_error_map``, the one check).  ValueError for a device tensor, another dtype
    (nothing is cast), another shape or a larger entry.  Host-only."""
    if isinstance(dmap, torch.Tensor):
        if dmap.is_cuda:
            raise ValueError(f"{who}the bound map must be a host array: it is checked before it is uploaded")
        dmap = dmap.numpy()
    return np.ascontiguousarray(_check_error_map(dmap, H, W, who))


def _is_map(d) -> bool:
    return isinstance(d, (np.ndarray, torch.Tensor)) and d.ndim > 0


def class_weights(k: int) -> np.ndarray:
    """int64 [L_k + 1]: w(0) .. w(L_k) of class k"""
    w, out = 1 << 24, []
    while w > 0 and len(out) <= MAX_SUPPORT:
        out.append(w)
        w = (w * RATIOS[k]) >> 16
    return np.asarray(out, dtype=np.int64)


SUPPORTS = tuple(len(class_weights(k)) - 1 for k in range(NCLASSES))


class ResidualTables:
    """the static tables of the residual layer: rows 0 .. 18 the classes' laws, row 19 uniform over the classes.
    ``cdf`` int32 [20, stride], ``sizes`` and ``offsets`` int32 [20] (host, numpy); ``crc``: CRC-32 over the three as
    little-endian int32, what an ICMR stream records."""

    def __init__(self):
        from .ans import pmf_to_quantized_cdf
        rows, offsets = [], []
        for k in range(NCLASSES):
            w = class_weights(k)
            pmf = np.concatenate([w[:0:-1], w, [1]]).astype(np.float32) * np.float32(2.0 ** -24)
            rows.append(pmf_to_quantized_cdf(pmf.tolist()))
            offsets.append(-(len(w) - 1))
        rows.append(pmf_to_quantized_cdf([1.0] * NCLASSES + [2.0 ** -24]))
        offsets.append(0)
        self.sizes = np.asarray([len(r) for r in rows], dtype=np.int32)
        self.offsets = np.asarray(offsets, dtype=np.int32)
        self.cdf = np.zeros((len(rows), int(self.sizes.max())), dtype=np.int32)
        for i, r in enumerate(rows):
            self.cdf[i, :len(r)] = r
        crc = 0
        for a in (self.cdf, self.sizes, self.offsets):
            crc = zlib.crc32(a.astype("<i4").tobytes(), crc)
        self.crc = crc & 0xFFFFFFFF
        self._host = None
        self._device = {}

    def _tables(self):
        if self._host is None:
            from .ans import _Tables
            self._host = _Tables(self.cdf, self.sizes, self.offsets)
        return self._host

    def _device_tables(self, device=None):
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device not in self._device:
            self._device[device] = tuple(torch.from_numpy(a).to(device) for a in (self.cdf, self.sizes, self.offsets))
        return self._device[device]


_TABLES = None


def tables() -> ResidualTables:
    """the one set of tables, built on first use"""
    global _TABLES
    if _TABLES is None:
        _TABLES = ResidualTables()
    return _TABLES


def _u8(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype != torch.uint8 or t.dim() != 3 or t.size(2) != 3 or not t.is_cuda:
        raise ValueError(f"residual: {what} must be a device 8-bit [H, W, 3], got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def residual_code(x: torch.Tensor, xhat: torch.Tensor, d):
    """device 8-bit [H, W, 3] original and reconstruction -> (symbols int32 [3, H, W], indexes int32 [3, H, W], classes
    int32 [gh, gw]) on the device.  ``d``: the bound, an int (``icm_residual_code``) or a host map of bounds per cell
    (``check_error_map``; ``icm_residual_code_map``)"""
    x, xhat = _u8(x, "the image"), _u8(xhat, "the reconstruction")
    if x.shape != xhat.shape:
        raise ValueError(f"residual: image {tuple(x.shape)} and reconstruction {tuple(xhat.shape)} differ in size")
    H, W = x.size(0), x.size(1)
    sym = torch.empty((3, H, W), dtype=torch.int32, device=x.device)
    idx = torch.empty_like(sym)
    cls = torch.empty(grid(H, W), dtype=torch.int32, device=x.device)
    if _is_map(d):
        dmap = torch.from_numpy(check_error_map(d, H, W, "residual: ")).to(x.device)
        check(L.lib().icm_residual_code_map(x.data_ptr(), xhat.data_ptr(), H, W, dmap.data_ptr(), sym.data_ptr(),
                                            idx.data_ptr(), cls.data_ptr(), L.stream()), "residual_code_map")
    else:
        check(L.lib().icm_residual_code(x.data_ptr(), xhat.data_ptr(), H, W, d, sym.data_ptr(), idx.data_ptr(),
                                        cls.data_ptr(), L.stream()), "residual_code")
    return sym, idx, cls


def _check_band(band, H: int, W: int) -> Tuple[int, int]:
    e_lo, e_hi = int(band[0]), int(band[1])
    if not 0 <= e_lo < e_hi <= H * W:
        raise ValueError(f"residual: [{e_lo}, {e_hi}) is not a band of the {H}x{W} planes")
    return e_lo, e_hi


def residual_indexes(classes: torch.Tensor, H: int, W: int, band=None) -> torch.Tensor:
    """device int32 classes [gh, gw] (as decoded) -> int32 [3, H, W], every sample's class (``icm_residual_indexes``).
    ``band`` = (e_lo, e_hi): only the elements e_lo <= e < e_hi of every row-major plane, int32 [3, e_hi - e_lo]
    (``icm_residual_indexes_band``); the band may start and end inside a row"""
    if classes.dtype != torch.int32 or classes.numel() != grid(H, W)[0] * grid(H, W)[1] or not classes.is_cuda:
        raise ValueError(f"residual: classes must be {grid(H, W)} device int32, got {classes.dtype} {tuple(classes.shape)}")
    classes = classes.contiguous()
    if band is not None:
        e_lo, e_hi = _check_band(band, H, W)
        idx = torch.empty((3, e_hi - e_lo), dtype=torch.int32, device=classes.device)
        check(L.lib().icm_residual_indexes_band(classes.data_ptr(), H, W, e_lo, e_hi, idx.data_ptr(), L.stream()),
              "residual_indexes_band")
        return idx
    idx = torch.empty((3, H, W), dtype=torch.int32, device=classes.device)
    check(L.lib().icm_residual_indexes(classes.data_ptr(), H, W, idx.data_ptr(), L.stream()), "residual_indexes")
    return idx


def residual_apply(xhat: torch.Tensor, symbols: torch.Tensor, window, d, band=None, size=None) -> torch.Tensor:
    """device 8-bit [h, w, 3] reconstruction of the window (y0, x0, h, w) and the image's symbols int32 [3, H, W] -> the
    window with the residual applied, 8-bit [h, w, 3].  ``d``: the bound, an int (``icm_residual_apply``) or the host
    map of the whole image's cells (``icm_residual_apply_map``): a window pixel takes the bound of the cell of its image
    position.  With ``band`` = (e_lo, e_hi) and ``size`` = (H, W), ``symbols`` is int32 [3, e_hi - e_lo], that band of
    the planes (``icm_residual_apply_band`` / ``icm_residual_apply_map_band``); the window must lie inside it"""
    xhat = _u8(xhat, "the reconstruction")
    y0, x0, h, w = window
    if band is not None:
        H, W = size
        e_lo, e_hi = _check_band(band, H, W)
        fits = symbols.dim() == 2 and symbols.size(1) == e_hi - e_lo
        if fits and not (0 <= y0 and 0 <= x0 and 1 <= h and 1 <= w and y0 + h <= H and x0 + w <= W and
                         y0 * W + x0 >= e_lo and (y0 + h - 1) * W + x0 + w <= e_hi):
            raise ValueError(f"residual: window {window} does not lie inside the band [{e_lo}, {e_hi}) of the {H}x{W} "
                             f"planes")
    else:
        fits = symbols.dim() == 3
    if symbols.dtype != torch.int32 or not fits or symbols.size(0) != 3 or tuple(xhat.shape[:2]) != (h, w):
        raise ValueError(f"residual: symbols {symbols.dtype} {tuple(symbols.shape)} / window {window} / reconstruction "
                         f"{tuple(xhat.shape)} do not fit")
    symbols = symbols.contiguous()
    out = torch.empty_like(xhat)
    if band is None:
        H, W = symbols.size(1), symbols.size(2)
    dmap = torch.from_numpy(check_error_map(d, H, W, "residual: ")).to(xhat.device) if _is_map(d) else None
    if band is not None and dmap is not None:
        check(L.lib().icm_residual_apply_map_band(xhat.data_ptr(), symbols.data_ptr(), H, W, e_lo, e_hi, y0, x0, h, w,
                                                  dmap.data_ptr(), out.data_ptr(), L.stream()), "residual_apply_map_band")
    elif band is not None:
        check(L.lib().icm_residual_apply_band(xhat.data_ptr(), symbols.data_ptr(), H, W, e_lo, e_hi, y0, x0, h, w, d,
                                              out.data_ptr(), L.stream()), "residual_apply_band")
    elif dmap is not None:
        check(L.lib().icm_residual_apply_map(xhat.data_ptr(), symbols.data_ptr(), H, W, y0, x0, h, w, dmap.data_ptr(),
                                             out.data_ptr(), L.stream()), "residual_apply_map")
    else:
        check(L.lib().icm_residual_apply(xhat.data_ptr(), symbols.data_ptr(), H, W, y0, x0, h, w, d, out.data_ptr(),
                                         L.stream()), "residual_apply")
    return out


def encode_residual(x: torch.Tensor, xhat: torch.Tensor, d, coder) -> Tuple[bytes, Tuple[int, int]]:
    """the residual string of x against xhat under the bound ``d`` (an int, or a host map per cell) and ``coder`` (an
    object of ``ans.coder_for``) -> (string, (smallest, largest class in the map))"""
    sym, idx, cls = residual_code(x, xhat, d)
    n, cells = sym[0].numel(), cls.numel()
    symbols = torch.cat([cls.reshape(-1), sym.reshape(-1)])
    indexes = torch.cat([torch.full((cells,), NCLASSES, dtype=torch.int32, device=cls.device), idx.reshape(-1)])
    string = coder.encode(symbols, indexes, [cells, n, n, n], tables())
    lo, hi = torch.aminmax(cls)
    return string, (int(lo), int(hi))


class RegionPlan(NamedTuple):
    """what a window of an H x W image needs of a residual string of G waves (``region_plan``)"""
    plane_waves: Tuple[int, int]     # [pa, pb): the waves of runs 1 .. 3 that hold the window's rows
    band: Tuple[int, int]            # [e_lo, e_hi) = [pa c, min(H W, pb c)): the plane elements those waves own
    cell_rows: Tuple[int, int]       # [cr0, cr1): the rows of cells the band touches
    class_waves: Tuple[int, int]     # [ka, kb): the waves of run 0 that hold the classes of those rows of cells


def region_plan(H: int, W: int, G: int, window) -> RegionPlan:
    """the waves of a residual string of ``G`` waves that the window (y0, x0, h, w) of an H x W image needs; pure
    host arithmetic.  The window's rows y0 .. y0 + h - 1, at full width, are the plane elements [y0 W, (y0 + h) W), which
    lie in the waves [pa, pb).  A wave decodes its whole chunk, so it needs the class of every pixel of the band
    [pa c, min(H W, pb c)), not only of the window's rows: the band's first and last row give the rows of cells, whose
    classes are the elements [cr0 gw, cr1 gw) of run 0 and lie in its waves [ka, kb)."""
    y0, x0, h, w = (int(v) for v in window)
    if not (H >= 1 and W >= 1 and G >= 1 and 0 <= y0 and 0 <= x0 and h >= 1 and w >= 1 and y0 + h <= H and x0 + w <= W):
        raise ValueError(f"residual: window {(y0, x0, h, w)} is not inside the {H}x{W} image (G = {G})")
    from .ans import lanes_chunk
    n = H * W
    c = lanes_chunk(n, G)
    pa, pb = (y0 * W) // c, ((y0 + h) * W - 1) // c + 1
    e_lo, e_hi = pa * c, min(n, pb * c)
    gh, gw = grid(H, W)
    cr0, cr1 = (e_lo // W) // CELL, ((e_hi - 1) // W) // CELL + 1
    kc = lanes_chunk(gh * gw, G)
    ka, kb = (cr0 * gw) // kc, (cr1 * gw - 1) // kc + 1
    return RegionPlan((pa, pb), (e_lo, e_hi), (cr0, cr1), (ka, kb))


class ResidualBand(NamedTuple):
    """the symbols a window needs: ``symbols`` int32 [3, e_hi - e_lo] on the device, the elements ``band`` =
    (e_lo, e_hi) of every plane; ``waves`` = (distinct waves that decoded anything, G of the string), None for a
    host-coded string"""
    symbols: torch.Tensor
    band: Tuple[int, int]
    waves: Optional[Tuple[int, int]]


def decode_residual(string: bytes, H: int, W: int, coder, device, window=None):
    """inverse of ``encode_residual``: the symbols, int32 [3, H, W] on ``device``.  With the lanes coder the class run
    is decoded, expanded to indexes on the device and the planes decoded without anything coming back to the host
    before ``finish()``.  ValueError for a string that is not one of this layer's.

    ``window`` = (y0, x0, h, w): a ``ResidualBand`` instead, with at least the symbols of that window.  With the lanes
    coder only the waves of ``region_plan`` are decoded: run 0 by the class waves and the plane waves (a wave is given
    its runs in order, so the plane waves take their part of run 0 too, often an empty one) into the full class
    buffer, the band's indexes are expanded, runs 1 .. 3 are decoded by the plane waves into the band, and then the
    plane waves are held to the end checks and the class-only waves, which stop after run 0, to their status alone.
    With the host coder, whose stream is one chain, or when the window's waves own the whole planes, the string is
    decoded whole and the band is [0, H W)."""
    gh, gw = grid(H, W)
    n, cells = H * W, gh * gw
    dec = coder.decoder(string, tables())
    try:
        G = dec.waves
        plan = region_plan(H, W, G, window) if window is not None and G is not None else None
        if plan is None or plan.band == (0, n):
            cls = dec.decode_run(torch.full((cells,), NCLASSES, dtype=torch.int32, device=device))
            idx = residual_indexes(cls.reshape(gh, gw), H, W)
            sym = torch.empty((3, H, W), dtype=torch.int32, device=device)
            for c in range(3):
                dec.decode_run(idx[c], out=sym[c])
            dec.finish()
            return sym if window is None else ResidualBand(sym.reshape(3, n), (0, n), None if G is None else (G, G))
        (pa, pb), (e_lo, e_hi), _, (ka, kb) = plan
        only = [(a, b) for a, b in ((ka, min(kb, pa)), (max(ka, pb), kb)) if a < b]     # class waves outside [pa, pb)
        cls = torch.zeros((cells,), dtype=torch.int32, device=device)      # cells no wave decodes are never looked at
        idx0 = torch.full((cells,), NCLASSES, dtype=torch.int32, device=device)
        for a, b in only + [(pa, pb)]:
            dec.decode_run_waves(a, b, 0, idx0, cells, out=cls)
        idx = residual_indexes(cls.reshape(gh, gw), H, W, band=(e_lo, e_hi))
        sym = torch.empty((3, e_hi - e_lo), dtype=torch.int32, device=device)
        for c in range(3):
            dec.decode_run_waves(pa, pb, e_lo, idx[c], n, out=sym[c])
        dec.finish_waves(pa, pb, True)
        for a, b in only:
            dec.finish_waves(a, b, False)
        return ResidualBand(sym, (e_lo, e_hi), (pb - pa + sum(b - a for a, b in only), G))
    finally:
        dec.close()
