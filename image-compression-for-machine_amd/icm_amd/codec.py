"""``python -m icm_amd.codec`` -- image file to bit-stream file and back, in two processes that share a checkpoint.

    python -m icm_amd.codec encode IMAGE -o FILE -a cnn -p CKPT [--tile N [--overlap M]] [--coder {host,lanes}]
                                   [--qstep K | --target-bytes N | --target-bpp F] [--roi Y0,X0,H,W:D ...] [--rdoq W]
                                   [--aq S] [--max-error D [--error-roi Y0,X0,H,W:D' ...]]
    python -m icm_amd.codec decode FILE -o IMAGE.png -p CKPT [--reference IMAGE] [--region Y0,X0,H,W]

Parity unpinned: no counterpart in the reference (upstream CompressAI's ``examples/codec.py`` is not in its tree).  The
conventions are those of ``icm_amd.eval_model``: ``-a`` architecture, ``-p`` checkpoint (``weights_only=True``), exit
codes 2 = argument error, 3 = no GPU, 4 = bad input.  ``decode`` takes the architecture from the stream (``-a``, if
given, must agree) and refuses, before it touches the payload, a stream whose model fingerprint is not the
checkpoint's.  Both commands print one JSON line.

The image boundary runs on the device: the 8-bit image crosses PCIe as bytes, ``icm_image_u8_to_f32`` converts and
pads in one pass (``ToTensor`` + ``utils.pad_to_multiple``, bit for bit), and ``icm_image_f32_to_u8`` crops, quantises
(``datasets.to_pil_image``) and, given the original, sums the squared 8-bit differences that the PSNR is formed from.
The container is ``icm_amd.bitstream``; one image per stream.

Large images are coded as a grid of independently coded tiles (``--tile``): the convolution kernels address a plane
set with 32-bit offsets, which bounds one ``compress()`` call near 11 megapixels, and activation memory grows with the
image.  Each tile is a complete single-image stream of its crop, all of them wrapped in an ``ICMT`` container; the
decoder adds the decoded tiles into an f32 canvas, their overlap bands weighted by a linear ramp
(``icm_image_tile_blend``), and quantises the canvas once.  ``--region`` decodes only the tiles a region touches.

``--coder lanes`` codes the strings as lane streams on the device (csrc/rans_lanes.hip; format in
``icm_amd.bitstream``) instead of the host's scalar stream, the default.  The stream records its coder, so ``decode``
takes no flag.

``--qstep K`` is the quality knob of one checkpoint: a scalar quantiser step 2^(K/8) on the latent y, K in -16 .. 32
(csrc/qstep.hip; ``icm_amd.bitstream`` for how K travels).  K = 0, the default, is the codec without a step, and its
files are byte for byte what they were.  ``--target-bytes`` / ``--target-bpp`` search K for a budget with real encodes
as probes (``search_qstep``: at most 8, the analysis transform run once); a budget the coarsest step misses exits 4
and writes nothing.  ``decode`` reads K from the stream.  Parity unpinned: no counterpart in the reference.

``--roi Y0,X0,H,W:D`` (repeatable) spends the bits where a downstream task looks: the 16 x 16-pixel cells of the latent
that hold a pixel of the rectangle are coded with the step index K + D instead of K (D negative: finer), clamped to the
range; later rectangles win.  K is ``--qstep``, the step a budget search finds (it runs over K as without rectangles,
the map rebuilt per probe), or 0.  The per-position map travels in the stream (``icm_amd.bitstream``, "Quality map"),
per tile in a tiled one, and ``decode`` needs no flag; rectangles that change no cell leave the file what it is without
them.  Parity unpinned: no counterpart in the reference, whose own answer is a task loss at training time.

``--rdoq W`` turns on rate-distortion optimised quantisation in the encoder: each latent element is coded as the nearest
integer or, where W x the added squared error in quantiser steps is less than the bits the coder's tables say it saves,
as its neighbour toward zero (``icm_gc_code_rdo`` in csrc/qstep.hip).  It combines with every other flag, changes
nothing in the stream's format, and ``decode`` neither has nor needs a flag.  Parity unpinned.

``--aq S`` derives the quality map from the picture, as video encoders' variance-based adaptive quantisation does: one
pass over the 8-bit image gives every cell the variance v of its luma (``icm_image_cell_stats`` in csrc/imageio.hip),
and the cell is coded with the step index K + clip(rint(4 S (log2(1 + v) - the image's mean of it)), -16, 16).  S > 0
spends bits on flat cells and saves them on busy ones, S < 0 the reverse; |S| <= 4.  S = 1 makes the step follow the
cell's standard deviation: a rule, not a measured optimum.  ``--roi`` rectangles win over it, a budget search runs over K
with the offsets fixed, tiles share the image's mean, and ``decode`` needs no flag.  Parity unpinned.

``--max-error D`` gives a guarantee per sample where every flag above steers an average: the file decodes to an image
whose every 8-bit sample lies within D of the original's, D in 0 .. 32, and D = 0 gives the original back bit for bit.
The base is coded as without the flag (every flag above applies to it; a byte budget contradicts a bound and is refused);
the encoder then decodes it on the device, as the decoder will, and codes the quantised differences as a second layer
(``icm_amd.residual``, csrc/residual.hip: a uniform quantiser of step 2 D + 1, one context class per 16 x 16-pixel cell,
static two-sided geometric tables, the coder ``--coder`` names), both wrapped in an ``ICMR`` container
(``icm_amd.bitstream``).  ``decode`` needs no flag; with ``--region`` it decodes the base's region, and of a residual
string coded with ``--coder lanes`` only the wave bodies that hold the window's rows and their cells' classes (the report's
"residual_waves": [decoded, G]) -- whole waves, so rows and not columns are saved; a host-coded residual string is one
chain and decodes whole.  Files written without the flag are
byte for byte what they were.  Parity unpinned: no counterpart in the reference.

``--error-roi Y0,X0,H,W:D'`` (repeatable, with ``--max-error``) gives the bound the form every other knob has: the
16 x 16-pixel cells of the residual layer's grid that hold a pixel of the rectangle are held to the absolute bound D'
instead of D -- D' = 0: that part of the picture comes back bit for bit -- and later rectangles win (``error_map``).
The map of bounds travels in an ``ICME`` container (``icm_amd.bitstream``), ``decode`` needs no flag and reports the
map's range and, with ``--reference``, the number of samples outside their cell's bound, which is 0.  Rectangles that
change no cell leave the ``ICMR`` file what it is without them.  What a loose background saves in bytes depends on the
base model and is not measured against trained weights.  Parity unpinned."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import bitstream as B
from . import residual as R
from ._lib import check
from .ans import coder_for
from .residual import ResidualTables      # noqa: F401  part of this module's surface

PAD_MULTIPLE = 64      # six stride-2 stages (utils.pad_to_multiple)


def arch_of(model) -> str:
    """name of the model's class in ``zoo.models``; ValueError unless the bit-stream format knows it (``stf6`` has no
    entropy coder loop: its ``compress`` raises NotImplementedError).  Host-only: no GPU work."""
    from .zoo import models
    name = next((k for k, cls in models.items() if type(model) is cls), None)
    if name is None:
        raise ValueError(f"codec: {type(model).__name__} is not an architecture of icm_amd.zoo.models")
    if name not in B.ARCHS:
        raise ValueError(f"codec: architecture {name!r} has no bit-stream codec (compress() is not implemented); "
                         f"choose from {list(B.ARCHS)}")
    return name


def center_pads(h: int, w: int, p: int = PAD_MULTIPLE) -> Tuple[int, int, int, int]:
    """(left, right, top, bottom) of ``utils.pad_to_multiple``: centre padding, the extra pixel right / bottom"""
    new_h, new_w = (h + p - 1) // p * p, (w + p - 1) // p * p
    left, top = (new_w - w) // 2, (new_h - h) // 2
    return left, new_w - w - left, top, new_h - h - top


def _as_u8_image(img, device, what: str = "image") -> torch.Tensor:
    """8-bit [H, W, 3] on ``device``, contiguous; the copy to the device moves bytes"""
    if isinstance(img, torch.Tensor):
        t = img
    else:
        a = np.asarray(img)
        if not (a.flags.writeable and a.flags.c_contiguous):     # PIL hands out read-only views
            a = np.array(a, order="C")
        t = torch.from_numpy(a)
    if t.dtype != torch.uint8 or t.dim() != 3 or t.size(2) != 3 or t.size(0) < 1 or t.size(1) < 1:
        raise ValueError(f"codec: {what} must be 8-bit [H, W, 3], got {t.dtype} {tuple(t.shape)}")
    return t.to(device).contiguous()


def image_u8_to_f32(img: torch.Tensor, pads: Tuple[int, int, int, int]) -> torch.Tensor:
    """device 8-bit [H, W, 3] -> f32 [1, 3, top + H + bottom, left + W + right], zeros around the image"""
    H, W = img.size(0), img.size(1)
    left, right, top, bottom = pads
    out = torch.empty((1, 3, top + H + bottom, left + W + right), dtype=torch.float32, device=img.device)
    check(L.lib().icm_image_u8_to_f32(img.data_ptr(), H, W, out.data_ptr(), out.size(2), out.size(3), top, left,
                                      L.stream()), "image_u8_to_f32")
    return out


def image_f32_to_u8(x: torch.Tensor, pads: Tuple[int, int, int, int],
                    reference: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """device f32 [1, 3, PH, PW] -> (8-bit [H, W, 3] of the window inside ``pads``, sum of squared 8-bit differences to
    ``reference`` as a device int64 scalar, or None)"""
    if x.dim() != 4 or x.size(0) != 1 or x.size(1) != 3 or x.dtype != torch.float32:
        raise ValueError(f"codec: expected f32 [1, 3, H, W], got {x.dtype} {tuple(x.shape)}")
    x = x.contiguous()
    left, right, top, bottom = pads
    H, W = x.size(2) - top - bottom, x.size(3) - left - right
    if H < 1 or W < 1:
        raise ValueError(f"codec: pads {pads} leave nothing of {tuple(x.shape)}")
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=x.device)
    sse = ws = None
    ws_bytes = 0
    if reference is not None:
        if tuple(reference.shape) != (H, W, 3) or reference.dtype != torch.uint8:
            raise ValueError(f"codec: reference must be 8-bit {(H, W, 3)}, got {reference.dtype} {tuple(reference.shape)}")
        reference = reference.to(x.device).contiguous()
        ws_bytes = int(L.lib().icm_image_workspace_bytes(H, W))
        ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=x.device)
        sse = torch.empty((), dtype=torch.int64, device=x.device)
    check(L.lib().icm_image_f32_to_u8(x.data_ptr(), x.size(2), x.size(3), top, left, out.data_ptr(), H, W,
                                      L.ptr(reference), L.ptr(sse), L.ptr(ws), ws_bytes, L.stream()), "image_f32_to_u8")
    return out, sse


def _ready(model) -> str:
    arch = arch_of(model)                      # refuses before any GPU work
    if model.training:
        raise ValueError("codec: the model must be in eval mode")
    if model.entropy_bottleneck._offset.numel() == 0:
        model.update(force=True)
    return arch


def plan_tiles(H: int, W: int, tile: int, overlap: int):
    """(rows, cols, [(y0, x0, h, w), ...] row-major) of ``bitstream.tile_grid``: tiles of extent ``tile`` at a stride
    of ``tile - overlap``, the last of each axis cut at the image.  Host-only."""
    rows, cols = B.tile_grid(H, W, tile, overlap)
    S = tile - overlap
    return rows, cols, [(r * S, c * S, min(tile, H - r * S), min(tile, W - c * S))
                        for r in range(rows) for c in range(cols)]


def tile_edges(r: int, c: int, rows: int, cols: int) -> int:
    """the sides of tile (r, c) that have a neighbour, as ``icm_image_tile_blend`` takes them"""
    return ((L.TILE_EDGE_LEFT if c > 0 else 0) | (L.TILE_EDGE_RIGHT if c < cols - 1 else 0) |
            (L.TILE_EDGE_TOP if r > 0 else 0) | (L.TILE_EDGE_BOTTOM if r < rows - 1 else 0))


def blend_ramp(m: int) -> np.ndarray:
    """weights across an overlap band of m pixels, (i + 0.5) / m in f32: i + 0.5 is exact and the quotient is rounded
    once, on the host, so nothing depends on how the device divides"""
    return (np.arange(m, dtype=np.float32) + np.float32(0.5)) / np.float32(max(m, 1))


def image_tile_blend(x: torch.Tensor, pads: Tuple[int, int, int, int], canvas: torch.Tensor, y0: int, x0: int,
                     ramp: Optional[torch.Tensor], edges: int) -> None:
    """canvas [3, H, W] += weights x the window of the f32 [1, 3, PH, PW] tile ``x`` inside ``pads``, at (y0, x0)"""
    left, right, top, bottom = pads
    h, w = x.size(2) - top - bottom, x.size(3) - left - right
    m = 0 if ramp is None else ramp.numel()
    check(L.lib().icm_image_tile_blend(x.data_ptr(), x.size(2), x.size(3), top, left, h, w, canvas.data_ptr(),
                                       canvas.size(1), canvas.size(2), y0, x0, L.ptr(ramp), m, edges, L.stream()),
          "image_tile_blend")


def _pack_one(arch: str, fp: int, H: int, W: int, pads, enc: Dict, coder: str) -> bytes:
    """the ICMB stream of one ``compress()`` result; a quantiser step travels as a third, one-byte string, a quality
    map as a third string of its runs"""
    header = {"arch": arch, "height": H, "width": W, "pads": pads, "shape": tuple(int(s) for s in enc["shape"]),
              "fingerprint": fp}
    strings = [s for part in enc["strings"] for s in part]
    if enc.get("qmap") is not None:
        strings.append(B.qmap_string(enc["qmap"]))
    elif enc["qstep"]:
        strings.append(B.qstep_string(enc["qstep"]))
    return B.pack(header, strings, coder=coder)


def _rdoq_kw(rdoq) -> Dict:
    """the keyword of ``compress`` / ``compress_latent`` for a checked RDOQ weight; none at all when it is off"""
    return {} if rdoq is None else {"rdoq": rdoq}


def _encode_one(model, arch: str, fp: int, u8: torch.Tensor, coder: str = "host",
                symbols_per_wave: Optional[int] = None, qstep: int = 0, qmap=None,
                rdoq: Optional[float] = None) -> bytes:
    H, W = u8.size(0), u8.size(1)
    pads = center_pads(H, W)
    enc = model.compress(image_u8_to_f32(u8, pads), coder=coder, symbols_per_wave=symbols_per_wave, qstep=qstep,
                         qmap=qmap, **_rdoq_kw(rdoq))
    return _pack_one(arch, fp, H, W, pads, enc, coder)


# ------------------------------------------------------------------------------------------- regions of interest
CELL = 16              # pixels per latent position and axis: four stride-2 stages of the analysis transform


def check_rois(rois, H: int, W: int) -> List[Tuple[int, int, int, int, int]]:
    """``rois`` as a list of (y0, x0, h, w, d) of ints: rectangles of image pixels inside the H x W image, each with
    an integer offset d to the background step index.  ValueError otherwise.  Host-only."""
    out = []
    try:
        rois = list(rois)
    except TypeError:
        raise ValueError(f"codec: roi must be a list of (y0, x0, h, w, d), got {rois!r}")
    for r in rois:
        try:
            if len(r) != 5 or any(isinstance(v, bool) or not hasattr(v, "__index__") for v in r):
                raise TypeError
            y0, x0, h, w, d = (int(v) for v in r)
        except TypeError:
            raise ValueError(f"codec: a region of interest is five integers (y0, x0, h, w, d), got {r!r}")
        if y0 < 0 or x0 < 0 or h < 1 or w < 1 or y0 + h > H or x0 + w > W:
            raise ValueError(f"codec: region of interest {(y0, x0, h, w)} is not inside the {H}x{W} image")
        out.append((y0, x0, h, w, d))
    return out


def roi_map(H: int, W: int, pads, base: int, rois) -> np.ndarray:
    """The quality map of an H x W image padded by ``pads`` = (left, right, top, bottom): int8 [(top + H + bottom) / 16,
    (left + W + right) / 16].  Every cell starts at the step index ``base``; the rectangles (``check_rois``) are
    painted in list order, each onto every cell that holds at least one of its pixels, with clamp(base + d, QSTEP_MIN,
    QSTEP_MAX); later rectangles win, and a cell that lies wholly in the padding keeps ``base``.  Host-only."""
    base = B.check_qstep(base, "codec: ")
    left, right, top, bottom = (int(p) for p in pads)
    PH, PW = top + H + bottom, left + W + right
    if PH % CELL or PW % CELL:
        raise ValueError(f"codec: the padded image {PH}x{PW} is not a whole number of {CELL}-pixel cells")
    m = np.full((PH // CELL, PW // CELL), base, dtype=np.int8)
    for y0, x0, h, w, d in check_rois(rois, H, W):
        k = min(max(base + d, B.QSTEP_MIN), B.QSTEP_MAX)
        m[(top + y0) // CELL:(top + y0 + h - 1) // CELL + 1, (left + x0) // CELL:(left + x0 + w - 1) // CELL + 1] = k
    return m


def clip_rois(rois, y0: int, x0: int, h: int, w: int) -> List[Tuple[int, int, int, int, int]]:
    """the rectangles' parts inside the tile (y0, x0, h, w), in the tile's coordinates and in list order"""
    out = []
    for ry, rx, rh, rw, d in rois:
        a, b = max(ry, y0), min(ry + rh, y0 + h)
        c, e = max(rx, x0), min(rx + rw, x0 + w)
        if a < b and c < e:
            out.append((a - y0, c - x0, b - a, e - c, d))
    return out


# ------------------------------------------------------------------------------------------- error bounds per cell
def check_error_rois(rois, H: int, W: int) -> List[Tuple[int, int, int, int, int]]:
    """``rois`` as a list of (y0, x0, h, w, d) of ints: rectangles of image pixels inside the H x W image, each with
    an absolute error bound d in 0 .. 32 (not an offset).  ValueError otherwise.  Host-only."""
    out = []
    for y0, x0, h, w, d in check_rois(rois, H, W):
        out.append((y0, x0, h, w, R.check_max_error(d, f"codec: error region {(y0, x0, h, w)}: ")))
    return out


def error_map(H: int, W: int, base: int, rois) -> np.ndarray:
    """The bound map of an H x W image: uint8 [gh, gw] over the residual layer's grid (``residual.grid``: 16 x 16-pixel
    cells anchored at pixel (0, 0), no padding).  Every cell starts at the bound ``base``; the rectangles
    (``check_error_rois``) are painted in list order, each onto every cell that holds at least one of its pixels, with
    its own d; later rectangles win.  ``roi_map``'s rules on the unpadded grid.  Host-only."""
    base = R.check_max_error(base, "codec: ")
    if base is None:
        raise ValueError("codec: error_map needs a background bound")
    m = np.full(R.grid(H, W), base, dtype=np.uint8)
    for y0, x0, h, w, d in check_error_rois(rois, H, W):
        m[y0 // R.CELL:(y0 + h - 1) // R.CELL + 1, x0 // R.CELL:(x0 + w - 1) // R.CELL + 1] = d
    return m


# ------------------------------------------------------------------------------------ variance-adaptive quantisation
AQ_STRENGTH_MAX = 4.0  # |strength| of ``--aq``
AQ_MAX_OFFSET = 16     # |offset| to the background step index: two octaves of the step


def check_aq(strength, who: str = "") -> Optional[float]:
    """The strength of the encoder's variance-adaptive quantisation: None and 0 mean off and come back as None;
    otherwise a real number, not a bool, finite, with 0 < |strength| <= AQ_STRENGTH_MAX, as a Python float.
    ValueError otherwise.  Nothing of it travels in a stream."""
    if strength is None:
        return None
    if isinstance(strength, bool) or not isinstance(strength, (int, float, np.integer, np.floating)):
        raise ValueError(f"{who}aq must be a number, got {strength!r}")
    s = float(strength)
    if not (math.isfinite(s) and abs(s) <= AQ_STRENGTH_MAX):
        raise ValueError(f"{who}aq must be finite with |aq| <= {AQ_STRENGTH_MAX}, got {strength!r}")
    return s if s else None


def cell_stats(u8: torch.Tensor, pads: Tuple[int, int, int, int]) -> np.ndarray:
    """device 8-bit [H, W, 3] -> host int32 [gh, gw, 3]: per 16 x 16 cell of the grid of the image padded by ``pads`` =
    (left, right, top, bottom) the number of image pixels in it, the sum of their integer luma and the sum of its
    squares (``icm_image_cell_stats``; pad pixels are not counted).  gh, gw = ceil((top + H + bottom) / 16), ...: with
    ``pads`` = (0, 0, 0, 0) the grid anchored at the image's first pixel."""
    H, W = u8.size(0), u8.size(1)
    left, right, top, bottom = (int(p) for p in pads)
    gh, gw = -(-(top + H + bottom) // CELL), -(-(left + W + right) // CELL)
    out = torch.empty((gh, gw, 3), dtype=torch.int32, device=u8.device)
    check(L.lib().icm_image_cell_stats(u8.data_ptr(), H, W, top, left, gh, gw, out.data_ptr(), L.stream()),
          "image_cell_stats")
    return out.cpu().numpy()


def aq_activity(stats) -> np.ndarray:
    """float64 [gh, gw]: log2(1 + v), v = (n s2 - s1^2) / n^2 the variance of the luma over the cell's image pixels
    (``cell_stats``; the numerator is an exact integer in float64); nan where the cell holds none.  Host-only."""
    s = np.asarray(stats).astype(np.float64)
    n, s1, s2 = s[..., 0], s[..., 1], s[..., 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        act = np.log2(1.0 + (n * s2 - s1 * s1) / (n * n))
    act[n == 0] = np.nan
    return act


def aq_reference(stats) -> float:
    """what "average" means to ``aq_offsets``: the mean activity over the cells that hold a pixel, of the anchored grid
    of the whole image (``cell_stats`` with pads (0, 0, 0, 0)), so that all tiles of a tiled image share it.  Host-only."""
    act = aq_activity(stats)
    return float(np.mean(act[~np.isnan(act)]))


def aq_offsets(stats, strength: float, ref: float) -> np.ndarray:
    """int8 [gh, gw], the cells' offsets to the background step index: clip(rint(4 strength (activity - ref)),
    -AQ_MAX_OFFSET, AQ_MAX_OFFSET), ties to even, 0 where the cell holds no pixel.  The step index has 8 steps per octave
    of the step and a doubled variance is half an octave of amplitude, hence the 4: at strength 1 the step follows the
    cell's standard deviation relative to the reference's.  A rule, not a measured optimum.  Positive strength: flat
    cells finer, busy cells coarser.  Host-only."""
    act = aq_activity(stats)
    d = np.rint(4.0 * float(strength) * (np.where(np.isnan(act), ref, act) - ref))
    return np.clip(d, -AQ_MAX_OFFSET, AQ_MAX_OFFSET).astype(np.int8)


def quality_map(H: int, W: int, pads, base: int, rois, offsets=None) -> np.ndarray:
    """``roi_map`` on a background that varies: every cell starts at clamp(base + offsets[cell], QSTEP_MIN, QSTEP_MAX)
    (``aq_offsets`` of the same grid), then the rectangles are painted as ``roi_map`` paints them, each with
    clamp(base + d): they win over the offsets.  ``offsets`` None: ``roi_map`` itself.  Host-only."""
    m = roi_map(H, W, pads, base, rois)
    if offsets is None:
        return m
    offsets = np.asarray(offsets)
    if offsets.shape != m.shape or offsets.dtype.kind != "i":
        raise ValueError(f"codec: offsets must be integers of the map's size {m.shape}, got {offsets.dtype} "
                         f"{offsets.shape}")
    left, top = int(pads[0]), int(pads[2])
    m = np.clip(int(base) + offsets.astype(np.int64), B.QSTEP_MIN, B.QSTEP_MAX).astype(np.int8)
    for y0, x0, h, w, d in check_rois(rois, H, W):
        k = min(max(int(base) + d, B.QSTEP_MIN), B.QSTEP_MAX)
        m[(top + y0) // CELL:(top + y0 + h - 1) // CELL + 1, (left + x0) // CELL:(left + x0 + w - 1) // CELL + 1] = k
    return m


def search_qstep(fits, lo: int = B.QSTEP_MIN, hi: int = B.QSTEP_MAX) -> Tuple[int, int]:
    """Smallest step index the bisection finds whose encode fits a budget -> (k, number of probes).  ``fits(k)`` makes
    the encode at k and says whether it fits; the size need not be monotone in k, and the guarantee asks for nothing
    of it: fits(k) was seen true, and k == lo or fits(k - 1) was seen false.  ``hi`` is probed first (ValueError if
    even the coarsest step does not fit), then ``lo`` (returned if it fits), then the integers between are bisected
    under the invariant "lo does not fit, hi fits": 2 + ceil(log2(hi - lo)) probes at the most, 8 over -16 .. 32.
    Pure host code."""
    if hi < lo:
        raise ValueError(f"search_qstep: empty range [{lo}, {hi}]")
    probes = 1
    if not fits(hi):
        raise ValueError(f"search_qstep: the budget is out of reach: the encode at the coarsest step, qstep = {hi}, "
                         f"does not fit")
    if hi == lo:
        return hi, probes
    probes += 1
    if fits(lo):
        return lo, probes
    while hi - lo > 1:
        mid = (lo + hi) // 2
        probes += 1
        if fits(mid):
            hi = mid
        else:
            lo = mid
    return hi, probes


@torch.no_grad()
def encode_image_info(model, img, tile: Optional[int] = None, overlap: int = 0, coder: str = "host",
                      symbols_per_wave: Optional[int] = None, qstep: int = 0,
                      max_bytes: Optional[int] = None, roi: Optional[Sequence] = None,
                      rdoq: Optional[float] = None, aq: Optional[float] = None,
                      max_error: Optional[int] = None, error_roi: Optional[Sequence] = None) -> Tuple[bytes, Dict]:
    """``encode_image`` with its outcome: (stream, {"qstep": k, "step": 2^(k/8), "probes": encodes made}); k is the
    background step.  With ``roi`` or ``aq`` also "roi_cells", the number of latent cells (summed over the tiles) whose
    step index differs from k, and "qmap_range": [smallest, largest step index in the maps].  With ``rdoq`` also "rdoq",
    the weight as the kernel took it.  With ``aq`` also "aq", the strength as checked, "aq_ref", the image's reference
    activity, and "aq_offset_range": [smallest, largest offset over all tiles].  With ``max_error`` also "max_error",
    "base_bytes" and "residual_bytes" (the base stream and the residual string inside the ICMR container) and
    "residual_class_range": [smallest, largest context class of the cells].  With ``error_roi`` (``max_error`` is then
    the background's bound) also "max_error_range": [smallest, largest bound in the map] and "error_roi_cells", the
    number of cells whose bound differs from ``max_error``."""
    B.check_coder(coder, "codec: ")
    max_error = R.check_max_error(max_error, "codec: ")
    if error_roi is not None and max_error is None:
        raise ValueError("codec: error_roi gives the exceptions to max_error, the background's bound: give max_error")
    if max_error is not None and max_bytes is not None:
        raise ValueError("codec: give a byte budget or an error bound, not both: the bound decides the size")
    qstep = B.check_qstep(qstep, "codec: ")
    rdoq = B.check_rdoq(rdoq, "codec: ")
    aq = check_aq(aq, "codec: ")
    rd = _rdoq_kw(rdoq)
    if max_bytes is not None:
        if qstep != 0:
            raise ValueError("codec: give a quantiser step or a byte budget, not both")
        if isinstance(max_bytes, bool) or not hasattr(max_bytes, "__index__") or int(max_bytes) < 1:
            raise ValueError(f"codec: max_bytes must be a positive integer, got {max_bytes!r}")
        max_bytes = int(max_bytes)
    arch = _ready(model)
    device = next(model.parameters()).device
    u8 = _as_u8_image(img, device)
    H, W = u8.size(0), u8.size(1)
    if max_error is not None and max(H, W) > B.RESIDUAL_SIDE_MAX:
        raise ValueError(f"codec: max_error takes images of at most {B.RESIDUAL_SIDE_MAX} pixels a side, got {H}x{W}")
    dmap = None if error_roi is None else error_map(H, W, max_error, error_roi)
    if tile is None:
        if overlap:
            raise ValueError("codec: overlap needs a tile extent")
        plan = [(0, 0, H, W)]
    else:
        plan = plan_tiles(H, W, tile, overlap)[2]
    fp = B.fingerprint(model)
    outer = {"arch": arch, "height": H, "width": W, "tile": tile, "overlap": overlap, "fingerprint": fp}
    crops = [u8] if len(plan) == 1 else [u8[y0:y0 + h, x0:x0 + w].contiguous() for y0, x0, h, w in plan]
    # regions of interest: per tile the rectangles clipped to it, in its coordinates; the map of a tile is built from
    # them with the tile's own pads, per probe, and a map that comes out uniform is coded as its scalar step
    rois = None if roi is None else check_rois(roi, H, W)
    tile_rois = [[]] * len(plan) if roi is None else [clip_rois(rois, *t) for t in plan]
    # variance-adaptive quantisation: once per encode the reference activity of the whole image on the grid anchored at
    # its first pixel, and per tile the offsets of its own grid (the tile's pads) against that one reference; the
    # probes of a budget search move k under fixed offsets
    offsets, told = [None] * len(plan), dict(rd)
    if aq is not None:
        aq_ref = aq_reference(cell_stats(u8, (0, 0, 0, 0)))
        offsets = [aq_offsets(cell_stats(c, center_pads(c.size(0), c.size(1))), aq, aq_ref) for c in crops]
        told.update(aq=aq, aq_ref=aq_ref, aq_offset_range=[int(min(o.min() for o in offsets)),
                                                           int(max(o.max() for o in offsets))])

    def maps(k):
        """the tiles' quality maps at the background step k (None: neither rectangles nor offsets were given), and
        what they hold"""
        if roi is None and aq is None:
            return [None] * len(plan), {}
        ms = [quality_map(h, w, center_pads(h, w), k, r, o) for (_, _, h, w), r, o in zip(plan, tile_rois, offsets)]
        return ms, {"roi_cells": int(sum(int((m != k).sum()) for m in ms)),
                    "qmap_range": [int(min(m.min() for m in ms)), int(max(m.max() for m in ms))]}

    def wrap(streams):
        return streams[0] if len(plan) == 1 else B.pack_tiled(outer, streams)

    if max_bytes is None:
        ms, extra = maps(qstep)
        data = wrap([_encode_one(model, arch, fp, c, coder, symbols_per_wave, 0 if m is not None else qstep, m, rdoq)
                     for c, m in zip(crops, ms)])
        told = {"qstep": qstep, "step": B.step_of(qstep)[0], "probes": 1, **extra, **told}
        if max_error is not None:
            # the residual layer: the base decoded on the device as the decoder will decode it, the quantised
            # differences coded as one string, both wrapped.  A bound map that came out uniform gives the symbols of
            # its one bound, and ``pack_residual_map`` writes it as that bound's ICMR stream
            xhat = _decode_device(model, data)[0]
            string, classes = R.encode_residual(u8, xhat, max_error if dmap is None else dmap,
                                                coder_for(coder, symbols_per_wave))
            told.update(max_error=max_error, base_bytes=len(data), residual_bytes=len(string),
                        residual_class_range=list(classes))
            head = {"coder": coder, "height": H, "width": W, "table_crc": R.tables().crc}
            if dmap is not None:
                told.update(max_error_range=[int(dmap.min()), int(dmap.max())],
                            error_roi_cells=int((dmap != max_error).sum()))
            data = (B.pack_residual({**head, "max_error": max_error}, data, string) if dmap is None else
                    B.pack_residual_map(head, data, dmap, string))
        return data, told
    # encode to size: the analysis transform once per tile, then only the latent coder per probe; a probe is the very
    # container that would be written (headers, CRCs and the lanes coder's flushes included), and the answer is the
    # stream of its probe, not a second encode
    tiles = []
    for c in crops:
        pads = center_pads(c.size(0), c.size(1))
        tiles.append((c.size(0), c.size(1), pads, model.analysis(image_u8_to_f32(c, pads))))
    sizes, kept = {}, {}

    def fits(k):
        ms, extra = maps(k)
        data = wrap([_pack_one(arch, fp, h, w, pads,
                               model.compress_latent(y, coder=coder, symbols_per_wave=symbols_per_wave,
                                                     qstep=0 if m is not None else k, qmap=m, **rd), coder)
                     for (h, w, pads, y), m in zip(tiles, ms)])
        sizes[k] = len(data)
        if len(data) <= max_bytes:
            kept.clear()
            kept[k] = (data, extra)
            return True
        return False

    try:
        k, probes = search_qstep(fits)
    except ValueError:
        raise ValueError(f"codec: {max_bytes} bytes are out of reach: the coarsest step (qstep {B.QSTEP_MAX}) still "
                         f"takes {min(sizes.values())} bytes")
    return kept[k][0], {"qstep": k, "step": B.step_of(k)[0], "probes": probes, **kept[k][1], **told}


def encode_image(model, img, tile: Optional[int] = None, overlap: int = 0, coder: str = "host",
                 symbols_per_wave: Optional[int] = None, qstep: int = 0, max_bytes: Optional[int] = None,
                 roi: Optional[Sequence] = None, rdoq: Optional[float] = None, aq: Optional[float] = None,
                 max_error: Optional[int] = None, error_roi: Optional[Sequence] = None) -> bytes:
    """8-bit [H, W, 3] image (tensor on any device, or anything ``numpy.asarray`` accepts) -> one bit-stream.  With
    ``tile``, an image of more than one tile (``plan_tiles``) becomes an ICMT stream whose tile k is
    ``encode_image(model, crop k)``, the tiles coded one after another; an image of one tile is written untiled.
    ``coder`` / ``symbols_per_wave``: as ``model.compress``; every ICMB stream records its coder.
    ``qstep``: step index of a quantiser step on the latent (``model.compress``; 0, the default: none, and the stream
    is what it was before the step existed).  ``max_bytes`` (instead of ``qstep``): the finest step ``search_qstep``
    finds at which the whole stream, of all tiles with one step, has at most that many bytes; ValueError if the
    coarsest step does not get there.  ``encode_image_info`` also returns the step and the number of encodes.
    ``roi``: regions of interest [(y0, x0, h, w, d), ...], rectangles of image pixels inside the image, each with an
    integer offset d to the background step index (negative: finer): the latent cells they touch are coded with
    clamp(k + d) (``roi_map``), k being ``qstep`` or the step the search finds; the map travels in the stream, per
    tile in a tiled one.  No rectangle, or none that changes a cell, gives byte for byte the stream without ``roi``.
    ``rdoq``: weight of rate-distortion optimised quantisation (``model.compress``; None, the default: off, and the
    stream is what it is without).  Every tile and, with ``max_bytes``, every probe of the unchanged search is coded
    with it.  The stream says nothing of it and decodes as any other.
    ``aq``: strength of variance-adaptive quantisation, 0 < |aq| <= AQ_STRENGTH_MAX (None or 0, the default: off, and
    the stream is what it is without): the quality map is derived from the image, each cell's offset to k following the
    variance of its luma against the image's average (``aq_offsets``; positive: flat cells finer, busy cells coarser).
    Rectangles of ``roi`` win over it; a budget search moves k under the fixed offsets; the tiles of a tiled image
    share one reference.  A flat image, or a strength at which every offset rounds to 0, gives the stream without.
    ``max_error``: an integer D in 0 .. 32 (None, the default: off, and the stream is what it is without): the stream
    becomes an ICMR container of the very stream the other arguments give, the base, and the residual string that
    brings every sample of the decode within D of the image's (0: the image itself).  ``coder`` codes that string too.
    Not with ``max_bytes``: ValueError.
    ``error_roi``: exceptions to that bound [(y0, x0, h, w, d), ...], rectangles of image pixels inside the image, each
    with an absolute bound d in 0 .. 32: the 16 x 16-pixel cells of the residual layer's grid they touch are coded under
    d instead of D (``error_map``; later rectangles win), and every sample of the decode lies within its cell's bound
    -- the rectangle bit for bit at d = 0.  The stream is an ICME container, which carries the map; no rectangle, or
    none that changes a cell, gives byte for byte the ICMR stream of D.  Needs ``max_error``: ValueError without."""
    return encode_image_info(model, img, tile, overlap, coder, symbols_per_wave, qstep, max_bytes, roi, rdoq, aq,
                             max_error, error_roi)[0]


def _check_model(header: Dict, arch: str, fp: int, what: str = "the stream") -> None:
    if header["arch"] != arch:
        raise ValueError(f"codec: {what} was written by architecture {header['arch']!r}, the model is {arch!r}")
    if header["fingerprint"] != fp:
        raise ValueError(f"codec: model fingerprint mismatch: {what} was written with entropy tables "
                         f"{header['fingerprint']:#010x}, this checkpoint has {fp:#010x}")


def _check_strings(arch: str, strings, what: str = "this one") -> int:
    """the stream's quantiser step index: two strings, or three with a valid step byte (``B.qstep_from_strings``)"""
    if len(strings) not in (2, 3):
        raise ValueError(f"codec: {arch} streams hold two strings, or three with a quantiser step; {what} holds "
                         f"{len(strings)}")
    try:
        return B.qstep_from_strings(strings)
    except ValueError as e:
        raise ValueError(f"codec: {what}: {e}")


def _check_quality(arch: str, header: Dict, strings, what: str = "this one"):
    """(step index, None) of a stream with a scalar step or none, (None, quality map) of a mapped one"""
    if len(strings) == 3 and len(strings[2]) >= B.QMAP_STRING_MIN:
        try:
            return B.quality_from_strings(strings, header["shape"])
        except ValueError as e:
            raise ValueError(f"codec: {what}: {e}")
    return _check_strings(arch, strings, what), None


def _decompress_one(model, arch: str, header: Dict, strings, coder: str = "host") -> torch.Tensor:
    H, W, pads = header["height"], header["width"], header["pads"]
    k, qmap = B.quality_from_strings(strings, header["shape"])
    x_hat = model.decompress([[strings[0]], [strings[1]]], header["shape"], coder=coder, qstep=k or 0,
                             qmap=qmap)["x_hat"]
    left, right, top, bottom = pads
    if tuple(x_hat.shape) != (1, 3, top + H + bottom, left + W + right):
        raise ValueError(f"codec: latent shape {header['shape']} decodes to {tuple(x_hat.shape)}, not to a padded "
                         f"{H}x{W} image")
    return x_hat


def _check_region(region, H: int, W: int) -> Tuple[int, int, int, int]:
    if region is None:
        return 0, 0, H, W
    try:
        y0, x0, h, w = region
        if any(isinstance(v, bool) or not hasattr(v, "__index__") for v in region):
            raise TypeError
        y0, x0, h, w = int(y0), int(x0), int(h), int(w)
    except (TypeError, ValueError):
        raise ValueError(f"codec: region must be four integers (y0, x0, h, w), got {region!r}")
    if y0 < 0 or x0 < 0 or h < 1 or w < 1 or y0 + h > H or x0 + w > W:
        raise ValueError(f"codec: region {(y0, x0, h, w)} is not inside the {H}x{W} image")
    return y0, x0, h, w


@torch.no_grad()
def decode_image(model, data: bytes, reference=None, region=None) -> Tuple[torch.Tensor, Dict]:
    """one bit-stream, ICMB, ICMT, ICMR or ICME -> (8-bit [H, W, 3] host tensor, info); ``info``: "bpp" = 8 x the whole stream
    length / (H W), header included, and, given ``reference`` (the original 8-bit image), "psnr" of the two 8-bit
    images.  ``region`` = (y0, x0, h, w): only that window is returned ([h, w, 3]; "sse" / "psnr" are over it, against
    the same window of ``reference``); of a tiled stream only the tiles that touch it are decoded
    (``info["tiles_decoded"]``), and the result is bit for bit the same crop of the full decode.  "qstep": the step
    index the stream was coded with (0: none), or the list per tile should they differ; None for a stream (in the
    list: a tile) coded with a quality map, which "qmap" then holds: the int8 map, or of a tiled stream the list per
    tile with None for the tiles of a scalar step.  Streams without a map have no "qmap".
    An ICMR stream: the base is decoded as above (with ``region``, only that region); of a residual string coded with
    the lanes coder only the wave bodies that hold the window's rows, and those that hold their cells' classes, are
    decoded (``residual.region_plan``), into a band of the planes instead of the planes; the residual is applied to
    the window, and a region decode is bit for bit the crop of the full decode.  A window costs whole waves: every row
    of the waves that hold its rows, at full width (rows, not columns).  A host-coded residual string is one chain and
    is decoded whole.  ``info`` is the base's with "bytes" and "bpp" of the whole file, and "max_error", "base_bytes",
    "residual_bytes" and "residual_waves": [the distinct waves of the residual string that decoded anything, its G],
    [G, G] without a region, None for a host-coded string; with ``reference`` also
    "max_abs_error", the largest absolute difference of a sample to the reference's, and "sse" / "psnr" of the final
    image.
    An ICME stream, an ICMR stream with a bound per 16 x 16-pixel cell, decodes the same way, each sample under its own
    cell's bound.  "max_error" is then the largest bound in the map, the file's overall guarantee; "max_error_range":
    [smallest, largest bound]; "max_error_map": the uint8 [gh, gw] map; and with ``reference`` also "bound_violations",
    the number of returned samples farther from the reference's than their cell's bound: 0 for a file that is what it
    says."""
    if B.is_residual(data) or B.is_residual_map(data):
        if B.is_residual_map(data):
            head, base, dmap, string = B.unpack_residual_map(data, R.tables().crc)
        else:
            (head, base, string), dmap = B.unpack_residual(data, R.tables().crc), None
        device = next(model.parameters()).device
        out, _, info, (ry, rx, rh, rw) = _decode_device(model, base, None, region)
        H, W, D = head["height"], head["width"], head["max_error"]
        if (info["height"], info["width"]) != (H, W):
            raise ValueError(f"codec: the ICMR stream holds a {H}x{W} image, its base a {info['height']}x{info['width']}")
        res = R.decode_residual(string, H, W, coder_for(head["coder"]), device, window=(ry, rx, rh, rw))
        out = R.residual_apply(out, res.symbols, (ry, rx, rh, rw), D if dmap is None else dmap, band=res.band,
                               size=(H, W))
        info.update(bytes=len(data), bpp=8.0 * len(data) / (H * W), max_error=D, base_bytes=len(base),
                    residual_bytes=len(string), residual_waves=None if res.waves is None else list(res.waves))
        if dmap is not None:
            info.update(max_error_range=[int(dmap.min()), int(dmap.max())], max_error_map=dmap)
        if reference is not None:
            ref = _as_u8_image(reference, device, "reference")
            if tuple(ref.shape) != (H, W, 3):
                raise ValueError(f"codec: the reference is {ref.size(0)}x{ref.size(1)}, the stream holds a {H}x{W} image")
            d = out.to(torch.int32) - ref[ry:ry + rh, rx:rx + rw].to(torch.int32)
            info["max_abs_error"] = int(d.abs().max().item())
            if dmap is not None:
                # every returned sample against the bound of the cell of its image position
                cells = torch.from_numpy(dmap.astype(np.int32)).to(device)
                ys = torch.arange(ry, ry + rh, device=device) // R.CELL
                xs = torch.arange(rx, rx + rw, device=device) // R.CELL
                info["bound_violations"] = int((d.abs() > cells[ys][:, xs][..., None]).sum().item())
            info["sse"] = int((d.to(torch.int64) ** 2).sum().item())
            info["psnr"] = 10.0 * math.log10(255.0 ** 2 / (info["sse"] / (rh * rw * 3))) if info["sse"] else math.inf
        return out.cpu(), info
    out, sse, info, (ry, rx, rh, rw) = _decode_device(model, data, reference, region)
    if sse is not None:
        info["sse"] = int(sse.item())
        info["psnr"] = 10.0 * math.log10(255.0 ** 2 / (info["sse"] / (rh * rw * 3))) if info["sse"] else math.inf
    return out.cpu(), info


def _decode_device(model, data: bytes, reference=None, region=None):
    """the device-side body of ``decode_image`` for an ICMB or ICMT stream, shared with the encoder of the residual
    layer -> (8-bit [h, w, 3] device tensor of the region, the device scalar of the squared differences to
    ``reference`` or None, info without "sse" / "psnr", the region as checked (y0, x0, h, w)).  The image stays on the
    device."""
    arch = _ready(model)
    fp = B.fingerprint(model)
    device = next(model.parameters()).device
    tiled = B.is_tiled(data)
    if tiled:
        outer, streams = B.unpack_tiled(data)
        _check_model(outer, arch, fp)
        H, W = outer["height"], outer["width"]
        rows, cols, plan = plan_tiles(H, W, outer["tile"], outer["overlap"])
        inner = [B.unpack(s) for s in streams]          # every header checked before any payload is decoded
        coders = [B.coder_of(s) for s in streams]
        quality = []
        for k, ((y0, x0, h, w), (hd, tile_strings)) in enumerate(zip(plan, inner)):
            _check_model(hd, arch, fp, f"tile {k}")
            quality.append(_check_quality(arch, hd, tile_strings, f"tile {k}"))
            if (hd["height"], hd["width"]) != (h, w):
                raise ValueError(f"codec: tile {k} holds a {hd['height']}x{hd['width']} image, the plan has {h}x{w}")
    else:
        header, strings = B.unpack(data)
        coder = B.coder_of(data)
        _check_model(header, arch, fp)
        H, W = header["height"], header["width"]
        quality = [_check_quality(arch, header, strings)]
    ry, rx, rh, rw = _check_region(region, H, W)
    ref = None if reference is None else _as_u8_image(reference, device, "reference")
    if ref is not None and tuple(ref.shape) != (H, W, 3):
        raise ValueError(f"codec: the reference is {ref.size(0)}x{ref.size(1)}, the stream holds a {H}x{W} image")
    if ref is not None and region is not None:
        ref = ref[ry:ry + rh, rx:rx + rw].contiguous()
    qsteps, qmaps = [q[0] for q in quality], [q[1] for q in quality]
    info = {"arch": arch, "height": H, "width": W, "bytes": len(data), "bpp": 8.0 * len(data) / (H * W),
            "qstep": qsteps[0] if len(set(qsteps)) == 1 else qsteps}
    if any(m is not None for m in qmaps):
        info["qmap"] = qmaps if tiled else qmaps[0]
    if tiled:
        sel = [k for k, (y0, x0, h, w) in enumerate(plan)
               if y0 < ry + rh and ry < y0 + h and x0 < rx + rw and rx < x0 + w]
        by, bx = min(plan[k][0] for k in sel), min(plan[k][1] for k in sel)      # the canvas: their bounding box
        bh = max(plan[k][0] + plan[k][2] for k in sel) - by
        bw = max(plan[k][1] + plan[k][3] for k in sel) - bx
        canvas = torch.zeros((3, bh, bw), dtype=torch.float32, device=device)
        m = outer["overlap"]
        ramp = torch.from_numpy(blend_ramp(m)).to(device) if m else None
        for k in sel:                                    # plan order, one stream: a fixed order of additions per pixel
            hd, strings = inner[k]
            x_hat = _decompress_one(model, arch, hd, strings, coders[k])
            image_tile_blend(x_hat, hd["pads"], canvas, plan[k][0] - by, plan[k][1] - bx, ramp,
                             tile_edges(k // cols, k % cols, rows, cols))
        x_hat, top, left = canvas[None], ry - by, rx - bx
        info.update(tile=outer["tile"], overlap=m, tiles=rows * cols, tiles_decoded=len(sel))
    else:
        x_hat = _decompress_one(model, arch, header, strings, coder)
        top, left = header["pads"][2] + ry, header["pads"][0] + rx
    if region is not None:
        info["region"] = [ry, rx, rh, rw]
    out, sse = image_f32_to_u8(x_hat, (left, x_hat.size(3) - left - rw, top, x_hat.size(2) - top - rh), ref)
    return out, sse, info, (ry, rx, rh, rw)


# ------------------------------------------------------------------------------------------------------------ CLI
def read_image_u8(path: str) -> np.ndarray:
    from PIL import Image
    if not os.path.isfile(path):
        raise ValueError(f"{path}: no such file")
    try:
        return np.asarray(Image.open(path).convert("RGB"))
    except OSError as e:       # PIL.UnidentifiedImageError is one
        raise ValueError(f"{path}: not an image ({e})")


def _region(text: str) -> Tuple[int, int, int, int]:
    try:
        v = tuple(int(t) for t in text.split(","))
    except ValueError:
        v = ()
    if len(v) != 4:
        raise argparse.ArgumentTypeError(f"expected Y0,X0,H,W, got {text!r}")
    return v


def _roi(text: str) -> Tuple[int, int, int, int, int]:
    try:
        rect, d = text.split(":")
        v = tuple(int(t) for t in rect.split(",")) + (int(d),)
    except ValueError:
        v = ()
    if len(v) != 5:
        raise argparse.ArgumentTypeError(f"expected Y0,X0,H,W:D, got {text!r}")
    return v


def _residual_base(payload: bytes) -> bytes:
    """the base stream of an ICMR or ICME file, checked; any other payload as it is"""
    if B.is_residual_map(payload):
        return B.unpack_residual_map(payload, R.tables().crc)[1]
    return B.unpack_residual(payload, R.tables().crc)[1] if B.is_residual(payload) else payload


def _qmap_range(qmap) -> List[int]:
    ms = [m for m in (qmap if isinstance(qmap, list) else [qmap]) if m is not None]
    return [int(min(m.min() for m in ms)), int(max(m.max() for m in ms))]


def setup_args() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="icm_amd.codec")
    sub = p.add_subparsers(dest="command", required=True)
    enc = sub.add_parser("encode", help="image file -> bit-stream file")
    enc.add_argument("input", help="image file")
    enc.add_argument("-a", "--architecture", default="cnn", type=str, help="model architecture")
    dec = sub.add_parser("decode", help="bit-stream file -> image file")
    dec.add_argument("input", help="bit-stream file")
    dec.add_argument("-a", "--architecture", default=None, type=str,
                     help="model architecture (default: the stream's; must agree with it)")
    dec.add_argument("--reference", default=None, help="the original image: report the PSNR of the reconstruction")
    dec.add_argument("--region", default=None, type=_region, metavar="Y0,X0,H,W",
                     help="decode only this window of the image (of a tiled stream: only the tiles it touches)")
    enc.add_argument("--tile", default=None, type=int, metavar="N",
                     help="code the image as tiles of N x N pixels (a multiple of 64); one tile: the untiled stream")
    enc.add_argument("--overlap", default=0, type=int, metavar="M",
                     help="pixels neighbouring tiles share, blended by the decoder (needs --tile; at most N / 2)")
    enc.add_argument("--coder", default="host", choices=list(B.CODERS),
                     help="entropy coder of the strings: the host's scalar stream, or lane streams coded on the GPU")
    enc.add_argument("--qstep", default=None, type=int, metavar="K",
                     help=f"quantiser step 2^(K/8) on the latent, K in {B.QSTEP_MIN}..{B.QSTEP_MAX} (0: none; larger: "
                          f"smaller file)")
    enc.add_argument("--target-bytes", default=None, type=int, metavar="N",
                     help="the finest quantiser step at which the file has at most N bytes")
    enc.add_argument("--target-bpp", default=None, type=float, metavar="F",
                     help="the same for floor(F x height x width / 8) bytes")
    enc.add_argument("--roi", default=None, type=_roi, action="append", metavar="Y0,X0,H,W:D",
                     help="region of interest, repeatable: the latent cells this rectangle of image pixels touches are "
                          "coded with the step index K + D (D < 0: finer), K the background step; later ones win")
    enc.add_argument("--rdoq", default=None, type=float, metavar="W",
                     help="rate-distortion optimised quantisation: code a latent element one symbol nearer zero where "
                          "W x the added squared error (in quantiser steps) is less than the bits it saves; W > 0, "
                          "smaller: smaller file (default: off)")
    enc.add_argument("--aq", default=None, type=float, metavar="S",
                     help=f"variance-adaptive quantisation: derive the quality map from the image, each 16 x 16 cell's "
                          f"step index offset by 4 S x (log2 of its luma variance against the image's mean), within "
                          f"+-{AQ_MAX_OFFSET}; S > 0: flat cells finer, busy cells coarser; |S| <= {AQ_STRENGTH_MAX:g} "
                          f"(default: off)")
    enc.add_argument("--max-error", default=None, type=int, metavar="D",
                     help=f"error bound: add a residual layer so that every 8-bit sample of the decode lies within D of "
                          f"the original's, D in 0..{B.MAX_ERROR}; 0: lossless (default: off; not with --target-bytes / "
                          f"--target-bpp)")
    enc.add_argument("--error-roi", default=None, type=_roi, action="append", metavar="Y0,X0,H,W:D",
                     help=f"exception to --max-error, repeatable: the 16 x 16-pixel cells this rectangle of image pixels "
                          f"touches are held to the absolute bound D in 0..{B.MAX_ERROR} instead (0: bit-exact); later ones "
                          f"win (needs --max-error)")
    for s in (enc, dec):
        s.add_argument("-o", "--output", required=True, help="file to write")
        s.add_argument("-p", "--path", dest="paths", required=True, type=str, help="checkpoint path")
    return p


def _load(arch: str, path: str):
    from .eval_model import load_checkpoint
    model = load_checkpoint(arch, path).to("cuda")
    model.update(force=True)
    return model


def main(argv) -> int:
    from .zoo import models
    args = setup_args().parse_args(argv)
    arch = args.architecture
    if arch is not None and (arch not in models or arch not in B.ARCHS):
        known = f"choose from {list(B.ARCHS)}"
        why = "has no bit-stream codec" if arch in models else "is not an architecture"
        print(f"Error: -a {arch}: {why}; {known}.", file=sys.stderr)
        return 2
    if args.command == "encode" and (args.tile is not None or args.overlap):
        try:
            if args.tile is None:
                raise ValueError("--overlap needs --tile")
            B.tile_grid(1, 1, args.tile, args.overlap)
        except ValueError as e:
            print(f"Error: {e}", file=sys.stderr)
            return 2
    if args.command == "encode":
        try:
            if sum(v is not None for v in (args.qstep, args.target_bytes, args.target_bpp)) > 1:
                raise ValueError("give at most one of --qstep, --target-bytes and --target-bpp")
            if args.qstep is not None:
                B.check_qstep(args.qstep, "--")
            if args.target_bytes is not None and args.target_bytes < 1:
                raise ValueError(f"--target-bytes must be at least 1, got {args.target_bytes}")
            if args.target_bpp is not None and not (args.target_bpp > 0 and math.isfinite(args.target_bpp)):
                raise ValueError(f"--target-bpp must be a positive number, got {args.target_bpp}")
            B.check_rdoq(args.rdoq, "--")
            check_aq(args.aq, "--")
            R.check_max_error(args.max_error, "--")
            if args.max_error is not None and (args.target_bytes is not None or args.target_bpp is not None):
                raise ValueError("give --max-error or a byte budget (--target-bytes / --target-bpp), not both")
            if args.error_roi is not None:
                if args.max_error is None:
                    raise ValueError("--error-roi gives the exceptions to --max-error: give --max-error")
                for r in args.error_roi:
                    R.check_max_error(r[4], f"--error-roi {r[0]},{r[1]},{r[2]},{r[3]}: ")
        except ValueError as e:
            print(f"Error: {e}", file=sys.stderr)
            return 2
    try:
        if args.command == "encode":
            payload = read_image_u8(args.input)
            if args.roi is not None:
                try:
                    check_rois(args.roi, *payload.shape[:2])
                except ValueError as e:
                    print(f"Error: --roi: {e}", file=sys.stderr)
                    return 2
            if args.error_roi is not None:
                try:
                    check_error_rois(args.error_roi, *payload.shape[:2])
                except ValueError as e:
                    print(f"Error: --error-roi: {e}", file=sys.stderr)
                    return 2
        else:
            if not os.path.isfile(args.input):
                raise ValueError(f"{args.input}: no such file")
            with open(args.input, "rb") as f:
                payload = f.read()
            inner = _residual_base(payload)
            header, _ = B.unpack_tiled(inner) if B.is_tiled(inner) else B.unpack(inner)
            if arch is not None and arch != header["arch"]:
                print(f"Error: -a {arch} disagrees with the stream, written by {header['arch']!r}.", file=sys.stderr)
                return 2
            arch = header["arch"]
            reference = read_image_u8(args.reference) if args.reference else None
    except ValueError as e:
        print(f"Error: {e}", file=sys.stderr)
        return 4
    if not torch.cuda.is_available():
        print("Error: no GPU (the HIP path has no CPU fallback).", file=sys.stderr)
        return 3
    try:
        model = _load(arch, args.paths)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if args.command == "encode":
            h, w = payload.shape[:2]
            budget = args.target_bytes if args.target_bpp is None else int(math.floor(args.target_bpp * h * w / 8))
            data, found = encode_image_info(model, payload, args.tile, args.overlap, coder=args.coder,
                                            qstep=args.qstep or 0, max_bytes=budget, roi=args.roi, rdoq=args.rdoq,
                                            aq=args.aq, max_error=args.max_error, error_roi=args.error_roi)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            with open(args.output, "wb") as f:
                f.write(data)
            report = {"command": "encode", "arch": arch, "height": h, "width": w, "bytes": len(data),
                      "bpp": 8.0 * len(data) / (h * w), "encode_time": dt, **found}
        else:
            img, info = decode_image(model, payload, reference, args.region)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            from PIL import Image
            Image.fromarray(img.numpy()).save(args.output)
            report = {"command": "decode", **{k: v for k, v in info.items() if k not in ("sse", "qmap", "max_error_map")},
                      "decode_time": dt}
            if "qmap" in info:
                report["qmap_range"] = _qmap_range(info["qmap"])
    except (ValueError, FileNotFoundError) as e:
        print(f"Error: {e}", file=sys.stderr)
        return 4
    print(json.dumps(report))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
