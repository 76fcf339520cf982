"""Container of one compressed image: the bytes ``python -m icm_amd.codec`` writes and reads.

Parity unpinned: no counterpart in the reference (upstream CompressAI's ``examples/codec.py`` is not in its tree), so
the layout below is this project's own.  Pure Python; importing it needs neither torch nor the HIP library.

Layout -- fixed-width little-endian integers, no padding between fields:

    offset  size  field
         0     4  magic, the bytes ``ICMB``
         4     2  format version (u16), ``VERSION`` = 1
         6     2  low byte: architecture id, index into ``ARCHS`` = ("cnn", "stf"); high byte: coder id, index into
                  ``CODERS`` = ("host", "lanes"): what kind of stream every string is (see "lane stream" below).
                  Files of the host coder have a zero high byte, as before the field was split, and a reader from
                  before refuses a lanes file as an unknown architecture id
         8     4  original image height (u32, >= 1)
        12     4  original image width (u32, >= 1)
        16     8  pad amounts left, right, top, bottom (4 x u16): what the encoder added around the image
        24     4  latent ``shape``: z height, z width (2 x u16), the ``shape`` entry of ``compress()``
        28     4  model fingerprint (u32), see ``fingerprint``
        32     2  number of strings n (u16)
        34   4 n  length of each string (u32), in the order of ``compress()["strings"]`` flattened
                  (cnn / stf: the y string, then the z string)
    34 + 4 n   ...  the strings, back to back
       end-4     4  CRC-32 (``zlib.crc32``) of every byte before it

A stream of two strings therefore carries ``HEADER_BYTES_2`` = 46 bytes besides its payloads, and the file size is
what ``bpp`` is computed from.  ``unpack`` raises ``ValueError`` -- and nothing else -- for anything that is not
exactly one such stream; each message names the condition that failed.

Quantiser step -- a stream coded with a step on the latent y (``step_of``: step index k in ``QSTEP_MIN`` .. ``QSTEP_MAX``
= -16 .. 32, step = 2^(k/8); k = 0 is no step) carries a third string of exactly one byte after the y and z strings:
k as a signed byte (``qstep_string`` / ``qstep_from_strings``).  It is written only when k != 0 -- a stream without a
step is byte for byte what it was before the step existed -- and a stored 0, a k outside the range or a third string
of another length is refused, so one content has one encoding.  Only k is stored; both sides derive the two floats
the kernels use from it.  The fixed header, the version and the coder ids are unchanged: a reader from before the step
refuses a stepped stream for its string count ("holds 3", exit code 4 of the CLI) instead of decoding garbage.

Quality map -- a stream whose step varies over the latent (region-of-interest coding) carries as its third string a
map string instead of the step byte: one step index per latent position (a 16 x 16-pixel cell of the padded image),
shared by all channels, run-length coded in row-major order (``qmap_string`` / ``qmap_from_string``):

    u16 h, u16 w                       the latent's spatial size; must equal 4 x the header's z shape
    then runs (u16 count >= 1, i8 k)   row-major, covering h w positions exactly

The string is canonical: runs are maximal (neighbouring runs differ in k, except that a run of 65535 may be followed by
one of the same k), every k lies in ``QSTEP_MIN`` .. ``QSTEP_MAX``, and at least two distinct k occur -- a map whose
entries are all k is written as the scalar stream of k (no third string for k = 0), so one content keeps one encoding.
The shortest map string has ``QMAP_STRING_MIN`` = 10 bytes, and a reader tells the two kinds of third string apart by
their length (``quality_from_strings``).  A wrong size against the header, a count of 0, runs short of or past h w,
trailing bytes, a non-maximal run, a k outside the range or a single distinct k is refused.  ``qstep_from_strings`` is
what it was: a reader from before the map refuses a mapped stream there ("must be one byte", exit code 4 of the CLI).
The kernels take a map byte as an index into a table of 256 (step, inv) pairs, ``step_table``, built from ``step_of``.

Rate-distortion optimised quantisation (``check_rdoq``, ``code_length_table``) is the encoder's own business: it picks
between two ordinary symbols per element, so nothing of it is stored and every stream above reads as it did.

A tiled image is a second container with its own magic: a grid of independently coded tiles (``tile_grid`` below gives
the grid), each of them one complete ``ICMB`` stream.  ``ICMB`` and ``unpack`` are unchanged by it, and each reader
refuses the other's files for their magic.

    offset  size  field
         0     4  magic, the bytes ``ICMT``
         4     2  format version (u16), ``TILED_VERSION`` = 1
         6     2  architecture id (u16), index into ``ARCHS``
         8     4  image height (u32, >= 1)
        12     4  image width (u32, >= 1)
        16     2  tile extent (u16): a multiple of 64 in 64..32768
        18     2  overlap of neighbouring tiles in pixels (u16), 2 x overlap <= extent
        20     2  rows of the tile grid (u16)
        22     2  cols of the tile grid (u16)
        24     4  model fingerprint (u32)
        28  4 rows cols  length of each tile stream (u32), row-major
       ...   ...  the tile streams, back to back
       end-4     4  CRC-32 of every byte before it

rows / cols are redundant with the four numbers before them, and a reader refuses a file in which they disagree.
The coder id lives in the tile streams alone: the high byte of the ICMT architecture field stays zero.  So does the
quantiser step: every tile stream of a stepped image carries its own byte (the encoder writes the same k in all), and
every tile of a region-of-interest encode its own map string, or the step byte where its map came out uniform.

An error-bounded image is a third container with its own magic: one ordinary stream, ``ICMB`` or ``ICMT``, the base,
followed by the string of the residual layer (``icm_amd.residual``: the quantised differences between the original and
the decoder's reconstruction of the base, which bound the error of every sample by D).

    offset  size  field
         0     4  magic, the bytes ``ICMR``
         4     2  format version (u16), ``RESIDUAL_VERSION`` = 1
         6     1  D (u8), 0..``MAX_ERROR`` = 32: every sample of the decode is within D of the original; 0 = lossless
         7     1  coder id of the residual string (u8), index into ``CODERS``; the base names its own
         8     4  image height (u32, 1..32768)
        12     4  image width (u32, 1..32768)
        16     4  CRC-32 of the residual layer's static tables (cdf, sizes, offsets as little-endian int32)
        20     4  length of the base stream (u32)
        24     4  length of the residual string (u32)
        28   ...  the base stream, then the residual string
       end-4     4  CRC-32 of every byte before it

``unpack_residual`` refuses, with ValueError, anything that is not exactly one such stream, a D above 32, a base that
begins with neither inner magic and -- given the reader's own table CRC -- a file written with other tables, so that a
reader built with other tables stops instead of decoding garbage.  ``unpack`` and ``unpack_tiled`` are unchanged and
refuse the magic, as a reader from before this container does (exit code 4 of the CLI).  The residual string is one
string of four runs under the layer's tables: the class map, then the R, G and B planes.  Coded as a lane stream it can
be decoded in part without any change to these bytes: its G wave bodies share nothing, and body g holds the elements
[g c, min(n, (g + 1) c)) of every run of n (c: the lane stream's share per wave, below), so the rows of a window are a
range of bodies, the same for the three planes, and their cells' classes another range of the class run
(``icm_amd.residual.region_plan``; a decoder hands a body its runs in order, none skipped).

An error-bounded image whose bound varies over the picture is a fourth container with its own magic: the bound is one
byte per 16 x 16-pixel cell of the residual layer's grid (``error_grid``: anchored at pixel (0, 0) of the whole image,
tiled base or not; edge cells partial), every sample of the decode lies within its own cell's bound, and the cells at
0 come back bit for bit.  ``ICMR``, ``pack_residual`` and ``unpack_residual`` are unchanged by it.

    offset  size  field
         0     4  magic, the bytes ``ICME``
         4     2  format version (u16), ``RESIDUAL_MAP_VERSION`` = 1
         6     1  the largest bound in the map (u8, <= ``MAX_ERROR``): the file's overall guarantee
         7     1  coder id of the residual string (u8), index into ``CODERS``; the base names its own
         8     4  image height (u32, 1..32768)
        12     4  image width (u32, 1..32768)
        16     4  CRC-32 of the residual layer's static tables
        20     4  length of the base stream (u32)
        24     4  length of the bound-map string (u32)
        28     4  length of the residual string (u32)
        32   ...  the base stream, the bound-map string, the residual string
       end-4     4  CRC-32 of every byte before it

The bound-map string is run-length coded like the quality map (``error_map_string`` / ``error_map_from_string``):

    u16 gh, u16 gw                     the grid; must be ``error_grid`` of the header's height and width
    then runs (u16 count >= 1, u8 d)   row-major, covering gh gw cells exactly

and canonical in the same way: runs are maximal (except after a run of 65535), every d is at most 32, and at least two
distinct d occur -- ``pack_residual_map`` writes a map whose entries are all D as the ``ICMR`` stream of D, byte for
byte, so one content keeps one encoding.  ``unpack_residual_map`` refuses, with ValueError, what ``unpack_residual``
refuses and a wrong grid against the header, a header maximum that is not the map's, a count of 0, runs short of or
past the grid, a non-maximal run, a d above 32, a single distinct d and trailing bytes.  ``unpack_residual`` refuses
the new magic, as a reader from before this container does (exit code 4 of the CLI), and ``unpack_residual_map`` an
``ICMR`` stream.  The residual string is what it is in an ``ICMR`` stream; only the quantiser behind its symbols
differs from cell to cell.

Lane stream -- the string format of coder id 1, made to be coded by one GPU wave per body (csrc/rans_lanes.hip; the
executable definition is csrc/rans_lanes_common.h, the arithmetic of a lane's step that host and kernels both compile,
under the loops of ``icm_rans_lanes_encode`` / ``icm_rans_lanes_decoder_*`` of csrc/rans.cpp).  Parity unpinned: no
counterpart in the reference.  A stream codes R runs; run r holds n_r (symbol, CDF index) pairs -- the y string
one run per slice in slice order, each flat in (n, c, h, w) order, a z string one run -- with the tables, offsets and
sizes of the host coder (16-bit precision, the last bin of a table is the escape bin).

    offset  size  field
         0     4  magic, the bytes ``ICML``
         4     2  version (u16) = 1
         6     2  G = number of waves (u16, 1..4096)
         8   4 G  byte length of each wave body (u32); each >= 256 and even
       ...   ...  the G bodies, back to back; nothing after them
    body:  64 x u32  the decoder's initial state of lanes 0..63 (little-endian)
           then u16 words in the order the decoder reads them

G = clamp(ceil(max_r n_r / symbols_per_wave), 1, 4096), chosen by the encoder; the decoder takes it from the stream.
With c_r = ceil(n_r / G) rounded up to a multiple of 64, wave g owns elements [g c_r, min(n_r, (g + 1) c_r)) of run r
(possibly none) and in step t its lane l handles element g c_r + 64 t + l, idle when that lies past the end.  States
and the word cursor carry over from run to run: a lane is flushed once per stream.  Per lane a 32-bit rANS state with
16-bit words and L = 2^16: the encoder's put of (start, freq) out of 2^16 emits ``x & 0xFFFF`` and shifts x right by
16 if x >= freq << 16, then sets x = ((x / freq) << 16) + x % freq + start; the decoder takes cum = x & 0xFFFF, finds
s with cdf[s] <= cum < cdf[s + 1], sets x = freq (x >> 16) + cum - start and, if x < L, x = (x << 16) | next word.
A step has four phases: the table symbol of every active lane, then -- for the lanes whose symbol fell in the escape
bin only -- bits 0-15, 16-31 and 32-47 of the escape value (the host coder's zig-zag: -2 v - 1 below the table,
2 (v - overflow) above it), each a put with freq = 1 and start = the 16 bits.  Within a phase the lanes that read a
word take consecutive words in ascending lane order.  The encoder is the mirror: runs, steps and phases backwards
from x = L, words written downwards.  A valid body leaves every decoder lane at exactly L with the cursor at its end;
an escape whose symbol does not fit int32 is an error.  The format costs about 4 + 260 G bytes per string.
"""
from __future__ import annotations

import math
import struct
import zlib
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MAGIC = b"ICMB"
VERSION = 1
ARCHS = ("cnn", "stf")
CODERS = ("host", "lanes")                  # high byte of the architecture field

_FIXED = struct.Struct("<4sHHII4H2HIH")     # magic .. number of strings
_U32 = struct.Struct("<I")
FIXED_BYTES = _FIXED.size                   # 34
CRC_BYTES = 4
HEADER_BYTES_2 = FIXED_BYTES + 2 * 4 + CRC_BYTES   # everything but the payloads of a two-string stream
assert FIXED_BYTES == 34 and HEADER_BYTES_2 == 46

U16_MAX, U32_MAX = 0xFFFF, 0xFFFFFFFF
HEADER_KEYS = ("arch", "height", "width", "pads", "shape", "fingerprint")


def _uint(name: str, v, hi: int, lo: int = 0) -> int:
    if isinstance(v, bool) or not isinstance(v, int) and not hasattr(v, "__index__"):
        raise ValueError(f"bitstream: {name} must be an integer, got {v!r}")
    v = int(v)
    if not lo <= v <= hi:
        raise ValueError(f"bitstream: {name} = {v} outside [{lo}, {hi}]")
    return v


def check_coder(coder, who: str = "") -> str:
    """``coder`` if CODERS names it, ValueError otherwise: the one check of a coder's name (``icm_amd.ans`` imports
    CODERS and this check from here, the module that defines what the names mean in a stream)"""
    if coder not in CODERS:
        raise ValueError(f"{who}unknown coder {coder!r}; choose from {list(CODERS)}")
    return coder


def pack(header: Dict, strings: Sequence[bytes], coder: str = "host") -> bytes:
    """``header``: {"arch": name in ARCHS, "height", "width", "pads": (left, right, top, bottom),
    "shape": (z height, z width), "fingerprint": u32}; ``strings``: the flattened ``compress()["strings"]``;
    ``coder``: the name in CODERS that made them."""
    check_coder(coder, "bitstream: ")
    missing = [k for k in HEADER_KEYS if k not in header]
    if missing:
        raise ValueError(f"bitstream: header lacks {missing}")
    if header["arch"] not in ARCHS:
        raise ValueError(f"bitstream: unknown architecture {header['arch']!r}; the format knows {list(ARCHS)}")
    pads, shape = tuple(header["pads"]), tuple(header["shape"])
    if len(pads) != 4 or len(shape) != 2:
        raise ValueError("bitstream: pads must have four entries and shape two")
    strings = [bytes(s) for s in strings]
    n = _uint("number of strings", len(strings), U16_MAX)
    out = bytearray(_FIXED.pack(
        MAGIC, VERSION, ARCHS.index(header["arch"]) | CODERS.index(coder) << 8,
        _uint("height", header["height"], U32_MAX, 1), _uint("width", header["width"], U32_MAX, 1),
        *(_uint("pad", p, U16_MAX) for p in pads), *(_uint("shape", s, U16_MAX) for s in shape),
        _uint("fingerprint", header["fingerprint"], U32_MAX), n))
    for s in strings:
        out += _U32.pack(_uint("string length", len(s), U32_MAX))
    for s in strings:
        out += s
    out += _U32.pack(zlib.crc32(bytes(out)) & U32_MAX)
    return bytes(out)


def _arch_field(field: int) -> Tuple[int, int]:
    """(architecture id, coder id) of the u16 field, both known to this reader"""
    arch_id, coder_id = field & 0xFF, field >> 8
    if coder_id >= len(CODERS):
        raise ValueError(f"bitstream: unknown coder id {coder_id} (this reader knows 0..{len(CODERS) - 1})")
    if arch_id >= len(ARCHS):
        raise ValueError(f"bitstream: unknown architecture id {arch_id} (this reader knows 0..{len(ARCHS) - 1})")
    return arch_id, coder_id


def coder_of(data: bytes) -> str:
    """name of the coder that made the strings of an ICMB stream (``unpack`` does not report it: its header dict is
    unchanged).  Looks at the magic, the version and the field alone; ValueError for anything else."""
    data = bytes(data[:FIXED_BYTES]) if isinstance(data, (bytes, bytearray, memoryview)) else b""
    if len(data) < 8 or data[:4] != MAGIC:
        raise ValueError("bitstream: bad magic (not an ICMB stream)")
    version, field = struct.unpack_from("<HH", data, 4)
    if version != VERSION:
        raise ValueError(f"bitstream: unknown format version {version} (this reader knows {VERSION})")
    return CODERS[_arch_field(field)[1]]


def unpack(data: bytes) -> Tuple[Dict, List[bytes]]:
    """inverse of ``pack``: (header, strings).  ValueError for a bad magic, an unknown version, architecture or coder
    id, a declared length that runs past the data, trailing bytes or a CRC mismatch.  The coder: ``coder_of``."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise ValueError(f"bitstream: expected bytes, got {type(data).__name__}")
    data = bytes(data)
    if not MAGIC.startswith(data[:4]):
        raise ValueError("bitstream: bad magic (not an ICMB stream)")
    if len(data) < FIXED_BYTES + CRC_BYTES:
        raise ValueError(f"bitstream: truncated: {len(data)} bytes, the fixed header and CRC need {FIXED_BYTES + CRC_BYTES}")
    (_, version, arch_id, height, width, pl, pr, pt, pb, zh, zw, fp, n) = _FIXED.unpack_from(data, 0)
    if version != VERSION:
        raise ValueError(f"bitstream: unknown format version {version} (this reader knows {VERSION})")
    arch_id, _ = _arch_field(arch_id)
    if height < 1 or width < 1:
        raise ValueError(f"bitstream: empty image {height}x{width}")
    pos = FIXED_BYTES + 4 * n
    if pos + CRC_BYTES > len(data):
        raise ValueError(f"bitstream: truncated: the length table of {n} strings runs past the data")
    lengths = [_U32.unpack_from(data, FIXED_BYTES + 4 * i)[0] for i in range(n)]
    end = pos + sum(lengths)
    if end + CRC_BYTES > len(data):
        raise ValueError(f"bitstream: truncated: declared string lengths {lengths} run past the data "
                         f"({len(data)} bytes, {end + CRC_BYTES} needed)")
    if end + CRC_BYTES < len(data):
        raise ValueError(f"bitstream: {len(data) - end - CRC_BYTES} trailing bytes after the CRC")
    crc = _U32.unpack_from(data, end)[0]
    if crc != zlib.crc32(data[:end]) & U32_MAX:
        raise ValueError("bitstream: CRC mismatch (corrupt stream)")
    strings = []
    for ln in lengths:
        strings.append(data[pos:pos + ln])
        pos += ln
    header = {"arch": ARCHS[arch_id], "height": height, "width": width, "pads": (pl, pr, pt, pb), "shape": (zh, zw),
              "fingerprint": fp}
    return header, strings


# ------------------------------------------------------------------------------------------------- quantiser step
QSTEP_MIN, QSTEP_MAX = -16, 32              # step index k: step = 2^(k/8), 0.25 .. 16; 0 = no step


def check_qstep(k, who: str = "") -> int:
    """``k`` as an int if it is an integer in [QSTEP_MIN, QSTEP_MAX], ValueError otherwise"""
    if isinstance(k, bool) or not isinstance(k, int) and not hasattr(k, "__index__"):
        raise ValueError(f"{who}qstep must be an integer, got {k!r}")
    k = int(k)
    if not QSTEP_MIN <= k <= QSTEP_MAX:
        raise ValueError(f"{who}qstep = {k} outside [{QSTEP_MIN}, {QSTEP_MAX}]")
    return k


def step_of(k) -> Tuple[float, float]:
    """(step, inv) of step index k, each the value of an f32: step = f32(2^(k/8)), inv = f32(1 / step).  The one place
    the two floats the kernels take are derived; encoder and decoder both call it, and only k is stored."""
    k = check_qstep(k, "bitstream: ")
    step = struct.unpack("<f", struct.pack("<f", 2.0 ** (k / 8)))[0]
    return step, struct.unpack("<f", struct.pack("<f", 1.0 / step))[0]


def qstep_string(k) -> bytes:
    """the third string of a stepped stream: k as one signed byte.  k = 0 has no string (ValueError)."""
    k = check_qstep(k, "bitstream: ")
    if k == 0:
        raise ValueError("bitstream: qstep 0 is written as no string at all")
    return struct.pack("<b", k)


def qstep_from_strings(strings: Sequence[bytes]) -> int:
    """step index of the flattened strings of a cnn / stf stream: 0 for two strings, the signed byte for three.
    ValueError for any other count, a third string that is not one byte, a k outside the range, or a stored 0."""
    if len(strings) == 2:
        return 0
    if len(strings) != 3:
        raise ValueError(f"bitstream: a stream holds two strings, or three with a quantiser step; this one holds "
                         f"{len(strings)}")
    if len(strings[2]) != 1:
        raise ValueError(f"bitstream: the quantiser-step string must be one byte, this one has {len(strings[2])}")
    k = check_qstep(struct.unpack("<b", bytes(strings[2]))[0], "bitstream: stored ")
    if k == 0:
        raise ValueError("bitstream: a stored qstep of 0 (a stream without a step has two strings)")
    return k


# ------------------------------------------------------------------------------ rate-distortion optimised quantisation
def check_rdoq(w, who: str = "") -> Optional[float]:
    """The weight of the encoder's rate-distortion optimised quantisation: None (off) passes through; otherwise ``w``
    must be a real number, not a bool, that is finite and > 0 once rounded to f32, and that f32 value comes back as a
    Python float (what the kernel is given).  ValueError otherwise.  Nothing of it travels in a stream."""
    if w is None:
        return None
    if isinstance(w, bool) or not isinstance(w, (int, float, np.integer, np.floating)):
        raise ValueError(f"{who}rdoq must be a positive number, got {w!r}")
    try:
        v = struct.unpack("<f", struct.pack("<f", float(w)))[0]
    except (OverflowError, struct.error):
        v = math.inf
    if not (math.isfinite(v) and v > 0.0):
        raise ValueError(f"{who}rdoq must be finite and > 0 as an f32, got {w!r}")
    return v


def code_length_table(cdf, sizes) -> np.ndarray:
    """The code lengths the entropy coder's tables imply, as the encoder's RDOQ kernel reads them: float32 of the shape
    of ``cdf`` ([rows, stride], the quantised CDFs out of 2^16), bits[r][v] = f32(16 - log2(f64(cdf[r][v + 1] -
    cdf[r][v]))) for v < sizes[r] - 2 -- the table proper without its escape bin -- and 0 elsewhere (never read).
    Computed in float64 and rounded once.  Pure host code; ValueError for shapes that do not fit or a bin of no width."""
    cdf = np.asarray(cdf)
    sizes = np.asarray(sizes).reshape(-1)
    if cdf.ndim != 2 or cdf.dtype.kind not in "iu" or sizes.dtype.kind not in "iu" or len(sizes) != cdf.shape[0]:
        raise ValueError(f"bitstream: code_length_table takes integer CDFs [rows, stride] and a size per row, got "
                         f"{cdf.dtype} {cdf.shape} and {sizes.dtype} {sizes.shape}")
    if cdf.shape[0] and (int(sizes.min()) < 2 or int(sizes.max()) > cdf.shape[1]):
        raise ValueError(f"bitstream: CDF sizes must lie in 2 .. {cdf.shape[1]}, the stride")
    width = np.diff(cdf.astype(np.int64), axis=1)
    inside = np.arange(cdf.shape[1] - 1)[None, :] < (sizes.astype(np.int64) - 2)[:, None]
    if bool((width[inside] < 1).any()):
        raise ValueError("bitstream: a CDF holds a bin of no width inside its table")
    bits = np.zeros(cdf.shape, dtype=np.float32)
    bits[:, :-1][inside] = (16.0 - np.log2(width[inside].astype(np.float64))).astype(np.float32)
    return bits


# ------------------------------------------------------------------------------------------------- quality map
_MAP_HEAD = struct.Struct("<HH")            # h, w
_MAP_RUN = struct.Struct("<Hb")             # count, k
QMAP_STRING_MIN = _MAP_HEAD.size + 2 * _MAP_RUN.size        # two runs: the shortest string of a non-uniform map
assert QMAP_STRING_MIN == 10


def check_qmap(qmap, shape, qstep=0, who: str = "") -> np.ndarray:
    """``qmap`` as a C-contiguous int8 host array if it is a 2-D integer array or tensor of exactly ``shape`` (the
    latent's spatial size) with every entry in [QSTEP_MIN, QSTEP_MAX] and ``qstep`` is 0; ValueError otherwise.  The
    one check of a quality map: the kernels index their step table with its bytes and check nothing."""
    if check_qstep(qstep, who) != 0:
        raise ValueError(f"{who}give a quality map or a quantiser step, not both (qstep = {qstep})")
    if hasattr(qmap, "detach") and hasattr(qmap, "cpu"):       # a tensor, on any device
        qmap = qmap.detach().cpu().numpy()
    a = np.asarray(qmap)
    if a.dtype.kind not in "iu":
        raise ValueError(f"{who}qmap must hold integers, got dtype {a.dtype}")
    if a.ndim != 2 or tuple(a.shape) != tuple(int(s) for s in shape):
        raise ValueError(f"{who}qmap must have the latent's spatial size {tuple(int(s) for s in shape)}, got "
                         f"{tuple(a.shape)}")
    if a.size == 0:
        raise ValueError(f"{who}qmap is empty")
    lo, hi = int(a.min()), int(a.max())
    if lo < QSTEP_MIN or hi > QSTEP_MAX:
        raise ValueError(f"{who}qmap holds {lo if lo < QSTEP_MIN else hi}, outside [{QSTEP_MIN}, {QSTEP_MAX}]")
    return np.ascontiguousarray(a, dtype=np.int8)


def uniform_qmap(qmap: np.ndarray) -> Optional[int]:
    """k if every entry of a checked map is k (such a map *is* the scalar step k), None otherwise"""
    k = int(qmap.flat[0])
    return k if bool((qmap == k).all()) else None


def step_table() -> np.ndarray:
    """the kernels' table: float32 [256, 2], row b = ``step_of(k)`` for the map byte b read as unsigned (k = b below
    128, b - 256 from there), (1, 1) for the bytes that are no valid k.  No byte indexes outside it."""
    t = np.ones((256, 2), dtype=np.float32)
    for k in range(QSTEP_MIN, QSTEP_MAX + 1):
        t[k & 0xFF] = step_of(k)
    return t


def qmap_string(qmap) -> bytes:
    """the third string of a mapped stream.  A uniform map has none (ValueError): it is written as its scalar step."""
    a = np.asarray(qmap)
    a = check_qmap(a, a.shape, 0, "bitstream: ")
    h, w = _uint("map height", a.shape[0], U16_MAX, 1), _uint("map width", a.shape[1], U16_MAX, 1)
    if uniform_qmap(a) is not None:
        raise ValueError(f"bitstream: a uniform quality map (every entry {int(a.flat[0])}) is written as the quantiser "
                         f"step, not as a map string")
    flat = a.reshape(-1)
    starts = np.flatnonzero(np.concatenate(([True], flat[1:] != flat[:-1])))
    ends = np.append(starts[1:], flat.size)
    out = bytearray(_MAP_HEAD.pack(h, w))
    for s, e in zip(starts.tolist(), ends.tolist()):
        n, k = e - s, int(flat[s])
        while n > 0:                                # a maximal run longer than a count holds: full counts first
            c = min(n, U16_MAX)
            out += _MAP_RUN.pack(c, k)
            n -= c
    return bytes(out)


def qmap_from_string(data: bytes, shape) -> np.ndarray:
    """inverse of ``qmap_string`` -> int8 [h, w]; ``shape``: the header's z shape, which the map must be 4 x of.
    ValueError, naming the condition, for anything that is not the one canonical string of such a map."""
    data = bytes(data)
    zh, zw = (int(s) for s in shape)
    if len(data) < QMAP_STRING_MIN:
        raise ValueError(f"bitstream: a quality-map string has at least {QMAP_STRING_MIN} bytes, this one has {len(data)}")
    h, w = _MAP_HEAD.unpack_from(data, 0)
    if (h, w) != (4 * zh, 4 * zw):
        raise ValueError(f"bitstream: the quality map is {h}x{w}, the header's latent is {4 * zh}x{4 * zw}")
    if (len(data) - _MAP_HEAD.size) % _MAP_RUN.size:
        raise ValueError(f"bitstream: {(len(data) - _MAP_HEAD.size) % _MAP_RUN.size} trailing bytes after the last "
                         f"whole run of the quality map")
    total, flat, pos, prev = h * w, np.empty(h * w, dtype=np.int8), 0, None
    for off in range(_MAP_HEAD.size, len(data), _MAP_RUN.size):
        if pos == total:
            raise ValueError(f"bitstream: {len(data) - off} trailing bytes after the quality map's {total} positions")
        count, k = _MAP_RUN.unpack_from(data, off)
        if count == 0:
            raise ValueError("bitstream: a run of the quality map has a count of 0")
        check_qstep(k, "bitstream: quality map: stored ")
        if prev is not None and prev[1] == k and prev[0] != U16_MAX:
            raise ValueError(f"bitstream: the quality map's runs are not maximal: a run of {prev[0]} is followed by "
                             f"another of the same k = {k}")
        if pos + count > total:
            raise ValueError(f"bitstream: the quality map's runs go past its {total} positions")
        flat[pos:pos + count] = k
        pos, prev = pos + count, (count, k)
    if pos != total:
        raise ValueError(f"bitstream: the quality map's runs cover {pos} of its {total} positions")
    if bool((flat == flat[0]).all()):
        raise ValueError(f"bitstream: the quality map holds a single k = {int(flat[0])} (a uniform map is written as "
                         f"the quantiser step)")
    return flat.reshape(h, w)


def quality_from_strings(strings: Sequence[bytes], shape) -> Tuple[Optional[int], Optional[np.ndarray]]:
    """(k, None) of a stream with a scalar step or none (``qstep_from_strings``), (None, map) of a mapped one; the two
    kinds of third string are told apart by length.  ``shape``: the header's z shape."""
    if len(strings) == 3 and len(strings[2]) >= QMAP_STRING_MIN:
        return None, qmap_from_string(strings[2], shape)
    return qstep_from_strings(strings), None


def fingerprint(model) -> int:
    """CRC-32 over the integer tables the entropy coder works from: ``_quantized_cdf``, ``_cdf_length``, ``_offset`` of
    ``model.entropy_bottleneck`` and then of ``model.gaussian_conditional``, each copied to the host as little-endian
    int32.  Call it after ``update(force=True)``.  The tables are exact integer work and depend on the trained entropy
    parameters, so a decoder that holds another checkpoint is told so before it touches the payload.  It covers the
    entropy parameters only: two checkpoints that differ in their transforms alone share a fingerprint."""
    crc = 0
    for mod in (model.entropy_bottleneck, model.gaussian_conditional):
        for name in ("_quantized_cdf", "_cdf_length", "_offset"):
            t = getattr(mod, name)
            if t.numel() == 0:
                raise ValueError("fingerprint: the entropy tables are empty; call model.update(force=True) first")
            crc = zlib.crc32(t.detach().cpu().numpy().astype("<i4").tobytes(), crc)
    return crc & U32_MAX


# ------------------------------------------------------------------------------------------------- tiled images
TILED_MAGIC = b"ICMT"
TILED_VERSION = 1
TILE_MIN, TILE_MAX = 64, 32768              # extents: multiples of TILE_MIN (the codec pads every tile to one)
_TFIXED = struct.Struct("<4sHHIIHHHHI")     # magic .. fingerprint
TILED_FIXED_BYTES = _TFIXED.size            # 28
assert TILED_FIXED_BYTES == 28
TILED_HEADER_KEYS = ("arch", "height", "width", "tile", "overlap", "fingerprint")


def tile_grid(height: int, width: int, tile: int, overlap: int) -> Tuple[int, int]:
    """(rows, cols) of the tile plan.  Per axis of length L, with extent E = tile, overlap m and stride S = E - m:
    n = max(1, ceil((L - m) / S)) tiles at origins k S with sizes min(E, L - k S).  Neighbours share exactly m pixels,
    every tile is wider than m and a pixel lies in at most two tiles per axis.  ValueError unless tile is a multiple of
    64 in 64..32768 and 0 <= 2 overlap <= tile."""
    height, width = _uint("height", height, U32_MAX, 1), _uint("width", width, U32_MAX, 1)
    tile, overlap = _uint("tile", tile, TILE_MAX, TILE_MIN), _uint("overlap", overlap, TILE_MAX)
    if tile % TILE_MIN:
        raise ValueError(f"bitstream: tile = {tile} is not a multiple of {TILE_MIN}")
    if 2 * overlap > tile:
        raise ValueError(f"bitstream: overlap = {overlap} is more than half the tile extent {tile}")
    stride = tile - overlap
    return tuple(max(1, -(-(length - overlap) // stride)) for length in (height, width))


def pack_tiled(header: Dict, streams: Sequence[bytes]) -> bytes:
    """``header``: {"arch", "height", "width", "tile", "overlap", "fingerprint"} ("rows" / "cols", if given, must be
    those of ``tile_grid``); ``streams``: one complete ICMB stream per tile, row-major."""
    missing = [k for k in TILED_HEADER_KEYS if k not in header]
    if missing:
        raise ValueError(f"bitstream: tiled header lacks {missing}")
    if header["arch"] not in ARCHS:
        raise ValueError(f"bitstream: unknown architecture {header['arch']!r}; the format knows {list(ARCHS)}")
    rows, cols = tile_grid(header["height"], header["width"], header["tile"], header["overlap"])
    if (header.get("rows", rows), header.get("cols", cols)) != (rows, cols):
        raise ValueError(f"bitstream: header says {header.get('rows')}x{header.get('cols')} tiles, the plan has {rows}x{cols}")
    rows, cols = _uint("rows", rows, U16_MAX), _uint("cols", cols, U16_MAX)
    streams = [bytes(s) for s in streams]
    if len(streams) != rows * cols:
        raise ValueError(f"bitstream: {len(streams)} tile streams for a plan of {rows}x{cols} tiles")
    out = bytearray(_TFIXED.pack(TILED_MAGIC, TILED_VERSION, ARCHS.index(header["arch"]), int(header["height"]),
                                 int(header["width"]), int(header["tile"]), int(header["overlap"]), rows, cols,
                                 _uint("fingerprint", header["fingerprint"], U32_MAX)))
    for s in streams:
        out += _U32.pack(_uint("tile stream length", len(s), U32_MAX))
    for s in streams:
        out += s
    out += _U32.pack(zlib.crc32(bytes(out)) & U32_MAX)
    return bytes(out)


def is_tiled(data) -> bool:
    """True if ``data`` begins with the magic of a tiled stream (says nothing else about it)"""
    return isinstance(data, (bytes, bytearray, memoryview)) and bytes(data[:4]) == TILED_MAGIC


def unpack_tiled(data: bytes) -> Tuple[Dict, List[bytes]]:
    """inverse of ``pack_tiled``: (header with "rows" and "cols", tile streams).  ValueError for a bad magic, an unknown
    version or architecture id, a tile geometry ``tile_grid`` refuses or whose rows / cols are not the stored ones, a
    declared length that runs past the data, trailing bytes or a CRC mismatch.  The tile streams are returned as they
    lie; ``unpack`` checks each."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise ValueError(f"bitstream: expected bytes, got {type(data).__name__}")
    data = bytes(data)
    if not TILED_MAGIC.startswith(data[:4]):
        raise ValueError("bitstream: bad magic (not an ICMT stream)")
    if len(data) < TILED_FIXED_BYTES + CRC_BYTES:
        raise ValueError(f"bitstream: truncated: {len(data)} bytes, the fixed tiled header and CRC need "
                         f"{TILED_FIXED_BYTES + CRC_BYTES}")
    (_, version, arch_id, height, width, tile, overlap, rows, cols, fp) = _TFIXED.unpack_from(data, 0)
    if version != TILED_VERSION:
        raise ValueError(f"bitstream: unknown tiled format version {version} (this reader knows {TILED_VERSION})")
    if arch_id >= len(ARCHS):
        raise ValueError(f"bitstream: unknown architecture id {arch_id} (this reader knows 0..{len(ARCHS) - 1})")
    if height < 1 or width < 1:
        raise ValueError(f"bitstream: empty image {height}x{width}")
    try:
        plan = tile_grid(height, width, tile, overlap)
    except ValueError as e:
        raise ValueError(f"bitstream: bad tile geometry: {e}")
    if plan != (rows, cols):
        raise ValueError(f"bitstream: tile grid mismatch: the header says {rows}x{cols} tiles, a {height}x{width} image "
                         f"in tiles of {tile} overlapping by {overlap} has {plan[0]}x{plan[1]}")
    n = rows * cols
    pos = TILED_FIXED_BYTES + 4 * n
    if pos + CRC_BYTES > len(data):
        raise ValueError(f"bitstream: truncated: the length table of {n} tiles runs past the data")
    lengths = [_U32.unpack_from(data, TILED_FIXED_BYTES + 4 * i)[0] for i in range(n)]
    end = pos + sum(lengths)
    if end + CRC_BYTES > len(data):
        raise ValueError(f"bitstream: truncated: declared tile stream lengths run past the data ({len(data)} bytes, "
                         f"{end + CRC_BYTES} needed)")
    if end + CRC_BYTES < len(data):
        raise ValueError(f"bitstream: {len(data) - end - CRC_BYTES} trailing bytes after the CRC")
    if _U32.unpack_from(data, end)[0] != zlib.crc32(data[:end]) & U32_MAX:
        raise ValueError("bitstream: CRC mismatch (corrupt stream)")
    streams = []
    for ln in lengths:
        streams.append(data[pos:pos + ln])
        pos += ln
    header = {"arch": ARCHS[arch_id], "height": height, "width": width, "tile": tile, "overlap": overlap, "rows": rows,
              "cols": cols, "fingerprint": fp}
    return header, streams


# ------------------------------------------------------------------------------------------- error-bounded images
RESIDUAL_MAGIC = b"ICMR"
RESIDUAL_VERSION = 1
MAX_ERROR = 32                              # largest bound D of the residual layer
RESIDUAL_SIDE_MAX = 32768                   # what the layer's kernels take
_RFIXED = struct.Struct("<4sHBBIIIII")      # magic .. residual length
RESIDUAL_FIXED_BYTES = _RFIXED.size         # 28
assert RESIDUAL_FIXED_BYTES == 28
RESIDUAL_HEADER_KEYS = ("max_error", "coder", "height", "width", "table_crc")


def pack_residual(header: Dict, base: bytes, residual: bytes) -> bytes:
    """``header``: {"max_error": D in 0..MAX_ERROR, "coder": name in CODERS of the residual string, "height", "width",
    "table_crc": u32}; ``base``: one complete ICMB or ICMT stream; ``residual``: the residual layer's string."""
    missing = [k for k in RESIDUAL_HEADER_KEYS if k not in header]
    if missing:
        raise ValueError(f"bitstream: residual header lacks {missing}")
    check_coder(header["coder"], "bitstream: ")
    base, residual = bytes(base), bytes(residual)
    if base[:4] not in (MAGIC, TILED_MAGIC):
        raise ValueError("bitstream: the base of an ICMR stream must be an ICMB or ICMT stream")
    out = bytearray(_RFIXED.pack(
        RESIDUAL_MAGIC, RESIDUAL_VERSION, _uint("max_error", header["max_error"], MAX_ERROR),
        CODERS.index(header["coder"]), _uint("height", header["height"], RESIDUAL_SIDE_MAX, 1),
        _uint("width", header["width"], RESIDUAL_SIDE_MAX, 1), _uint("table_crc", header["table_crc"], U32_MAX),
        _uint("base length", len(base), U32_MAX), _uint("residual length", len(residual), U32_MAX)))
    out += base
    out += residual
    out += _U32.pack(zlib.crc32(bytes(out)) & U32_MAX)
    return bytes(out)


def is_residual(data) -> bool:
    """True if ``data`` begins with the magic of an error-bounded stream (says nothing else about it)"""
    return isinstance(data, (bytes, bytearray, memoryview)) and bytes(data[:4]) == RESIDUAL_MAGIC


def unpack_residual(data: bytes, table_crc: Optional[int] = None) -> Tuple[Dict, bytes, bytes]:
    """inverse of ``pack_residual``: (header, base stream, residual string).  ValueError for a bad magic, an unknown
    version or coder id, D above MAX_ERROR, an image side outside 1..32768, declared lengths that run past the data,
    trailing bytes, a CRC mismatch, a base that begins with neither inner magic and, with ``table_crc`` (the reader's
    own), a stream written with other tables.  The base is returned as it lies; ``unpack`` / ``unpack_tiled`` check
    it."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise ValueError(f"bitstream: expected bytes, got {type(data).__name__}")
    data = bytes(data)
    if not RESIDUAL_MAGIC.startswith(data[:4]):
        raise ValueError("bitstream: bad magic (not an ICMR stream)")
    if len(data) < RESIDUAL_FIXED_BYTES + CRC_BYTES:
        raise ValueError(f"bitstream: truncated: {len(data)} bytes, the fixed residual header and CRC need "
                         f"{RESIDUAL_FIXED_BYTES + CRC_BYTES}")
    (_, version, d, coder_id, height, width, tcrc, nbase, nres) = _RFIXED.unpack_from(data, 0)
    if version != RESIDUAL_VERSION:
        raise ValueError(f"bitstream: unknown residual format version {version} (this reader knows {RESIDUAL_VERSION})")
    if d > MAX_ERROR:
        raise ValueError(f"bitstream: max_error = {d} outside [0, {MAX_ERROR}]")
    if coder_id >= len(CODERS):
        raise ValueError(f"bitstream: unknown coder id {coder_id} (this reader knows 0..{len(CODERS) - 1})")
    if not (1 <= height <= RESIDUAL_SIDE_MAX and 1 <= width <= RESIDUAL_SIDE_MAX):
        raise ValueError(f"bitstream: image {height}x{width} outside 1..{RESIDUAL_SIDE_MAX} a side")
    end = RESIDUAL_FIXED_BYTES + nbase + nres
    if end + CRC_BYTES > len(data):
        raise ValueError(f"bitstream: truncated: declared lengths {nbase} + {nres} run past the data ({len(data)} "
                         f"bytes, {end + CRC_BYTES} needed)")
    if end + CRC_BYTES < len(data):
        raise ValueError(f"bitstream: {len(data) - end - CRC_BYTES} trailing bytes after the CRC")
    if _U32.unpack_from(data, end)[0] != zlib.crc32(data[:end]) & U32_MAX:
        raise ValueError("bitstream: CRC mismatch (corrupt stream)")
    base = data[RESIDUAL_FIXED_BYTES:RESIDUAL_FIXED_BYTES + nbase]
    if base[:4] not in (MAGIC, TILED_MAGIC):
        raise ValueError("bitstream: the base of the ICMR stream is neither an ICMB nor an ICMT stream")
    if table_crc is not None and tcrc != table_crc & U32_MAX:
        raise ValueError(f"bitstream: residual table mismatch: the stream was written with tables {tcrc:#010x}, this "
                         f"reader has {table_crc & U32_MAX:#010x}")
    header = {"max_error": d, "coder": CODERS[coder_id], "height": height, "width": width, "table_crc": tcrc}
    return header, base, data[RESIDUAL_FIXED_BYTES + nbase:end]


# -------------------------------------------------------------------------- error-bounded images, a bound per cell
RESIDUAL_MAP_MAGIC = b"ICME"
RESIDUAL_MAP_VERSION = 1
ERROR_CELL = 16                             # pixels per cell and axis of the bound map: the residual layer's grid
_EFIXED = struct.Struct("<4sHBBIIIIII")     # magic .. residual length
RESIDUAL_MAP_FIXED_BYTES = _EFIXED.size     # 32
assert RESIDUAL_MAP_FIXED_BYTES == 32
RESIDUAL_MAP_HEADER_KEYS = ("coder", "height", "width", "table_crc")
_EMAP_RUN = struct.Struct("<HB")            # count, d


def error_grid(height: int, width: int) -> Tuple[int, int]:
    """(gh, gw): the 16 x 16-pixel cells of the image, anchored at pixel (0, 0), edge cells partial"""
    return -(-int(height) // ERROR_CELL), -(-int(width) // ERROR_CELL)


def check_error_map(dmap, height: int, width: int, who: str = "") -> np.ndarray:
    """``dmap`` as a uint8 [gh, gw] array of bounds in 0 .. MAX_ERROR over ``error_grid``; ValueError otherwise
    (another dtype is not cast)"""
    a = np.asarray(dmap)
    if a.dtype != np.uint8:
        raise ValueError(f"{who}the bound map must be uint8, got {a.dtype}")
    if a.shape != error_grid(height, width):
        raise ValueError(f"{who}the bound map of a {height}x{width} image is {error_grid(height, width)}, got {a.shape}")
    if int(a.max()) > MAX_ERROR:
        raise ValueError(f"{who}the bound map holds max_error = {int(a.max())} outside [0, {MAX_ERROR}]")
    return a


def error_map_string(dmap) -> bytes:
    """the bound-map string of an ICME stream.  A uniform map has none (ValueError): it is written as an ICMR stream."""
    a = np.asarray(dmap)
    if a.ndim != 2 or a.dtype != np.uint8:
        raise ValueError(f"bitstream: the bound map must be a uint8 [gh, gw] array, got {a.dtype} {a.shape}")
    gh, gw = _uint("map height", a.shape[0], U16_MAX, 1), _uint("map width", a.shape[1], U16_MAX, 1)
    flat = a.reshape(-1)
    if int(flat.max()) > MAX_ERROR:
        raise ValueError(f"bitstream: the bound map holds max_error = {int(flat.max())} outside [0, {MAX_ERROR}]")
    if bool((flat == flat[0]).all()):
        raise ValueError(f"bitstream: a uniform bound map (every entry {int(flat[0])}) is written as an ICMR stream, "
                         f"not as a map string")
    starts = np.flatnonzero(np.concatenate(([True], flat[1:] != flat[:-1])))
    ends = np.append(starts[1:], flat.size)
    out = bytearray(_MAP_HEAD.pack(gh, gw))
    for s, e in zip(starts.tolist(), ends.tolist()):
        n, d = e - s, int(flat[s])
        while n > 0:                                # a maximal run longer than a count holds: full counts first
            c = min(n, U16_MAX)
            out += _EMAP_RUN.pack(c, d)
            n -= c
    return bytes(out)


def error_map_from_string(data: bytes, height: int, width: int) -> np.ndarray:
    """inverse of ``error_map_string`` -> uint8 [gh, gw]; the grid must be that of the height x width image.
    ValueError, naming the condition, for anything that is not the one canonical string of such a map."""
    data = bytes(data)
    if len(data) < _MAP_HEAD.size:
        raise ValueError(f"bitstream: truncated: a bound-map string begins with {_MAP_HEAD.size} bytes of grid, this one "
                         f"has {len(data)}")
    gh, gw = _MAP_HEAD.unpack_from(data, 0)
    if (gh, gw) != error_grid(height, width):
        want = error_grid(height, width)
        raise ValueError(f"bitstream: the bound map's grid is {gh}x{gw}, a {height}x{width} image has {want[0]}x{want[1]} "
                         f"cells")
    if (len(data) - _MAP_HEAD.size) % _EMAP_RUN.size:
        raise ValueError(f"bitstream: {(len(data) - _MAP_HEAD.size) % _EMAP_RUN.size} trailing bytes after the last "
                         f"whole run of the bound map")
    total, flat, pos, prev = gh * gw, np.empty(gh * gw, dtype=np.uint8), 0, None
    for off in range(_MAP_HEAD.size, len(data), _EMAP_RUN.size):
        if pos == total:
            raise ValueError(f"bitstream: {len(data) - off} trailing bytes after the bound map's {total} cells")
        count, d = _EMAP_RUN.unpack_from(data, off)
        if count == 0:
            raise ValueError("bitstream: a run of the bound map has a count of 0")
        if d > MAX_ERROR:
            raise ValueError(f"bitstream: bound map: stored max_error = {d} outside [0, {MAX_ERROR}]")
        if prev is not None and prev[1] == d and prev[0] != U16_MAX:
            raise ValueError(f"bitstream: the bound map's runs are not maximal: a run of {prev[0]} is followed by "
                             f"another of the same d = {d}")
        if pos + count > total:
            raise ValueError(f"bitstream: the bound map's runs go past its {total} cells")
        flat[pos:pos + count] = d
        pos, prev = pos + count, (count, d)
    if pos != total:
        raise ValueError(f"bitstream: the bound map's runs cover {pos} of its {total} cells")
    if bool((flat == flat[0]).all()):
        raise ValueError(f"bitstream: the bound map holds a single d = {int(flat[0])} (a uniform map is written as an "
                         f"ICMR stream)")
    return flat.reshape(gh, gw)


def pack_residual_map(header: Dict, base: bytes, dmap, residual: bytes) -> bytes:
    """``header``: {"coder": name in CODERS of the residual string, "height", "width", "table_crc": u32} ("max_error",
    if given, must be the map's largest entry); ``base``: one complete ICMB or ICMT stream; ``dmap``: the bounds of the
    image's cells (``check_error_map``); ``residual``: the residual layer's string under that map.  A uniform map gives
    the ICMR stream of its one bound, ``pack_residual``'s bytes: one content keeps one encoding."""
    missing = [k for k in RESIDUAL_MAP_HEADER_KEYS if k not in header]
    if missing:
        raise ValueError(f"bitstream: residual header lacks {missing}")
    check_coder(header["coder"], "bitstream: ")
    height = _uint("height", header["height"], RESIDUAL_SIDE_MAX, 1)
    width = _uint("width", header["width"], RESIDUAL_SIDE_MAX, 1)
    a = check_error_map(dmap, height, width, "bitstream: ")
    top = int(a.max())
    if header.get("max_error", top) != top:
        raise ValueError(f"bitstream: header says max_error = {header['max_error']}, the largest bound in the map is {top}")
    if int(a.min()) == top:
        return pack_residual({**{k: header[k] for k in RESIDUAL_MAP_HEADER_KEYS}, "max_error": top}, base, residual)
    base, residual, string = bytes(base), bytes(residual), error_map_string(a)
    if base[:4] not in (MAGIC, TILED_MAGIC):
        raise ValueError("bitstream: the base of an ICME stream must be an ICMB or ICMT stream")
    out = bytearray(_EFIXED.pack(
        RESIDUAL_MAP_MAGIC, RESIDUAL_MAP_VERSION, top, CODERS.index(header["coder"]), height, width,
        _uint("table_crc", header["table_crc"], U32_MAX), _uint("base length", len(base), U32_MAX),
        _uint("map length", len(string), U32_MAX), _uint("residual length", len(residual), U32_MAX)))
    out += base
    out += string
    out += residual
    out += _U32.pack(zlib.crc32(bytes(out)) & U32_MAX)
    return bytes(out)


def is_residual_map(data) -> bool:
    """True if ``data`` begins with the magic of an error-bounded stream with a bound map (says nothing else about it)"""
    return isinstance(data, (bytes, bytearray, memoryview)) and bytes(data[:4]) == RESIDUAL_MAP_MAGIC


def unpack_residual_map(data: bytes, table_crc: Optional[int] = None) -> Tuple[Dict, bytes, np.ndarray, bytes]:
    """inverse of ``pack_residual_map`` for a map of more than one value: (header with "max_error" = the largest bound,
    base stream, bound map uint8 [gh, gw], residual string).  ValueError for a bad magic, an unknown version or coder
    id, a maximum above MAX_ERROR, an image side outside 1..32768, declared lengths that run past the data, trailing
    bytes, a CRC mismatch, a base that begins with neither inner magic, with ``table_crc`` (the reader's own) a stream
    written with other tables, a bound-map string ``error_map_from_string`` refuses, and a header maximum that is not
    the map's.  The base is returned as it lies; ``unpack`` / ``unpack_tiled`` check it."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise ValueError(f"bitstream: expected bytes, got {type(data).__name__}")
    data = bytes(data)
    if not RESIDUAL_MAP_MAGIC.startswith(data[:4]):
        raise ValueError("bitstream: bad magic (not an ICME stream)")
    if len(data) < RESIDUAL_MAP_FIXED_BYTES + CRC_BYTES:
        raise ValueError(f"bitstream: truncated: {len(data)} bytes, the fixed bound-map header and CRC need "
                         f"{RESIDUAL_MAP_FIXED_BYTES + CRC_BYTES}")
    (_, version, top, coder_id, height, width, tcrc, nbase, nmap, nres) = _EFIXED.unpack_from(data, 0)
    if version != RESIDUAL_MAP_VERSION:
        raise ValueError(f"bitstream: unknown bound-map format version {version} (this reader knows "
                         f"{RESIDUAL_MAP_VERSION})")
    if top > MAX_ERROR:
        raise ValueError(f"bitstream: max_error = {top} outside [0, {MAX_ERROR}]")
    if coder_id >= len(CODERS):
        raise ValueError(f"bitstream: unknown coder id {coder_id} (this reader knows 0..{len(CODERS) - 1})")
    if not (1 <= height <= RESIDUAL_SIDE_MAX and 1 <= width <= RESIDUAL_SIDE_MAX):
        raise ValueError(f"bitstream: image {height}x{width} outside 1..{RESIDUAL_SIDE_MAX} a side")
    end = RESIDUAL_MAP_FIXED_BYTES + nbase + nmap + nres
    if end + CRC_BYTES > len(data):
        raise ValueError(f"bitstream: truncated: declared lengths {nbase} + {nmap} + {nres} run past the data "
                         f"({len(data)} bytes, {end + CRC_BYTES} needed)")
    if end + CRC_BYTES < len(data):
        raise ValueError(f"bitstream: {len(data) - end - CRC_BYTES} trailing bytes after the CRC")
    if _U32.unpack_from(data, end)[0] != zlib.crc32(data[:end]) & U32_MAX:
        raise ValueError("bitstream: CRC mismatch (corrupt stream)")
    p0 = RESIDUAL_MAP_FIXED_BYTES
    base = data[p0:p0 + nbase]
    if base[:4] not in (MAGIC, TILED_MAGIC):
        raise ValueError("bitstream: the base of the ICME stream is neither an ICMB nor an ICMT stream")
    if table_crc is not None and tcrc != table_crc & U32_MAX:
        raise ValueError(f"bitstream: residual table mismatch: the stream was written with tables {tcrc:#010x}, this "
                         f"reader has {table_crc & U32_MAX:#010x}")
    dmap = error_map_from_string(data[p0 + nbase:p0 + nbase + nmap], height, width)
    if int(dmap.max()) != top:
        raise ValueError(f"bitstream: the header says max_error = {top}, the largest bound in the map is "
                         f"{int(dmap.max())}")
    header = {"max_error": top, "coder": CODERS[coder_id], "height": height, "width": width, "table_crc": tcrc}
    return header, base, dmap, data[p0 + nbase + nmap:end]
