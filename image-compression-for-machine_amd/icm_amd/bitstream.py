"""Container of one compressed image: the bytes ``python -m icm_amd.codec`` writes and reads.

Parity unpinned: no counterpart in the reference (upstream CompressAI's ``examples/codec.py`` is not in its tree), so
the layout below is this project's own.  Pure Python; importing it needs neither torch nor the HIP library.

Layout -- fixed-width little-endian integers, no padding between fields:

    offset  size  field
         0     4  magic, the bytes ``ICMB``
         4     2  format version (u16), ``VERSION`` = 1
         6     2  architecture id (u16), index into ``ARCHS`` = ("cnn", "stf")
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
"""
from __future__ import annotations

import struct
import zlib
from typing import Dict, List, Sequence, Tuple

MAGIC = b"ICMB"
VERSION = 1
ARCHS = ("cnn", "stf")

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


def pack(header: Dict, strings: Sequence[bytes]) -> bytes:
    """``header``: {"arch": name in ARCHS, "height", "width", "pads": (left, right, top, bottom),
    "shape": (z height, z width), "fingerprint": u32}; ``strings``: the flattened ``compress()["strings"]``."""
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
        MAGIC, VERSION, ARCHS.index(header["arch"]),
        _uint("height", header["height"], U32_MAX, 1), _uint("width", header["width"], U32_MAX, 1),
        *(_uint("pad", p, U16_MAX) for p in pads), *(_uint("shape", s, U16_MAX) for s in shape),
        _uint("fingerprint", header["fingerprint"], U32_MAX), n))
    for s in strings:
        out += _U32.pack(_uint("string length", len(s), U32_MAX))
    for s in strings:
        out += s
    out += _U32.pack(zlib.crc32(bytes(out)) & U32_MAX)
    return bytes(out)


def unpack(data: bytes) -> Tuple[Dict, List[bytes]]:
    """inverse of ``pack``: (header, strings).  ValueError for a bad magic, an unknown version or architecture id, a
    declared length that runs past the data, trailing bytes or a CRC mismatch."""
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
    if arch_id >= len(ARCHS):
        raise ValueError(f"bitstream: unknown architecture id {arch_id} (this reader knows 0..{len(ARCHS) - 1})")
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
