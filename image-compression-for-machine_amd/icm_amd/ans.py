"""compressai.ans mirror: RansEncoder / RansDecoder / BufferedRansEncoder over the C ABI (csrc/rans.cpp).

The reference imports these three classes from a binary-only pybind11 extension (``compressai/ans.cpython-38-*.so``,
used at entropy_models/entropy_models.py:32-36,200-208,268-276 and models/cnn.py:5,228,263-264,300-318); the
interface below keeps their call signatures -- Python lists (or anything ``numpy.asarray`` accepts) in, ``bytes`` /
``list[int]`` out -- and hands flat int32 arrays to ``icm_rans_*``.  Host-side, like the reference's coder.

Below them: the lane-stream coder (``coder="lanes"``, format in ``icm_amd.bitstream``; parity unpinned: no counterpart
in the reference) -- ``lanes_encode`` / ``LanesDecoder`` on the host, the executable definition of the format (the
host loops of csrc/rans.cpp over the lane arithmetic of csrc/rans_lanes_common.h), and ``lanes_encode_gpu`` /
``LanesDecoderGpu`` over the kernels of csrc/rans_lanes.hip, which compile the same arithmetic and take device tensors.
Last: ``coder_for``, the one object behind every ``coder=`` keyword, so that no caller asks which coder it holds."""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace
from typing import List, Sequence

import numpy as np

from . import _lib as L
from .bitstream import CODERS, check_coder      # noqa: F401  defined with the container format, part of this surface

_i32p = C.POINTER(C.c_int32)


def _arr(v) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(v, dtype=np.int32).reshape(-1))


class _Tables:
    """cdfs as one [ncdf, stride] int32 block + sizes + offsets (accepts the reference's list-of-lists)"""

    def __init__(self, cdfs, cdfs_sizes, offsets):
        if isinstance(cdfs, np.ndarray) and cdfs.ndim == 2:
            m = np.ascontiguousarray(cdfs.astype(np.int32, copy=False))
        else:
            rows = [np.asarray(r, dtype=np.int32).reshape(-1) for r in cdfs]
            stride = max((len(r) for r in rows), default=0)
            m = np.zeros((len(rows), stride), dtype=np.int32)
            for i, r in enumerate(rows):
                m[i, :len(r)] = r
        self.cdfs, self.sizes, self.offsets = m, _arr(cdfs_sizes), _arr(offsets)
        if m.ndim != 2 or m.shape[0] == 0 or len(self.sizes) != m.shape[0] or len(self.offsets) != m.shape[0]:
            raise ValueError("cdfs, cdfs_sizes and offsets must describe the same number of tables")

    def args(self):
        return (self.cdfs.ctypes.data_as(_i32p), int(self.cdfs.shape[1]), self.sizes.ctypes.data_as(_i32p),
                self.offsets.ctypes.data_as(_i32p), int(self.cdfs.shape[0]))


def _encode(symbols: np.ndarray, indexes: np.ndarray, t: _Tables) -> bytes:
    if symbols.shape != indexes.shape:
        raise ValueError("symbols and indexes must have the same length")
    lib = L.lib()
    n = int(symbols.size)
    sp, ip = symbols.ctypes.data_as(_i32p), indexes.ctypes.data_as(_i32p)
    cap = 4 * n + 64     # a regular symbol costs <= 16 bits; escapes are measured first
    buf = (C.c_uint8 * cap)()
    nb = lib.icm_rans_encode_with_indexes(sp, ip, n, *t.args(), buf, cap)
    if nb < 0:           # escape-heavy input or bad tables: measure, then encode into an exact buffer
        need = lib.icm_rans_encode_with_indexes(sp, ip, n, *t.args(), None, 0)
        if need < 0:
            raise ValueError("rANS encode: invalid symbols / indexes / CDF tables")
        buf = (C.c_uint8 * need)()
        nb = lib.icm_rans_encode_with_indexes(sp, ip, n, *t.args(), buf, need)
        if nb < 0:
            raise ValueError("rANS encode failed")
    return bytes(bytearray(buf)[:nb])


class RansEncoder:
    def encode_with_indexes(self, symbols, indexes, cdfs, cdfs_sizes, offsets) -> bytes:
        return _encode(_arr(symbols), _arr(indexes), _Tables(cdfs, cdfs_sizes, offsets))


class BufferedRansEncoder:
    """symbols of several calls are concatenated and coded as ONE stream by flush() (cnn.py:228,263-264)"""

    def __init__(self):
        self._sym: List[np.ndarray] = []
        self._idx: List[np.ndarray] = []
        self._tables = None

    def encode_with_indexes(self, symbols, indexes, cdfs, cdfs_sizes, offsets) -> None:
        s, i = _arr(symbols), _arr(indexes)
        if s.shape != i.shape:
            raise ValueError("symbols and indexes must have the same length")
        self._sym.append(s)
        self._idx.append(i)
        self._tables = _Tables(cdfs, cdfs_sizes, offsets)

    def flush(self) -> bytes:
        if self._tables is None:
            raise ValueError("nothing to flush")
        out = _encode(np.concatenate(self._sym), np.concatenate(self._idx), self._tables)
        self._sym, self._idx, self._tables = [], [], None
        return out


class RansDecoder:
    def __init__(self):
        self._h = None
        self._keep = None

    def _close(self):
        if self._h:
            L.lib().icm_rans_decoder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self._close()
        except Exception:
            pass

    def set_stream(self, stream: bytes) -> None:
        self._close()
        self._keep = (C.c_uint8 * len(stream)).from_buffer_copy(stream)
        self._h = L.lib().icm_rans_decoder_create(self._keep, len(stream))
        if not self._h:
            raise ValueError("rANS decode: not a stream (length must be a multiple of 4, at least 8 bytes)")

    def decode_stream(self, indexes, cdfs, cdfs_sizes, offsets) -> List[int]:
        if not self._h:
            raise ValueError("set_stream() first")
        return self.decode_stream_np(_arr(indexes), _Tables(cdfs, cdfs_sizes, offsets)).tolist()

    def decode_stream_np(self, idx: np.ndarray, t: "_Tables") -> np.ndarray:
        out = np.empty(idx.size, dtype=np.int32)
        rc = L.lib().icm_rans_decoder_decode(self._h, idx.ctypes.data_as(_i32p), int(idx.size), *t.args(),
                                             out.ctypes.data_as(_i32p))
        if rc:
            raise ValueError("rANS decode: corrupt stream or invalid indexes / CDF tables")
        return out

    def decode_with_indexes(self, stream: bytes, indexes, cdfs, cdfs_sizes, offsets) -> List[int]:
        self.set_stream(stream)
        try:
            return self.decode_stream(indexes, cdfs, cdfs_sizes, offsets)
        finally:
            self._close()


def pmf_to_quantized_cdf(pmf: Sequence[float], precision: int = 16) -> List[int]:
    """compressai._CXX.pmf_to_quantized_cdf (entropy_models.py:13,60-63)"""
    p = np.ascontiguousarray(np.asarray(pmf, dtype=np.float32).reshape(-1))
    out = np.empty(p.size + 1, dtype=np.int32)
    rc = L.lib().icm_pmf_to_quantized_cdf(p.ctypes.data_as(C.POINTER(C.c_float)), int(p.size), int(precision),
                                          out.ctypes.data_as(_i32p))
    if rc:
        raise ValueError("pmf_to_quantized_cdf: invalid pmf (negative / non-finite / empty / all zero)")
    return out.tolist()


# ---------------------------------------------------------------------------------------------------- lane streams
SYMBOLS_PER_WAVE = 16384      # what ``symbols_per_wave=None`` means: ``coder_for`` (why this value)
_i64p = C.POINTER(C.c_int64)
_LANES_STATUS = ((1, "a body ran out of words"), (2, "a value no table bin holds"), (4, "an escape outside int32"),
                 (8, "a CDF index outside the tables"), (16, "a lane did not end at 2^16"),
                 (32, "words of a body were left unread"))


def _lanes_status(st: int) -> None:
    if st:
        why = [text for bit, text in _LANES_STATUS if st & bit] or [f"runtime failure ({st})"]
        raise ValueError("lane stream decode: corrupt stream or wrong indexes / CDF tables: " + "; ".join(why))


def _runs(run_lengths, total: int):
    runs = np.ascontiguousarray(np.asarray(run_lengths, dtype=np.int64).reshape(-1))
    if (runs < 0).any() or int(runs.sum()) != total:
        raise ValueError("run_lengths must be non-negative and add up to the number of symbols")
    return runs


def lanes_waves(run_lengths, symbols_per_wave: int = SYMBOLS_PER_WAVE) -> int:
    """G of the lane stream that codes runs of these lengths"""
    runs = np.ascontiguousarray(np.asarray(run_lengths, dtype=np.int64).reshape(-1))
    g = L.lib().icm_rans_lanes_waves(runs.ctypes.data_as(_i64p), int(runs.size), int(symbols_per_wave))
    if g < 1:
        raise ValueError("lane stream: run lengths must be non-negative and symbols_per_wave at least 1")
    return g


def lanes_chunk(n: int, G: int) -> int:
    """c of a run of ``n`` elements in a stream of ``G`` waves: wave g owns the elements [g c, min(n, (g + 1) c)) -- the
    per-wave share rounded up to whole steps of 64 lanes (``chunk`` of csrc/rans_lanes_common.h)"""
    return (-(-int(n) // int(G)) + 63) // 64 * 64


def _wave_range(G: int, g0: int, g1: int, elem0: int, n: int, have: int) -> None:
    """the checks of a ranged call that the C entry makes, plus the one it cannot: the buffers' length"""
    if not (0 <= g0 <= g1 <= G and 0 <= elem0 <= g0 * lanes_chunk(n, G)):
        raise ValueError(f"lane stream: waves [{g0}, {g1}) from element {elem0} are not a range of a run of {n} in "
                         f"{G} waves")
    need = max(0, min(n, g1 * lanes_chunk(n, G)) - elem0) if g1 > g0 else 0
    if have < need:
        raise ValueError(f"lane stream: waves [{g0}, {g1}) from element {elem0} need {need} indexes, got {have}")


def lanes_encode(symbols, indexes, run_lengths, t: _Tables, symbols_per_wave: int = SYMBOLS_PER_WAVE) -> bytes:
    """host encoder: the runs back to back in ``symbols`` / ``indexes`` -> one lane stream"""
    sym, idx = _arr(symbols), _arr(indexes)
    if sym.shape != idx.shape:
        raise ValueError("symbols and indexes must have the same length")
    runs = _runs(run_lengths, int(sym.size))
    lanes_waves(runs, symbols_per_wave)
    args = (sym.ctypes.data_as(_i32p), idx.ctypes.data_as(_i32p), runs.ctypes.data_as(_i64p), int(runs.size), *t.args(),
            int(symbols_per_wave))
    need = L.lib().icm_rans_lanes_encode(*args, None, 0)
    if need < 0:
        raise ValueError("lane stream encode: invalid symbols / indexes / CDF tables")
    buf = (C.c_uint8 * need)()
    if L.lib().icm_rans_lanes_encode(*args, buf, need) != need:
        raise ValueError("lane stream encode failed")
    return bytes(buf)


class _LanesHandle:
    """what the host and the device decoder of a lane stream share: the C handle (made and freed by the functions
    that ``_create`` and ``_destroy`` name) on a copy of the string"""

    def __init__(self, stream: bytes, *stream_arg):
        self._keep = (C.c_uint8 * max(1, len(stream))).from_buffer_copy(bytes(stream) or b"\0")
        self._h = getattr(L.lib(), self._create)(self._keep, len(stream), *stream_arg)
        if not self._h:
            raise ValueError("lane stream decode: not a lane stream (magic, version, G or a length table that "
                             "disagrees with the string's length)")
        self.G = getattr(L.lib(), self._waves)(self._h)      # the stream's wave bodies

    def close(self):
        if self._h:
            getattr(L.lib(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LanesDecoder(_LanesHandle):
    """host decoder of one lane stream: ``decode_run`` per run in stream order, then ``finish``.

    The waves of a stream share nothing, so a range of them can be decoded alone: ``decode_run_waves(g0, g1, elem0,
    ...)`` has the waves g0 <= g < g1 decode their elements of the run, and ``finish_waves(g0, g1, end)`` answers for
    those waves only and leaves the decoder open (``close`` it).  The caller's contract: a wave is given the runs of
    the stream in their order, none skipped; different waves may stand at different runs.  ``G``: the stream's waves."""
    _create, _destroy = "icm_rans_lanes_decoder_create", "icm_rans_lanes_decoder_destroy"
    _waves = "icm_rans_lanes_decoder_waves"

    def decode_run(self, indexes, t: _Tables) -> np.ndarray:
        idx = _arr(indexes)
        out = np.empty(idx.size, dtype=np.int32)
        rc = L.lib().icm_rans_lanes_decoder_decode_run(self._h, idx.ctypes.data_as(_i32p), int(idx.size), *t.args(),
                                                       out.ctypes.data_as(_i32p))
        if rc:
            _lanes_status(L.lib().icm_rans_lanes_decoder_finish(self._h) or -1)
        return out

    def decode_run_waves(self, g0: int, g1: int, elem0: int, indexes, n: int, t: _Tables) -> np.ndarray:
        """the waves [g0, g1) decode their elements of a run of ``n`` (the whole run's length).  ``indexes`` holds the
        run's elements from ``elem0`` (at most g0 c, ``lanes_chunk``) up to at least the last one of wave g1 - 1; the
        result has its shape, element e at e - elem0, and only the elements of those waves are written"""
        idx = _arr(indexes)
        _wave_range(self.G, g0, g1, elem0, n, int(idx.size))
        out = np.zeros(idx.size, dtype=np.int32)
        rc = L.lib().icm_rans_lanes_decoder_decode_run_waves(self._h, g0, g1, elem0, idx.ctypes.data_as(_i32p), int(n),
                                                             *t.args(), out.ctypes.data_as(_i32p))
        if rc:
            _lanes_status(L.lib().icm_rans_lanes_decoder_finish_waves(self._h, g0, g1, 0) or -1)
        return out

    def finish(self) -> None:
        st = L.lib().icm_rans_lanes_decoder_finish(self._h)
        self.close()
        _lanes_status(st)

    def finish_waves(self, g0: int, g1: int, end: bool = True) -> None:
        """ValueError unless the waves [g0, g1) decoded cleanly; ``end``: and have reached the end of their bodies
        (for waves that have decoded their last run).  The decoder stays open."""
        _lanes_status(L.lib().icm_rans_lanes_decoder_finish_waves(self._h, g0, g1, 1 if end else 0))


def lanes_decode(stream: bytes, indexes, run_lengths, t: _Tables) -> np.ndarray:
    """host decode of a whole stream whose indexes are known up front (tests, z strings)"""
    idx = _arr(indexes)
    runs = _runs(run_lengths, int(idx.size))
    dec = LanesDecoder(stream)
    out, pos = [], 0
    for n in runs.tolist():
        out.append(dec.decode_run(idx[pos:pos + n], t))
        pos += n
    dec.finish()
    return np.concatenate(out) if out else np.empty(0, np.int32)


def _dev_tables(cdf, sizes, offsets):
    import torch
    for b in (cdf, sizes, offsets):
        if not (b.is_cuda and b.dtype == torch.int32 and b.is_contiguous()):
            raise ValueError("lane stream: the CDF tables must be contiguous int32 device tensors")
    if cdf.dim() != 2 or sizes.numel() != cdf.size(0) or offsets.numel() != cdf.size(0):
        raise ValueError("cdfs, cdfs_sizes and offsets must describe the same number of tables")
    return (cdf.data_ptr(), int(cdf.size(1)), sizes.data_ptr(), offsets.data_ptr(), int(cdf.size(0)))


def lanes_encode_gpu(symbols, indexes, run_lengths, cdf, sizes, offsets,
                     symbols_per_wave: int = SYMBOLS_PER_WAVE) -> bytes:
    """device encoder: flat int32 device tensors (the runs back to back) and the device-resident tables -> the same
    bytes as ``lanes_encode``.  Only the finished string crosses to the host."""
    import torch
    if symbols.shape != indexes.shape or symbols.dim() != 1:
        raise ValueError("symbols and indexes must be flat tensors of the same length")
    for b in (symbols, indexes):
        if not (b.is_cuda and b.dtype == torch.int32 and b.is_contiguous()):
            raise ValueError("lane stream: symbols and indexes must be contiguous int32 device tensors")
    runs = _runs(run_lengths, int(symbols.numel()))
    lanes_waves(runs, symbols_per_wave)
    tabs = _dev_tables(cdf, sizes, offsets)
    lib, rp = L.lib(), runs.ctypes.data_as(_i64p)
    off = C.c_int64(0)
    for worst in (0, 1):          # optimistic: one word per symbol; escape-heavy input: the worst case, once
        nws = lib.icm_rans_lanes_encode_gpu_workspace(rp, int(runs.size), int(symbols_per_wave), worst)
        if nws < 0:
            raise ValueError("lane stream encode: the runs are too long for one stream")
        ws = torch.empty(nws, dtype=torch.uint8, device=symbols.device)
        nb = lib.icm_rans_lanes_encode_gpu(symbols.data_ptr(), indexes.data_ptr(), rp, int(runs.size), *tabs,
                                           int(symbols_per_wave), worst, ws.data_ptr(), nws, C.byref(off), L.stream())
        if nb != -2:
            break
    if nb == -1:
        raise ValueError("lane stream encode: invalid symbols / indexes / CDF tables")
    if nb < 0:
        raise L.IcmError(f"lane stream encode failed (code {nb})")
    return ws[off.value:off.value + nb].cpu().numpy().tobytes()


class LanesDecoderGpu(_LanesHandle):
    """device decoder of one lane stream.  ``decode_run`` is one launch on the current stream and returns a device
    tensor; nothing is known to be valid until ``finish`` has looked at the status words.  ``decode_run_waves`` /
    ``finish_waves`` / ``G``: the ranged forms, as on ``LanesDecoder`` and bit for bit its results; a ranged launch
    holds the range's waves alone."""

    _create, _destroy = "icm_rans_lanes_decoder_gpu_create", "icm_rans_lanes_decoder_gpu_destroy"
    _waves = "icm_rans_lanes_decoder_gpu_waves"

    def __init__(self, stream: bytes):
        super().__init__(stream, L.stream())

    def decode_run(self, indexes, cdf, sizes, offsets, out=None):
        import torch
        if not (indexes.is_cuda and indexes.dtype == torch.int32 and indexes.is_contiguous()):
            raise ValueError("lane stream: indexes must be a contiguous int32 device tensor")
        if out is None:
            out = torch.empty(indexes.shape, dtype=torch.int32, device=indexes.device)
        L.check(L.lib().icm_rans_lanes_decoder_gpu_decode_run(self._h, indexes.data_ptr(), int(indexes.numel()),
                                                              *_dev_tables(cdf, sizes, offsets), out.data_ptr(),
                                                              L.stream()), "lanes decode_run")
        return out

    def decode_run_waves(self, g0: int, g1: int, elem0: int, indexes, n: int, cdf, sizes, offsets, out=None):
        """as ``LanesDecoder.decode_run_waves`` on flat device tensors; ``out`` (same length as ``indexes``) is written
        only where those waves own elements -- a fresh one is zero elsewhere"""
        import torch
        if not (indexes.is_cuda and indexes.dtype == torch.int32 and indexes.is_contiguous()):
            raise ValueError("lane stream: indexes must be a contiguous int32 device tensor")
        _wave_range(self.G, g0, g1, elem0, n, int(indexes.numel()))
        if out is None:
            out = torch.zeros(indexes.shape, dtype=torch.int32, device=indexes.device)
        elif not (out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and out.numel() == indexes.numel()):
            raise ValueError("lane stream: out must be a contiguous int32 device tensor as long as indexes")
        L.check(L.lib().icm_rans_lanes_decoder_gpu_decode_run_waves(self._h, g0, g1, elem0, indexes.data_ptr(), int(n),
                                                                    *_dev_tables(cdf, sizes, offsets), out.data_ptr(),
                                                                    L.stream()), "lanes decode_run_waves")
        return out

    def finish(self) -> None:
        st = L.lib().icm_rans_lanes_decoder_gpu_finish(self._h, L.stream())
        self.close()
        _lanes_status(st)

    def finish_waves(self, g0: int, g1: int, end: bool = True) -> None:
        _lanes_status(L.lib().icm_rans_lanes_decoder_gpu_finish_waves(self._h, g0, g1, 1 if end else 0, L.stream()))


# ------------------------------------------------------------------------------------------- one coder behind both
class HostCoder:
    """the reference's scalar stream, coded on the host from ``em._tables()`` (``em``: the EntropyModel whose tables
    apply).  ``encode``: flat int32 symbols and indexes cross to the host once each; the runs are concatenated.
    ``decoder(string, em)``: ``decode_run(indexes, out=None)`` -> int32 symbols shaped like ``indexes`` on its device (a
    copy down and one up per call), ``finish()`` (the scalar stream has no end mark to check) and ``close()``.
    ``waves`` is None: the scalar stream is one chain and has no ranged forms."""
    name = "host"

    def encode(self, symbols, indexes, run_lengths, em) -> bytes:
        _runs(run_lengths, int(symbols.numel()))
        return _encode(_arr(symbols.detach().cpu().numpy()), _arr(indexes.detach().cpu().numpy()), em._tables())

    def decoder(self, string: bytes, em):
        import torch
        dec, t = RansDecoder(), em._tables()
        dec.set_stream(string)

        def decode_run(indexes, out=None):
            sym = torch.from_numpy(dec.decode_stream_np(_arr(indexes.detach().cpu().numpy()), t).reshape(indexes.shape))
            return sym.to(indexes.device) if out is None else out.copy_(sym)
        return SimpleNamespace(decode_run=decode_run, finish=lambda: None, close=dec._close, waves=None)


class LanesCoder(HostCoder):
    """lane streams, coded by the kernels from ``em._device_tables()`` where the symbols lie: the same surface; host
    indexes are brought to the device, ``decode_run`` is one launch without a wait and answers on the device, and
    nothing is known to be valid until ``finish`` has read the status words.  Its decoder also has ``waves`` (G of the
    string), ``decode_run_waves(g0, g1, elem0, indexes, n, out=None)`` and ``finish_waves(g0, g1, end=True)``, the
    ranged forms of ``LanesDecoderGpu``; after ``finish_waves`` the decoder is still to be closed."""
    name = "lanes"

    def __init__(self, symbols_per_wave):
        self.symbols_per_wave = symbols_per_wave

    def encode(self, symbols, indexes, run_lengths, em) -> bytes:
        import torch
        return lanes_encode_gpu(symbols.contiguous(), indexes.to(symbols.device, torch.int32).contiguous(), run_lengths,
                                *em._device_tables(), symbols_per_wave=self.symbols_per_wave)

    def decoder(self, string: bytes, em):
        import torch
        dec, t = LanesDecoderGpu(string), em._device_tables()
        return SimpleNamespace(finish=dec.finish, close=dec.close, decode_run=lambda indexes, out=None: dec.decode_run(
            indexes.to(t[0].device, torch.int32).contiguous(), *t, out=out), waves=dec.G, finish_waves=dec.finish_waves,
            decode_run_waves=lambda g0, g1, elem0, indexes, n, out=None: dec.decode_run_waves(
                g0, g1, elem0, indexes.to(t[0].device, torch.int32).contiguous(), n, *t, out=out))


def coder_for(coder, symbols_per_wave=None):
    """the coder object of a ``coder=`` keyword (one that already is an object passes through): the one place that
    checks the name and gives ``symbols_per_wave=None`` its meaning, SYMBOLS_PER_WAVE; 0 is refused by the encoder"""
    if isinstance(coder, str):
        spw = SYMBOLS_PER_WAVE if symbols_per_wave is None else symbols_per_wave
        coder = HostCoder() if check_coder(coder) == "host" else LanesCoder(spw)
    return coder
