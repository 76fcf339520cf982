"""Exact-integer restatement of the lane-stream format (the ``coder="lanes"`` strings), written from the format's
definition in words -- the docstring of icm_amd/bitstream.py -- and not from csrc/rans.cpp.  Plain Python integers
and lists; slow, and meant to be: every rule of the text is one line here.

    encode(symbols, indexes, run_lengths, cdfs, sizes, offsets, symbols_per_wave) -> bytes
    decode(stream, indexes, run_lengths, cdfs, sizes, offsets) -> list of int     (Corrupt on any failure)

``cdfs``: one list per table; ``sizes[i]`` entries of table i count, the last bin (``sizes[i] - 2``) is the escape."""
import struct

L = 1 << 16
LANES = 64
MAX_G = 4096
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


class Corrupt(ValueError):
    pass


def waves(run_lengths, symbols_per_wave):
    n = max(run_lengths, default=0)
    return min(max(-(-n // symbols_per_wave), 1), MAX_G)


def chunk(n, G):
    return -(-(-(-n // G)) // LANES) * LANES


def _elements(n, G, g):
    """steps of wave g in a run of n elements: a list of steps, each the list of (lane, element) that are active"""
    c = chunk(n, G)
    lo, hi = g * c, min(n, (g + 1) * c)
    steps = []
    t = 0
    while lo + LANES * t < hi:
        steps.append([(lane, lo + LANES * t + lane) for lane in range(LANES) if lo + LANES * t + lane < hi])
        t += 1
    return steps


def _puts(symbol, idx, cdfs, sizes, offsets):
    """the (start, freq) of phases 0..3 of one element; None for a phase the lane does not take"""
    if not 0 <= idx < len(cdfs) or not 2 <= sizes[idx] <= len(cdfs[idx]):
        raise ValueError("bad CDF index")
    cdf, overflow = cdfs[idx], sizes[idx] - 2
    v = symbol - offsets[idx]
    raw = None
    if v < 0:
        raw, v = -2 * v - 1, overflow
    elif v >= overflow:
        raw, v = 2 * (v - overflow), overflow
    start, freq = cdf[v], cdf[v + 1] - cdf[v]
    if freq <= 0 or freq >= L:
        raise ValueError("zero-width symbol")
    if raw is None:
        return [(start, freq), None, None, None]
    return [(start, freq)] + [((raw >> (16 * k)) & 0xFFFF, 1) for k in range(3)]


def encode(symbols, indexes, run_lengths, cdfs, sizes, offsets, symbols_per_wave=16384):
    G = waves(run_lengths, symbols_per_wave)
    starts = [sum(run_lengths[:r]) for r in range(len(run_lengths))]
    bodies = []
    for g in range(G):
        x = [L] * LANES
        words = []                                  # as the decoder reads them; the encoder writes downwards
        for r in reversed(range(len(run_lengths))):
            for step in reversed(_elements(run_lengths[r], G, g)):
                puts = {lane: _puts(symbols[starts[r] + e], indexes[starts[r] + e], cdfs, sizes, offsets)
                        for lane, e in step}
                for phase in (3, 2, 1, 0):
                    emitted = []
                    for lane, _ in step:            # ascending lanes
                        if puts[lane][phase] is None:
                            continue
                        start, freq = puts[lane][phase]
                        if x[lane] >= freq << 16:
                            emitted.append(x[lane] & 0xFFFF)
                            x[lane] >>= 16
                        x[lane] = ((x[lane] // freq) << 16) + x[lane] % freq + start
                    words[:0] = emitted             # the emitting lanes land in ascending lane order, below the rest
        bodies.append(struct.pack("<64I", *x) + struct.pack(f"<{len(words)}H", *words))
    return b"ICML" + struct.pack("<HH", 1, G) + b"".join(struct.pack("<I", len(b)) for b in bodies) + b"".join(bodies)


def parse(stream):
    """[(initial states, words)] per wave; Corrupt unless the header and the length table describe the string"""
    stream = bytes(stream)
    if len(stream) < 8 or stream[:4] != b"ICML":
        raise Corrupt("magic")
    version, G = struct.unpack_from("<HH", stream, 4)
    if version != 1 or not 1 <= G <= MAX_G or 8 + 4 * G > len(stream):
        raise Corrupt("version / G")
    lengths = struct.unpack_from(f"<{G}I", stream, 8)
    if any(n < 4 * LANES or n % 2 for n in lengths) or 8 + 4 * G + sum(lengths) != len(stream):
        raise Corrupt("length table")
    out, pos = [], 8 + 4 * G
    for n in lengths:
        out.append((list(struct.unpack_from("<64I", stream, pos)),
                    list(struct.unpack_from(f"<{(n - 4 * LANES) // 2}H", stream, pos + 4 * LANES))))
        pos += n
    return out


def decode(stream, indexes, run_lengths, cdfs, sizes, offsets):
    bodies = parse(stream)
    G = len(bodies)
    starts = [sum(run_lengths[:r]) for r in range(len(run_lengths))]
    out = [0] * sum(run_lengths)
    for g, (x, words) in enumerate(bodies):
        cursor = 0

        def read():
            nonlocal cursor
            if cursor >= len(words):
                raise Corrupt("overrun")
            cursor += 1
            return words[cursor - 1]

        for r, n in enumerate(run_lengths):
            for step in _elements(n, G, g):
                escaped = []
                for lane, e in step:                # phase 0
                    idx = indexes[starts[r] + e]
                    if not 0 <= idx < len(cdfs) or not 2 <= sizes[idx] <= len(cdfs[idx]):
                        raise Corrupt("CDF index")
                    cdf, overflow = cdfs[idx], sizes[idx] - 2
                    cum = x[lane] & 0xFFFF
                    s = next((s for s in range(overflow + 1) if cdf[s] <= cum < cdf[s + 1]), None)
                    if s is None:
                        raise Corrupt("no bin")
                    x[lane] = (cdf[s + 1] - cdf[s]) * (x[lane] >> 16) + cum - cdf[s]
                    if x[lane] < L:
                        x[lane] = (x[lane] << 16) | read()
                    out[starts[r] + e] = s + offsets[idx]
                    if s == overflow:
                        escaped.append((lane, starts[r] + e, overflow, offsets[idx]))
                raw = {lane: 0 for lane, *_ in escaped}
                for phase in range(3):              # phases 1..3
                    for lane, *_ in escaped:
                        raw[lane] |= (x[lane] & 0xFFFF) << (16 * phase)
                        x[lane] = ((x[lane] >> 16) << 16) | read()     # freq 1, start = the value: always renormalises
                for lane, pos, overflow, offset in escaped:
                    v = (-(raw[lane] >> 1) - 1 if raw[lane] & 1 else (raw[lane] >> 1) + overflow) + offset
                    if not INT32_MIN <= v <= INT32_MAX:
                        raise Corrupt("escape outside int32")
                    out[pos] = v
        if cursor != len(words) or any(v != L for v in x):
            raise Corrupt("final state")
    return out
