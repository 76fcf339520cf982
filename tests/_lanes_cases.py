"""Inputs shared by tests/test_rans_lanes.py (host implementation) and tests/test_gpu_rans_lanes.py (kernels): small
CDF tables, the (n, G) cases the format's partition rule makes interesting, and corrupt streams classified by the
restatement in tests/_lanes_ref.py.  Everything is derived from fixed seeds; nothing here touches the library."""
import functools
import struct

import numpy as np

import _lanes_ref as R

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1

# four tables of stride 12; the last bin of each is the escape bin.  Table 3 has zero-probability bins (0, 2 and 5).
CDFS = [
    [0, 2000, 9000, 30000, 52000, 61000, 65000, 65536, 0, 0, 0, 0],
    [0, 1, 50, 700, 5000, 20000, 44000, 60000, 64900, 65500, 65535, 65536],
    [0, 65535, 65536, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    [0, 0, 3000, 3000, 40000, 65000, 65000, 65530, 65536, 0, 0, 0],
]
SIZES = [8, 12, 3, 9]
OFFSETS = [-3, -5, 0, -4]


def tables_np():
    return np.array(CDFS, np.int32), np.array(SIZES, np.int32), np.array(OFFSETS, np.int32)


def _draw(rng, n, escapes=0.02, only=None):
    """n (symbol, index) pairs: regular symbols drawn from the table's own distribution, a few escapes around it"""
    idx = rng.integers(0, len(CDFS), n) if only is None else np.full(n, only)
    sym = np.empty(n, np.int64)
    for i, t in enumerate(idx):
        cdf, overflow = CDFS[t], SIZES[t] - 2
        while True:
            s = int(np.searchsorted(cdf[:overflow + 2], rng.integers(0, 1 << 16), side="right")) - 1
            if s < overflow:
                break
            if rng.random() < 0.5:               # the escape bin was drawn: a value outside the table
                s = int(rng.choice([-1, -2, -40, overflow, overflow + 1, overflow + 300, 70000, -70000]))
                break
        if rng.random() < escapes:
            s = int(rng.choice([-1, overflow, -1000, 100000]))
        sym[i] = s + OFFSETS[t]
    return sym.astype(np.int32), idx.astype(np.int32)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (symbols, indexes, run_lengths, symbols_per_wave, G)"""
    rng = np.random.default_rng(20240611)
    out = {}

    def add(name, runs, spw, G, sym=None, idx=None, **kw):
        if sym is None:
            sym, idx = _draw(rng, sum(runs), **kw)
        assert R.waves(runs, spw) == G, name
        out[name] = (sym, idx, list(runs), spw, G)

    add("n63_g1", [63], 16384, 1)
    add("n64_g1", [64], 16384, 1)
    add("n65_g1", [65], 16384, 1)
    add("n100_g2_partial_second_wave", [100], 50, 2)
    add("n64_g2_empty_second_wave", [64], 32, 2)
    add("r10_unequal", [130, 0, 64, 1, 200, 77, 5, 300, 64, 129], 100, 3)
    add("n5000_g3", [5000], 2000, 3, escapes=0.005)
    # escapes at the ends of int32 and just outside each end of every table
    sym, idx = [], []
    for t in range(len(CDFS)):
        overflow = SIZES[t] - 2
        for v in (INT32_MIN, INT32_MAX, OFFSETS[t] - 1, OFFSETS[t] + overflow, OFFSETS[t] - 2, OFFSETS[t] + overflow + 1):
            sym.append(v)
            idx.append(t)
    fill_s, fill_i = _draw(rng, 70 - len(sym))
    order = rng.permutation(70)
    add("escapes_int32_ends", [70], 16384, 1, sym=np.concatenate([np.array(sym, np.int64), fill_s])[order].astype(np.int32),
        idx=np.concatenate([np.array(idx, np.int32), fill_i])[order].astype(np.int32))
    add("zero_probability_bins", [150, 90], 80, 2, only=3)
    return out


def ref_encode(name):
    sym, idx, runs, spw, _ = cases()[name]
    return R.encode(sym.tolist(), idx.tolist(), runs, CDFS, SIZES, OFFSETS, spw)


def ref_decode(stream, name):
    """symbols, or None where the restatement reports failure"""
    _, idx, runs, _, _ = cases()[name]
    try:
        return R.decode(stream, idx.tolist(), runs, CDFS, SIZES, OFFSETS)
    except R.Corrupt:
        return None


@functools.lru_cache(maxsize=None)
def corruptions():
    """[(label, case name, bytes, symbols the restatement decodes or None)]: single flipped bits and truncations of two
    valid streams, and length tables that disagree with the string.  Positions come from a fixed seed; which of them
    fail is decided by running the restatement."""
    rng = np.random.default_rng(7)
    out = []
    for name in ("r10_unequal", "escapes_int32_ends"):
        good = ref_encode(name)
        G = cases()[name][4]
        head = 8 + 4 * G
        spots = list(range(8 * head))                                           # every bit of header and length table
        spots += [8 * head + int(b) for b in rng.integers(0, 8 * 256 * G, 24)]    # initial states (bodies are >= 256)
        spots += [int(b) for b in rng.integers(8 * head, 8 * len(good), 40)]      # anywhere in the bodies
        for bit in sorted(set(spots)):
            bad = bytearray(good)
            bad[bit // 8] ^= 1 << (bit % 8)
            out.append((f"{name}:bit{bit}", name, bytes(bad)))
        for cut in (1, 2, 3, 64, len(good) // 2, len(good) - 7, len(good)):
            out.append((f"{name}:cut{cut}", name, good[:len(good) - cut]))
        out.append((f"{name}:extra2", name, good + b"\0\0"))
        # a length table that disagrees with the string: two words moved from the last body to the first
        if G > 1:
            lens = list(struct.unpack_from(f"<{G}I", good, 8))
            lens[0] += 4
            lens[-1] -= 4
            out.append((f"{name}:lengths_shifted", name, good[:8] + struct.pack(f"<{G}I", *lens) + good[head:]))
    return [(label, name, data, ref_decode(data, name)) for label, name, data in out]
