"""The input of the ranged lane-decoder tests (tests/test_rans_lanes_waves.py on the host decoder,
tests/test_gpu_rans_lanes_waves.py on the device decoder): a residual string in small -- four runs under the residual
layer's tables, the class map and three planes, escapes included -- coded by the host encoder with a small
``symbols_per_wave``, so that a 40 x 50 image gives G = 16 waves; and the wave arithmetic the tests compare against,
restated here from the format's words (icm_amd/bitstream.py): wave g owns the elements [g c, min(n, (g + 1) c)) of a run
of n, c = the per-wave share rounded up to whole steps of 64."""
import struct

import numpy as np

H, W = 40, 50
SPW = 128
NCLASSES = 19


def chunk(n, G):
    return (-(-n // G) + 63) // 64 * 64


def owned(n, G, g0, g1):
    """[lo, hi): the elements of a run of n that the waves [g0, g1) own (empty: lo == hi)"""
    c = chunk(n, G)
    lo, hi = min(n, g0 * c), min(n, g1 * c)
    return lo, max(lo, hi)


def make():
    """(symbols, indexes, run lengths, string, G, host tables)"""
    from icm_amd import ans
    from icm_amd import residual as R
    rng = np.random.default_rng(2024)
    gh, gw = R.grid(H, W)
    cls = rng.integers(0, NCLASSES, size=(gh, gw)).astype(np.int32)
    idx_plane = np.repeat(np.repeat(cls, R.CELL, axis=0), R.CELL, axis=1)[:H, :W]
    idx = np.broadcast_to(idx_plane, (3, H, W)).astype(np.int32)
    # magnitudes that follow the class, and one sample in 23 far outside every table's support: the escape path
    q = np.rint(rng.laplace(0.0, 0.2 + idx / 2.0)).astype(np.int64)
    far = rng.integers(0, 23, size=q.shape) == 0
    q = np.where(far, rng.integers(-70000, 70001, size=q.shape), q).astype(np.int32)
    symbols = np.concatenate([cls.reshape(-1), q.reshape(-1)]).astype(np.int32)
    indexes = np.concatenate([np.full(cls.size, NCLASSES, np.int32), idx.reshape(-1)]).astype(np.int32)
    runs = [int(cls.size), H * W, H * W, H * W]
    t = R.tables()._tables()
    string = ans.lanes_encode(symbols, indexes, runs, t, SPW)
    G = struct.unpack_from("<H", string, 6)[0]
    # the cases need escapes in every plane, at least one wave that owns nothing of the class run, and words everywhere
    sup = np.asarray(R.SUPPORTS)[idx]
    assert (np.abs(q.astype(np.int64)) > sup).reshape(3, -1).any(axis=1).all()
    assert G == 16 and owned(runs[0], G, 1, G) == (runs[0], runs[0])
    return symbols, indexes, runs, string, G, t


def run_slices(runs):
    """[(offset of run r in the concatenated arrays, its length)]"""
    offs = np.concatenate([[0], np.cumsum(runs)[:-1]]).tolist()
    return list(zip(offs, runs))


def ranges(G):
    """(g0, g1, lead): the ranges of the issue -- the first wave, the last, an empty one, a middle one whose buffers
    start ``lead`` elements before its first (elem0 = g0 c - lead > 0), and all waves"""
    return [(0, 1, 0), (G - 1, G, 0), (5, 5, 0), (3, 9, 0), (3, 9, 70), (0, G, 0)]


def body_spans(string):
    """[(offset of the body's first word, number of its words)] from the header's length table"""
    G = struct.unpack_from("<H", string, 6)[0]
    lens = struct.unpack_from(f"<{G}I", string, 8)
    pos, out = 8 + 4 * G, []
    for n in lens:
        out.append((pos + 256, (n - 256) // 2))
        pos += n
    return out


def corrupt_word(string, g):
    """the string with the first 16-bit word of body g inverted: the low half of lane 0's initial state, the first
    cumulative value that lane decodes, so the damage runs through the lane's whole chain and its end state.  (The three
    payload words of an escape, by contrast, are raw bits that no check of the format covers.)"""
    off, _ = body_spans(string)[g]
    bad = bytearray(string)
    p = off - 256
    bad[p] ^= 0xFF
    bad[p + 1] ^= 0xFF
    return bytes(bad)


def buffers(n, G, g0, g1, lead):
    """(elem0, end): the elements [elem0, end) that the buffers of a ranged call hold -- from ``lead`` before the first
    element of wave g0 (never before the run's first) to the last element the range owns"""
    lo, hi = owned(n, G, g0, g1)
    elem0 = max(0, g0 * chunk(n, G) - lead)
    return elem0, max(elem0, hi)
