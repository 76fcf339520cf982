"""CPU: the tile plan of a tiled image (icm_amd/codec.py ``plan_tiles``) and its container (icm_amd/bitstream.py
``pack_tiled`` / ``unpack_tiled``).  Host only: nothing here loads the HIP library."""
import math
import struct
import zlib

import numpy as np
import pytest

import _tiles_ref as R
from icm_amd import bitstream as B
from icm_amd import codec

LENGTHS = [1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 160, 161, 191, 192, 193, 200, 255, 256, 257, 280,
           300, 383, 384, 385, 1000]
GEOMETRIES = [(t, m) for t in (64, 128) for m in sorted({0, 1, 32, t // 2})]


def _axis(L, tile, m):
    """(origin, size) of the tiles along one axis, read off a plan whose other axis is one pixel long"""
    rows, cols, plan = codec.plan_tiles(L, 1, tile, m)
    assert cols == 1 and len(plan) == rows and all(t[1] == 0 and t[3] == 1 for t in plan)
    return [(t[0], t[2]) for t in plan]


@pytest.mark.parametrize("tile,m", GEOMETRIES)
def test_axis_follows_the_formula(tile, m):
    S = tile - m
    for L in LENGTHS:
        ax = _axis(L, tile, m)
        n = max(1, math.ceil((L - m) / S))
        assert len(ax) == n, (L, tile, m)
        assert [o for o, _ in ax] == [k * S for k in range(n)]
        assert [s for _, s in ax] == [min(tile, L - k * S) for k in range(n)]
        assert all(m < s <= tile for _, s in ax) or (n == 1 and ax[0][1] == L)     # wider than the band, within the extent
        cover = np.zeros(L, np.int64)
        for o, s in ax:
            assert 0 <= o and o + s <= L
            cover[o:o + s] += 1
        assert cover.min() >= 1 and cover.max() <= 2, (L, tile, m)                 # every pixel in one or two tiles
        for (o0, s0), (o1, _) in zip(ax, ax[1:]):
            assert o0 + s0 - o1 == m                                               # the shared band: exactly m wide
        assert int((cover == 2).sum()) == m * (n - 1)
        if L <= tile:
            assert ax == [(0, L)]


@pytest.mark.parametrize("tile,m", GEOMETRIES)
def test_plan_is_the_row_major_product_of_its_axes(tile, m):
    for H, W in [(1, 1), (64, 64), (100, 120), (200, 280), (129, 63), (257, 385), (tile, tile + 1), (tile + 1, tile)]:
        rows, cols, plan = codec.plan_tiles(H, W, tile, m)
        ys, xs = _axis(H, tile, m), _axis(W, tile, m)
        assert (rows, cols) == (len(ys), len(xs)) == B.tile_grid(H, W, tile, m)
        assert plan == [(y, x, h, w) for y, h in ys for x, w in xs]
        if H <= tile and W <= tile:
            assert plan == [(0, 0, H, W)]                                          # fits one tile: a one-entry plan


@pytest.mark.parametrize("tile,m", GEOMETRIES)
def test_blend_weights_sum_to_one_at_every_pixel(tile, m):
    """float64 weights of all tiles over a pixel: (a + b)(c + d) expanded, a + b = c + d = 1 up to one rounding of each
    ramp entry -- at most four products and three sums of numbers <= 1, each within 2^-53: far inside 2e-15"""
    for H, W in [(200, 280), (129, 63), (257, 385), (64, 300)]:
        rows, cols, plan = codec.plan_tiles(H, W, tile, m)
        total = np.zeros((H, W), np.float64)
        for k, (y0, x0, h, w) in enumerate(plan):
            e = R.edges_of(k // cols, k % cols, rows, cols)
            assert e == codec.tile_edges(k // cols, k % cols, rows, cols)
            wy = R.weights(h, m, e & R.EDGE_TOP, e & R.EDGE_BOTTOM, np.float64)
            wx = R.weights(w, m, e & R.EDGE_LEFT, e & R.EDGE_RIGHT, np.float64)
            total[y0:y0 + h, x0:x0 + w] += wy[:, None] * wx[None, :]
        assert np.abs(total - 1.0).max() <= 2e-15, (H, W, tile, m)


def test_ramp_is_the_f32_quotient():
    for m in (1, 2, 8, 32, 64):
        r = codec.blend_ramp(m)
        assert r.dtype == np.float32 and r.shape == (m,)
        assert r.tobytes() == R.ramp(m).tobytes()
        assert r.tobytes() == np.array([np.float32(i + 0.5) / np.float32(m) for i in range(m)], np.float32).tobytes()


@pytest.mark.parametrize("tile,m", [(0, 0), (32, 0), (63, 0), (65, 0), (96, 0), (100, 10), (32768 + 64, 0), (65536, 0),
                                    (64, -1), (128, -32), (64, 33), (128, 65), (128, 128), (64.0, 0), ("64", 0)])
def test_refused_plans(tile, m):
    with pytest.raises(ValueError):
        codec.plan_tiles(100, 100, tile, m)
    with pytest.raises(ValueError):
        B.tile_grid(100, 100, tile, m)


def test_plan_edges_of_the_accepted_range():
    assert codec.plan_tiles(100, 100, 64, 32)[:2] == (3, 3)           # 2 overlap == tile is allowed
    assert codec.plan_tiles(40000, 10, 32768, 0)[:2] == (2, 1)
    with pytest.raises(ValueError):
        codec.plan_tiles(0, 10, 64, 0)


# ------------------------------------------------------------------------------------------------------ container
HDR = {"arch": "cnn", "height": 200, "width": 280, "tile": 128, "overlap": 32, "fingerprint": 0xDEADBEEF}
STREAMS = [b"\x01\x02\x03", b"", b"\xff" * 5, b"tile-3", b"\x00", b"last one"]


def _recrc(body: bytes) -> bytes:
    return body + struct.pack("<I", zlib.crc32(body) & 0xFFFFFFFF)


@pytest.mark.parametrize("header,streams", [
    (HDR, STREAMS),
    (HDR, [b""] * 6),
    ({**HDR, "arch": "stf", "overlap": 0, "fingerprint": 0}, [bytes([k]) * (k + 1) for k in range(6)]),
    ({**HDR, "height": 64, "width": 65, "tile": 64, "overlap": 0}, [b"a", b"b"]),
    ({**HDR, "height": 10, "width": 10}, [b"only"]),                               # a one-tile grid packs too
    ({**HDR, "rows": 2, "cols": 3}, STREAMS),
    ({**HDR, "height": 32768 * 65535, "width": 1, "tile": 32768, "overlap": 0}, [b"x"] * 65535),   # the most rows
])
def test_pack_tiled_unpack_tiled_round_trip(header, streams):
    data = B.pack_tiled(header, streams)
    assert isinstance(data, bytes) and B.is_tiled(data)
    assert len(data) == B.TILED_FIXED_BYTES + 4 * len(streams) + sum(map(len, streams)) + B.CRC_BYTES
    h, s = B.unpack_tiled(data)
    rows, cols = B.tile_grid(header["height"], header["width"], header["tile"], header["overlap"])
    assert h == {**header, "rows": rows, "cols": cols} and s == list(streams)
    assert B.unpack_tiled(bytearray(data)) == (h, s)


def test_tiled_layout_is_the_documented_one():
    data = B.pack_tiled(HDR, STREAMS)
    assert data[:4] == b"ICMT" and B.TILED_FIXED_BYTES == 28
    assert struct.unpack_from("<HHIIHHHHI", data, 4) == (1, 0, 200, 280, 128, 32, 2, 3, 0xDEADBEEF)
    assert struct.unpack_from("<6I", data, 28) == tuple(len(s) for s in STREAMS)
    assert data[52:-4] == b"".join(STREAMS)
    assert struct.unpack_from("<I", data, len(data) - 4)[0] == zlib.crc32(data[:-4])


def test_every_proper_prefix_of_a_tiled_stream_is_refused():
    data = B.pack_tiled(HDR, STREAMS)
    for n in range(len(data)):
        with pytest.raises(ValueError):
            B.unpack_tiled(data[:n])


def test_every_single_byte_change_of_a_tiled_stream_is_refused():
    data = B.pack_tiled(HDR, STREAMS)
    assert 70 <= len(data) <= 110
    for i in range(len(data)):
        for delta in (1, 0x80, 0xFF):
            bad = bytearray(data)
            bad[i] = (bad[i] + delta) & 0xFF
            with pytest.raises(ValueError):
                B.unpack_tiled(bytes(bad))


def test_each_container_refuses_the_other_by_magic():
    tiled = B.pack_tiled(HDR, STREAMS)
    plain = B.pack({"arch": "cnn", "height": 175, "width": 201, "pads": (27, 28, 8, 9), "shape": (3, 4),
                    "fingerprint": 0xDEADBEEF}, [b"abc", b"de"])
    with pytest.raises(ValueError, match="magic"):
        B.unpack(tiled)
    with pytest.raises(ValueError, match="magic"):
        B.unpack_tiled(plain)
    assert B.is_tiled(tiled) and not B.is_tiled(plain) and not B.is_tiled(b"ICM") and not B.is_tiled(None)
    # whole ICMB streams travel inside an ICMT stream unchanged
    wrapped = B.pack_tiled({**HDR, "height": 64, "width": 65, "tile": 64, "overlap": 0}, [plain, plain])
    assert B.unpack(B.unpack_tiled(wrapped)[1][1])[1] == [b"abc", b"de"]


def test_tiled_refusals_are_named():
    body = bytearray(B.pack_tiled(HDR, STREAMS)[:-4])
    assert B.unpack_tiled(_recrc(bytes(body)))[1] == STREAMS                       # the helper writes a valid CRC

    def patched(fmt, offset, value):
        b = bytearray(body)
        struct.pack_into(fmt, b, offset, value)
        return _recrc(bytes(b))

    for data, name in [(patched("<H", 4, 2), "version"), (patched("<H", 6, len(B.ARCHS)), "architecture"),
                       (patched("<H", 20, 3), "tile grid"), (patched("<H", 22, 2), "tile grid"),
                       (patched("<I", 8, 100), "tile grid"),                      # 100 rows of pixels: one row of tiles
                       (patched("<H", 16, 100), "tile geometry"), (patched("<H", 18, 65), "tile geometry"),
                       (patched("<I", 8, 0), "empty"), (patched("<I", 28, 2 ** 32 - 1), "past the data"),
                       (_recrc(b"ICMX" + bytes(body[4:])), "magic"), (bytes(body) + b"\x00" * 4, "CRC")]:
        with pytest.raises(ValueError, match=name):
            B.unpack_tiled(data)
    good = _recrc(bytes(body))
    for extra in (b"\x00", b"ICMT", good):
        with pytest.raises(ValueError, match="trailing"):
            B.unpack_tiled(good + extra)
    for bad in (None, "ICMT", 7, [1, 2]):
        with pytest.raises(ValueError):
            B.unpack_tiled(bad)


def test_pack_tiled_refuses_bad_headers():
    for patch in ({"arch": "stf6"}, {"height": 0}, {"width": 2 ** 32}, {"tile": 100}, {"tile": 32}, {"overlap": 65},
                  {"overlap": -1}, {"fingerprint": -1}, {"fingerprint": 2 ** 32}, {"rows": 3}, {"cols": 2},
                  {"height": 1.5}):
        with pytest.raises(ValueError):
            B.pack_tiled({**HDR, **patch}, STREAMS)
    with pytest.raises(ValueError, match="lacks"):
        B.pack_tiled({k: v for k, v in HDR.items() if k != "tile"}, STREAMS)
    with pytest.raises(ValueError, match="tile streams"):
        B.pack_tiled(HDR, STREAMS[:5])
    with pytest.raises(ValueError):                                                # 65536 rows do not fit the field
        B.pack_tiled({**HDR, "height": 64 * 65536, "width": 1, "tile": 64, "overlap": 0}, [])
