"""CPU: the residual layer under a bound per 16 x 16-pixel cell without a GPU -- the guarantee over every (x, xhat, D)
with the bounds laid out as a map, ``codec.error_map`` against the pixel-by-pixel painter of
tests/_residual_map_ref.py, the ICME container of icm_amd/bitstream.py with each of its refusals, and that every case
of the GPU kernel test reaches the path it is named for."""
import struct
import zlib

import numpy as np
import pytest

import _residual_map_ref as MR


# ------------------------------------------------------------------------------------------------- arithmetic
def test_the_bound_holds_for_every_triple_under_every_cells_bound_and_zero_is_the_identity():
    """the exhaustive walk of tests/test_residual_ref.py, per cell: an image of 33 cells in a row, cell D holding every
    (x, xhat) byte pair under the bound D"""
    pair = np.arange(65536)
    n = MR.MAX_ERROR + 1
    # 256 rows of cells, each cell holding 256 of the 65536 pairs; 33 columns of cells, column D under the bound D
    col_x, col_xhat = ((v.reshape(256 * 16, 16)[..., None]).astype(np.uint8) for v in (pair // 256, pair % 256))
    X, Xh = (np.tile(v, (1, n, 3)) for v in (col_x, col_xhat))
    dmap = np.tile(np.arange(n, dtype=np.uint8), (256, 1))
    assert dmap.shape == MR.grid(*X.shape[:2])
    q = MR.quantise_map(X, Xh, dmap)
    out = MR.reconstruct_map(Xh, q, dmap)
    err = np.abs(out.astype(np.int64) - X.astype(np.int64))
    bound = MR.per_pixel(dmap, *X.shape[:2])
    assert (err <= bound[..., None]).all()
    for d in range(n):
        col = slice(d * 16, (d + 1) * 16)
        assert int(err[:, col].max()) == d                                         # attained: the bound is tight
        assert int(np.abs(q[:, :, col]).max()) == (255 + d) // (2 * d + 1)
        # every pair occurs in the column
        seen = set(zip(X[:, col, 0].reshape(-1).tolist(), Xh[:, col, 0].reshape(-1).tolist()))
        assert len(seen) == 65536
    assert np.array_equal(out[:, :16], X[:, :16])                                  # D = 0 is the identity


def test_a_uniform_map_is_the_scalar_rule_and_a_window_is_a_crop():
    import _residual_ref as RR
    x, xhat = MR.random_pair(37, 53, 3)
    for d in (0, 1, 32):
        dmap = np.full(MR.grid(37, 53), d, np.uint8)
        q = MR.quantise_map(x, xhat, dmap)
        assert np.array_equal(q, RR.quantise(x, xhat, d))
        assert np.array_equal(MR.reconstruct_map(xhat, q, dmap), RR.reconstruct(xhat, q, d))
    dmap = MR.random_map(37, 53, 1)
    q = MR.quantise_map(x, xhat, dmap)
    full = MR.reconstruct_map(xhat, q, dmap)
    for win in ((3, 13, 21, 31), (15, 15, 2, 2), (36, 52, 1, 1)):
        y0, x0, h, w = win
        assert np.array_equal(MR.reconstruct_map(xhat[y0:y0 + h, x0:x0 + w], q, dmap, win), full[y0:y0 + h, x0:x0 + w])
    over = dmap.copy()
    over[dmap == 32] = 200                                                         # a byte above 32 counts as 32
    assert np.array_equal(MR.quantise_map(x, xhat, over), q)


def test_the_kernels_reciprocal_is_the_division_for_every_clamped_byte():
    for byte in range(256):
        s = 2 * min(byte, 32) + 1
        nn = np.arange(0, 255 + 32 + 1, dtype=np.int64)
        assert np.array_equal((nn * (65536 // s + 1)) >> 16, nn // s), byte


# ------------------------------------------------------------------------------------------------- painter
PAINT = [
    ("one-pixel-on-a-cell-corner", 37, 53, 4, [(16, 16, 1, 1, 0)]),
    ("one-pixel-before-the-corner", 37, 53, 4, [(15, 15, 1, 1, 0)]),
    ("across-the-corner", 37, 53, 4, [(15, 15, 2, 2, 1)]),
    ("partial-edge-cells", 37, 53, 4, [(33, 49, 4, 4, 0), (0, 48, 37, 5, 2)]),
    ("last-pixel", 37, 53, 7, [(36, 52, 1, 1, 32)]),
    ("later-wins", 64, 48, 4, [(0, 0, 40, 40, 32), (10, 10, 10, 10, 0), (16, 20, 1, 20, 1)]),
    ("later-loses-to-none", 64, 48, 4, [(10, 10, 10, 10, 0), (0, 0, 40, 40, 32)]),
    ("whole-image", 17, 33, 9, [(0, 0, 17, 33, 0)]),
    ("equal-to-the-background", 17, 33, 9, [(3, 3, 5, 20, 9)]),
    ("none", 17, 33, 9, []),
]


@pytest.mark.parametrize("name,H,W,base,rois", PAINT, ids=[c[0] for c in PAINT])
def test_error_map_is_the_pixel_by_pixel_painter(name, H, W, base, rois):
    from icm_amd import codec
    got = codec.error_map(H, W, base, rois)
    want = MR.paint(H, W, base, rois)
    assert got.dtype == np.uint8 and got.shape == MR.grid(H, W) and np.array_equal(got, want)
    if name == "one-pixel-on-a-cell-corner":
        assert int((got != base).sum()) == 1 and got[1, 1] == 0
    if name == "across-the-corner":
        assert int((got != base).sum()) == 4
    if name == "later-wins":
        assert got[0, 0] == 0 and got[1, 1] == 1 and got[2, 2] == 32 and got[3, 0] == 4
    if name == "later-loses-to-none":
        assert (got[:3, :3] == 32).all()


def test_error_rois_are_checked_in_one_place():
    from icm_amd import codec
    assert codec.check_error_rois([(0, 0, 1, 1, 0), (36, 52, 1, 1, np.int64(32))], 37, 53) == \
        [(0, 0, 1, 1, 0), (36, 52, 1, 1, 32)]
    for bad in ([(0, 0, 1, 1, -1)], [(0, 0, 1, 1, 33)], [(0, 0, 1, 1, 1.0)], [(0, 0, 1, 1)], [(0, 0, 38, 1, 1)],
                [(0, 50, 1, 4, 1)], [(-1, 0, 1, 1, 1)], [(0, 0, 0, 1, 1)], 5):
        with pytest.raises(ValueError):
            codec.check_error_rois(bad, 37, 53)
        with pytest.raises(ValueError):
            codec.error_map(37, 53, 4, bad)
    for base in (-1, 33, None, 2.0):
        with pytest.raises(ValueError):
            codec.error_map(37, 53, base, [])


def test_the_wrappers_check_the_host_map():
    from icm_amd import residual as R
    good = np.zeros(MR.grid(37, 53), np.uint8)
    assert R.check_error_map(good, 37, 53) is not None
    for bad in (good.astype(np.int32), good[:, :-1], good.reshape(-1), np.full_like(good, 33)):
        with pytest.raises(ValueError):
            R.check_error_map(bad, 37, 53)


# ------------------------------------------------------------------------------------------------- container
def _base():
    from icm_amd import bitstream as B
    return B.pack({"arch": "cnn", "height": 37, "width": 53, "pads": (5, 6, 13, 14), "shape": (1, 1),
                   "fingerprint": 0x1234ABCD}, [b"yy" * 9, b"z" * 5])


HEAD = {"coder": "lanes", "height": 37, "width": 53, "table_crc": 0xDEADBEEF}
DMAP = MR.paint(37, 53, 4, [(0, 0, 20, 20, 32), (3, 3, 5, 5, 0), (20, 40, 3, 3, 1)])


def _recrc(body: bytes) -> bytes:
    return body + struct.pack("<I", zlib.crc32(body) & 0xFFFFFFFF)


def _with_map_string(data: bytes, string: bytes, top=None) -> bytes:
    """``data`` with its bound-map string replaced (lengths and CRC made right, the header's maximum set to ``top``)"""
    nbase, nmap, nres = struct.unpack_from("<III", data, 20)
    body = bytearray(data[:32 + nbase] + string + data[32 + nbase + nmap:-4])
    struct.pack_into("<I", body, 24, len(string))
    if top is not None:
        body[6] = top
    return _recrc(bytes(body))


def test_the_map_string_is_the_restatements():
    from icm_amd import bitstream as B
    for dmap in (DMAP, MR.random_map(64, 48, 2), MR.window_map(37, 53)):
        s = B.error_map_string(dmap)
        assert s == MR.map_string(dmap) and np.array_equal(MR.map_from_string(s), dmap)
    # a run longer than a count holds: full counts first, and the reader takes the one exception to maximal runs
    big = np.zeros((300, 300), np.uint8)
    big[-1, -1] = 32
    s = B.error_map_string(big)
    assert s == MR.map_string(big) and struct.unpack_from("<HB", s, 4) == (65535, 0)
    assert np.array_equal(B.error_map_from_string(s, 300 * 16, 300 * 16), big)


def test_container_pack_and_unpack_are_inverse():
    from icm_amd import bitstream as B
    base, res = _base(), bytes(range(200))
    data = B.pack_residual_map(HEAD, base, DMAP, res)
    assert B.is_residual_map(data) and not B.is_residual(data) and not B.is_tiled(data) and not B.is_residual_map(base)
    assert data[:4] == b"ICME" and struct.unpack_from("<H", data, 4)[0] == 1 and data[6] == 32 and data[7] == 1
    string = MR.map_string(DMAP)
    assert struct.unpack_from("<IIIIII", data, 8) == (37, 53, 0xDEADBEEF, len(base), len(string), len(res))
    assert data[32:-4] == base + string + res
    assert len(data) == B.RESIDUAL_MAP_FIXED_BYTES + len(base) + len(string) + len(res) + B.CRC_BYTES
    assert struct.unpack_from("<I", data, len(data) - 4)[0] == zlib.crc32(data[:-4]) & 0xFFFFFFFF
    head, b2, m2, r2 = B.unpack_residual_map(data)
    assert head == {**HEAD, "max_error": 32} and b2 == base and r2 == res
    assert m2.dtype == np.uint8 and np.array_equal(m2, DMAP)
    assert B.unpack_residual_map(data, 0xDEADBEEF)[0] == head
    assert B.pack_residual_map(head, b2, m2, r2) == data
    tiled = B.pack_tiled({"arch": "cnn", "height": 37, "width": 53, "tile": 64, "overlap": 0, "fingerprint": 1}, [base])
    assert B.unpack_residual_map(B.pack_residual_map(HEAD, tiled, DMAP, res))[1] == tiled
    # the header's maximum is the map's, not the format's
    low = np.minimum(DMAP, 5)
    assert B.unpack_residual_map(B.pack_residual_map(HEAD, base, low, res))[0]["max_error"] == 5


def test_a_uniform_map_yields_the_bytes_of_pack_residual():
    from icm_amd import bitstream as B
    base, res = _base(), bytes(range(100))
    for d in (0, 4, 32):
        data = B.pack_residual_map(HEAD, base, np.full(MR.grid(37, 53), d, np.uint8), res)
        assert data == B.pack_residual({**HEAD, "max_error": d}, base, res) and B.is_residual(data)
    with pytest.raises(ValueError, match="uniform"):
        B.error_map_string(np.full((3, 4), 2, np.uint8))


def test_the_writer_refuses_a_bad_map():
    from icm_amd import bitstream as B
    base, res = _base(), b"r"
    for bad, what in ((DMAP.astype(np.int8), "uint8"), (DMAP[:, :-1], "bound map of a"), (np.maximum(DMAP, 33), "max_error")):
        with pytest.raises(ValueError, match=what):
            B.pack_residual_map(HEAD, base, bad, res)
    with pytest.raises(ValueError, match="largest bound"):
        B.pack_residual_map({**HEAD, "max_error": 31}, base, DMAP, res)
    with pytest.raises(ValueError, match="base"):
        B.pack_residual_map(HEAD, b"nope" + base[4:], DMAP, res)
    with pytest.raises(ValueError, match="lacks"):
        B.pack_residual_map({"coder": "host"}, base, DMAP, res)


def _runs(dmap):
    s = MR.map_string(dmap)
    return [struct.unpack_from("<HB", s, off) for off in range(4, len(s), 3)]


def _string(gh, gw, runs):
    return struct.pack("<HH", gh, gw) + b"".join(struct.pack("<HB", c, d) for c, d in runs)


def test_every_refusal_raises_value_error_naming_its_condition():
    from icm_amd import bitstream as B
    base, res = _base(), bytes(range(100))
    data = B.pack_residual_map(HEAD, base, DMAP, res)
    gh, gw = DMAP.shape
    runs = _runs(DMAP)
    assert _with_map_string(data, _string(gh, gw, runs)) == data
    first = next(i for i, (c, d) in enumerate(runs) if c >= 2)
    split = runs[:first] + [(1, runs[first][1]), (runs[first][0] - 1, runs[first][1])] + runs[first + 1:]
    top_run = next(i for i, (c, d) in enumerate(runs) if d == 32)
    refusals = [
        ("a wrong grid against H, W", _with_map_string(data, _string(gw, gh, runs)), "grid"),
        ("a header maximum that is not the map's", _with_map_string(data, _string(gh, gw, runs), top=31), "largest bound"),
        ("a zero count", _with_map_string(data, _string(gh, gw, runs[:1] + [(0, 7)] + runs[1:])), "count of 0"),
        ("runs short of the grid", _with_map_string(data, _string(gh, gw, runs[:-1])), "cover"),
        ("runs past the grid", _with_map_string(data, _string(gh, gw, runs[:-1] + [(runs[-1][0] + 1, runs[-1][1])])),
         "go past"),
        ("a non-maximal run", _with_map_string(data, _string(gh, gw, split)), "not maximal"),
        ("a d above 32", _with_map_string(data, _string(gh, gw, [(c, 33 if i == top_run else d)
                                                                 for i, (c, d) in enumerate(runs)]), top=32), "outside"),
        ("a single distinct value", _with_map_string(data, _string(gh, gw, [(gh * gw, 4)]), top=4), "single"),
        ("trailing bytes in the map string", _with_map_string(data, _string(gh, gw, runs) + b"\0"), "trailing"),
        ("a trailing run in the map string", _with_map_string(data, _string(gh, gw, runs + [(1, 9)])), "trailing"),
        ("trailing bytes after the CRC", data + b"\0", "trailing"),
        ("a bad CRC", data[:-1] + bytes([data[-1] ^ 1]), "CRC"),
        ("a bad base magic", _recrc(data[:32] + b"nope" + data[36:-4]), "base"),
    ]
    for what, bad, match in refusals:
        with pytest.raises(ValueError, match=match):
            B.unpack_residual_map(bad)
            pytest.fail(what)
    with pytest.raises(ValueError, match="table mismatch"):                  # other tables
        B.unpack_residual_map(data, 0xDEADBEEE)
    # a single distinct value on the right grid, in runs the 65535 exception allows
    big = np.zeros((256, 256), np.uint8)
    big[-1, -1] = 1
    bh = {**HEAD, "height": 4096, "width": 4096}
    bdata = B.pack_residual_map(bh, base, big, res)
    assert np.array_equal(B.unpack_residual_map(bdata)[2], big)
    with pytest.raises(ValueError, match="single"):
        B.unpack_residual_map(_with_map_string(bdata, _string(256, 256, [(65535, 0), (1, 0)]), top=0))
    # a flipped byte anywhere, the map string included: ValueError and nothing else
    nmap = struct.unpack_from("<I", data, 24)[0]
    for pos in [0, 5, 6, 7, 9, 17, 21, 25, 29, len(data) - 1] + list(range(32 + len(base), 32 + len(base) + nmap)):
        bad = bytearray(data)
        bad[pos] ^= 0x40
        with pytest.raises(ValueError):
            B.unpack_residual_map(bytes(bad))
    for cut in (0, 3, 10, B.RESIDUAL_MAP_FIXED_BYTES, len(data) - 1):           # truncated
        with pytest.raises(ValueError):
            B.unpack_residual_map(data[:cut])
    for field, v in ((4, 2), (7, 2)):                                         # version, coder id
        bad = bytearray(data[:-4])
        bad[field] = v
        with pytest.raises(ValueError, match="version|coder"):
            B.unpack_residual_map(_recrc(bytes(bad)))
    with pytest.raises(ValueError):
        B.unpack_residual_map("ICME")


def test_each_reader_refuses_the_others_magic():
    from icm_amd import bitstream as B
    base, res = _base(), bytes(range(50))
    mapped = B.pack_residual_map(HEAD, base, DMAP, res)
    scalar = B.pack_residual({**HEAD, "max_error": 3}, base, res)
    with pytest.raises(ValueError, match="magic"):
        B.unpack_residual(mapped)                        # what a reader from before the container does
    with pytest.raises(ValueError, match="magic"):
        B.unpack_residual_map(scalar)
    for reader in (B.unpack, B.unpack_tiled):
        with pytest.raises(ValueError, match="magic"):
            reader(mapped)
    with pytest.raises(ValueError):
        B.coder_of(mapped)
    assert B.RESIDUAL_VERSION == 1 and B.RESIDUAL_MAGIC == b"ICMR"


# ------------------------------------------------------------------------------------------------- CLI
def test_cli_refuses_before_any_gpu_work(tmp_path, capsys):
    """exit 2 for what the arguments rule out, exit 4 for a file that is not one stream: both before the GPU is asked for"""
    from PIL import Image
    from icm_amd import bitstream as B
    from icm_amd import codec
    src, stream = str(tmp_path / "in.png"), str(tmp_path / "x.icme")
    Image.fromarray(MR.random_pair(37, 53, 1)[0]).save(src)
    common = ["encode", src, "-o", stream, "-a", "cnn", "-p", str(tmp_path / "none.pt")]
    assert codec.main(common + ["--error-roi", "0,0,16,16:0"]) == 2
    assert "max-error" in capsys.readouterr().err
    for roi in ("30,0,8,1:0", "0,50,1,4:0", "0,0,16,16:33", "0,0,16,16:-1"):   # outside the image; a bound outside 0..32
        assert codec.main(common + ["--max-error", "4", "--error-roi", roi]) == 2, roi
        assert "error-roi" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:                                       # not five integers: argparse's own exit
        codec.main(common + ["--max-error", "4", "--error-roi", "0,0,16:1"])
    assert e.value.code == 2
    assert codec.main(common + ["--max-error", "4", "--error-roi", "0,0,16,16:0", "--target-bytes", "5000"]) == 2
    assert "max-error" in capsys.readouterr().err
    assert not (tmp_path / "x.icme").exists()
    # decode: a flipped byte in the map string, and a stream cut short
    data = B.pack_residual_map(HEAD, _base(), DMAP, b"r" * 40)
    bad = bytearray(data)
    bad[32 + len(_base()) + 5] ^= 0x10
    for k, (payload, what) in enumerate(((bytes(bad), "CRC"), (data[:-7], "truncated"))):
        path = str(tmp_path / f"bad{k}.icme")
        with open(path, "wb") as f:
            f.write(payload)
        assert codec.main(["decode", path, "-o", str(tmp_path / "out.png"), "-p", str(tmp_path / "none.pt")]) == 4
        assert what in capsys.readouterr().err
    assert not (tmp_path / "out.png").exists()


# ------------------------------------------------------------------------------------------------- the GPU cases
def test_every_gpu_case_reaches_the_path_it_is_named_for():
    cases = MR.kernel_cases()
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    seen, seen_map = set(), set()
    for c in cases:
        H, W = c["x"].shape[:2]
        got = MR.run_paths(H, W, c["byte_offset"], c["elem_offset"])
        assert c["paths"] <= got, c["name"]
        if "odd-pointers" in c["name"]:
            assert "dword" not in got and "vec" not in got, c["name"]
        assert c["map_paths"] <= MR.map_paths(c["dmap"]), c["name"]
        assert c["dmap"].dtype == np.uint8 and c["dmap"].shape == MR.grid(H, W) and int(c["dmap"].max()) <= 32
        seen |= got
        seen_map |= MR.map_paths(c["dmap"])
    assert seen == {"dword", "byte", "vec", "scalar", "full", "partial"} and {"0|32", "uniform"} <= seen_map
    for H, W in MR.SHAPES:
        assert f"random-{H}x{W}" in names and f"extreme-{H}x{W}" in names and f"extreme-rev-{H}x{W}" in names
    # bounds 0 and 32 in neighbouring cells of every shape that has neighbours
    for c in cases:
        if c["name"].startswith(("random-", "extreme")) and max(c["x"].shape[:2]) > 16 and "16x16" not in c["name"]:
            assert "0|32" in MR.map_paths(c["dmap"]), c["name"]
    # the clamp has work to do on either side under a map too
    lo = hi = False
    for c in cases:
        s = 2 * MR.per_pixel(c["dmap"], *c["x"].shape[:2])[..., None] + 1
        v = c["xhat"].astype(np.int64) + MR.quantise_map(c["x"], c["xhat"], c["dmap"]).transpose(1, 2, 0) * s
        lo, hi = lo or bool((v < 0).any()), hi or bool((v > 255).any())
    assert lo and hi


def test_every_window_case_reaches_the_path_it_is_named_for():
    cases = MR.window_cases()
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    seen = set()
    for c in cases:
        H, W = c["shape"]
        y0, x0, h, w = c["window"]
        assert 0 <= y0 and 0 <= x0 and h >= 1 and w >= 1 and y0 + h <= H and x0 + w <= W, c["name"]
        got = MR.window_paths(H, W, c["window"], c["dmap"])
        assert c["paths"] <= got, (c["name"], got)
        seen |= got
    # "a run of four crosses a cell boundary between two different bounds", 0 against 32, at x = 16 and at x = 32
    assert {"straddle", "straddle-differ", "straddle-0|32", "partial-straddle", "row-boundary", "one-cell"} <= seen
    for H, W in MR.WINDOW_SHAPES:
        for y0 in MR.WINDOW_Y0:
            for x0 in MR.WINDOW_X0:
                c = cases[names.index(f"{H}x{W}-y{y0}-x{x0}")]
                assert c["window"][:2] == (y0, x0)
                if x0 in (13, 14, 15):
                    # runs that hold pixels on both sides of x = 16, and of x = 32
                    w = c["window"][3]
                    crossing = [x0 + r for r in range(0, w, 4) if x0 + r < 16 <= x0 + min(r + 3, w - 1)]
                    crossing32 = [x0 + r for r in range(0, w, 4) if x0 + r < 32 <= x0 + min(r + 3, w - 1)]
                    assert crossing and crossing32, c["name"]
    one = cases[names.index("37x53-one-pixel")]
    assert one["window"][2:] == (1, 1)
    # a run that takes the first pixel's bound for all four, or the last one's, is caught: the windows hold runs whose
    # pixels differ in their bound, with the boundary after the first, the second and the third pixel
    splits = set()
    for c in cases:
        H, W = c["shape"]
        y0, x0, h, w = c["window"]
        for r in range(0, w, 4):
            px = [x0 + r + j for j in range(min(4, w - r))]
            cut = [j for j in range(1, len(px)) if px[j] // 16 != px[j - 1] // 16]
            splits |= set(cut)
    assert splits == {1, 2, 3}
