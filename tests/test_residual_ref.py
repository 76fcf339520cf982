"""CPU: the error-bounded residual layer without a GPU -- the arithmetic's guarantee over every (x, xhat, D), the static
tables of icm_amd/residual.py against the restatement of tests/_residual_ref.py, round trips of the one string through
the host coder and the host lanes coder (escapes, a 1 x 1 image and a partial edge cell among them), the ICMR container
of icm_amd/bitstream.py, and that every case of the GPU kernel test reaches the path it is named for."""
import struct
import zlib

import numpy as np
import pytest
import torch

import _residual_ref as RR


# ------------------------------------------------------------------------------------------------- arithmetic
def test_the_bound_holds_for_every_triple_and_zero_is_the_identity():
    x, xhat = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    x, xhat = x.reshape(-1, 1, 1).repeat(3, 2).astype(np.uint8), xhat.reshape(-1, 1, 1).repeat(3, 2).astype(np.uint8)
    for d in range(RR.MAX_ERROR + 1):
        q = RR.quantise(x, xhat, d)
        out = RR.reconstruct(xhat, q, d)
        err = np.abs(out.astype(np.int64) - x.astype(np.int64))
        assert int(err.max()) <= d, d
        assert int(np.abs(q).max()) == RR.max_symbol(d)
        if d == 0:
            assert np.array_equal(out, x)
        else:
            assert int(err.max()) == d                                        # the bound is attained: it is tight


def test_the_kernels_reciprocal_is_the_division():
    """csrc/residual.hip divides by s = 2 D + 1 as (n m) >> 16 with m = 65536 div s + 1, n = |r| + D"""
    for d in range(RR.MAX_ERROR + 1):
        s = 2 * d + 1
        n = np.arange(0, 255 + d + 1, dtype=np.int64)
        assert np.array_equal((n * (65536 // s + 1)) >> 16, n // s), d


def test_apply_saturates_like_the_exact_integers_for_any_symbol():
    """the kernel clamps q to +-256 before the product; the reference does not"""
    xhat = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, 2)
    for qv in (-2 ** 31, -257, -256, -255, 255, 256, 257, 2 ** 31 - 1):
        q = np.full((3, 1, 256), qv, np.int64)
        for d in (0, 32):
            exact = RR.reconstruct(xhat, q, d)
            assert np.array_equal(exact, RR.reconstruct(xhat, np.clip(q, -256, 256), d))


# ------------------------------------------------------------------------------------------------- tables
def test_constants_agree_with_the_restatement():
    from icm_amd import residual as R
    assert list(R.THRESHOLDS) == RR.THRESHOLDS and R.NCLASSES == RR.NCLASSES == len(R.THRESHOLDS) + 1
    assert list(R.RATIOS) == [RR.ratio(k) for k in range(RR.NCLASSES)]
    assert list(R.SUPPORTS) == [len(RR.weights(k)) - 1 for k in range(RR.NCLASSES)]
    assert R.SUPPORTS[0] == 4 and R.SUPPORTS[-1] == 255 and list(R.SUPPORTS) == sorted(R.SUPPORTS)
    for k in range(RR.NCLASSES):
        assert [int(v) for v in R.class_weights(k)] == RR.weights(k, R.RATIOS[k])
        # the law's E|q| = 2 r / (1 - r^2) is the geometric mean of the class's bounds, to the ratio's 16 bits
        r = R.RATIOS[k] / 65536
        lo, hi = RR.class_bounds(k)
        assert 2 * r / (1 - r * r) == pytest.approx((lo * hi) ** 0.5, rel=2e-3)


def test_tables_are_the_restatements_and_well_formed():
    from icm_amd import residual as R
    t = R.ResidualTables()
    cdf, sizes, offsets = RR.tables()
    assert np.array_equal(t.cdf, cdf) and np.array_equal(t.sizes, sizes) and np.array_equal(t.offsets, offsets)
    assert t.cdf.dtype == t.sizes.dtype == t.offsets.dtype == np.int32 and t.cdf.shape[0] == RR.NCLASSES + 1
    for k in range(RR.NCLASSES + 1):
        row = t.cdf[k, :t.sizes[k]].astype(np.int64)
        assert row[0] == 0 and row[-1] == 1 << 16 and (np.diff(row) > 0).all(), k   # strictly increasing, ends at 2^16
    for k in range(RR.NCLASSES):
        L = R.SUPPORTS[k]
        assert t.sizes[k] == 2 * L + 3 and t.offsets[k] == -L                # the support -L .. L is symmetric; the escape bin
        f = np.diff(t.cdf[k, :t.sizes[k]].astype(np.int64))[:-1]            # without the escape bin
        assert int(np.argmax(f)) == L and (f[L] >= f).all() and (f >= 1).all()   # the mode is v = 0
    assert t.sizes[RR.NCLASSES] == RR.NCLASSES + 2 and t.offsets[RR.NCLASSES] == 0
    f = np.diff(t.cdf[RR.NCLASSES, :RR.NCLASSES + 1])
    assert (f == f[0]).all()                                                 # uniform over the classes
    again = R.ResidualTables()
    assert np.array_equal(again.cdf, t.cdf) and np.array_equal(again.sizes, t.sizes) and again.crc == t.crc
    assert np.array_equal(again.offsets, t.offsets) and R.tables().crc == t.crc
    crc = 0
    for a in (cdf, sizes, offsets):
        crc = zlib.crc32(a.astype("<i4").tobytes(), crc)
    assert t.crc == crc & 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------- round trips
def _planes(H, W, seed, spread):
    """synthetic q planes: small values, a busy corner, and samples far beyond any class's support"""
    rng = np.random.default_rng(seed)
    q = np.rint(rng.laplace(0, spread, size=(3, H, W))).astype(np.int32)
    q[:, :min(H, 5), :min(W, 7)] = rng.integers(-255, 256, size=(3, min(H, 5), min(W, 7)))
    if H > 16 and W > 16:                                # lone spikes in quiet cells: beyond their class's support
        q[0, H - 1, W - 1], q[1, H - 2, W - 3], q[2, 0, W - 1] = 200, -300, 70000
    return q


ROUND_TRIPS = [("1x1", 1, 1, 0.3), ("partial-edge-cell", 20, 37, 0.5), ("busy", 33, 48, 9.0)]


@pytest.mark.parametrize("name,H,W,spread", ROUND_TRIPS, ids=[c[0] for c in ROUND_TRIPS])
@pytest.mark.parametrize("coder", ["host", "lanes"])
def test_the_string_round_trips_through_the_host_coders(coder, name, H, W, spread):
    from icm_amd import ans
    from icm_amd import residual as R
    q = _planes(H, W, 3, spread)
    if name == "1x1":
        q[:] = [[[1000]], [[-3]], [[0]]]                 # the cell's class is the last one; 1000 is beyond its 255
    cls = RR.classes(q)
    sym, idx, runs = RR.string_layout(q, cls)
    t = R.tables()
    # escapes: samples beyond the support of their cell's class
    L = np.asarray(R.SUPPORTS)[idx[runs[0]:]]
    assert int((np.abs(sym[runs[0]:]) > L).sum()) >= 1
    if name == "partial-edge-cell":
        assert RR.grid(H, W) == (2, 3) and cls.shape == (2, 3)
    if coder == "host":
        c = ans.HostCoder()
        string = c.encode(torch.from_numpy(sym), torch.from_numpy(idx), runs, t)
        dec = c.decoder(string, t)
        got, pos = [], 0
        for n in runs:
            got.append(dec.decode_run(torch.from_numpy(idx[pos:pos + n])).numpy())
            pos += n
        dec.finish()
        dec.close()
        got = np.concatenate(got)
    else:
        string = ans.lanes_encode(sym, idx, runs, t._tables(), symbols_per_wave=256)
        got = ans.lanes_decode(string, idx, runs, t._tables())
    assert np.array_equal(got, sym)
    # what the decoder does with it: the class run gives the indexes of the rest
    assert np.array_equal(RR.indexes(got[:runs[0]], H, W).reshape(-1), idx[runs[0]:])


# ------------------------------------------------------------------------------------------------- container
def _base():
    from icm_amd import bitstream as B
    return B.pack({"arch": "cnn", "height": 20, "width": 37, "pads": (13, 14, 22, 22), "shape": (1, 1),
                   "fingerprint": 0x1234ABCD}, [b"yy" * 9, b"z" * 5])


HEAD = {"max_error": 3, "coder": "lanes", "height": 20, "width": 37, "table_crc": 0xDEADBEEF}


def test_container_pack_and_unpack_are_inverse():
    from icm_amd import bitstream as B
    base, res = _base(), bytes(range(200))
    data = B.pack_residual(HEAD, base, res)
    assert B.is_residual(data) and not B.is_tiled(data) and not B.is_residual(base)
    assert len(data) == B.RESIDUAL_FIXED_BYTES + len(base) + len(res) + B.CRC_BYTES
    head, b2, r2 = B.unpack_residual(data)
    assert head == HEAD and b2 == base and r2 == res
    assert B.unpack_residual(data, 0xDEADBEEF)[0] == HEAD
    assert B.pack_residual(head, b2, r2) == data
    for d in (0, 32):
        assert B.unpack_residual(B.pack_residual({**HEAD, "max_error": d, "coder": "host"}, base, b""))[0]["max_error"] == d
    # a tiled base
    tiled = B.pack_tiled({"arch": "cnn", "height": 20, "width": 37, "tile": 64, "overlap": 0, "fingerprint": 1}, [base])
    assert B.unpack_residual(B.pack_residual(HEAD, tiled, res))[1] == tiled


def _recrc(body: bytes) -> bytes:
    return body + struct.pack("<I", zlib.crc32(body) & 0xFFFFFFFF)


def test_container_refuses_what_is_not_one_stream():
    from icm_amd import bitstream as B
    base, res = _base(), bytes(range(100))
    data = B.pack_residual(HEAD, base, res)
    for pos in (0, 5, 6, 7, 9, 17, 21, 25, 30, len(data) // 2, len(data) - 5, len(data) - 1):   # a flipped byte
        bad = bytearray(data)
        bad[pos] ^= 0x40
        with pytest.raises(ValueError):
            B.unpack_residual(bytes(bad))
    with pytest.raises(ValueError, match="table mismatch"):                  # a reader with other tables
        B.unpack_residual(data, 0xDEADBEEE)
    for cut in (0, 3, 10, B.RESIDUAL_FIXED_BYTES, len(data) - 1):            # truncated
        with pytest.raises(ValueError):
            B.unpack_residual(data[:cut])
    body = bytearray(data[:-4])
    for off, delta in ((20, 1), (24, 1), (20, -1), (24, 1 << 20)):           # lengths that disagree with the data
        bad = bytearray(body)
        struct.pack_into("<I", bad, off, (struct.unpack_from("<I", bad, off)[0] + delta) & 0xFFFFFFFF)
        with pytest.raises(ValueError, match="truncated|trailing"):
            B.unpack_residual(_recrc(bytes(bad)))
    with pytest.raises(ValueError, match="trailing"):
        B.unpack_residual(data + b"\0")
    bad = bytearray(body)                                                    # D = 33 under a valid CRC
    bad[6] = 33
    with pytest.raises(ValueError, match="max_error"):
        B.unpack_residual(_recrc(bytes(bad)))
    with pytest.raises(ValueError, match="max_error"):
        B.pack_residual({**HEAD, "max_error": 33}, base, res)
    bad = bytearray(body)
    bad[7] = 2
    with pytest.raises(ValueError, match="coder"):
        B.unpack_residual(_recrc(bytes(bad)))
    bad = bytearray(body)
    bad[4] = 2
    with pytest.raises(ValueError, match="version"):
        B.unpack_residual(_recrc(bytes(bad)))
    with pytest.raises(ValueError, match="base"):
        B.pack_residual(HEAD, b"nope" + base[4:], res)
    with pytest.raises(ValueError):
        B.pack_residual({**HEAD, "coder": "stf"}, base, res)
    with pytest.raises(ValueError):
        B.unpack_residual("ICMR")
    # the other readers refuse the magic, as a reader from before the container does
    with pytest.raises(ValueError, match="magic"):
        B.unpack(data)
    with pytest.raises(ValueError, match="magic"):
        B.unpack_tiled(data)
    with pytest.raises(ValueError, match="magic"):
        B.unpack_residual(base)
    with pytest.raises(ValueError):
        B.coder_of(data)


def test_max_error_is_checked_in_one_place():
    from icm_amd import residual as R
    assert R.check_max_error(None) is None and R.check_max_error(0) == 0 and R.check_max_error(np.int64(32)) == 32
    for bad in (-1, 33, 1.0, True, "3"):
        with pytest.raises(ValueError):
            R.check_max_error(bad)


# ------------------------------------------------------------------------------------------------- the GPU cases
def test_every_gpu_case_reaches_the_path_it_is_named_for():
    cases = RR.kernel_cases()
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    seen = set()
    for c in cases:
        H, W = c["x"].shape[:2]
        got = RR.run_paths(H, W, c["byte_offset"], c["elem_offset"])
        assert c["paths"] <= got, c["name"]
        if "odd-pointers" in c["name"]:
            assert "dword" not in got and "vec" not in got, c["name"]
        seen |= got
        assert c["x"].dtype == c["xhat"].dtype == np.uint8 and c["x"].shape == c["xhat"].shape
    assert seen == {"dword", "byte", "vec", "scalar", "full", "partial"}
    for H, W in RR.SHAPES:
        for d in RR.BOUNDS:
            assert f"random-{H}x{W}-D{d}" in names and f"extreme-{H}x{W}-D{d}" in names
            assert f"extreme-rev-{H}x{W}-D{d}" in names
    # the extremes give the largest symbol of either sign and the clamp has work to do
    for d in RR.BOUNDS:
        x, xhat = RR.extreme_pair(17, 33, False)
        q = RR.quantise(x, xhat, d)
        assert (q == RR.max_symbol(d)).all() and (RR.quantise(xhat, x, d) == -RR.max_symbol(d)).all()
    # and the clamp has work to do on either side in the cases of every D > 0
    for d in RR.BOUNDS[1:]:
        lo = hi = False
        for c in cases:
            if c["d"] == d:
                v = c["xhat"].astype(np.int64) + RR.quantise(c["x"], c["xhat"], d).transpose(1, 2, 0) * (2 * d + 1)
                lo, hi = lo or bool((v < 0).any()), hi or bool((v > 255).any())
        assert lo and hi, d


@pytest.mark.parametrize("d", RR.BOUNDS)
def test_threshold_cells_sit_on_each_threshold_from_both_sides(d):
    x, xhat, want = RR.threshold_image(d)
    q = RR.quantise(x, xhat, d)
    N, S = RR.cell_sums(q)
    cls = RR.classes(q)
    js = RR.threshold_js(d)
    assert js == list(range(len(js))) and (d != 0 or len(js) == 18)           # D = 0 reaches every threshold
    assert sorted({j for _, _, j, _ in want}) == js
    for cy, cx, j, k in want:
        assert N[cy, cx] == 768
        if k == j:
            assert 16 * S[cy, cx] == N[cy, cx] * RR.THRESHOLDS[j]             # on the threshold: not above it
        else:
            assert 16 * S[cy, cx] == N[cy, cx] * RR.THRESHOLDS[j] + 16        # the next sum there is
        assert cls[cy, cx] == k, (j, k)
    odd = RR.odd_threshold_strips(d)
    assert [j for j, _, _ in odd] == [j for j in js if RR.THRESHOLDS[j] % 2]
    for j, sx, sxhat in odd:
        q = RR.quantise(sx, sxhat, d)
        N, S = RR.cell_sums(q)
        assert N.shape == (1, 1) and 16 * S[0, 0] == N[0, 0] * RR.THRESHOLDS[j] + 1
        assert RR.classes(q)[0, 0] == j + 1
