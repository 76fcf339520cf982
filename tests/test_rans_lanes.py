"""CPU: the host implementation of the lane-stream format (csrc/rans.cpp ``icm_rans_lanes_*`` through
``icm_amd.ans``) against the exact-integer restatement of the format (tests/_lanes_ref.py), byte for byte and round
trip, on the cases of tests/_lanes_cases.py; corrupt streams, which the host decoder must refuse exactly where the
restatement does; the coder objects of ``icm_amd.ans.coder_for`` (the host one on CPU tensors); and the coder id of
the ICMB container (icm_amd/bitstream.py)."""
import struct
import zlib

import numpy as np
import pytest

import _lanes_cases as K
import _lanes_ref as R


@pytest.fixture(scope="module")
def tabs():
    from icm_amd.ans import _Tables
    return _Tables(*K.tables_np())


@pytest.mark.parametrize("name", list(K.cases()))
def test_host_encoder_writes_the_bytes_of_the_restatement(name, tabs):
    from icm_amd import ans
    sym, idx, runs, spw, G = K.cases()[name]
    want = K.ref_encode(name)
    got = ans.lanes_encode(sym, idx, runs, tabs, spw)
    assert got == want
    assert ans.lanes_waves(runs, spw) == G == struct.unpack_from("<H", got, 6)[0]
    assert got[:6] == b"ICML\x01\x00" and len(got) == 8 + 4 * G + sum(struct.unpack_from(f"<{G}I", got, 8))


@pytest.mark.parametrize("name", list(K.cases()))
def test_round_trip_host_and_restatement(name, tabs):
    from icm_amd import ans
    sym, idx, runs, spw, _ = K.cases()[name]
    stream = K.ref_encode(name)
    assert K.ref_decode(stream, name) == sym.tolist()
    assert np.array_equal(ans.lanes_decode(stream, idx, runs, tabs), sym)


def test_the_cases_reach_what_they_are_named_for():
    c = K.cases()
    sym, idx, *_ = c["escapes_int32_ends"]
    assert {K.INT32_MIN, K.INT32_MAX} <= set(sym.tolist())
    for t in range(len(K.CDFS)):
        got = set((sym[idx == t].astype(np.int64) - K.OFFSETS[t]).tolist())
        assert {-1, K.SIZES[t] - 2} <= got          # just below the table, just above its last regular bin
    sym, idx, *_ = c["zero_probability_bins"]
    used = set((sym.astype(np.int64) - K.OFFSETS[3]).tolist())
    assert (idx == 3).all() and not used & {0, 2, 5} and {1, 3, 4} <= used      # bins 0, 2 and 5 have no width
    # partition: the second wave of (64, 2) owns nothing, that of (100, 2) a partial step
    assert R._elements(64, 2, 1) == [] and len(R._elements(100, 2, 1)[0]) == 36
    assert [R.chunk(n, 3) for n in c["r10_unequal"][2]] == [64, 0, 64, 64, 128, 64, 64, 128, 64, 64]


def test_state_carries_over_the_runs(tabs):
    """ten decode_run calls on one decoder, and the format's cost: one flush per stream, not one per run"""
    from icm_amd import ans
    sym, idx, runs, spw, G = K.cases()["r10_unequal"]
    stream = ans.lanes_encode(sym, idx, runs, tabs, spw)
    dec, pos = ans.LanesDecoder(stream), 0
    for n in runs:
        assert np.array_equal(dec.decode_run(idx[pos:pos + n], tabs), sym[pos:pos + n])
        pos += n
    dec.finish()
    apart = sum(len(ans.lanes_encode(sym[a:a + n], idx[a:a + n], [n], tabs, spw))
                for a, n in zip(np.cumsum([0] + runs[:-1]), runs))
    assert len(stream) < apart - 5 * 256      # nine non-empty runs coded apart flush 64 lanes each at least once


def test_encoder_refusals(tabs):
    from icm_amd import ans
    one = np.zeros(4, np.int32)
    with pytest.raises(ValueError):
        ans.lanes_encode(one, np.full(4, 4, np.int32), [4], tabs)            # CDF index past the tables
    with pytest.raises(ValueError):
        ans.lanes_encode(one, np.full(4, -1, np.int32), [4], tabs)
    with pytest.raises(ValueError):
        ans.lanes_encode(np.full(4, K.OFFSETS[3], np.int32), np.full(4, 3, np.int32), [4], tabs)   # zero-width bin
    with pytest.raises(ValueError):
        ans.lanes_encode(one, one, [3], tabs)                                # runs do not add up
    with pytest.raises(ValueError):
        ans.lanes_encode(one, one, [4], tabs, symbols_per_wave=0)
    assert ans.lanes_waves([10 ** 9], 1) == 4096 and ans.lanes_waves([], 5) == 1 and ans.lanes_waves([0, 0]) == 1
    empty = ans.lanes_encode(one[:0], one[:0], [0, 0], tabs)
    assert empty == R.encode([], [], [0, 0], K.CDFS, K.SIZES, K.OFFSETS) and len(empty) == 12 + 256
    assert ans.lanes_decode(empty, one[:0], [0, 0], tabs).size == 0


def test_corrupt_streams_fail_exactly_where_the_restatement_fails(tabs):
    from icm_amd import ans
    bad = ok = 0
    for label, name, data, want in K.corruptions():
        _, idx, runs, _, _ = K.cases()[name]
        if want is None:
            bad += 1
            with pytest.raises(ValueError):
                ans.lanes_decode(data, idx, runs, tabs)
        else:       # a flip the format cannot see: a bit of a raw escape group changes that value and nothing else
            ok += 1     # (the container's CRC is what catches it); the two decoders must still agree
            assert ans.lanes_decode(data, idx, runs, tabs).tolist() == want, label
    assert bad >= 150 and ok >= 1, (bad, ok)


def test_a_length_table_that_disagrees_with_the_string_is_refused_before_decoding(tabs):
    from icm_amd import ans
    good = K.ref_encode("r10_unequal")
    for data in (good[:-2], good + b"\0\0", good[:8] + struct.pack("<I", 258) + good[12:], good[:11], b"", b"ICML",
                 good[:8] + struct.pack("<I", struct.unpack_from("<I", good, 8)[0] + 1) + good[12:],
                 b"ICMX" + good[4:], good[:4] + b"\x02\x00" + good[6:], good[:6] + b"\x00\x00" + good[8:]):
        with pytest.raises(ValueError, match="not a lane stream"):
            ans.LanesDecoder(data)
        with pytest.raises(R.Corrupt):
            R.parse(data)


def test_wrong_indexes_are_reported_not_read(tabs):
    from icm_amd import ans
    sym, idx, runs, spw, _ = K.cases()["n65_g1"]
    stream = ans.lanes_encode(sym, idx, runs, tabs, spw)
    wrong = idx.copy()
    wrong[7] = 99
    with pytest.raises(ValueError, match="CDF index"):
        ans.lanes_decode(stream, wrong, runs, tabs)


# ------------------------------------------------------------------------------------------------------ coder objects
@pytest.fixture(scope="module")
def em():
    """an EntropyModel on the CPU whose tables are those of the cases"""
    import torch
    from icm_amd.entropy_models import EntropyModel
    m = EntropyModel()
    m._quantized_cdf, m._cdf_length, m._offset = (torch.from_numpy(a) for a in K.tables_np())
    return m


@pytest.mark.parametrize("name", list(K.cases()))
def test_host_coder_object_is_the_rans_classes(name, em):
    """coder_for("host") on CPU tensors: the bytes of RansEncoder, and run by run what RansDecoder gives -- the
    symbols, or its refusal: the scalar stream's decoder checks an escape against int32 before it adds the table's
    offset, so it refuses INT32_MAX under a negative offset, which only the case made of the ends of int32 holds"""
    import torch
    from icm_amd import ans
    sym, idx, runs, _, _ = K.cases()[name]
    lists = [a.tolist() for a in K.tables_np()]
    coder = ans.coder_for("host")
    string = coder.encode(torch.from_numpy(sym), torch.from_numpy(idx), runs, em)
    assert string == ans.RansEncoder().encode_with_indexes(sym.tolist(), idx.tolist(), *lists)
    ref = ans.RansDecoder()
    ref.set_stream(string)
    dec, pos, refused = coder.decoder(string, em), 0, False
    for n in runs:
        try:
            want = ref.decode_stream(idx[pos:pos + n].tolist(), *lists)
        except ValueError:
            refused = True
            with pytest.raises(ValueError, match="rANS decode"):
                dec.decode_run(torch.from_numpy(idx[pos:pos + n]))
            break
        got = dec.decode_run(torch.from_numpy(idx[pos:pos + n]))
        assert got.dtype == torch.int32 and got.device.type == "cpu" and tuple(got.shape) == (n,)
        assert got.tolist() == want == sym[pos:pos + n].tolist()
        pos += n
    assert refused == (name == "escapes_int32_ends")
    dec.finish()
    dec.close()
    with pytest.raises(ValueError, match="run_lengths"):
        coder.encode(torch.from_numpy(sym), torch.from_numpy(idx), runs + [1], em)


def test_coder_for_checks_the_name_and_resolves_the_default():
    from icm_amd import ans
    from icm_amd import bitstream as B
    with pytest.raises(ValueError, match=r"unknown coder 'nope'; choose from \['host', 'lanes'\]"):
        ans.coder_for("nope")
    assert ans.coder_for("lanes", None).symbols_per_wave == ans.SYMBOLS_PER_WAVE == 16384
    assert ans.coder_for("lanes", 100).symbols_per_wave == 100
    assert ans.CODERS is B.CODERS and ans.check_coder is B.check_coder
    assert [ans.coder_for(n).name for n in ans.CODERS] == list(ans.CODERS)


# ------------------------------------------------------------------------------------------------------ container
HEADER = {"arch": "stf", "height": 100, "width": 120, "pads": (4, 4, 14, 14), "shape": (2, 2), "fingerprint": 0xDEADBEEF}


def _todays_bytes(header, strings):
    """the ICMB layout as it was before the architecture field carried a coder id"""
    from icm_amd import bitstream as B
    out = struct.pack("<4sHHII4H2HIH", b"ICMB", 1, B.ARCHS.index(header["arch"]), header["height"], header["width"],
                      *header["pads"], *header["shape"], header["fingerprint"], len(strings))
    out += b"".join(struct.pack("<I", len(s)) for s in strings) + b"".join(strings)
    return out + struct.pack("<I", zlib.crc32(out) & 0xFFFFFFFF)


def test_container_records_the_coder_and_host_files_do_not_change():
    from icm_amd import bitstream as B
    strings = [b"y" * 37, b"zz"]
    host = B.pack(HEADER, strings)
    assert host == B.pack(HEADER, strings, coder="host") == _todays_bytes(HEADER, strings)
    lanes = B.pack(HEADER, strings, coder="lanes")
    assert B.coder_of(host) == "host" and B.coder_of(lanes) == "lanes"
    assert len(lanes) == len(host) and struct.unpack_from("<H", lanes, 6)[0] == 0x0100 | B.ARCHS.index("stf")
    hd, got = B.unpack(lanes)
    assert hd == B.unpack(host)[0] == HEADER and tuple(hd) == B.HEADER_KEYS and got == strings
    with pytest.raises(ValueError, match="unknown coder"):
        B.pack(HEADER, strings, coder="gpu")


def test_coder_id_2_is_refused_by_name():
    from icm_amd import bitstream as B
    data = bytearray(B.pack(HEADER, [b"a", b"b"], coder="lanes"))
    data[7] = 2
    data[-4:] = struct.pack("<I", zlib.crc32(bytes(data[:-4])) & 0xFFFFFFFF)
    with pytest.raises(ValueError, match="unknown coder id 2"):
        B.unpack(bytes(data))
    with pytest.raises(ValueError, match="unknown coder id 2"):
        B.coder_of(bytes(data))
    data[7], data[6] = 1, 9
    with pytest.raises(ValueError, match="unknown architecture id 9"):
        B.unpack(bytes(data))
    with pytest.raises(ValueError, match="bad magic"):
        B.coder_of(b"ICMT" + bytes(data[4:]))
