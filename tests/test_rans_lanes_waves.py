"""CPU: the ranged forms of the host lane decoder (csrc/rans.cpp ``icm_rans_lanes_decoder_decode_run_waves`` /
``_finish_waves`` / ``_waves`` through ``icm_amd.ans.LanesDecoder``): a range of waves decodes exactly its slice of the
whole decode and touches no other wave, a damaged body outside the range goes unnoticed by it (and is refused by the
whole decode), and the argument checks.  The input is tests/_lanes_waves_cases.py."""
import ctypes as C

import numpy as np
import pytest

import _lanes_waves_cases as K


@pytest.fixture(scope="module")
def case():
    from icm_amd import ans
    sym, idx, runs, string, G, t = K.make()
    whole = ans.lanes_decode(string, idx, runs, t)
    assert np.array_equal(whole, sym)
    return dict(sym=sym, idx=idx, runs=runs, string=string, G=G, t=t)


def _decode_range(dec, case, g0, g1, lead=0):
    """the four runs through the waves [g0, g1) of ``dec`` -> per run (elem0, the decoded buffer)"""
    out = []
    for off, n in K.run_slices(case["runs"]):
        elem0, end = K.buffers(n, case["G"], g0, g1, lead)
        out.append((elem0, dec.decode_run_waves(g0, g1, elem0, case["idx"][off + elem0:off + end], n, case["t"])))
    return out


def _assert_slices(case, got, g0, g1):
    for (off, n), (elem0, buf) in zip(K.run_slices(case["runs"]), got):
        lo, hi = K.owned(n, case["G"], g0, g1)
        assert np.array_equal(buf[lo - elem0:hi - elem0], case["sym"][off + lo:off + hi]) if hi > lo else True
        assert not buf[:max(0, lo - elem0)].any()          # nothing written in front of the range's first element


def test_the_decoder_knows_its_waves(case):
    from icm_amd import ans
    assert ans.LanesDecoder(case["string"]).G == case["G"] == ans.lanes_waves(case["runs"], K.SPW)
    assert [ans.lanes_chunk(n, case["G"]) for n in case["runs"]] == [K.chunk(n, case["G"]) for n in case["runs"]]
    assert [ans.lanes_chunk(n, g) for n, g in ((0, 1), (1, 1), (64, 1), (65, 1), (12_000_000, 4096))] == \
        [0, 64, 64, 128, 2944]


@pytest.mark.parametrize("g0,g1,lead", K.ranges(16))
def test_a_range_of_waves_decodes_its_slice_of_the_whole_decode(case, g0, g1, lead):
    from icm_amd import ans
    dec = ans.LanesDecoder(case["string"])
    got = _decode_range(dec, case, g0, g1, lead)
    _assert_slices(case, got, g0, g1)
    assert lead == 0 or all(e > 0 for e, _ in got[1:])
    dec.finish_waves(g0, g1, True)
    dec.finish_waves(g0, g1, False)
    if (g0, g1) != (0, case["G"]):
        with pytest.raises(ValueError, match="left unread|did not end"):
            dec.finish()                                   # the other waves have not moved: the stream is not finished


def test_a_range_then_its_complement_is_the_whole_decode(case):
    from icm_amd import ans
    G = case["G"]
    dec = ans.LanesDecoder(case["string"])
    parts = [(4, 11), (0, 4), (11, G)]
    full = [np.zeros(n, np.int32) for n in case["runs"]]
    for g0, g1 in parts:
        for r, (elem0, buf) in enumerate(_decode_range(dec, case, g0, g1)):
            lo, hi = K.owned(case["runs"][r], G, g0, g1)
            full[r][lo:hi] = buf[lo - elem0:hi - elem0]
    assert np.array_equal(np.concatenate(full), case["sym"])
    dec.finish()                                           # the old whole-stream check: every body at its end


def test_waves_may_stand_at_different_runs(case):
    """the class waves of a region decode stop after run 0 and are held to ``end=False`` alone"""
    from icm_amd import ans
    dec = ans.LanesDecoder(case["string"])
    n0 = case["runs"][0]
    cls = dec.decode_run_waves(0, 1, 0, case["idx"][:n0], n0, case["t"])
    assert np.array_equal(cls, case["sym"][:n0])
    dec.finish_waves(0, 1, False)
    with pytest.raises(ValueError, match="left unread"):
        dec.finish_waves(0, 1, True)
    _assert_slices(case, _decode_range(dec, case, 6, 8), 6, 8)
    dec.finish_waves(6, 8, True)


@pytest.mark.parametrize("g0,g1,bad_g", [(3, 9, 1), (3, 9, 12), (0, 1, 15), (15, 16, 0)])
def test_a_damaged_body_outside_the_range_is_not_read(case, g0, g1, bad_g):
    from icm_amd import ans
    bad = K.corrupt_word(case["string"], bad_g)
    assert bad != case["string"] and len(bad) == len(case["string"])
    dec = ans.LanesDecoder(bad)
    _assert_slices(case, _decode_range(dec, case, g0, g1), g0, g1)
    dec.finish_waves(g0, g1, True)
    with pytest.raises(ValueError, match="lane stream decode"):
        ans.lanes_decode(bad, case["idx"], case["runs"], case["t"])
    # and a range that holds the damaged body answers for it
    dec = ans.LanesDecoder(bad)
    with pytest.raises(ValueError, match="lane stream decode"):
        _decode_range(dec, case, bad_g, bad_g + 1)
        dec.finish_waves(bad_g, bad_g + 1, True)


def test_bad_arguments(case):
    from icm_amd import _lib as L
    from icm_amd import ans
    lib, G, t = L.lib(), case["G"], case["t"]
    dec = ans.LanesDecoder(case["string"])
    n = case["runs"][1]
    c = K.chunk(n, G)
    idx = np.ascontiguousarray(case["idx"][case["runs"][0]:case["runs"][0] + n])
    out = np.zeros(n, np.int32)
    i32p = C.POINTER(C.c_int32)

    def call(g0, g1, elem0, handle=dec._h, length=n):
        part = np.ascontiguousarray(idx[max(0, elem0):])  # the buffers begin at element elem0 (a refused call reads none)
        return lib.icm_rans_lanes_decoder_decode_run_waves(handle, g0, g1, elem0, part.ctypes.data_as(i32p), length,
                                                           *t.args(), out.ctypes.data_as(i32p))
    for g0, g1, elem0 in ((-1, 2, 0), (3, 2, 0), (0, G + 1, 0), (2, 4, -1), (2, 4, 2 * c + 1), (0, 1, 1)):
        assert call(g0, g1, elem0) == 1, (g0, g1, elem0)   # ICM_ERR_ARG
    assert call(0, 1, 0, handle=None) == 1 and call(0, 1, 0, length=-1) == 1
    for g0, g1 in ((-1, 2), (3, 2), (0, G + 1)):
        assert lib.icm_rans_lanes_decoder_finish_waves(dec._h, g0, g1, 1) == -1
    assert lib.icm_rans_lanes_decoder_finish_waves(None, 0, 1, 1) == -1 and lib.icm_rans_lanes_decoder_waves(None) == -1
    assert not out.any()                                  # a refused call does nothing
    assert call(5, 5, 5 * c) == 0 and lib.icm_rans_lanes_decoder_finish_waves(dec._h, 5, 5, 1) == 0 and not out.any()
    assert call(2, 4, 2 * c) == 0 and np.array_equal(out[:2 * c], case["sym"][case["runs"][0] + 2 * c:][:2 * c])
    # the Python surface refuses the same, and buffers too short for the range
    for args in ((-1, 2, 0), (3, 2, 0), (0, G + 1, 0), (2, 4, 2 * c + 1)):
        with pytest.raises(ValueError, match="not a range"):
            dec.decode_run_waves(*args, idx, n, t)
    with pytest.raises(ValueError, match="need"):
        dec.decode_run_waves(2, 4, 2 * c, idx[:2 * c - 1], n, t)
