"""GPU: the ranged forms of the device lane decoder (csrc/rans_lanes.hip ``icm_rans_lanes_decoder_gpu_decode_run_waves`` /
``_finish_waves`` / ``_waves`` through ``icm_amd.ans.LanesDecoderGpu`` and the decoder of ``LanesCoder``), bit for bit
against the host decoder's ranged forms on the cases of tests/test_rans_lanes_waves.py (input:
tests/_lanes_waves_cases.py): a launch of g1 - g0 waves decodes exactly that range's slice into buffers that begin at
``elem0``, writes nothing else, and leaves the other waves where they stood."""
import numpy as np
import pytest
import torch

import _lanes_waves_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 0x5A5A5A5A


@pytest.fixture(scope="module")
def case():
    from icm_amd import residual as R
    sym, idx, runs, string, G, t = K.make()
    return dict(sym=sym, idx=idx, runs=runs, string=string, G=G, t=t, dt=R.tables()._device_tables(DEV))


def _host_range(dec, case, g0, g1, lead=0):
    out = []
    for off, n in K.run_slices(case["runs"]):
        elem0, end = K.buffers(n, case["G"], g0, g1, lead)
        out.append(dec.decode_run_waves(g0, g1, elem0, case["idx"][off + elem0:off + end], n, case["t"]))
    return out


def _gpu_range(dec, case, g0, g1, lead=0):
    """as ``_host_range`` on the device decoder, into buffers pre-filled with a sentinel -> numpy, the sentinel zeroed
    after a check that it stands exactly where the range owns nothing"""
    out = []
    for off, n in K.run_slices(case["runs"]):
        elem0, end = K.buffers(n, case["G"], g0, g1, lead)
        lo, hi = K.owned(n, case["G"], g0, g1)
        idx = torch.from_numpy(np.ascontiguousarray(case["idx"][off + elem0:off + end])).to(DEV)
        buf = torch.full((end - elem0 + 8,), SENT, dtype=torch.int32, device=DEV)
        dec.decode_run_waves(g0, g1, elem0, idx, n, *case["dt"], out=buf[:end - elem0])
        got = buf.cpu().numpy()
        written = np.zeros(got.size, bool)
        written[lo - elem0:hi - elem0] = hi > lo
        assert (got[~written] == SENT).all(), "an element outside the range was written"
        out.append(np.where(written, got, 0)[:end - elem0])
    return out


def test_the_decoder_knows_its_waves(case):
    from icm_amd import ans
    from icm_amd import residual as R
    dec = ans.LanesDecoderGpu(case["string"])
    assert dec.G == case["G"]
    dec.close()
    ns = ans.LanesCoder(K.SPW).decoder(case["string"], R.tables())
    assert ns.waves == case["G"]
    ns.close()
    assert ans.HostCoder().decoder(b"\0" * 8, R.tables()).waves is None


@pytest.mark.parametrize("g0,g1,lead", K.ranges(16))
def test_a_range_of_waves_is_the_hosts_bit_for_bit(case, g0, g1, lead):
    from icm_amd import ans
    host, dev = ans.LanesDecoder(case["string"]), ans.LanesDecoderGpu(case["string"])
    want, got = _host_range(host, case, g0, g1, lead), _gpu_range(dev, case, g0, g1, lead)
    for r, (w, g) in enumerate(zip(want, got)):
        assert np.array_equal(w, g), r
    host.finish_waves(g0, g1, True)
    dev.finish_waves(g0, g1, True)
    dev.finish_waves(g0, g1, False)
    if (g0, g1) != (0, case["G"]):
        with pytest.raises(ValueError, match="left unread|did not end"):
            dev.finish()                                   # the other waves have not moved
    dev.close()


def test_a_range_then_its_complement_is_the_whole_decode(case):
    from icm_amd import ans
    G = case["G"]
    dev = ans.LanesDecoderGpu(case["string"])
    full = [np.zeros(n, np.int32) for n in case["runs"]]
    for g0, g1 in ((4, 11), (0, 4), (11, G)):
        for r, buf in enumerate(_gpu_range(dev, case, g0, g1)):
            lo, hi = K.owned(case["runs"][r], G, g0, g1)
            elem0 = K.buffers(case["runs"][r], G, g0, g1, 0)[0]
            full[r][lo:hi] = buf[lo - elem0:hi - elem0]
    assert np.array_equal(np.concatenate(full), case["sym"])
    dev.finish()                                           # every body at its end, every lane at 2^16


def test_the_whole_run_entries_are_the_full_range(case):
    """decode_run / finish, whose kernels the ranged forms share, on the same string"""
    from icm_amd import ans
    dev = ans.LanesDecoderGpu(case["string"])
    got = []
    for off, n in K.run_slices(case["runs"]):
        got.append(dev.decode_run(torch.from_numpy(case["idx"][off:off + n].copy()).to(DEV), *case["dt"]).cpu().numpy())
    dev.finish()
    assert np.array_equal(np.concatenate(got), case["sym"])


@pytest.mark.parametrize("g0,g1,bad_g", [(3, 9, 1), (3, 9, 12), (0, 1, 15), (15, 16, 0)])
def test_a_damaged_body_outside_the_range_is_not_read(case, g0, g1, bad_g):
    from icm_amd import ans
    bad = K.corrupt_word(case["string"], bad_g)
    host, dev = ans.LanesDecoder(bad), ans.LanesDecoderGpu(bad)
    for w, g in zip(_host_range(host, case, g0, g1), _gpu_range(dev, case, g0, g1)):
        assert np.array_equal(w, g)
    dev.finish_waves(g0, g1, True)
    dev.close()
    whole = ans.LanesDecoderGpu(bad)
    for off, n in K.run_slices(case["runs"]):
        whole.decode_run(torch.from_numpy(case["idx"][off:off + n].copy()).to(DEV), *case["dt"])
    with pytest.raises(ValueError, match="lane stream decode"):
        whole.finish()


def test_bad_arguments(case):
    from icm_amd import _lib as L
    from icm_amd import ans
    lib, G = L.lib(), case["G"]
    dev = ans.LanesDecoderGpu(case["string"])
    n = case["runs"][1]
    c = K.chunk(n, G)
    idx = torch.from_numpy(case["idx"][case["runs"][0]:case["runs"][0] + n].copy()).to(DEV)
    out = torch.full((n,), SENT, dtype=torch.int32, device=DEV)
    tabs = ans._dev_tables(*case["dt"])
    for g0, g1, elem0 in ((-1, 2, 0), (3, 2, 0), (0, G + 1, 0), (2, 4, -1), (2, 4, 2 * c + 1), (0, 1, 1)):
        assert lib.icm_rans_lanes_decoder_gpu_decode_run_waves(dev._h, g0, g1, elem0, idx.data_ptr(), n, *tabs,
                                                               out.data_ptr(), L.stream()) == 1, (g0, g1, elem0)
    assert lib.icm_rans_lanes_decoder_gpu_decode_run_waves(None, 0, 1, 0, idx.data_ptr(), n, *tabs, out.data_ptr(),
                                                           L.stream()) == 1
    for g0, g1 in ((-1, 2), (3, 2), (0, G + 1)):
        assert lib.icm_rans_lanes_decoder_gpu_finish_waves(dev._h, g0, g1, 1, L.stream()) == -1
    assert lib.icm_rans_lanes_decoder_gpu_finish_waves(None, 0, 1, 1, L.stream()) == -1
    assert lib.icm_rans_lanes_decoder_gpu_waves(None) == -1
    assert lib.icm_rans_lanes_decoder_gpu_finish_waves(dev._h, 5, 5, 1, L.stream()) == 0        # an empty range
    torch.cuda.synchronize()
    assert (out == SENT).all()                             # a refused call launches nothing
    for args in ((-1, 2, 0), (3, 2, 0), (0, G + 1, 0), (2, 4, 2 * c + 1)):
        with pytest.raises(ValueError, match="not a range"):
            dev.decode_run_waves(*args, idx, n, *case["dt"])
    with pytest.raises(ValueError, match="need"):
        dev.decode_run_waves(2, 4, 2 * c, idx[:2 * c - 1], n, *case["dt"])
    dev.close()
