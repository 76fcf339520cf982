"""CPU: the host side of the codec's quantiser step -- the float32 restatement of the kernels' arithmetic
(tests/_qstep_ref.py) against today's codec at k = 0 and against its error bound, ``bitstream.step_of``, the rate
search ``codec.search_qstep`` on table-driven size functions, the one-byte string the step travels in, and the CLI's
argument errors, which come before any GPU check."""
import math
import struct

import numpy as np
import pytest
import torch

import _qstep_ref as Q
from icm_amd import bitstream as B
from oracle import wacnn_oracle as O

F = np.float32
HDR = {"arch": "cnn", "height": 175, "width": 201, "pads": (27, 28, 8, 9), "shape": (3, 4), "fingerprint": 0xDEADBEEF}
ALL_K = list(range(B.QSTEP_MIN, B.QSTEP_MAX + 1))


def _data(seed, n=20000):
    rng = np.random.default_rng(seed)
    y = (rng.standard_normal(n) * 3).astype(F)
    mu = rng.standard_normal(n).astype(F)
    table = O.scale_table().numpy()
    scale = (table[rng.integers(0, 64, n)] * rng.uniform(0.7, 1.4, n)).astype(F)
    scale[:64] = table
    scale[64:70] = np.array([0.11, 0.0, -1.0, 300.0, 0.05, 256.0], dtype=F)
    return y, mu, scale, table


# ------------------------------------------------------------------------------------------------ the restatement
def test_k0_is_the_codec_without_a_step():
    y, mu, scale, table = _data(1)
    y[:6] = mu[:6] + np.array([0.5, -0.5, 1.5, 2.5, -2.5, -0.0], dtype=F)       # ties go to even
    step, inv = Q.step_of(0)
    assert step == 1.0 and inv == 1.0
    sym, idx, yh = Q.code(y, mu, scale, table, O.SCALE_BOUND, step, inv)
    r = np.rint(y - mu)
    assert r.dtype == np.float32
    assert np.array_equal(sym, r.astype(np.int32))
    assert np.array_equal(yh, r + mu)
    assert np.array_equal(idx, O.gc_build_indexes(torch.from_numpy(scale), torch.from_numpy(table)).numpy())
    assert np.array_equal(Q.dequantize(sym, mu, step), yh)


@pytest.mark.parametrize("k", [-16, -8, -3, 0, 5, 8, 16, 32])
def test_reconstruction_lies_within_half_a_step(k):
    y, mu, scale, table = _data(100 + k)
    step, inv = Q.step_of(k)
    sym, _, yh = Q.code(y, mu, scale, table, O.SCALE_BOUND, step, inv)
    err = np.abs(yh.astype(np.float64) - y.astype(np.float64)).max()
    limit = float(step) / 2 * (1 + 2.0 ** -20)
    print(f"k = {k}: step {float(step):.6f}, max |yh - y| = {err:.9f}, limit {limit:.9f}")
    assert err <= limit
    assert np.abs(sym).max() < 2 ** 30           # no clamped symbol in this data: the bound is about the rounding


def test_symbols_clamp_at_two_to_the_thirty():
    step, inv = Q.step_of(-16)
    y = np.array([3e9, -3e9, 1e30, -1e30], dtype=F)
    sym = Q.symbols(y, np.zeros(4, dtype=F), inv)
    assert sym.tolist() == [2 ** 30, -2 ** 30, 2 ** 30, -2 ** 30]


# ------------------------------------------------------------------------------------------------ step_of
def test_step_of():
    for k in ALL_K:
        step, inv = B.step_of(k)
        rs, ri = Q.step_of(k)
        assert isinstance(step, float) and isinstance(inv, float)
        assert step == float(rs) and inv == float(ri)                       # both are float32 values, the reference's
        assert struct.unpack("<f", struct.pack("<f", step))[0] == step
        assert struct.unpack("<f", struct.pack("<f", inv))[0] == inv
        assert step == pytest.approx(2.0 ** (k / 8), rel=2.0 ** -24)
        if k % 8 == 0:
            assert step == 2.0 ** (k // 8) and inv == 2.0 ** -(k // 8)      # exact powers of two
    assert B.step_of(0) == (1.0, 1.0)
    assert (B.QSTEP_MIN, B.QSTEP_MAX) == (-16, 32) == (Q.QSTEP_MIN, Q.QSTEP_MAX)
    assert B.step_of(B.QSTEP_MIN)[0] == 0.25 and B.step_of(B.QSTEP_MAX)[0] == 16.0
    for bad in (-17, 33, 99, 1.0, 0.5, "3", None, True):
        with pytest.raises(ValueError):
            B.step_of(bad)
        with pytest.raises(ValueError):
            B.check_qstep(bad)
    assert B.check_qstep(np.int64(5)) == 5 and isinstance(B.check_qstep(np.int64(5)), int)


def test_bitstream_still_imports_without_torch_or_the_library():
    import subprocess
    import sys
    code = ("import sys, icm_amd.bitstream as B; assert B.step_of(8) == (2.0, 0.5); "
            "assert 'torch' not in sys.modules and 'icm_amd._lib' not in sys.modules")
    import os
    pkg = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "image-compression-for-machine_amd")
    env = {**os.environ, "PYTHONPATH": os.pathsep.join([pkg] + [p for p in [os.environ.get("PYTHONPATH")] if p])}
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ search_qstep
def _sizes(kind):
    if kind == "monotone":
        return {k: 5000 - 90 * k for k in ALL_K}
    if kind == "constant":
        return {k: 1000 for k in ALL_K}
    if kind == "non_monotone":                    # falls on the whole, with bumps that cross a budget more than once
        return {k: 5000 - 90 * k + (260 if k % 5 == 0 else 0) - (240 if k % 7 == 3 else 0) for k in ALL_K}
    raise AssertionError(kind)


@pytest.mark.parametrize("kind", ["monotone", "constant", "non_monotone"])
def test_search_qstep_keeps_its_guarantee(kind):
    from icm_amd.codec import search_qstep
    sizes = _sizes(kind)
    lo_size, hi_size = min(sizes.values()), max(sizes.values())
    budgets = sorted({sizes[B.QSTEP_MAX], sizes[B.QSTEP_MAX] + 1, hi_size, hi_size + 1, 10 ** 9,
                      *range(max(lo_size, sizes[B.QSTEP_MAX]), hi_size + 200, 37), *sizes.values()})
    tried = 0
    for budget in budgets:
        if sizes[B.QSTEP_MAX] > budget:
            continue
        seen = {}

        def fits(k):
            assert k not in seen, "a step was probed twice"
            seen[k] = sizes[k] <= budget
            return seen[k]

        k, probes = search_qstep(fits)
        assert probes == len(seen) <= 8
        assert seen[k] is True
        assert k == B.QSTEP_MIN or seen.get(k - 1) is False, (kind, budget, k, seen)
        assert list(seen)[0] == B.QSTEP_MAX                      # the coarsest step is probed first
        if kind == "monotone":
            assert k == min(j for j in ALL_K if sizes[j] <= budget)
        tried += 1
    assert tried > (5 if kind == "constant" else 20)


def test_search_qstep_ends():
    from icm_amd.codec import search_qstep
    calls = []

    def never(k):
        calls.append(k)
        return False
    with pytest.raises(ValueError, match="out of reach"):
        search_qstep(never)
    assert calls == [B.QSTEP_MAX]                                 # nothing fits: one probe, then the error
    calls.clear()

    def always(k):
        calls.append(k)
        return True
    assert search_qstep(always) == (B.QSTEP_MIN, 2) and calls == [B.QSTEP_MAX, B.QSTEP_MIN]
    # a narrower range, and a range of one value
    assert search_qstep(lambda k: k >= 3, 0, 8) == (3, 5)
    assert search_qstep(lambda k: True, 4, 4) == (4, 1)
    with pytest.raises(ValueError):
        search_qstep(lambda k: True, 5, 4)
    assert 2 + math.ceil(math.log2(B.QSTEP_MAX - B.QSTEP_MIN)) == 8


# ------------------------------------------------------------------------------------------------ the step's string
def test_qstep_string_round_trip_and_refusals():
    assert B.qstep_from_strings([b"y", b"z"]) == 0
    for k in ALL_K:
        if k == 0:
            with pytest.raises(ValueError):
                B.qstep_string(0)                                 # no step: no string, one encoding per content
            continue
        s = B.qstep_string(k)
        assert isinstance(s, bytes) and len(s) == 1 and struct.unpack("<b", s)[0] == k
        assert B.qstep_from_strings([b"y", b"z", s]) == k
        h, strings = B.unpack(B.pack(HDR, [b"yyyy", b"zz", s]))
        assert h == HDR and strings == [b"yyyy", b"zz", s] and B.qstep_from_strings(strings) == k
        assert B.unpack(B.pack(HDR, [b"yyyy", b"zz", s], coder="lanes")) == (h, strings)
    for bad in ([], [b"y"], [b"y", b"z", b"\x05", b""], [b"y", b"z", b""], [b"y", b"z", b"\x05\x00"],
                [b"y", b"z", b"\x00"], [b"y", b"z", struct.pack("<b", -17)], [b"y", b"z", struct.pack("<b", 33)],
                [b"y", b"z", b"\x7f"], [b"y", b"z", b"\x80"]):
        with pytest.raises(ValueError):
            B.qstep_from_strings(bad)
    for bad in (-17, 33, 2.0, "1"):
        with pytest.raises(ValueError):
            B.qstep_string(bad)


def test_codec_accepts_what_the_bitstream_accepts():
    from icm_amd import codec
    assert codec._check_strings("cnn", [b"y", b"z"]) == 0
    assert codec._check_strings("cnn", [b"y", b"z", B.qstep_string(-7)]) == -7
    with pytest.raises(ValueError, match="holds 4"):
        codec._check_strings("cnn", [b"y", b"z", b"\x01", b""])
    with pytest.raises(ValueError, match="holds 1"):
        codec._check_strings("cnn", [b"y"])
    for third in (b"", b"\x00", b"\x21", b"\x01\x02"):
        with pytest.raises(ValueError):
            codec._check_strings("cnn", [b"y", b"z", third], "tile 3")


# ------------------------------------------------------------------------------------------------ CLI argument errors
@pytest.mark.parametrize("flags", [["--qstep", "99"], ["--qstep", "-17"], ["--qstep", "3", "--target-bytes", "10"],
                                   ["--qstep", "3", "--target-bpp", "0.5"], ["--target-bytes", "10", "--target-bpp", "0.5"],
                                   ["--target-bpp", "0"], ["--target-bpp", "-0.25"], ["--target-bpp", "nan"],
                                   ["--target-bytes", "-1"], ["--target-bytes", "0"]],
                         ids=lambda f: " ".join(f))
def test_codec_cli_refuses_bad_flags_before_any_gpu_check(flags, tmp_path, capsys, monkeypatch):
    from icm_amd import codec

    def no_gpu_check():
        raise AssertionError("the GPU was asked for")
    monkeypatch.setattr(torch.cuda, "is_available", no_gpu_check)
    out = str(tmp_path / "o.icmb")
    assert codec.main(["encode", str(tmp_path / "missing.png"), "-o", out, "-p", "none.pt", *flags]) == 2
    assert "Error:" in capsys.readouterr().err
    assert not (tmp_path / "o.icmb").exists()


def test_eval_model_cli_refuses_bad_qstep(tmp_path, capsys, monkeypatch):
    from icm_amd import eval_model

    def no_gpu_check():
        raise AssertionError("the GPU was asked for")
    monkeypatch.setattr(torch.cuda, "is_available", no_gpu_check)
    assert eval_model.main(["-d", str(tmp_path), "--qstep", "40"]) == 2
    assert eval_model.main(["-d", str(tmp_path), "--qstep", "4", "--entropy-estimation"]) == 2
    assert capsys.readouterr().err.count("Error:") == 2


def test_models_refuse_a_bad_qstep_before_any_work():
    from icm_amd.zoo import models
    net = models["cnn"]().eval()
    x = torch.zeros(1, 3, 64, 64)
    for bad in (33, -17, 1.5, "2"):
        with pytest.raises(ValueError, match="qstep"):
            net.compress(x, qstep=bad)
        with pytest.raises(ValueError, match="qstep"):
            net.decompress([[b""], [b""]], (1, 1), qstep=bad)
        with pytest.raises(ValueError, match="qstep"):
            net.compress_latent(torch.zeros(1, 320, 4, 4), qstep=bad)
    stf6 = models["stf6"]().eval()
    with pytest.raises(NotImplementedError):
        stf6.compress(x, qstep=3)
    with pytest.raises(NotImplementedError):
        stf6.compress_latent(torch.zeros(1, 384, 4, 4), qstep=3)
    with pytest.raises(NotImplementedError):
        stf6.decompress([[b""], [b""]], (1, 1), qstep=3)
