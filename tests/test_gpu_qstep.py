"""GPU: the codec's quantiser step.  The three kernels of csrc/qstep.hip against the float32 restatement
(tests/_qstep_ref.py), bit for bit, and against today's kernels at k = 0; the models' compress / decompress with a
step on both coders and both forms of the slice loop; the container, the tiled container and region decode; the rate
search against budgets measured in the test; the CLI in child processes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import _qstep_ref as Q
from oracle import wacnn_oracle as O
from oracle import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(HERE, "..", "image-compression-for-machine_amd")
F = np.float32
SENT_F, SENT_I = -777.25, -7
BOUND = O.SCALE_BOUND
ERR_ARG = 1
KERNEL_KS = [-16, -3, 0, 5, 8, 32]
KERNEL_SHAPES = [(2, 3, 37), (1, 1, 1), (1, 32, 4096)]      # odd and strided; one element; more than one pass of the grid


def _lib():
    from icm_amd import _lib as L
    return L


class Wide:
    """a [N, C, HW] operand that is a channel slice of a wider, sentinel-filled buffer (batch stride != C * HW)"""

    def __init__(self, shape, before, after, data=None):
        N, C, HW = shape
        self.buf = torch.full((N, before + C + after, HW), SENT_F, dtype=torch.float32, device=DEV)
        self.view = self.buf[:, before:before + C]
        self.before, self.C = before, C
        if data is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data)).reshape(shape).to(DEV))
        self.ptr, self.bs = self.view.data_ptr(), self.buf.stride(0)
        assert self.bs != C * HW

    def numpy(self):
        return self.view.cpu().contiguous().numpy()

    def outside_untouched(self):
        b = self.buf.cpu()
        return bool((b[:, :self.before] == SENT_F).all() and (b[:, self.before + self.C:] == SENT_F).all())


def kernel_case(shape, k, seed=0):
    """(y, mu, scale, table) as float32 [N, C, HW]: generic values, and at the head of the flat order the cases the
    arithmetic can get wrong -- exact ties of u at the power-of-two steps, |t| up to 3e4, the special scales"""
    N, C, HW = shape
    n = N * C * HW
    rng = np.random.default_rng(1000 * seed + 17 * (k + 20) + n % 1000)
    step, inv = Q.step_of(k)
    table = O.scale_table().numpy()
    mu = (np.rint(rng.uniform(-3, 3, n) * 64) / 64).astype(F)
    t = (rng.standard_normal(n) * 5 * float(step)).astype(F)
    ties = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 3.5, 1000.5, -1001.5, 0.0, -0.25], dtype=np.float64) * float(step)
    big = np.array([3e4, -3e4, 12345.678, -29999.5, 1e4], dtype=np.float64)
    head = np.concatenate([ties, big]).astype(F)[:n]
    t[:len(head)] = head
    y = (mu + t).astype(F)
    if k % 8 == 0 and n > len(ties):         # the ties are exact: mu is a multiple of 1/64, t of step / 4 >= 1/16
        assert np.array_equal((y - mu)[:len(ties)], ties.astype(F))
        u = (y - mu)[:9] * inv
        assert np.array_equal(u - np.floor(u), np.full(9, 0.5, dtype=F))
    scale = (table[rng.integers(0, 64, n)] * rng.uniform(0.7, 1.4, n)).astype(F)
    special = np.concatenate([
        np.array([0.0, -1.0, 0.05, 0.11, BOUND, 300.0, 1e4, 256.0], dtype=F),
        np.array([300.0, 256.0], dtype=F) * step,                                   # above the table maximum
        (table[[0, 1, 7, 31, 62, 63]] * step).astype(F),                            # table[j] * step: se lands on or next to table[j]
        np.nextafter((table[[3, 40]] * step).astype(F), F(np.inf)), np.nextafter((table[[3, 40]] * step).astype(F), F(-np.inf)),
    ]).astype(F)[:n]
    scale[:len(special)] = special
    return y.reshape(shape), mu.reshape(shape), scale.reshape(shape), table


def run_code_q(shape, y, mu, scale, table, k, step_inv=None):
    L = _lib()
    N, C, HW = shape
    step, inv = Q.step_of(k) if step_inv is None else step_inv
    ys, ms, ss = Wide(shape, 2, 1, y), Wide(shape, 0, 3, mu), Wide(shape, 1, 1, scale)
    yh = Wide(shape, 3, 2)
    sym = torch.full(shape, SENT_I, dtype=torch.int32, device=DEV)
    idx = torch.full(shape, SENT_I, dtype=torch.int32, device=DEV)
    td = torch.from_numpy(table).to(DEV)
    rc = L.lib().icm_gc_code_q(ys.ptr, ys.bs, ms.ptr, ms.bs, ss.ptr, ss.bs, td.data_ptr(), len(table), BOUND, float(step),
                               float(inv), sym.data_ptr(), idx.data_ptr(), yh.ptr, yh.bs, N, C, HW, L.stream())
    torch.cuda.synchronize()
    return rc, sym, idx, yh, (ys, ms, ss, td)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("k", KERNEL_KS)
def test_kernels_equal_the_restatement_bit_for_bit(shape, k):
    L = _lib()
    N, C, HW = shape
    y, mu, scale, table = kernel_case(shape, k)
    step, inv = Q.step_of(k)
    want_sym, want_idx, want_yh = Q.code(y, mu, scale, table, BOUND, step, inv)
    rc, sym, idx, yh, (ys, ms, ss, td) = run_code_q(shape, y, mu, scale, table, k)
    assert rc == 0
    assert np.array_equal(sym.cpu().numpy(), want_sym)
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    assert np.array_equal(Q.bits(yh.numpy()), Q.bits(want_yh))
    assert yh.outside_untouched()
    for w, a in ((ys, y), (ms, mu), (ss, scale)):                                  # inputs are read only
        assert w.outside_untouched() and np.array_equal(Q.bits(w.numpy()), Q.bits(a))
    if N * C * HW > 30:
        assert np.abs(want_sym).max() >= (100000 if k == -16 else 1800)            # escape-range symbols were in it
        assert want_idx.max() == 63 and (k < 0 or want_idx.min() == 0)
    # the decoder's two kernels, fed the fused kernel's symbols, reproduce its indexes and y_hat exactly
    idx2 = torch.full(shape, SENT_I, dtype=torch.int32, device=DEV)
    assert L.lib().icm_gc_indexes_q(ss.ptr, ss.bs, td.data_ptr(), len(table), BOUND, float(inv), idx2.data_ptr(), N, C, HW,
                                    L.stream()) == 0
    yh2 = Wide(shape, 1, 4)
    assert L.lib().icm_dequantize_q(sym.data_ptr(), ms.ptr, ms.bs, float(step), yh2.ptr, yh2.bs, N, C, HW,
                                    L.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(idx2, idx)
    assert np.array_equal(Q.bits(yh2.numpy()), Q.bits(yh.numpy())) and yh2.outside_untouched()


@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_k0_equals_todays_kernels(shape):
    L = _lib()
    N, C, HW = shape
    y, mu, scale, table = kernel_case(shape, 0, seed=3)
    rc, sym, idx, yh, (ys, ms, ss, td) = run_code_q(shape, y, mu, scale, table, 0)
    assert rc == 0
    sym0 = torch.full(shape, SENT_I, dtype=torch.int32, device=DEV)
    L.check(L.lib().icm_quantize(ys.ptr, ys.bs, ms.ptr, ms.bs, HW, 1, sym0.data_ptr(), 0, N, C, HW, L.stream()), "quantize")
    idx0 = torch.full(shape, SENT_I, dtype=torch.int32, device=DEV)
    L.check(L.lib().icm_gc_build_indexes(ss.ptr, ss.bs, td.data_ptr(), len(table), BOUND, idx0.data_ptr(), N, C, HW,
                                         L.stream()), "gc_build_indexes")
    lik, yh0 = Wide(shape, 1, 1), Wide(shape, 2, 2)
    L.check(L.lib().icm_gc_likelihood_ste_fwd(ys.ptr, ys.bs, ms.ptr, ms.bs, ss.ptr, ss.bs, 0, 0, lik.ptr, lik.bs, yh0.ptr,
                                              yh0.bs, 0, 0, N, C, HW, BOUND, 1e-9, L.stream()), "gc_fwd")
    torch.cuda.synchronize()
    assert torch.equal(sym, sym0) and torch.equal(idx, idx0)
    assert np.array_equal(Q.bits(yh.numpy()), Q.bits(yh0.numpy()))


def test_argument_errors_leave_the_outputs_alone():
    L = _lib()
    shape = (2, 3, 37)
    N, C, HW = shape
    y, mu, scale, table = kernel_case(shape, 5)
    ys, ms, ss = Wide(shape, 2, 1, y), Wide(shape, 0, 3, mu), Wide(shape, 1, 1, scale)
    yh = Wide(shape, 3, 2)
    sym = torch.full(shape, SENT_I, dtype=torch.int32, device=DEV)
    idx = torch.full(shape, SENT_I, dtype=torch.int32, device=DEV)
    td = torch.from_numpy(table).to(DEV)
    step, inv = map(float, Q.step_of(5))
    st = L.stream()
    good_c = dict(y=ys.ptr, y_bs=ys.bs, mu=ms.ptr, mu_bs=ms.bs, sc=ss.ptr, sc_bs=ss.bs, table=td.data_ptr(), ns=64,
                  bound=BOUND, step=step, inv=inv, sym=sym.data_ptr(), idx=idx.data_ptr(), yh=yh.ptr, yh_bs=yh.bs, N=N,
                  C=C, HW=HW)

    def code_q(**kw):
        a = {**good_c, **kw}
        return L.lib().icm_gc_code_q(a["y"], a["y_bs"], a["mu"], a["mu_bs"], a["sc"], a["sc_bs"], a["table"], a["ns"],
                                     a["bound"], a["step"], a["inv"], a["sym"], a["idx"], a["yh"], a["yh_bs"], a["N"],
                                     a["C"], a["HW"], st)

    def indexes_q(**kw):
        a = {**good_c, **kw}
        return L.lib().icm_gc_indexes_q(a["sc"], a["sc_bs"], a["table"], a["ns"], a["bound"], a["inv"], a["idx"], a["N"],
                                        a["C"], a["HW"], st)

    def dequantize_q(**kw):
        a = {**good_c, **kw}
        return L.lib().icm_dequantize_q(a["sym"], a["mu"], a["mu_bs"], a["step"], a["yh"], a["yh_bs"], a["N"], a["C"],
                                        a["HW"], st)

    bad_float = [0.0, -1.0, float("inf"), float("-inf"), float("nan")]
    cases = []
    for name in ("y", "mu", "sc", "table", "sym", "idx", "yh"):
        cases.append((code_q, {name: 0}))
    for name in ("sc", "table", "idx"):
        cases.append((indexes_q, {name: 0}))
    for name in ("sym", "mu", "yh"):
        cases.append((dequantize_q, {name: 0}))
    for v in bad_float:
        cases += [(code_q, {"step": v}), (code_q, {"inv": v}), (indexes_q, {"inv": v}), (dequantize_q, {"step": v})]
    for fn in (code_q, indexes_q, dequantize_q):
        for dim in ("N", "C", "HW"):
            cases += [(fn, {dim: 0}), (fn, {dim: -1})]
    for fn in (code_q, indexes_q):
        cases += [(fn, {"ns": 0}), (fn, {"ns": -3})]
    for fn, kw in cases:
        assert fn(**kw) == ERR_ARG, (fn.__name__, kw)
    torch.cuda.synchronize()
    assert bool((sym == SENT_I).all()) and bool((idx == SENT_I).all()) and bool((yh.buf == SENT_F).all())
    # ns = 1, the smallest table: every index is 0
    assert code_q(ns=1) == 0
    torch.cuda.synchronize()
    assert bool((idx == 0).all())


# ------------------------------------------------------------------------------------------------ models
def _build(arch):
    from icm_amd.zoo import models
    m = models[arch]()
    m.load_state_dict(W.make_wacnn_state_dict() if arch == "cnn" else W.make_stf_state_dict())
    m = m.to(DEV).eval()
    m.update(force=True)
    return m


@pytest.fixture(scope="module")
def nets():
    return {}


def _net(nets, arch):
    if arch not in nets:
        nets[arch] = _build(arch)
    return nets[arch]


def _synthesis(m, arch, y_hat):
    from icm_amd import engine as E
    from icm_amd import models as M_
    with torch.no_grad():
        tape = E.Tape(need_grad=False, packed_cache=m._pack_cache())
        P = m._params()
        if arch == "cnn":
            return M_.wacnn_g_s(tape, P, y_hat.contiguous())
        return M_.stf_synthesis(tape, P, y_hat.contiguous(), None, m.window_size)


MODEL_INPUTS = {"1x64x128": (1, 3, 64, 128), "2x64x64": (2, 3, 64, 64)}


@pytest.mark.parametrize("k", [-8, 5, 16])
@pytest.mark.parametrize("inp", list(MODEL_INPUTS))
@pytest.mark.parametrize("split", [True, False], ids=["split_slices", "unsplit"])
@pytest.mark.parametrize("arch", ["cnn", "stf"])
def test_decoder_reproduces_the_encoder(nets, arch, split, inp, k, monkeypatch):
    from icm_amd import models as M_
    monkeypatch.setattr(M_, "SLICE_SPLIT", split)
    m = _net(nets, arch)
    x = W._u(f"qstep.x.{inp}", MODEL_INPUTS[inp], 0.0, 1.0).to(DEV)
    outs = {}
    for coder in ("host", "lanes"):
        d = {}
        enc = m.compress(x, _debug=d, coder=coder, qstep=k)
        assert enc["qstep"] == k and set(enc) == {"strings", "shape", "qstep"}
        assert len(enc["strings"]) == 2 and len(enc["strings"][0]) == 1 and isinstance(enc["strings"][0][0], bytes)
        assert d["y_hat"].is_cuda and d["y_hat"].shape[0] == x.shape[0]
        x_hat = m.decompress(enc["strings"], enc["shape"], coder=coder, qstep=k)["x_hat"]
        want = _synthesis(m, arch, d["y_hat"]).clamp(0.0, 1.0)
        assert torch.equal(x_hat, want), (arch, split, inp, k, coder)
        # the latent coder alone, on the analysis transform's output: the same strings
        lat = m.compress_latent(m.analysis(x), coder=coder, qstep=k)
        assert lat["strings"] == enc["strings"] and lat["qstep"] == k and tuple(lat["shape"]) == tuple(enc["shape"])
        outs[coder] = (x_hat, d["y_hat"], d["symbols"])
    assert torch.equal(outs["host"][0], outs["lanes"][0]) and torch.equal(outs["host"][1], outs["lanes"][1])
    assert np.array_equal(outs["host"][2], outs["lanes"][2])
    # the step is really applied: the symbols are those of another quantiser than today's
    d0 = {}
    m.compress(x, _debug=d0)
    assert not np.array_equal(d0["symbols"], outs["host"][2])


@pytest.mark.parametrize("split", [True, False], ids=["split_slices", "unsplit"])
@pytest.mark.parametrize("arch", ["cnn", "stf"])
def test_qstep_zero_is_todays_codec(nets, arch, split, monkeypatch):
    from icm_amd import models as M_
    monkeypatch.setattr(M_, "SLICE_SPLIT", split)
    m = _net(nets, arch)
    x = W._u("qstep.x.2x64x64", MODEL_INPUTS["2x64x64"], 0.0, 1.0).to(DEV)
    for coder in ("host", "lanes"):
        a, b = m.compress(x, coder=coder), m.compress(x, coder=coder, qstep=0)
        assert a["strings"] == b["strings"] and b["qstep"] == 0 and a["qstep"] == 0
        ra = m.decompress(a["strings"], a["shape"], coder=coder)["x_hat"]
        rb = m.decompress(b["strings"], b["shape"], coder=coder, qstep=0)["x_hat"]
        assert torch.equal(ra, rb)
        d = {}
        m.compress(x, _debug=d, coder=coder)
        assert torch.equal(_synthesis(m, arch, d["y_hat"]).clamp(0.0, 1.0), ra)       # _debug["y_hat"] without a step too


class _CountingLib:
    """the real library, with every entry point's calls counted"""

    def __init__(self, real):
        self._real, self.calls = real, {}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("icm_"):
            return fn

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


@pytest.mark.parametrize("split", [True, False], ids=["split_slices", "unsplit"])
def test_launches_per_slice(nets, split, monkeypatch):
    """with a step: one fused launch per slice on the encoder and no likelihood launch; the two step-aware launches
    around decode_run on the decoder; without a step: the launches of before"""
    from icm_amd import _lib
    from icm_amd import models as M_
    monkeypatch.setattr(M_, "SLICE_SPLIT", split)
    m = _net(nets, "cnn")
    S = m.num_slices
    x = W._u("qstep.x.1x64x128", MODEL_INPUTS["1x64x128"], 0.0, 1.0).to(DEV)
    m.compress(x, qstep=5)                                   # weights packed, tables built
    counting = _CountingLib(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: counting)

    def counts(fn):
        counting.calls.clear()
        r = fn()
        return r, dict(counting.calls)

    enc, c = counts(lambda: m.compress(x, qstep=5))
    assert c.get("icm_gc_code_q") == S
    assert "icm_gc_likelihood_ste_fwd" not in c and "icm_gc_build_indexes" not in c
    _, d = counts(lambda: m.decompress(enc["strings"], enc["shape"], qstep=5))
    assert d.get("icm_gc_indexes_q") == S and d.get("icm_dequantize_q") == S
    assert "icm_gc_build_indexes" not in d and "icm_gc_code_q" not in d
    enc0, c0 = counts(lambda: m.compress(x))
    assert c0.get("icm_gc_likelihood_ste_fwd") == S and c0.get("icm_gc_build_indexes") == S and "icm_gc_code_q" not in c0
    assert c0.get("icm_quantize", 0) == c.get("icm_quantize", 0) + S       # the others quantise z
    _, d0 = counts(lambda: m.decompress(enc0["strings"], enc0["shape"]))
    assert d0.get("icm_gc_build_indexes") == S and "icm_gc_indexes_q" not in d0 and "icm_dequantize_q" not in d0
    assert sum(c.values()) == sum(c0.values()) - 2 * S


# ------------------------------------------------------------------------------------------------ codec
def _image(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(yy * 3 + xx * 2 + 40 * c) % 256 for c in range(3)], -1)
    return np.clip(base + rng.integers(-12, 13, size=(h, w, 3)), 0, 255).astype(np.uint8)


IMAGES = {"100x150": (_image(100, 150, 4), {}), "200x300_tiled": (_image(200, 300, 5), {"tile": 128, "overlap": 16})}


@pytest.mark.parametrize("name", list(IMAGES))
@pytest.mark.parametrize("coder", ["host", "lanes"])
def test_streams_carry_the_step(nets, name, coder):
    from icm_amd import bitstream as B
    from icm_amd import codec
    m = _net(nets, "cnn")
    a, kw = IMAGES[name]
    plain = codec.encode_image(m, a, coder=coder, **kw)
    assert codec.encode_image(m, a, coder=coder, qstep=0, **kw) == plain            # byte for byte
    assert codec.decode_image(m, plain)[1]["qstep"] == 0
    for k in (5, -8):
        data, found = codec.encode_image_info(m, a, coder=coder, qstep=k, **kw)
        assert found == {"qstep": k, "step": B.step_of(k)[0], "probes": 1}
        assert data == codec.encode_image(m, a, coder=coder, qstep=k, **kw)
        streams = B.unpack_tiled(data)[1] if kw else [data]
        assert len(streams) == (6 if kw else 1) and B.is_tiled(data) == bool(kw)
        for s in streams:
            _, strings = B.unpack(s)
            assert len(strings) == 3 and strings[2] == B.qstep_string(k) and B.coder_of(s) == coder
        img, info = codec.decode_image(m, data, reference=a)
        assert info["qstep"] == k and tuple(img.shape) == a.shape and "psnr" in info
        if kw:
            region = (60, 90, 100, 130)                                               # touches four of the six tiles
            part, pinfo = codec.decode_image(m, data, region=region)
            assert pinfo["tiles_decoded"] == 4 and pinfo["qstep"] == k
            assert torch.equal(part, img[60:160, 90:220])


@pytest.mark.parametrize("name,coder", [("100x150", "host"), ("100x150", "lanes"), ("200x300_tiled", "lanes")])
def test_encode_to_size(nets, name, coder):
    from icm_amd import bitstream as B
    from icm_amd import codec
    m = _net(nets, "cnn")
    a, kw = IMAGES[name]

    def size(k):
        return len(codec.encode_image(m, a, coder=coder, qstep=k, **kw))

    s8, s16, smax = size(8), size(16), size(B.QSTEP_MAX)
    print(f"{name} {coder}: s(8) = {s8}, s(16) = {s16}, s({B.QSTEP_MAX}) = {smax}")
    for budget in (s8, s16):
        data, found = codec.encode_image_info(m, a, coder=coder, max_bytes=budget, **kw)
        k = found["qstep"]
        print(f"  budget {budget}: qstep {k}, {len(data)} bytes, {found['probes']} probes")
        assert len(data) <= budget and found["probes"] <= 8 and found["step"] == B.step_of(k)[0]
        assert k == B.QSTEP_MIN or size(k - 1) > budget
        assert data == codec.encode_image(m, a, coder=coder, qstep=k, **kw)         # the probe's stream is the encode
        assert codec.decode_image(m, data)[1]["qstep"] == k
        assert codec.encode_image(m, a, coder=coder, max_bytes=budget, **kw) == data
    with pytest.raises(ValueError, match=str(smax)):
        codec.encode_image(m, a, coder=coder, max_bytes=smax - 1, **kw)
    data, found = codec.encode_image_info(m, a, coder=coder, max_bytes=10 ** 9, **kw)
    assert found["qstep"] == B.QSTEP_MIN and found["probes"] == 2
    assert data == codec.encode_image(m, a, coder=coder, qstep=B.QSTEP_MIN, **kw)
    with pytest.raises(ValueError, match="not both"):
        codec.encode_image(m, a, coder=coder, qstep=3, max_bytes=10 ** 6, **kw)
    for bad in (0, -5, 1.5):
        with pytest.raises(ValueError):
            codec.encode_image(m, a, coder=coder, max_bytes=bad, **kw)


# ------------------------------------------------------------------------------------------------ CLI, child processes
@pytest.fixture(scope="module")
def cnn_ckpt(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ckpt") / "cnn_salt0.pt")
    torch.save(W.make_wacnn_state_dict(), path)
    return path


def _cli(*argv):
    env = {**os.environ, "PYTHONPATH": os.pathsep.join([PKG] + [p for p in [os.environ.get("PYTHONPATH")] if p])}
    return subprocess.run([sys.executable, "-m", "icm_amd.codec", *argv], env=env, capture_output=True, text=True,
                          timeout=420)


def test_cli_encodes_to_a_bpp_budget_and_a_second_process_decodes(nets, cnn_ckpt, tmp_path):
    from icm_amd import codec
    m = _net(nets, "cnn")
    a, _ = IMAGES["100x150"]
    src, stream, out = str(tmp_path / "in.png"), str(tmp_path / "in.icmb"), str(tmp_path / "out.png")
    Image.fromarray(a).save(src)
    s8 = len(codec.encode_image(m, a, qstep=8))
    bpp = 8.0 * (s8 + 0.5) / (100 * 150)
    budget = int(np.floor(bpp * 100 * 150 / 8))
    assert budget == s8
    r = _cli("encode", src, "-o", stream, "-a", "cnn", "-p", cnn_ckpt, "--target-bpp", repr(bpp))
    assert r.returncode == 0, r.stderr[-2000:]
    enc = json.loads(r.stdout.strip().splitlines()[-1])
    assert os.path.getsize(stream) == enc["bytes"] <= budget
    assert 2 <= enc["probes"] <= 8 and enc["step"] == pytest.approx(2.0 ** (enc["qstep"] / 8), rel=1e-6)
    data = open(stream, "rb").read()
    want, info = codec.decode_image(m, data, reference=a)
    assert info["qstep"] == enc["qstep"]
    r = _cli("decode", stream, "-o", out, "-p", cnn_ckpt, "--reference", src)
    assert r.returncode == 0, r.stderr[-2000:]
    dec = json.loads(r.stdout.strip().splitlines()[-1])
    assert dec["qstep"] == enc["qstep"] and dec["bytes"] == enc["bytes"]
    assert np.array_equal(np.asarray(Image.open(out)), want.numpy())


def test_cli_unreachable_budget_exits_4_and_writes_nothing(cnn_ckpt, tmp_path):
    a, _ = IMAGES["100x150"]
    src, stream = str(tmp_path / "in.png"), str(tmp_path / "never.icmb")
    Image.fromarray(a).save(src)
    r = _cli("encode", src, "-o", stream, "-a", "cnn", "-p", cnn_ckpt, "--target-bytes", "50")
    assert r.returncode == 4 and "out of reach" in r.stderr
    assert not os.path.exists(stream)
