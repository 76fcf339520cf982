"""GPU: the codec's quality maps (a quantiser step per latent position).  The three map kernels of csrc/qstep.hip
against the float32 restatement (tests/_qmap_ref.py), bit for bit, and against the scalar kernels on uniform maps; the
models' compress / decompress with a map on both coders and both forms of the slice loop, with the placement of the map
pinned through slice 0; region-of-interest encodes through the container, the tiled container, region decode and the
rate search; the CLI in child processes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import _qmap_ref as R
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
ALL_K = list(range(Q.QSTEP_MIN, Q.QSTEP_MAX + 1))


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


def kernel_map(kind, HW):
    i = np.arange(HW)
    if kind == "stride3":                   # ks[(3 i) % len(ks)]: neighbouring lanes on different steps
        return np.array(KERNEL_KS, dtype=np.int8)[(3 * i) % len(KERNEL_KS)]
    if kind == "stride5":                   # every entry of ks, and rows of a wave that are not periodic in 64
        return np.array(KERNEL_KS, dtype=np.int8)[(5 * i + i // 7) % len(KERNEL_KS)]
    if kind == "all49":
        return np.array(ALL_K, dtype=np.int8)[i % 49]
    raise AssertionError(kind)


KERNEL_CASES = [(s, "stride3") for s in KERNEL_SHAPES] + [((2, 3, 37), "stride5"), ((1, 32, 4096), "stride5"),
                                                          ((1, 32, 4096), "all49"), ((2, 3, 4096), "all49")]


def kernel_case(shape, qmap, seed=0):
    """(y, mu, scale, table) as float32 [N, C, HW], built like the scalar step's cases with the step of each element's
    position: generic values, and at the head of the flat order exact ties of u (exact where the position's step is a
    power of two), |t| up to 3e4, and the special scales times the position's step"""
    N, C, HW = shape
    n = N * C * HW
    rng = np.random.default_rng(1000 * seed + n % 1000 + 7 * int(np.asarray(qmap, dtype=np.int64).sum() % 101))
    step, inv = R.steps_of_map(qmap)
    ks = np.broadcast_to(np.asarray(qmap, dtype=np.int64), shape).reshape(-1)
    sf = np.broadcast_to(step, shape).reshape(-1).astype(np.float64)
    table = O.scale_table().numpy()
    mu = (np.rint(rng.uniform(-3, 3, n) * 64) / 64).astype(F)
    t = (rng.standard_normal(n) * 5 * sf).astype(F)
    ties = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 3.5, 1000.5, -1001.5, 0.0, -0.25], dtype=np.float64)
    big = np.array([3e4, -3e4, 12345.678, -29999.5, 1e4], dtype=np.float64)
    m = min(n, len(ties))
    t[:m] = (ties[:m] * sf[:m]).astype(F)
    m2 = min(n, len(ties) + len(big))
    t[m:m2] = big[:m2 - m].astype(F)
    y = (mu + t).astype(F)
    iv = np.broadcast_to(inv, shape).reshape(-1)
    for i in range(min(m, 9)):               # the ties are exact where the step is a power of two
        if ks[i] % 8 == 0:
            u = F(y[i] - mu[i]) * iv[i]
            assert (y[i] - mu[i]) == F(ties[i] * sf[i]) and u - np.floor(u) == F(0.5), (i, ks[i])
    scale = (table[rng.integers(0, 64, n)] * rng.uniform(0.7, 1.4, n)).astype(F)
    absolute = np.array([0.0, -1.0, 0.05, 0.11, BOUND, 300.0, 1e4, 256.0], dtype=F)
    rel = np.concatenate([np.array([300.0, 256.0]), table[[0, 1, 7, 31, 62, 63]].astype(np.float64)])
    near = table[[3, 40]].astype(np.float64)
    special = list(absolute)
    pos = len(special)
    for v in rel:                             # table[j] x the position's step: se lands on or next to table[j]
        if pos < n:
            special.append(F(v * sf[pos]))
            pos += 1
    for direction in (np.inf, -np.inf):
        for v in near:
            if pos < n:
                special.append(np.nextafter(F(v * sf[pos]), F(direction)))
                pos += 1
    special = np.array(special, dtype=F)[:n]
    scale[:len(special)] = special
    return y.reshape(shape), mu.reshape(shape), scale.reshape(shape), table


def _step_table_dev():
    from icm_amd import bitstream as B
    return torch.from_numpy(B.step_table()).to(DEV)


def run_code_qmap(shape, y, mu, scale, table, qmap):
    L = _lib()
    N, C, HW = shape
    ys, ms, ss = Wide(shape, 2, 1, y), Wide(shape, 0, 3, mu), Wide(shape, 1, 1, scale)
    yh = Wide(shape, 3, 2)
    sym = torch.full(shape, SENT_I, dtype=torch.int32, device=DEV)
    idx = torch.full(shape, SENT_I, dtype=torch.int32, device=DEV)
    td = torch.from_numpy(table).to(DEV)
    qd = torch.from_numpy(np.ascontiguousarray(qmap, dtype=np.int8)).to(DEV)
    st = _step_table_dev()
    assert qd.numel() == HW and st.numel() == 512
    rc = L.lib().icm_gc_code_qmap(ys.ptr, ys.bs, ms.ptr, ms.bs, ss.ptr, ss.bs, td.data_ptr(), len(table), BOUND,
                                  qd.data_ptr(), st.data_ptr(), sym.data_ptr(), idx.data_ptr(), yh.ptr, yh.bs, N, C, HW,
                                  L.stream())
    torch.cuda.synchronize()
    return rc, sym, idx, yh, (ys, ms, ss, td, qd, st)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("shape,kind", KERNEL_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_kernels_equal_the_restatement_bit_for_bit(shape, kind):
    L = _lib()
    N, C, HW = shape
    qmap = kernel_map(kind, HW)
    if kind == "all49":
        assert len(set(qmap.tolist())) == 49
    y, mu, scale, table = kernel_case(shape, qmap)
    want_sym, want_idx, want_yh = R.code(y, mu, scale, table, BOUND, qmap)
    rc, sym, idx, yh, (ys, ms, ss, td, qd, st) = run_code_qmap(shape, y, mu, scale, table, qmap)
    assert rc == 0
    assert np.array_equal(sym.cpu().numpy(), want_sym)
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    assert np.array_equal(Q.bits(yh.numpy()), Q.bits(want_yh))
    assert yh.outside_untouched()
    for w, a in ((ys, y), (ms, mu), (ss, scale)):                                  # inputs are read only
        assert w.outside_untouched() and np.array_equal(Q.bits(w.numpy()), Q.bits(a))
    assert np.array_equal(qd.cpu().numpy(), qmap) and np.array_equal(st.cpu().numpy(), R.step_table())
    if N * C * HW > 30:
        assert np.abs(want_sym).max() >= 1800 and want_idx.max() == 63              # escape-range symbols were in it
        # the map matters: at least one other assignment of the same steps gives other symbols
        other = R.code(y, mu, scale, table, BOUND, np.roll(qmap, 1))
        assert not np.array_equal(other[0], want_sym) and not np.array_equal(other[1], want_idx)
    # the decoder's two kernels, fed the fused kernel's symbols, reproduce its indexes and y_hat exactly
    idx2 = torch.full(shape, SENT_I, dtype=torch.int32, device=DEV)
    assert L.lib().icm_gc_indexes_qmap(ss.ptr, ss.bs, td.data_ptr(), len(table), BOUND, qd.data_ptr(), st.data_ptr(),
                                       idx2.data_ptr(), N, C, HW, L.stream()) == 0
    yh2 = Wide(shape, 1, 4)
    assert L.lib().icm_dequantize_qmap(sym.data_ptr(), ms.ptr, ms.bs, qd.data_ptr(), st.data_ptr(), yh2.ptr, yh2.bs, N,
                                       C, HW, L.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(idx2, idx)
    assert np.array_equal(Q.bits(yh2.numpy()), Q.bits(yh.numpy())) and yh2.outside_untouched()


@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("k", KERNEL_KS)
def test_a_uniform_map_gives_the_scalar_kernels_outputs(shape, k):
    L = _lib()
    N, C, HW = shape
    qmap = np.full(HW, k, dtype=np.int8)
    y, mu, scale, table = kernel_case(shape, qmap, seed=3)
    rc, sym, idx, yh, (ys, ms, ss, td, qd, st) = run_code_qmap(shape, y, mu, scale, table, qmap)
    assert rc == 0
    step, inv = map(float, Q.step_of(k))
    sym0 = torch.full(shape, SENT_I, dtype=torch.int32, device=DEV)
    idx0 = torch.full(shape, SENT_I, dtype=torch.int32, device=DEV)
    yh0 = Wide(shape, 2, 2)
    assert L.lib().icm_gc_code_q(ys.ptr, ys.bs, ms.ptr, ms.bs, ss.ptr, ss.bs, td.data_ptr(), len(table), BOUND, step, inv,
                                 sym0.data_ptr(), idx0.data_ptr(), yh0.ptr, yh0.bs, N, C, HW, L.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(sym, sym0) and torch.equal(idx, idx0)
    assert np.array_equal(Q.bits(yh.numpy()), Q.bits(yh0.numpy()))
    want = Q.code(y, mu, scale, table, BOUND, *Q.step_of(k))
    assert np.array_equal(sym.cpu().numpy(), want[0]) and np.array_equal(idx.cpu().numpy(), want[1])


def test_argument_errors_leave_the_outputs_alone():
    L = _lib()
    shape = (2, 3, 37)
    N, C, HW = shape
    qmap = kernel_map("stride3", HW)
    y, mu, scale, table = kernel_case(shape, qmap)
    ys, ms, ss = Wide(shape, 2, 1, y), Wide(shape, 0, 3, mu), Wide(shape, 1, 1, scale)
    yh = Wide(shape, 3, 2)
    sym = torch.full(shape, SENT_I, dtype=torch.int32, device=DEV)
    idx = torch.full(shape, SENT_I, dtype=torch.int32, device=DEV)
    td = torch.from_numpy(table).to(DEV)
    qd = torch.from_numpy(qmap).to(DEV)
    sd = _step_table_dev()
    st = L.stream()
    good = dict(y=ys.ptr, y_bs=ys.bs, mu=ms.ptr, mu_bs=ms.bs, sc=ss.ptr, sc_bs=ss.bs, table=td.data_ptr(), ns=64,
                bound=BOUND, qmap=qd.data_ptr(), steps=sd.data_ptr(), sym=sym.data_ptr(), idx=idx.data_ptr(), yh=yh.ptr,
                yh_bs=yh.bs, N=N, C=C, HW=HW)

    def code_qmap(**kw):
        a = {**good, **kw}
        return L.lib().icm_gc_code_qmap(a["y"], a["y_bs"], a["mu"], a["mu_bs"], a["sc"], a["sc_bs"], a["table"], a["ns"],
                                        a["bound"], a["qmap"], a["steps"], a["sym"], a["idx"], a["yh"], a["yh_bs"],
                                        a["N"], a["C"], a["HW"], st)

    def indexes_qmap(**kw):
        a = {**good, **kw}
        return L.lib().icm_gc_indexes_qmap(a["sc"], a["sc_bs"], a["table"], a["ns"], a["bound"], a["qmap"], a["steps"],
                                           a["idx"], a["N"], a["C"], a["HW"], st)

    def dequantize_qmap(**kw):
        a = {**good, **kw}
        return L.lib().icm_dequantize_qmap(a["sym"], a["mu"], a["mu_bs"], a["qmap"], a["steps"], a["yh"], a["yh_bs"],
                                           a["N"], a["C"], a["HW"], st)

    cases = []
    for name in ("y", "mu", "sc", "table", "qmap", "steps", "sym", "idx", "yh"):
        cases.append((code_qmap, {name: 0}))
    for name in ("sc", "table", "qmap", "steps", "idx"):
        cases.append((indexes_qmap, {name: 0}))
    for name in ("sym", "mu", "qmap", "steps", "yh"):
        cases.append((dequantize_qmap, {name: 0}))
    for fn in (code_qmap, indexes_qmap, dequantize_qmap):
        for dim in ("N", "C", "HW"):
            cases += [(fn, {dim: 0}), (fn, {dim: -1})]
    for fn in (code_qmap, indexes_qmap):
        cases += [(fn, {"ns": 0}), (fn, {"ns": -3})]
    for fn, kw in cases:
        assert fn(**kw) == ERR_ARG, (fn.__name__, kw)
    torch.cuda.synchronize()
    assert bool((sym == SENT_I).all()) and bool((idx == SENT_I).all()) and bool((yh.buf == SENT_F).all())
    # ns = 1, the smallest table: every index is 0
    assert code_qmap(ns=1) == 0
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
MODEL_KS = [-16, -3, 0, 5, 32]


def model_map(inp):
    """ks[(3 i + j) % 5] over the latent: not symmetric in i and j, so a transposed map is another map"""
    h, w = MODEL_INPUTS[inp][2] // 16, MODEL_INPUTS[inp][3] // 16
    i, j = np.mgrid[0:h, 0:w]
    m = np.array(MODEL_KS, dtype=np.int8)[(3 * i + j) % 5]
    assert not (h == w and np.array_equal(m, m.T))
    return m


@pytest.mark.parametrize("inp", list(MODEL_INPUTS))
@pytest.mark.parametrize("split", [True, False], ids=["split_slices", "unsplit"])
@pytest.mark.parametrize("arch", ["cnn", "stf"])
def test_decoder_reproduces_the_encoder(nets, arch, split, inp, monkeypatch):
    from icm_amd import models as M_
    monkeypatch.setattr(M_, "SLICE_SPLIT", split)
    m = _net(nets, arch)
    x = W._u(f"qstep.x.{inp}", MODEL_INPUTS[inp], 0.0, 1.0).to(DEV)
    qmap = model_map(inp)
    outs = {}
    for coder in ("host", "lanes"):
        d = {}
        enc = m.compress(x, _debug=d, coder=coder, qmap=qmap)
        assert set(enc) == {"strings", "shape", "qstep", "qmap"} and enc["qstep"] is None
        assert isinstance(enc["qmap"], np.ndarray) and enc["qmap"].dtype == np.int8 and np.array_equal(enc["qmap"], qmap)
        assert len(enc["strings"]) == 2 and len(enc["strings"][0]) == 1 and isinstance(enc["strings"][0][0], bytes)
        x_hat = m.decompress(enc["strings"], enc["shape"], coder=coder, qmap=qmap)["x_hat"]
        want = _synthesis(m, arch, d["y_hat"]).clamp(0.0, 1.0)
        assert torch.equal(x_hat, want), (arch, split, inp, coder)
        # the map may come as a tensor, on any device, or as wider integers
        again = m.decompress(enc["strings"], enc["shape"], coder=coder, qmap=torch.from_numpy(qmap.astype(np.int64)).to(DEV))
        assert torch.equal(again["x_hat"], x_hat)
        # the latent coder alone, on the analysis transform's output: the same strings
        lat = m.compress_latent(m.analysis(x), coder=coder, qmap=qmap)
        assert lat["strings"] == enc["strings"] and lat["qstep"] is None and np.array_equal(lat["qmap"], qmap)
        assert tuple(lat["shape"]) == tuple(enc["shape"])
        outs[coder] = (x_hat, d["y_hat"], d["symbols"])
    assert torch.equal(outs["host"][0], outs["lanes"][0]) and torch.equal(outs["host"][1], outs["lanes"][1])
    assert np.array_equal(outs["host"][2], outs["lanes"][2])
    # placement: slice 0's means and scales do not depend on the step, so its symbols are, position by position, those
    # of the uniform encode at that position's k
    N, (h, w) = x.shape[0], qmap.shape
    c = (320 if arch == "cnn" else 384) // m.num_slices
    n0 = N * c * h * w
    mapped = outs["host"][2][:n0].reshape(N, c, h, w)
    differs = 0
    for k in MODEL_KS:
        dk = {}
        m.compress(x, _debug=dk, qstep=k)
        uniform = dk["symbols"][:n0].reshape(N, c, h, w)
        at = qmap == k
        assert at.any() and np.array_equal(mapped[:, :, at], uniform[:, :, at]), (arch, split, inp, k)
        differs += int(not np.array_equal(mapped[:, :, ~at], uniform[:, :, ~at]))
    assert differs >= 3                                 # and elsewhere they are another quantiser's


@pytest.mark.parametrize("split", [True, False], ids=["split_slices", "unsplit"])
@pytest.mark.parametrize("arch", ["cnn", "stf"])
def test_a_uniform_map_is_the_scalar_step(nets, arch, split, monkeypatch):
    from icm_amd import models as M_
    monkeypatch.setattr(M_, "SLICE_SPLIT", split)
    m = _net(nets, arch)
    x = W._u("qstep.x.2x64x64", MODEL_INPUTS["2x64x64"], 0.0, 1.0).to(DEV)
    for coder, k in (("host", 5), ("lanes", -16), ("host", 0), ("lanes", 0)):
        a = m.compress(x, coder=coder, qmap=np.full((4, 4), k, dtype=np.int8))
        b = m.compress(x, coder=coder, qstep=k)
        assert set(a) == {"strings", "shape", "qstep"} and a["qstep"] == k == b["qstep"]
        assert a["strings"] == b["strings"]
        if k == 0:
            assert a["strings"] == m.compress(x, coder=coder)["strings"]
        ra = m.decompress(a["strings"], a["shape"], coder=coder, qmap=torch.full((4, 4), k, dtype=torch.int8))["x_hat"]
        rb = m.decompress(b["strings"], b["shape"], coder=coder, qstep=k)["x_hat"]
        assert torch.equal(ra, rb)


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
    """with a map: one fused map launch per slice on the encoder and no likelihood launch; the two map launches around
    decode_run on the decoder; in all the launch counts of the scalar step.  A uniform map launches the scalar kernels."""
    from icm_amd import _lib
    from icm_amd import models as M_
    monkeypatch.setattr(M_, "SLICE_SPLIT", split)
    m = _net(nets, "cnn")
    S = m.num_slices
    x = W._u("qstep.x.1x64x128", MODEL_INPUTS["1x64x128"], 0.0, 1.0).to(DEV)
    qmap = model_map("1x64x128")
    m.compress(x, qmap=qmap)                                 # weights packed, tables built, the step table uploaded
    counting = _CountingLib(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: counting)

    def counts(fn):
        counting.calls.clear()
        r = fn()
        return r, dict(counting.calls)

    enc, c = counts(lambda: m.compress(x, qmap=qmap))
    assert c.get("icm_gc_code_qmap") == S and "icm_gc_code_q" not in c
    assert "icm_gc_likelihood_ste_fwd" not in c and "icm_gc_build_indexes" not in c
    _, d = counts(lambda: m.decompress(enc["strings"], enc["shape"], qmap=qmap))
    assert d.get("icm_gc_indexes_qmap") == S and d.get("icm_dequantize_qmap") == S
    assert not {"icm_gc_build_indexes", "icm_gc_code_qmap", "icm_gc_indexes_q", "icm_dequantize_q"} & set(d)
    enc5, c5 = counts(lambda: m.compress(x, qstep=5))
    _, d5 = counts(lambda: m.decompress(enc5["strings"], enc5["shape"], qstep=5))
    assert c5.get("icm_gc_code_q") == S and d5.get("icm_gc_indexes_q") == S and d5.get("icm_dequantize_q") == S
    assert sum(c.values()) == sum(c5.values()) and sum(d.values()) == sum(d5.values())
    rename = {"icm_gc_code_qmap": "icm_gc_code_q", "icm_gc_indexes_qmap": "icm_gc_indexes_q",
              "icm_dequantize_qmap": "icm_dequantize_q"}
    assert {rename.get(k, k): v for k, v in c.items()} == c5 and {rename.get(k, k): v for k, v in d.items()} == d5
    encu, cu = counts(lambda: m.compress(x, qmap=np.full((4, 8), 5, dtype=np.int8)))
    assert cu == c5 and encu["strings"] == enc5["strings"]
    _, du = counts(lambda: m.decompress(encu["strings"], encu["shape"], qmap=np.full((4, 8), 5, dtype=np.int8)))
    assert du == d5


def test_models_refuse_a_bad_map(nets):
    m = _net(nets, "cnn")
    x = W._u("qstep.x.1x64x128", MODEL_INPUTS["1x64x128"], 0.0, 1.0).to(DEV)
    qmap = model_map("1x64x128")
    enc = m.compress(x, qmap=qmap)
    over = qmap.astype(np.int64)
    over[1, 1] = 33
    under = qmap.astype(np.int64)
    under[0, 0] = -17
    for bad in (qmap.T, qmap[:, :4], qmap.reshape(-1), qmap[None], over, under, qmap.astype(np.float32),
                torch.from_numpy(qmap.astype(np.float32)).to(DEV), qmap != 0):
        with pytest.raises(ValueError, match="qmap"):
            m.compress(x, qmap=bad)
        with pytest.raises(ValueError, match="qmap"):
            m.compress_latent(m.analysis(x), qmap=bad)
        with pytest.raises(ValueError, match="qmap"):
            m.decompress(enc["strings"], enc["shape"], qmap=bad)
    for k in (3, -16):
        with pytest.raises(ValueError, match="not both"):
            m.compress(x, qstep=k, qmap=qmap)
        with pytest.raises(ValueError, match="not both"):
            m.decompress(enc["strings"], enc["shape"], qstep=k, qmap=qmap)


# ------------------------------------------------------------------------------------------------ codec
def _image(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(yy * 3 + xx * 2 + 40 * c) % 256 for c in range(3)], -1)
    return np.clip(base + rng.integers(-12, 13, size=(h, w, 3)), 0, 255).astype(np.uint8)


IMAGES = {"100x150": (_image(100, 150, 4), {}), "200x300_tiled": (_image(200, 300, 5), {"tile": 128, "overlap": 16})}
ROI = [(30, 40, 40, 60, -24)]
TILES_200x300 = [(0, 0, 128, 128), (0, 112, 128, 128), (0, 224, 128, 76),
                 (112, 0, 88, 128), (112, 112, 88, 128), (112, 224, 88, 76)]


def _expected_maps(name, base, rois):
    """per tile (one for the untiled image) the restatement's map of the rectangles cut to the tile"""
    a, kw = IMAGES[name]
    tiles = TILES_200x300 if kw else [(0, 0, a.shape[0], a.shape[1])]
    out = []
    for ty, tx, th, tw in tiles:
        part = []
        for y0, x0, h, w, d in rois:
            ya, yb, xa, xb = max(y0, ty), min(y0 + h, ty + th), max(x0, tx), min(x0 + w, tx + tw)
            if ya < yb and xa < xb:
                part.append((ya - ty, xa - tx, yb - ya, xb - xa, d))
        out.append(R.roi_map(th, tw, R.center_pads(th, tw), base, part))
    return out


@pytest.mark.parametrize("name", list(IMAGES))
@pytest.mark.parametrize("coder", ["host", "lanes"])
def test_streams_carry_the_map(nets, name, coder):
    from icm_amd import bitstream as B
    from icm_amd import codec
    m = _net(nets, "cnn")
    a, kw = IMAGES[name]
    background = codec.encode_image(m, a, coder=coder, qstep=16, **kw)
    data, found = codec.encode_image_info(m, a, coder=coder, qstep=16, roi=ROI, **kw)
    assert data == codec.encode_image(m, a, coder=coder, qstep=16, roi=ROI, **kw) and data != background
    fine = codec.encode_image(m, a, coder=coder, qstep=-8, **kw)
    print(f"{name} {coder}: background only (qstep 16) {len(background)} bytes, with the region at -8 {len(data)}, "
          f"all at -8 {len(fine)}")
    want = _expected_maps(name, 16, ROI)
    mapped = [k for k, w_ in enumerate(want) if len(set(w_.reshape(-1).tolist())) > 1]
    assert mapped == [0]                                          # the rectangle lies in the first tile alone
    assert found == {"qstep": 16, "step": B.step_of(16)[0], "probes": 1, "roi_cells": int((want[0] != 16).sum()),
                     "qmap_range": [-8, 16]}
    streams = B.unpack_tiled(data)[1] if kw else [data]
    assert len(streams) == len(want) == (6 if kw else 1) and B.is_tiled(data) == bool(kw)
    for k, (s, w_) in enumerate(zip(streams, want)):
        hd, strings = B.unpack(s)
        assert len(strings) == 3 and B.coder_of(s) == coder
        if k in mapped:
            assert strings[2] == R.write_map(w_) and np.array_equal(R.read_map(strings[2]), w_)
            assert np.array_equal(B.qmap_from_string(strings[2], hd["shape"]), w_)
            with pytest.raises(ValueError, match="must be one byte"):            # a reader from before the map
                B.qstep_from_strings(strings)
        else:
            assert strings[2] == B.qstep_string(16) and s == B.unpack_tiled(background)[1][k]
    img, info = codec.decode_image(m, data, reference=a)
    assert tuple(img.shape) == a.shape and "psnr" in info
    if kw:
        assert info["qstep"] == [None, 16, 16, 16, 16, 16]
        assert isinstance(info["qmap"], list) and [q is None for q in info["qmap"]] == [False] + [True] * 5
        assert np.array_equal(info["qmap"][0], want[0]) and info["qmap"][0].dtype == np.int8
        region = (60, 90, 100, 130)                                               # touches four of the six tiles
        part, pinfo = codec.decode_image(m, data, region=region)
        assert pinfo["tiles_decoded"] == 4 and pinfo["qstep"] == info["qstep"]
        assert torch.equal(part, img[60:160, 90:220])
    else:
        assert info["qstep"] is None and np.array_equal(info["qmap"], want[0]) and info["qmap"].dtype == np.int8
    binfo = codec.decode_image(m, background)[1]
    assert binfo["qstep"] == 16 and "qmap" not in binfo
    # rectangles that change no cell leave the stream what it is without them
    assert codec.encode_image(m, a, coder=coder, qstep=16, roi=[], **kw) == background
    assert codec.encode_image(m, a, coder=coder, qstep=16, roi=[(30, 40, 40, 60, 0), (0, 0, 5, 5, 0)], **kw) == background
    with pytest.raises(ValueError, match="not inside"):
        codec.encode_image(m, a, coder=coder, qstep=16, roi=[(0, 0, a.shape[0] + 1, 10, -8)], **kw)


def test_roi_without_a_step_or_a_budget_paints_on_base_0(nets):
    from icm_amd import codec
    m = _net(nets, "cnn")
    a, _ = IMAGES["100x150"]
    data, found = codec.encode_image_info(m, a, roi=ROI)
    assert found["qstep"] == 0 and found["qmap_range"] == [-16, 0] and found["roi_cells"] == 20
    info = codec.decode_image(m, data)[1]
    assert info["qstep"] is None and np.array_equal(info["qmap"], _expected_maps("100x150", 0, ROI)[0])


@pytest.mark.parametrize("name,coder", [("100x150", "host"), ("200x300_tiled", "lanes")])
def test_encode_to_size_with_regions(nets, name, coder):
    from icm_amd import bitstream as B
    from icm_amd import codec
    m = _net(nets, "cnn")
    a, kw = IMAGES[name]
    budget = len(codec.encode_image(m, a, coder=coder, qstep=16, roi=ROI, **kw))
    data, found = codec.encode_image_info(m, a, coder=coder, max_bytes=budget, roi=ROI, **kw)
    k = found["qstep"]
    print(f"{name} {coder}: budget {budget}: background qstep {k}, {len(data)} bytes, {found['probes']} probes, "
          f"map range {found['qmap_range']}, {found['roi_cells']} cells")
    assert len(data) <= budget and found["probes"] <= 8 and found["step"] == B.step_of(k)[0]
    assert data == codec.encode_image(m, a, coder=coder, qstep=k, roi=ROI, **kw)     # the probe's stream is the encode
    assert found["qmap_range"] == [max(k - 24, B.QSTEP_MIN), k]
    assert codec.encode_image(m, a, coder=coder, max_bytes=budget, roi=ROI, **kw) == data
    with pytest.raises(ValueError, match="not both"):
        codec.encode_image(m, a, coder=coder, qstep=3, max_bytes=10 ** 6, roi=ROI, **kw)


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


def test_cli_encodes_with_a_region_and_a_second_process_decodes(nets, cnn_ckpt, tmp_path):
    from icm_amd import bitstream as B
    from icm_amd import codec
    m = _net(nets, "cnn")
    a, _ = IMAGES["100x150"]
    src, stream, out = str(tmp_path / "in.png"), str(tmp_path / "in.icmb"), str(tmp_path / "out.png")
    Image.fromarray(a).save(src)
    r = _cli("encode", src, "-o", stream, "-a", "cnn", "-p", cnn_ckpt, "--qstep", "16", "--roi", "30,40,40,60:-24")
    assert r.returncode == 0, r.stderr[-2000:]
    enc = json.loads(r.stdout.strip().splitlines()[-1])
    data = open(stream, "rb").read()
    assert data == codec.encode_image(m, a, qstep=16, roi=ROI)
    assert enc["bytes"] == len(data) and enc["qstep"] == 16 and enc["qmap_range"] == [-8, 16] and enc["roi_cells"] == 20
    want, info = codec.decode_image(m, data, reference=a)
    r = _cli("decode", stream, "-o", out, "-p", cnn_ckpt, "--reference", src)
    assert r.returncode == 0, r.stderr[-2000:]
    dec = json.loads(r.stdout.strip().splitlines()[-1])
    assert dec["qstep"] is None and dec["qmap_range"] == [-8, 16] and "qmap" not in dec and dec["bytes"] == len(data)
    assert dec["psnr"] == pytest.approx(info["psnr"])
    assert np.array_equal(np.asarray(Image.open(out)), want.numpy())
    # one flipped byte inside the map string: exit code 4, nothing written
    _, strings = B.unpack(data)
    at = len(data) - B.CRC_BYTES - len(strings[2]) + 6             # the first run's k
    assert data[at:at + 1] == b"\x10"
    bad, never = str(tmp_path / "bad.icmb"), str(tmp_path / "never.png")
    with open(bad, "wb") as f:
        f.write(data[:at] + b"\x11" + data[at + 1:])
    r = _cli("decode", bad, "-o", never, "-p", cnn_ckpt)
    assert r.returncode == 4 and "Error:" in r.stderr and not os.path.exists(never)


def test_cli_refuses_a_region_outside_the_image(cnn_ckpt, tmp_path):
    a, _ = IMAGES["100x150"]
    src, stream = str(tmp_path / "in.png"), str(tmp_path / "never.icmb")
    Image.fromarray(a).save(src)
    r = _cli("encode", src, "-o", stream, "-a", "cnn", "-p", cnn_ckpt, "--qstep", "16", "--roi", "0,0,200,10:-8")
    assert r.returncode == 2 and "not inside" in r.stderr and not os.path.exists(stream)
    r = _cli("encode", src, "-o", stream, "-a", "cnn", "-p", cnn_ckpt, "--qstep", "16", "--roi", "0,0,20,10")
    assert r.returncode == 2 and not os.path.exists(stream)
