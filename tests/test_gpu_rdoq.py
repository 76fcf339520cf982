"""GPU: rate-distortion optimised quantisation at the model and codec level -- the unchanged decoder reproduces what the
RDOQ encoder reconstructed, a weight of 1e30 gives the strings of the encoder without it, slice 0 (whose means and
scales depend on nothing coded before) trades symbols for code length the way the decision says, the container and both
CLIs carry the flag, and every bad weight is refused before any GPU work."""
import numpy as np
import pytest
import torch
from PIL import Image

from oracle import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INPUTS = {"64x64": (1, 3, 64, 64), "128x64": (1, 3, 128, 64)}
MODEL_KS = [-16, -3, 0, 5, 32]


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


def _x(inp):
    return W._u(f"rdoq.x.{inp}", INPUTS[inp], 0.0, 1.0).to(DEV)


def _map(inp):
    """ks[(3 i + j) % 5] over the latent: non-uniform, and not symmetric in i and j"""
    h, w = INPUTS[inp][2] // 16, INPUTS[inp][3] // 16
    i, j = np.mgrid[0:h, 0:w]
    return np.array(MODEL_KS, dtype=np.int8)[(3 * i + j) % 5]


def _synthesis(m, arch, y_hat):
    from icm_amd import engine as E
    from icm_amd import models as M_
    with torch.no_grad():
        tape = E.Tape(need_grad=False, packed_cache=m._pack_cache())
        P = m._params()
        if arch == "cnn":
            return M_.wacnn_g_s(tape, P, y_hat.contiguous())
        return M_.stf_synthesis(tape, P, y_hat.contiguous(), None, m.window_size)


QUALITIES = {"k0": {}, "k-16": {"qstep": -16}, "map": "map"}


def _quality(name, inp):
    return {"qmap": _map(inp)} if name == "map" else dict(QUALITIES[name])


# ------------------------------------------------------------------------------------------------ 1. round trip
@pytest.mark.parametrize("inp", list(INPUTS))
@pytest.mark.parametrize("arch", ["cnn", "stf"])
def test_the_unchanged_decoder_reproduces_the_rdoq_encoder(nets, arch, inp):
    m = _net(nets, arch)
    x = _x(inp)
    for quality in QUALITIES:
        kw = _quality(quality, inp)
        for coder, w in (("host", 0.05), ("lanes", 2.0)):
            d = {}
            enc = m.compress(x, _debug=d, coder=coder, rdoq=w, **kw)
            assert set(enc) == ({"strings", "shape", "qstep", "qmap"} if quality == "map" else
                                {"strings", "shape", "qstep"})                    # the result says nothing of RDOQ
            x_hat = m.decompress(enc["strings"], enc["shape"], coder=coder, **kw)["x_hat"]
            want = _synthesis(m, arch, d["y_hat"]).clamp(0.0, 1.0)
            assert torch.equal(x_hat, want), (arch, inp, quality, coder, w)
            lat = m.compress_latent(m.analysis(x), coder=coder, rdoq=w, **kw)
            assert lat["strings"] == enc["strings"]
            plain = m.compress(x, coder=coder, **kw)
            assert plain["strings"][1] == enc["strings"][1]                       # z knows no RDOQ


# ------------------------------------------------------------------------------------------------ 2. weight 1e30
@pytest.mark.parametrize("arch", ["cnn", "stf"])
def test_a_huge_weight_gives_the_strings_without_rdoq(nets, arch):
    m = _net(nets, arch)
    for inp in INPUTS:
        x = _x(inp)
        for kw in ({"qstep": -16}, {"qstep": 5}, {"qmap": _map(inp)}):
            for coder in ("host", "lanes"):
                a = m.compress(x, coder=coder, rdoq=1e30, **kw)
                b = m.compress(x, coder=coder, **kw)
                assert a["strings"] == b["strings"], (arch, inp, list(kw), coder)


# ------------------------------------------------------------------------------------------------ 3. slice 0
def _code_lengths(gc, symbols, indexes):
    """sum over the elements of the code length of the table bin each symbol falls in, float64 from the integer CDF
    widths; an escaped symbol is charged its row's escape bin (RDOQ never touches one, so its further bits cancel)"""
    cdf = gc._quantized_cdf.cpu().numpy().astype(np.int64)
    sizes = gc._cdf_length.cpu().numpy().astype(np.int64)
    off = gc._offset.cpu().numpy().astype(np.int64)
    idx = indexes.astype(np.int64)
    ov = sizes[idx] - 2
    v = symbols.astype(np.int64) - off[idx]
    v = np.where((v >= 0) & (v < ov), v, ov)
    width = cdf[idx, v + 1] - cdf[idx, v]
    assert (width >= 1).all()
    return float(np.sum(16.0 - np.log2(width.astype(np.float64))))


@pytest.mark.parametrize("inp", list(INPUTS))
@pytest.mark.parametrize("arch", ["cnn", "stf"])
def test_slice_0_trades_symbols_for_code_length(nets, arch, inp):
    """K = -16 on the formula weights' own inputs (no input scaling was needed: symbols change there)."""
    m = _net(nets, arch)
    x = _x(inp)
    K, w = -16, 0.05
    d0, d1 = {}, {}
    m.compress(x, _debug=d0, qstep=K)
    m.compress(x, _debug=d1, qstep=K, rdoq=w)
    N, h, wd = x.shape[0], x.shape[2] // 16, x.shape[3] // 16
    n0 = N * (m.M // m.num_slices) * h * wd
    s0, s1 = d0["symbols"][:n0].astype(np.int64), d1["symbols"][:n0].astype(np.int64)
    i0, i1 = d0["indexes"][:n0], d1["indexes"][:n0]
    assert np.array_equal(i0, i1)
    moved = s1 != s0
    assert np.array_equal(s1[moved], s0[moved] - np.sign(s0[moved])) and bool((s0[moved] != 0).all())
    b0, b1 = _code_lengths(m.gaussian_conditional, s0, i0), _code_lengths(m.gaussian_conditional, s1, i1)
    print(f"{arch} {inp}: slice 0 of {n0} elements, {int((s0 != 0).sum())} non-zero, {int(moved.sum())} moved one "
          f"toward zero; table code lengths {b0:.2f} -> {b1:.2f} bits")
    assert moved.any()
    assert b1 < b0


# ------------------------------------------------------------------------------------------------ launches
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


def test_one_launch_per_slice_and_none_of_the_others(nets, monkeypatch):
    from icm_amd import _lib
    m = _net(nets, "cnn")
    S = m.num_slices
    x = _x("128x64")
    for kw in ({}, {"qstep": 5}, {"qmap": _map("128x64")}):
        m.compress(x, rdoq=0.5, **kw)                         # weights packed, tables and code lengths uploaded
    counting = _CountingLib(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: counting)
    per_kind = []
    for kw in ({}, {"qstep": 5}, {"qmap": _map("128x64")}):
        counting.calls.clear()
        enc = m.compress(x, rdoq=0.5, **kw)
        c = dict(counting.calls)
        assert c.get("icm_gc_code_rdo") == S
        assert not {"icm_gc_code_q", "icm_gc_code_qmap", "icm_gc_build_indexes", "icm_gc_likelihood_ste_fwd"} & set(c), c
        assert c.get("icm_quantize") == 1                     # z's
        per_kind.append(c)
        counting.calls.clear()
        m.decompress(enc["strings"], enc["shape"], **kw)
        assert "icm_gc_code_rdo" not in counting.calls
    assert per_kind[0] == per_kind[1] == per_kind[2]
    counting.calls.clear()
    m.compress(x, qstep=5)                                    # off: the launches of before, and the same number
    c5 = dict(counting.calls)
    assert "icm_gc_code_rdo" not in c5 and c5.get("icm_gc_code_q") == S
    assert {("icm_gc_code_q" if k == "icm_gc_code_rdo" else k): v for k, v in per_kind[1].items()} == c5


# ------------------------------------------------------------------------------------------------ 4. files
def _image(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(yy * 3 + xx * 2 + 40 * c) % 256 for c in range(3)], -1)
    return np.clip(base + rng.integers(-12, 13, size=(h, w, 3)), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("tile", [None, 128], ids=["untiled", "tiled"])
@pytest.mark.parametrize("coder", ["host", "lanes"])
def test_files_keep_their_shape(nets, coder, tile):
    from icm_amd import bitstream as B
    from icm_amd import codec
    m = _net(nets, "cnn")
    a = _image(100, 150, 4) if tile is None else _image(150, 200, 5)
    kw = {} if tile is None else {"tile": tile, "overlap": 16}
    for q in (({}, {"qstep": 8}, {"roi": [(30, 40, 40, 60, -8)]}) if tile is None else ({"roi": [(30, 40, 40, 60, -8)]},)):
        plain, pinfo = codec.encode_image_info(m, a, coder=coder, **q, **kw)
        data, info = codec.encode_image_info(m, a, coder=coder, rdoq=0.5, **q, **kw)
        assert info == {**pinfo, "rdoq": 0.5} and "rdoq" not in pinfo
        assert B.is_tiled(data) == B.is_tiled(plain) == (tile is not None)
        streams, plains = ((B.unpack_tiled(data)[1], B.unpack_tiled(plain)[1]) if tile else ([data], [plain]))
        assert len(streams) == len(plains) == (4 if tile else 1)
        for s, p in zip(streams, plains):
            (hs, ss), (hp, sp) = B.unpack(s), B.unpack(p)
            assert hs == hp and hs["arch"] == "cnn" and B.coder_of(s) == B.coder_of(p) == coder
            assert len(ss) == len(sp) and ss[1] == sp[1] and ss[2:] == sp[2:]     # z and the quality string: untouched
        img, dinfo = codec.decode_image(m, data, reference=a)
        assert tuple(img.shape) == a.shape and "psnr" in dinfo and "rdoq" not in dinfo
        assert dinfo["qstep"] == codec.decode_image(m, plain)[1]["qstep"]
        print(f"{coder} tile={tile} {q}: {len(plain)} bytes without, {len(data)} with rdoq 0.5; psnr {dinfo['psnr']:.3f}")


def test_encode_to_size_codes_every_probe_with_the_weight(nets, monkeypatch):
    from icm_amd import codec
    m = _net(nets, "cnn")
    a = _image(100, 150, 4)
    budget = len(codec.encode_image(m, a, qstep=8))
    seen = []
    real = type(m).compress_latent

    def spy(self, y, **kw):
        seen.append(kw.get("rdoq"))
        return real(self, y, **kw)
    monkeypatch.setattr(type(m), "compress_latent", spy)
    data, info = codec.encode_image_info(m, a, max_bytes=budget, rdoq=0.25)
    assert len(data) <= budget and info["rdoq"] == 0.25 and info["probes"] == len(seen) <= 8
    assert seen and all(w == 0.25 for w in seen)
    assert data == codec.encode_image(m, a, qstep=info["qstep"], rdoq=0.25)        # the probe's stream is the encode
    plain, pinfo = codec.encode_image_info(m, a, max_bytes=budget)
    assert "rdoq" not in pinfo
    print(f"budget {budget}: qstep {pinfo['qstep']} / {len(plain)} bytes without, qstep {info['qstep']} / {len(data)} "
          f"bytes with rdoq 0.25")


def test_cli_encodes_with_rdoq_and_decodes_without_a_flag(nets, tmp_path, capsys):
    import json
    from icm_amd import codec
    m = _net(nets, "cnn")
    a = _image(100, 150, 4)
    ckpt, src = str(tmp_path / "cnn.pt"), str(tmp_path / "in.png")
    stream, out = str(tmp_path / "in.icmb"), str(tmp_path / "out.png")
    torch.save(W.make_wacnn_state_dict(), ckpt)
    Image.fromarray(a).save(src)
    assert codec.main(["encode", src, "-o", stream, "-a", "cnn", "-p", ckpt, "--qstep", "8", "--rdoq", "0.5"]) == 0
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    data = open(stream, "rb").read()
    assert report["rdoq"] == 0.5 and report["qstep"] == 8 and report["bytes"] == len(data)
    assert data == codec.encode_image(m, a, qstep=8, rdoq=0.5)
    assert codec.main(["decode", stream, "-o", out, "-p", ckpt, "--reference", src]) == 0
    dec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert dec["qstep"] == 8 and "rdoq" not in dec
    assert np.array_equal(np.asarray(Image.open(out)), codec.decode_image(m, data)[0].numpy())


def test_inference_takes_the_weight(nets):
    from icm_amd import utils
    m = _net(nets, "cnn")
    x = _x("64x64")[0]
    a = utils.inference(m, x, qstep=-16)
    b = utils.inference(m, x, qstep=-16, rdoq=0.05)
    c = utils.inference(m, x, qstep=-16, rdoq=1e30)
    print(f"inference at qstep -16: bpp {a['bpp']:.4f} psnr {a['psnr']:.3f}; rdoq 0.05: bpp {b['bpp']:.4f} psnr "
          f"{b['psnr']:.3f}")
    assert c["bpp"] == a["bpp"] and c["psnr"] == a["psnr"]
    assert (b["bpp"], b["psnr"]) != (a["bpp"], a["psnr"])


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_bad_weights_are_refused_before_any_gpu_work(nets, tmp_path, capsys, monkeypatch):
    from icm_amd import _lib, codec, eval_model, utils
    m = _net(nets, "cnn")
    x = _x("64x64")
    y = m.analysis(x)
    a = _image(100, 150, 4)

    def no_launch():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_lib, "lib", no_launch)
    for bad in (0, -1, float("nan"), True, "x"):
        with pytest.raises(ValueError, match="rdoq"):
            m.compress(x, rdoq=bad)
        with pytest.raises(ValueError, match="rdoq"):
            m.compress_latent(y, rdoq=bad)
        with pytest.raises(ValueError, match="rdoq"):
            codec.encode_image(m, a, rdoq=bad)
        with pytest.raises(ValueError, match="rdoq"):
            codec.encode_image_info(m, a, max_bytes=10 ** 6, rdoq=bad)
        with pytest.raises(ValueError, match="rdoq"):
            utils.inference(m, x[0], rdoq=bad)
        with pytest.raises(ValueError, match="rdoq"):
            eval_model.eval_model(m, ["never-read.png"], rdoq=bad)
    with pytest.raises(ValueError, match="rdoq"):
        eval_model.eval_model(m, ["never-read.png"], entropy_estimation=True, rdoq=0.5)
    assert eval_model.main(["-d", str(tmp_path), "--rdoq", "0.5", "--entropy-estimation"]) == 2
    assert "--rdoq needs the real codec" in capsys.readouterr().err
