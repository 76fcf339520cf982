"""CPU: rate-distortion optimised quantisation on the host side -- the float32 restatement of the decision
(tests/_rdoq_ref.py) on hand-computed elements, ``bitstream.code_length_table`` against integer widths and against the
restatement's table, ``bitstream.check_rdoq``, the argument errors of the two CLIs and of the models, which come before
any GPU work, and the regimes of the input sets that tests/test_gpu_rdoq_numerics.py runs on the device."""
import numpy as np
import pytest
import torch

import _qstep_ref as Q
import _rdoq_ref as D
from icm_amd import bitstream as B

F = np.float32


# ------------------------------------------------------------------------------------------------ the restatement
# One element each, at k = 0 (step = inv = 1) and mu = 0, so u = y, on the synthetic tables: the scale picks the row
# (<= 0.5: row 0, <= 1: row 1, <= 2: row 2, else row 3), whose symbols and code lengths in bits are
#   row 0  -1 .. 1   3 1 3                      row 1  -3 .. 3   6 4 3 1 3 4 6
#   row 2  -5 .. 5   10 10 6 5 3 1 3 5 6 10 10  row 3   1 .. 5   1 2 3 4 5      (offset +1: no symbol 0 in the table)
# (y, scale, w) -> the symbol coded, and why
HAND = {
    "s0 is 0":                        (0.3, 1.0, 1.0, 0),      # nothing to move
    "a change":                       (1.4, 1.0, 1.0, 0),      # J0 = 0.16 + 3, J1 = 1.96 + 1
    "a keep":                         (1.0, 1.0, 4.0, 1),      # J0 = 0 + 3, J1 = 4 + 1
    "a tie keeps":                    (2.0, 1.0, 1.0, 2),      # J0 = 0 + 4, J1 = 1 + 3: equal, and the comparison is strict
    "negative, a change":             (-1.4, 1.0, 1.0, 0),
    "negative, a tie keeps":          (-2.0, 1.0, 1.0, -2),
    "negative, a keep":               (-1.0, 1.0, 4.0, -1),
    "v0 at 0":                        (-2.6, 1.0, 1.0, -2),    # s0 = -3 is the row's first symbol: J0 = 0.16 + 6, J1 = 0.36 + 4
    "v0 at ov - 1":                   (2.6, 1.0, 1.0, 2),      # s0 = 3 is the row's last symbol
    "positive offset, s1 under it":   (1.2, 4.0, 1e-30, 1),    # row 3: s1 = 0 has v1 = -1, kept though 0 bits would win
    "positive offset, both inside":   (2.2, 4.0, 1e-30, 1),    # row 3: 2 bits -> 1 bit
    "above the table":                (4.2, 1.0, 1e-30, 4),    # v0 = 7 = ov: the escape bin, kept though s1 = 3 is inside
    "below the table":                (-4.2, 1.0, 1e-30, -4),
    "above a short row":              (2.2, 0.5, 1e-30, 2),    # row 0: v0 = 3 = ov
    "below a positive offset":        (-1.3, 4.0, 1e-30, -1),  # row 3: v0 = -2
    "far above":                      (3.0e4, 2.0, 1e-30, 30000),
    "clamped":                        (-1.0e30, 2.0, 1e-30, -2 ** 30),
}


def _hand(y, scale, w):
    cdf, sizes, offsets, table, bound = D.synthetic_tables()
    bits = D.code_length_table(cdf, sizes)
    shape = (1, 1, 1)
    return D.decide(np.full(shape, y, dtype=F), np.zeros(shape, dtype=F), np.full(shape, scale, dtype=F), table, bound,
                    F(1), F(1), sizes, offsets, bits, w)


@pytest.mark.parametrize("name", list(HAND))
def test_hand_computed_elements(name):
    y, scale, w, want = HAND[name]
    d = _hand(y, scale, w)
    assert d["sym"].item() == want, (name, {k: v.item() for k, v in d.items()})
    assert d["yh"].item() == float(want) and d["yh"].dtype == np.float32            # mu = 0, step = 1
    assert d["idx"].item() == {0.5: 0, 1.0: 1, 2.0: 2, 4.0: 3}[scale]


def test_hand_computed_costs():
    """the numbers the table above quotes, as the restatement forms them"""
    d = _hand(1.4, 1.0, 1.0)
    assert d["s0"].item() == 1 and d["s1"].item() == 0 and (d["v0"].item(), d["v1"].item()) == (4, 3)
    assert d["j0"].item() == pytest.approx(3.16, abs=1e-6) and d["j1"].item() == pytest.approx(2.96, abs=1e-6)
    assert d["change"].item()
    d = _hand(2.0, 1.0, 1.0)
    assert d["j0"].item() == 4.0 == d["j1"].item() and d["cand"].item() and not d["change"].item()
    d = _hand(-2.6, 1.0, 1.0)
    assert d["v0"].item() == 0 and d["v1"].item() == 1 and d["change"].item()
    d = _hand(2.6, 1.0, 1.0)
    assert d["v0"].item() == d["ov"].item() - 1 == 6 and d["change"].item()
    d = _hand(1.2, 4.0, 1e-30)
    assert (d["v0"].item(), d["v1"].item()) == (0, -1) and not d["cand"].item()
    d = _hand(4.2, 1.0, 1e-30)
    assert d["v0"].item() == d["ov"].item() == 7 and d["in1"].item() and not d["cand"].item()
    # with no table entry inside reach the outputs are the plain quantiser's
    for y in (3.0e4, -1.0e30, 0.3):
        d = _hand(y, 2.0, 1e-30)
        want = Q.code(np.full((1, 1, 1), y, dtype=F), np.zeros((1, 1, 1), dtype=F), np.full((1, 1, 1), 2.0, dtype=F),
                      D.synthetic_tables()[3], D.SYN_BOUND, F(1), F(1))
        assert d["sym"].item() == want[0].item() and d["idx"].item() == want[1].item() and d["yh"].item() == want[2].item()


def test_a_step_scales_the_decision_not_the_weight():
    """the decision lives in symbol units: the same u under another step gives the same choice, and y_hat scales"""
    cdf, sizes, offsets, table, bound = D.synthetic_tables()
    bits = D.code_length_table(cdf, sizes)
    u = np.array([1.4, 2.0, -2.6, 0.3, 1.0, 4.2], dtype=F).reshape(1, 1, -1)
    mu = np.zeros_like(u)
    base = D.decide(u, mu, np.full_like(u, 1.0), table, bound, F(1), F(1), sizes, offsets, bits, 1.0)
    for k in (-16, 8):                                                            # powers of two: u is exact
        step, inv = Q.step_of(k)
        d = D.decide(u * step, mu, np.full_like(u, 1.0) * step, table, bound, step, inv, sizes, offsets, bits, 1.0)
        assert np.array_equal(d["sym"], base["sym"]) and np.array_equal(d["idx"], base["idx"])
        assert np.array_equal(d["yh"], base["sym"].astype(F) * step)
    assert base["sym"].reshape(-1).tolist() == [0, 2, -2, 0, 0, 4]


# ------------------------------------------------------------------------------------------------ code_length_table
def test_code_length_table_on_integer_widths():
    widths = [65536 >> k for k in range(1, 16)]                                   # 32768 .. 2: k bits each
    cdf = np.zeros((2, 20), dtype=np.int32)
    cdf[0, 1:16] = np.cumsum(widths)
    cdf[0, 16] = 65536                                                            # the escape bin takes the last 2
    cdf[1, 1:4] = [1, 3, 65536]                                                   # widths 1 and 2, then the escape bin
    sizes = np.array([17, 4], dtype=np.int32)
    bits = B.code_length_table(cdf, sizes)
    assert bits.dtype == np.float32 and bits.shape == cdf.shape
    assert bits[0, :15].tolist() == [float(k) for k in range(1, 16)]
    assert bits[1, :2].tolist() == [16.0, 15.0]
    assert not bits[0, 15:].any() and not bits[1, 2:].any()                       # the escape bin and the padding: 0
    assert np.array_equal(bits, D.code_length_table(cdf, sizes))
    assert np.array_equal(B.code_length_table(torch.from_numpy(cdf).numpy().astype(np.int64), sizes.tolist()), bits)


@pytest.mark.parametrize("tables", ["synthetic", "model"])
def test_code_length_table_is_the_restatements(tables):
    cdf, sizes, offsets, table, bound = D.synthetic_tables() if tables == "synthetic" else D.oracle_model_tables()
    bits = B.code_length_table(cdf, sizes)
    want = D.code_length_table(cdf, sizes)
    assert bits.dtype == np.float32 and np.array_equal(bits.view(np.int32), want.view(np.int32))
    for r in (0, len(sizes) - 1):
        n = int(sizes[r]) - 2
        w = np.diff(cdf[r].astype(np.int64))[:n]
        assert np.allclose(bits[r, :n], 16 - np.log2(w), rtol=0, atol=2e-6) and not bits[r, n:].any()
        assert abs(float(np.sum(w * 2.0 ** -16)) + (65536 - int(cdf[r, n])) * 2.0 ** -16 - 1.0) < 1e-12
    if tables == "synthetic":
        assert bits[0, :3].tolist() == [3.0, 1.0, 3.0] and bits[3, :5].tolist() == [1.0, 2.0, 3.0, 4.0, 5.0]
        assert offsets.tolist() == [-1, -3, -5, 1] and sizes.tolist() == [5, 9, 13, 7]


def test_code_length_table_refuses_what_is_no_table():
    cdf, sizes, _, _, _ = D.synthetic_tables()
    for bad_cdf, bad_sizes in ((cdf[0], sizes), (cdf.astype(np.float32), sizes), (cdf, sizes[:3]),
                               (cdf, np.array([5, 9, 14, 7])), (cdf, np.array([5, 9, 1, 7])),
                               (cdf, sizes.astype(np.float64))):
        with pytest.raises(ValueError):
            B.code_length_table(bad_cdf, bad_sizes)
    flat = cdf.copy()
    flat[1, 3] = flat[1, 2]                                                       # a bin of no width inside the table
    with pytest.raises(ValueError, match="no width"):
        B.code_length_table(flat, sizes)


# ------------------------------------------------------------------------------------------------ check_rdoq
def test_check_rdoq():
    assert B.check_rdoq(None) is None
    for w in (0.25, 4.0, 1, 3, 1e30, 1e-30, 1e-45, np.float32(0.1), np.float64(2.5), np.int64(7)):
        v = B.check_rdoq(w, "x: ")
        assert isinstance(v, float) and v == float(np.float32(w)) and v > 0
    assert B.check_rdoq(0.1) == float(np.float32(0.1)) != 0.1                     # the f32 value, as the kernel takes it
    for bad in (0, 0.0, -1, -0.5, float("nan"), float("inf"), -float("inf"), 1e39, 1e-46, 10 ** 400, True, False, "x",
                "0.5", [1.0], (2.0,), 1 + 0j, np.array([1.0]), torch.tensor(1.0), np.float32("nan")):
        with pytest.raises(ValueError, match="rdoq"):
            B.check_rdoq(bad, "who: ")


# ------------------------------------------------------------------------------------------------ argument errors
@pytest.mark.parametrize("value", ["0", "-1", "nan", "inf", "1e39", "1e-46"])
def test_codec_cli_refuses_a_bad_rdoq_before_any_gpu_check(value, tmp_path, capsys, monkeypatch):
    from icm_amd import codec

    def no_gpu_check():
        raise AssertionError("the GPU was asked for")
    monkeypatch.setattr(torch.cuda, "is_available", no_gpu_check)
    monkeypatch.setattr(codec, "_load", lambda *a: (_ for _ in ()).throw(AssertionError("a checkpoint was loaded")))
    out = str(tmp_path / "o.icmb")
    assert codec.main(["encode", str(tmp_path / "missing.png"), "-o", out, "-p", "none.pt", "--rdoq", value]) == 2
    err = capsys.readouterr().err
    assert "Error:" in err and "rdoq" in err
    assert not (tmp_path / "o.icmb").exists()


def test_codec_cli_rdoq_is_an_encode_flag_and_a_number(tmp_path, capsys):
    from icm_amd import codec
    out = str(tmp_path / "o.icmb")
    with pytest.raises(SystemExit) as e:
        codec.main(["encode", str(tmp_path / "missing.png"), "-o", out, "-p", "none.pt", "--rdoq", "x"])
    assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        codec.main(["decode", str(tmp_path / "missing.icmb"), "-o", out, "-p", "none.pt", "--rdoq", "0.5"])
    assert e.value.code == 2
    assert "--rdoq" in capsys.readouterr().err and not (tmp_path / "o.icmb").exists()
    assert codec.setup_args().parse_args(["encode", "a.png", "-o", "b", "-p", "c"]).rdoq is None


def test_eval_model_refuses_a_bad_rdoq(tmp_path, capsys, monkeypatch):
    from icm_amd import eval_model

    def no_gpu_check():
        raise AssertionError("the GPU was asked for")
    monkeypatch.setattr(torch.cuda, "is_available", no_gpu_check)
    assert eval_model.main(["-d", str(tmp_path), "--rdoq", "0"]) == 2
    assert eval_model.main(["-d", str(tmp_path), "--rdoq", "nan"]) == 2
    assert eval_model.main(["-d", str(tmp_path), "--rdoq", "0.5", "--entropy-estimation"]) == 2
    err = capsys.readouterr().err
    assert err.count("Error:") == 3 and "entropy estimation" in err
    with pytest.raises(ValueError, match="rdoq"):
        eval_model.eval_model(None, [], entropy_estimation=True, rdoq=0.5)
    with pytest.raises(ValueError, match="rdoq"):
        eval_model.eval_model(None, [], rdoq=-1)


def test_models_refuse_a_bad_rdoq_before_any_work():
    from icm_amd import utils
    from icm_amd.zoo import models
    net = models["cnn"]().eval()
    x = torch.zeros(1, 3, 64, 64)
    for bad in (0, -1, float("nan"), True, "x"):
        with pytest.raises(ValueError, match="rdoq"):
            net.compress(x, rdoq=bad)
        with pytest.raises(ValueError, match="rdoq"):
            net.compress_latent(torch.zeros(1, 320, 4, 4), rdoq=bad)
        with pytest.raises(ValueError, match="rdoq"):
            utils.inference(net, x, rdoq=bad)
    with pytest.raises(TypeError):
        net.decompress([[b""], [b""]], (1, 1), rdoq=0.5)                          # the decoder knows no RDOQ
    stf6 = models["stf6"]().eval()
    with pytest.raises(NotImplementedError):
        stf6.compress(x, rdoq=0.5)
    with pytest.raises(NotImplementedError):
        stf6.compress_latent(torch.zeros(1, 384, 4, 4), rdoq=0)                   # its own override raises first


# ------------------------------------------------------------------------------------------------ regimes
_BITS = {}


def _tables(kind):
    t = D.synthetic_tables() if kind == "synthetic" else D.oracle_model_tables()
    if kind not in _BITS:
        _BITS[kind] = D.code_length_table(t[0], t[1])
    return t, _BITS[kind]


@pytest.mark.parametrize("shape", [s for s in D.SHAPES if s[2] == 257], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("form", D.FORMS)
@pytest.mark.parametrize("name", ["edges", "mixed"])
@pytest.mark.parametrize("tables", ["synthetic", "model"])
def test_input_sets_reach_every_branch(tables, name, form, shape):
    """What each input set of the device tests must exercise, per weight.  Every set: a zero, escaped symbols above and
    below the table, candidates of both signs.  w = 0.25 and 4: changes and strict keeps of both signs.  w = 1e-30: the
    distortion term vanishes and the tables' code lengths fall toward zero (but for a few tail bins of the quantised
    rows), so a candidate changes unless its two code lengths are equal (a tie: tail bins of equal width) -- changes
    and ties; a strict keep is not asked for.  w = 1e30:
    no change at all, keeps of both signs and, in the "edges" set at a step that is a power of two, exact ties (u on a
    half, the nearest even symbol further from zero: equal errors, and the code lengths vanish beside 1e30 / 4).  The
    synthetic tables also hold a positive offset: a symbol in the table whose neighbour is under it.  The models' rows
    are symmetric about 0 with negative offsets, so there a neighbour toward zero of a symbol inside is always inside.
    "edges" puts candidates on the first and the last symbol of a row."""
    (cdf, sizes, offsets, table, bound), bits = _tables(tables)
    step, inv, _ = D.form_steps(form, shape[2])
    y, mu, scale = D.inputs(name, shape, step, inv, table, bound, sizes, offsets)
    for w in D.WEIGHTS:
        d = D.decide(y, mu, scale, table, bound, step, inv, sizes, offsets, bits, w)
        b = D.branches(d)
        print(tables, name, form, shape, w, b)
        assert b["zero"] > 0 and b["below"] > 0 and b["above"] > 0
        assert (b["s1_outside"] > 0) == (tables == "synthetic")
        # (the scale bound times inv keeps a fine step out of the narrowest rows: 0.25 x 4 is row 1's entry)
        assert len(np.unique(d["idx"])) >= (len(sizes) - 1 if tables == "synthetic" else 20)
        if w == 1e30:
            assert b["change"] == 0 and b["keep_pos"] > 0 and b["keep_neg"] > 0
            if name == "edges" and form in ("k-16", "k0"):
                assert b["tie"] > 0
        else:
            assert b["change_pos"] > 0 and b["change_neg"] > 0
            if w == 1e-30:
                assert b["tie"] > 0
            else:
                assert b["keep_pos"] > 0 and b["keep_neg"] > 0
        if name == "edges":
            assert b["v0_first"] > 0 and b["v0_last"] > 0
        if name == "mixed" and tables == "model" and w == 0.25:
            n = b["elements"]
            unchanged = int(((d["s0"] != 0) & ~d["change"]).sum())
            assert b["change"] >= 0.2 * n and unchanged >= 0.2 * n, (b["change"] / n, unchanged / n)
    # y_hat is that of the symbol coded and the indexes are the plain quantiser's
    plain = Q.code(y, mu, scale, table, bound, np.broadcast_to(step, y.shape), np.broadcast_to(inv, y.shape))
    assert np.array_equal(d["idx"], plain[1]) and np.array_equal(d["sym"], plain[0])            # d: w = 1e30
    assert np.array_equal(Q.bits(d["yh"]), Q.bits(plain[2]))


def test_the_smallest_shapes_still_hold_the_fixed_cases():
    (cdf, sizes, offsets, table, bound), bits = _tables("synthetic")
    for shape in D.SHAPES[:2]:
        step, inv, _ = D.form_steps("k0", shape[2])
        y, mu, scale = D.inputs("edges", shape, step, inv, table, bound, sizes, offsets)
        d = D.decide(y, mu, scale, table, bound, step, inv, sizes, offsets, bits, 0.25)
        assert d["s0"].reshape(-1)[:6].tolist() == [0, 1, -1, 2, -2, 10 ** 4]
        assert d["sym"].reshape(-1)[5] == 10 ** 4
