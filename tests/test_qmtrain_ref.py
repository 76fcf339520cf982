"""What tests/test_gpu_qmtrain_numerics.py and tests/test_gpu_qmtrain.py rely on, checked without a GPU for every input
set they use: float32 and float64 round to the same symbol everywhere (a condition the inputs are built to meet), every
likelihood band and the floor are populated, the references with a map that is uniform over each image are those of
tests/_qtrain_ref.py, the loss reference's gradient is autograd's, the trainer's rectangles are non-empty, inside the
map and in range, and the numpy painter is ``codec.roi_map``.  The caps are those of tests/test_entropy_ref.py."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "image-compression-for-machine_amd"))
import _entropy_ref as R  # noqa: E402
import _qmtrain_ref as M  # noqa: E402
import _qstep_ref as Q  # noqa: E402
import _qtrain_ref as T  # noqa: E402
from icm_amd.losses import qmap_lmbda_table  # noqa: E402
from icm_amd.trainer import qmap_rects_of  # noqa: E402
from test_entropy_ref import GREY_MAX, ORACLE_BITS_MAX, SHARE_MIN  # noqa: E402


@pytest.mark.parametrize("case", M.MAP_CASES)
def test_float32_and_float64_round_alike(case):
    inp = M.inputs(case)
    N, C, H, W = M.shape_of(case)
    assert tuple(inp["y"].shape) == (N, C, H, W) and tuple(inp["qmap"].shape) == (N, H, W)
    assert inp["qmap"].dtype == torch.int8 and inp["step"].shape == (N, 1, H, W)
    assert M.round_flips(inp) == 0
    assert M.symbols(inp).abs().max() > 3
    k = inp["qmap"].double()[:, None]
    assert torch.allclose(inp["step"].double(), 2.0 ** (k / 8), rtol=1e-7)
    assert torch.allclose(inp["step"].double() * inp["inv"].double(), torch.ones_like(k), rtol=2e-7)


def test_the_map_cases_are_what_they_are_named():
    m = M.maps("strided")
    assert all(sorted(set(m[n].reshape(-1).tolist())) == list(M.KS) for n in range(m.shape[0]))
    assert not (m[0] == m[1]).all()
    assert M.maps("tiny").reshape(-1).tolist() == [-16, 5, 32]
    lg = M.maps("long")
    assert int(np.prod(M.shape_of("long"))) > 2048 * 256
    assert all(sorted(set(lg[n].reshape(-1).tolist())) == [-8, 12] for n in range(2)) and lg[0, 0, 0] != lg[1, 0, 0]
    assert M.maps("uniform")[:, 0, 0].tolist() == list(T.QSTEPS["strided"])
    # the table: bitstream.step_table, restated
    from icm_amd.bitstream import step_table
    assert np.array_equal(M.step_table().view(np.int32), step_table().view(np.int32))
    assert torch.equal(M.lmbda_table(), qmap_lmbda_table(M.LMBDA, M.LMBDA_EXP))
    assert torch.equal(M.lmbda_table(0.01, 1.5), qmap_lmbda_table(0.01, 1.5))


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", M.BANDED)
def test_map_inputs_populate_every_class(case, mode):
    inp = M.inputs(case)
    r = M.raw(inp, mode)
    lik32 = M.oracle(inp, mode, torch.float32)
    live, floor, grey = R.classify(r)
    shares = [R.share(m) for m in R.bands(r)]
    errs = R.band_bits(lik32, r)
    print(f"map {case} {mode}: n {r.numel()} grey {R.share(grey):.4f} floor {R.share(floor):.4f} bands "
          + " ".join(f"{s:.4f}" for s in shares) + " | float32 restatement bits " + " ".join(f"{e:.3e}" for e in errs))
    assert R.share(grey) <= GREY_MAX and R.share(floor) >= SHARE_MIN
    for s, e, b in zip(shares, errs, R.BAND_NAMES):
        assert s >= SHARE_MIN, (case, mode, b, s)
        assert math.isfinite(e) and e < ORACLE_BITS_MAX, (case, mode, b, e)
    below, above, sgrey = R.scale_classes(inp["scale"])
    assert int(sgrey.sum()) == 3 and R.share(below) >= 0.005 and R.share(above) >= 0.9
    assert live.any() and floor.any()


@pytest.mark.parametrize("mode", R.MODES)
def test_a_uniform_map_is_the_per_image_step(mode):
    """the reference with a map that is uniform over each image equals tests/_qtrain_ref.py's, in float64"""
    inp = M.inputs("uniform")
    per = {k: inp[k] for k in ("y", "mu", "scale", "noise")}
    per["steps"] = M.per_image_steps("uniform")
    assert torch.equal(M.symbols(inp), T.symbols(per)) and torch.equal(M.yhat(inp), T.yhat(per))
    r = M.raw(inp, mode)
    assert torch.equal(r, T.stepped_raw(per, mode))
    dlik = R.seed(r, "mixed", "qmn.uni." + mode)
    a, ga = M.oracle(inp, mode, torch.float64, dlik)
    b, gb = T.stepped_oracle(per, mode, torch.float64, dlik)
    assert torch.equal(a, b)
    for u, v in zip(ga, gb):
        assert torch.equal(u, v)
    assert ga[2].abs().max() > 0 and (mode == "eval" or ga[0].abs().max() > 0)


def test_yhat_is_the_dequantised_symbol_per_position():
    inp = M.inputs("strided")
    sym, yh = M.symbols(inp).numpy(), M.yhat(inp).numpy()
    m = M.maps("strided")
    for n, yy, xx in ((0, 0, 0), (1, 5, 7), (1, 23, 22)):
        step, inv = Q.step_of(int(m[n, yy, xx]))
        assert np.array_equal(sym[n, :, yy, xx], Q.symbols(inp["y"].numpy()[n, :, yy, xx], inp["mu"].numpy()[n, :, yy, xx], inv))
        assert np.array_equal(Q.bits(yh[n, :, yy, xx]), Q.bits(Q.dequantize(sym[n, :, yy, xx], inp["mu"].numpy()[n, :, yy, xx], step)))


# ------------------------------------------------------------------------------------------------ per-cell loss
@pytest.mark.parametrize("case", sorted(M.LOSS_CASES))
def test_per_cell_loss_reference(case):
    N, C, H, W = M.LOSS_CASES[case]
    x, xh, ly, lz, qm = M.loss_inputs(case)
    x, xh, ly, lz = (t.double() for t in (x, xh, ly, lz))
    assert qm.shape == (N, H // 16, W // 16) and qm.dtype == np.int8
    npix = N * H * W
    table = M.lmbda_table()
    lam = M.pixel_weights(qm, table)
    assert lam.shape == (N, 1, H, W)
    # a pixel's weight is its cell's
    for n, yy, xx in ((0, 0, 0), (N - 1, H - 1, W - 1), (0, 15, 15), (N - 1, 16 % H, 17 % W)):
        k = int(qm[n, yy // 16, xx // 16])
        assert lam[n, 0, yy, xx].item() == float(np.float32(M.LMBDA * 2.0 ** (-k * M.LMBDA_EXP / 8.0)))
    # maps uniform over each image: the per-image loss of tests/_qtrain_ref.py
    ks = [(-16, 5, 32)[n] for n in range(N)]
    uni = np.ascontiguousarray(np.asarray(ks, dtype=np.int8).reshape(N, 1, 1) * np.ones((1, H // 16, W // 16), dtype=np.int8))
    lam_n = table.double()[torch.tensor([k & 255 for k in ks])]
    a = M.m_loss(x, xh, ly, lz, npix, M.pixel_weights(uni, table))
    b = T.rdw_loss(x.reshape(N, -1), xh.reshape(N, -1), ly, lz, npix, lam_n)
    assert torch.allclose(a, b, rtol=1e-12, atol=0)
    # the gradient: autograd's is the closed form
    dxh, dly, dlz = M.m_grads(x, xh, ly, lz, npix, lam, 0.5)
    assert torch.allclose(dxh, 0.5 * lam * 255.0 ** 2 * 2.0 / x.numel() * (xh - x), rtol=1e-10, atol=0)
    assert torch.allclose(dly, 0.5 / (-math.log(2.0) * npix) / ly, rtol=1e-10)
    assert torch.allclose(dlz, 0.5 / (-math.log(2.0) * npix) / lz, rtol=1e-10)
    g = M.m_chains(N, C, H, W, ly.numel(), lz.numel())
    assert 4 * g["T"] <= 8192
    if case == "odd":
        assert g["rpb"] == 3 and g["bpi"] > 1            # 240 of 256 lanes, several workgroups per image
    if case == "span":
        assert qm.min() == -16 and qm.max() == 32


# ------------------------------------------------------------------------------------------------ rectangles, painter
@pytest.mark.parametrize("hw", [(4, 4), (1, 1)])
def test_drawn_rectangles_are_non_empty_inside_the_map_and_in_range(hw):
    h, w = hw
    lo, hi = -8, 16
    g = torch.Generator().manual_seed(11)
    u = torch.rand((10000, 5), generator=g)
    u[0], u[1] = 0.0, float(np.nextafter(np.float32(1), np.float32(0)))          # both ends of [0, 1)
    r = qmap_rects_of(u, h, w, lo, hi)
    assert r.dtype == torch.int32 and r.shape == (10000, 5)
    y0, x0, y1, x1, k = (r[:, i] for i in range(5))
    assert (y0 >= 0).all() and (x0 >= 0).all() and (y1 > y0).all() and (x1 > x0).all() and (y1 <= h).all() and (x1 <= w).all()
    assert (k >= lo).all() and (k <= hi).all()
    assert set(k.tolist()) == set(range(lo, hi + 1))
    if hw == (4, 4):
        assert set(y0.tolist()) == {0, 1, 2, 3} and set(x1.tolist()) == {1, 2, 3, 4}
    # a pure function of its arguments, in any leading shape
    assert torch.equal(qmap_rects_of(u.reshape(100, 100, 5), h, w, lo, hi).reshape(-1, 5), r)
    assert qmap_rects_of(u[:3], h, w, 5, 5)[:, 4].tolist() == [5, 5, 5]


def test_numpy_painter_is_roi_map():
    """rectangles in pixel units aligned to cells, painted by ``codec.roi_map`` and by the numpy painter"""
    from icm_amd.codec import roi_map
    rng = np.random.default_rng(3)
    for h, w in ((1, 1), (4, 4), (5, 7), (16, 16)):
        for R_ in (0, 1, 8):
            base = int(rng.integers(-16, 33))
            rects, rois = [], []
            for _ in range(R_):
                y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
                y1, x1 = int(rng.integers(y0 + 1, h + 1)), int(rng.integers(x0 + 1, w + 1))
                k = int(rng.integers(-16, 33))
                rects.append((y0, x0, y1, x1, k))
                rois.append((16 * y0, 16 * x0, 16 * (y1 - y0), 16 * (x1 - x0), k - base))
            want = roi_map(16 * h, 16 * w, (0, 0, 0, 0), base, rois)
            got = M.paint([base], np.asarray(rects, dtype=np.int32).reshape(1, R_, 5), h, w)
            assert got.dtype == np.int8 and np.array_equal(got[0], want), (h, w, R_)
    # empty and out-of-map rectangles: nothing, and the part inside
    got = M.paint([3, 4], [[(1, 1, 1, 3, 9), (-2, -2, 1, 1, 7)], [(2, 2, 9, 9, -5), (3, 0, 2, 4, 1)]], 4, 4)
    want0 = np.full((4, 4), 3)
    want0[0, 0] = 7
    want1 = np.full((4, 4), 4)
    want1[2:, 2:] = -5
    assert np.array_equal(got[0], want0) and np.array_equal(got[1], want1)
