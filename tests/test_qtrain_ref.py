"""What tests/test_gpu_qtrain_numerics.py relies on, checked without a GPU for every input set it uses: float32 and
float64 round to the same symbol everywhere, every likelihood band and the floor are populated, both arms of the scale
bound are reached, few elements are grey, and the float32 restatement (the yardstick the GPU limits are formed from) is
itself close to float64.  The caps are those of tests/test_entropy_ref.py.  Prints the shares (pytest -s)."""
import math

import pytest
import torch

import _entropy_ref as R
import _qtrain_ref as T
from test_entropy_ref import GREY_MAX, ORACLE_BITS_MAX, SHARE_MIN


@pytest.mark.parametrize("case", T.CASES)
def test_float32_and_float64_round_alike(case):
    inp = T.stepped_inputs(case)
    assert tuple(inp["y"].shape) == T.shape_of(case) and inp["steps"].shape == (inp["y"].shape[0], 2)
    assert T.round_flips(inp) == 0
    # the symbols are not all zero, and each image carries its own step
    assert T.symbols(inp).abs().max() > 3
    for n, k in enumerate(T.QSTEPS[case]):
        assert inp["steps"][n, 0].item() == pytest.approx(2.0 ** (k / 8), rel=1e-7)
        assert inp["steps"][n, 0].item() * inp["steps"][n, 1].item() == pytest.approx(1.0, rel=2e-7)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", T.BANDED)
def test_stepped_inputs_populate_every_class(case, mode):
    inp = T.stepped_inputs(case)
    r = T.stepped_raw(inp, mode)
    lik32 = T.stepped_oracle(inp, mode, torch.float32)
    live, floor, grey = R.classify(r)
    shares = [R.share(m) for m in R.bands(r)]
    errs = R.band_bits(lik32, r)
    print(f"stepped {case} {mode}: n {r.numel()} grey {R.share(grey):.4f} floor {R.share(floor):.4f} bands "
          + " ".join(f"{s:.4f}" for s in shares) + " | float32 restatement bits " + " ".join(f"{e:.3e}" for e in errs))
    assert R.share(grey) <= GREY_MAX and R.share(floor) >= SHARE_MIN
    for s, e, b in zip(shares, errs, R.BAND_NAMES):
        assert s >= SHARE_MIN, (case, mode, b, s)
        assert math.isfinite(e) and e < ORACLE_BITS_MAX, (case, mode, b, e)
    assert (lik32[floor] == torch.tensor(1e-9, dtype=torch.float32)).all()
    # both arms of both bounds: scales on either side of 0.11 (and its three grey neighbours), likelihoods on the floor
    below, above, sgrey = R.scale_classes(inp["scale"])
    assert int(sgrey.sum()) == 3 and R.share(below) >= 0.005 and R.share(above) >= 0.9
    assert live.any() and floor.any()


def test_tiny_case_reaches_three_steps():
    inp = T.stepped_inputs("tiny")
    assert inp["y"].shape == (3, 7, 1, 1) and T.QSTEPS["tiny"] == (-16, 5, 32)
    for mode in R.MODES:
        r = T.stepped_raw(inp, mode)
        assert torch.isfinite(r).all() and (r > 0).all() and (r <= 1).all()


def test_raw_restates_the_oracle_and_step_zero_the_scalar_form():
    """the un-bounded float64 likelihood used for the classification is the restatement's where the bound is inactive;
    with step 1 the restatement is the oracle's own Gaussian likelihood"""
    for case in ("strided", "zero"):
        inp = T.stepped_inputs(case)
        for mode in R.MODES:
            r, lik = T.stepped_raw(inp, mode), T.stepped_oracle(inp, mode, torch.float64)
            assert torch.equal(torch.clamp(r, min=1e-9), lik)
    inp = T.stepped_inputs("zero")
    assert torch.equal(inp["steps"], torch.ones(2, 2))
    plain = {k: inp[k] for k in ("y", "mu", "scale", "noise")}
    assert torch.equal(T.symbols(inp).float(), R.gaussian_round(plain))
    for mode in R.MODES:
        want = R.gaussian_oracle(plain, mode, torch.float64)
        got = T.stepped_oracle(inp, mode, torch.float64)
        assert torch.allclose(got, want, rtol=1e-12, atol=0)


def test_gradient_factors_of_the_step():
    """the chain rule the kernel implements, against autograd: through t the likelihood reaches y with the factor inv
    (and mu with its negative), through the scale with the factor inv, and in eval mode nothing reaches y or mu"""
    inp = T.stepped_inputs("strided")
    r = T.stepped_raw(inp, "train")
    dlik = R.seed(r, "mixed", "qtn.fac")
    _, (dy, dmu, dsc) = T.stepped_oracle(inp, "train", torch.float64, dlik)
    assert torch.equal(dy, -dmu) and dy.abs().max() > 0 and dsc.abs().max() > 0
    # the same inputs in symbol units and a unit step: d/dy' with y' = y * inv is d/dy / inv
    inv = inp["steps"][:, 1].double().reshape(-1, 1, 1, 1)
    unit = {"y": (inp["y"].double() - inp["mu"].double()) * inv, "mu": torch.zeros_like(r),
            "scale": torch.clamp(inp["scale"].double(), min=R.O.SCALE_BOUND) * inv, "noise": inp["noise"].double(),
            "steps": torch.ones(2, 2)}
    _, (uy, _, us) = T.stepped_oracle(unit, "train", torch.float64, dlik)
    # (where the unit-step form's own bound, 0.11 in symbols, stays inactive)
    live = R.classify(r)[0] & (unit["scale"] > R.O.SCALE_BOUND)
    above = inp["scale"].double() > R.O.SCALE_BOUND
    assert R.share(live) > 0.5 and R.share(live & above) > 0.5
    assert torch.allclose(dy[live], (uy * inv)[live], rtol=1e-9, atol=1e-300)
    assert torch.allclose(dsc[live & above], (us * inv)[live & above], rtol=1e-9, atol=1e-300)
    _, (ey, emu, _) = T.stepped_oracle(inp, "eval", torch.float64, dlik)
    assert (ey == 0).all() and (emu == 0).all()


@pytest.mark.parametrize("case", sorted(T.RDW_CASES))
def test_weighted_loss_reference(case):
    """equal weights give the scalar loss of tests/_pointwise_ref.py; unequal ones weigh each image's own error"""
    import _pointwise_ref as P
    N, per, ny, nz = T.RDW_CASES[case]
    x, xh, ly, lz, lam = (t.double() for t in T.rdw_inputs(case))
    npix = N * per // 3
    assert lam.numel() == N and len(set(lam.tolist())) == N
    same = torch.full((N,), 0.0067, dtype=torch.float64)
    want = P.rd_loss_fwd(x.reshape(-1), xh.reshape(-1), ly, lz, npix, 0.0067)
    assert torch.allclose(T.rdw_loss(x, xh, ly, lz, npix, same), want, rtol=1e-12)
    got = T.rdw_loss(x, xh, ly, lz, npix, lam)
    mse_n = ((xh - x) ** 2).mean(1)
    assert got[2].item() == pytest.approx(255.0 ** 2 * sum(l * m for l, m in zip(lam.tolist(), mse_n.tolist())) / N
                                          + got[0].item(), rel=1e-12)
    assert got[1].item() == pytest.approx(mse_n.mean().item(), rel=1e-12)
    dxh, dly, dlz = T.rdw_grads(x, xh, ly, lz, npix, lam, 0.5)
    for n in range(N):
        assert torch.allclose(dxh[n], 0.5 * lam[n] * 255.0 ** 2 * 2.0 / (N * per) * (xh[n] - x[n]), rtol=1e-10, atol=0)
    assert torch.allclose(dly, 0.5 / (-math.log(2.0) * npix) / ly, rtol=1e-10)
    g = T.rdw_chains(N, per, ny, nz)
    assert 3 * N * g["bpi"] <= 8192 and (g["bpi"] > 1) == (case == "blocks")
