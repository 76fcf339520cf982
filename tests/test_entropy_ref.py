"""What tests/test_gpu_entropy_numerics.py relies on, checked without a GPU for every input set it uses: float32 and
float64 take the same rounding decisions, few elements are grey, every likelihood band and the floor are populated, and
the float32 oracle (the yardstick the GPU limits are formed from) is itself close to float64.  Prints the shares and the
oracle's per-band errors (pytest -s)."""
import math

import pytest
import torch

import _entropy_ref as R

GREY_MAX, SHARE_MIN, ORACLE_BITS_MAX = 0.05, 0.02, 1e-3


def _check(name, r, lik32):
    live, floor, grey = R.classify(r)
    shares = [R.share(m) for m in R.bands(r)]
    errs = R.band_bits(lik32, r)
    print(f"{name}: n {r.numel()} grey {R.share(grey):.4f} floor {R.share(floor):.4f} bands "
          + " ".join(f"{s:.4f}" for s in shares) + " | float32 oracle bits " + " ".join(f"{e:.3e}" for e in errs))
    assert R.share(grey) <= GREY_MAX, (name, R.share(grey))
    assert R.share(floor) >= SHARE_MIN, (name, R.share(floor))
    for s, e, b in zip(shares, errs, R.BAND_NAMES):
        assert s >= SHARE_MIN, (name, b, s)
        assert math.isfinite(e) and e < ORACLE_BITS_MAX, (name, b, e)
    # on the floor the float32 oracle sits on the bound itself
    assert (lik32[floor] == torch.tensor(1e-9, dtype=torch.float32)).all()


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", [R.GC_SHAPE, R.GC_LONG_SHAPE], ids=["strided", "long"])
def test_gaussian_inputs(shape, mode):
    inp = R.gaussian_inputs(shape)
    assert R.gaussian_round_flips(inp) == 0
    r = R.gaussian_raw(inp, mode)
    _check(f"gaussian {tuple(shape)} {mode}", r, R.gaussian_oracle(inp, mode, torch.float32))
    below, above, grey = R.scale_classes(inp["scale"])
    assert int(grey.sum()) == 3 and R.share(below) >= 0.005 and R.share(above) >= 0.9


def test_gaussian_inputs_keep_the_corner_values():
    sc = R.gaussian_inputs()["scale"].reshape(-1)
    table = R.O.scale_table()
    assert sc[:7].tolist() == pytest.approx([0.11, R.SCALE_BELOW, R.SCALE_ABOVE, 0.0, -1.0, 1e-3, 300.0], rel=1e-7)
    assert sc[0].item() != sc[1].item() != sc[2].item() and sc[6] > 256
    ratio = sc[64:128] / table          # one full walk of the table
    assert (ratio >= 0.8 - 1e-6).all() and (ratio <= 1.25 + 1e-6).all()


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", R.EB_SHAPES, ids=[f"L{n * hw}" for n, _, hw in R.EB_SHAPES])
def test_bottleneck_inputs(shape, mode):
    inp, sd = R.eb_inputs(shape), R.eb_params(shape[1])
    assert R.eb_round_flips(inp, sd) == 0
    r = R.eb_raw(inp, sd, mode)
    _check(f"bottleneck {tuple(shape)} {mode}", r, R.eb_oracle(inp, sd, mode, torch.float32))


def test_raw_likelihoods_restate_the_oracle():
    """the un-bounded float64 likelihoods used for the classification are the oracle's, where the bound is inactive"""
    inp = R.gaussian_inputs()
    for mode in R.MODES:
        r, lik = R.gaussian_raw(inp, mode), R.gaussian_oracle(inp, mode, torch.float64)
        assert torch.equal(torch.clamp(r, min=1e-9), lik)
    shape = R.EB_SHAPES[2]
    inp, sd = R.eb_inputs(shape), R.eb_params(shape[1])
    for mode in R.MODES:
        r, lik = R.eb_raw(inp, sd, mode), R.eb_oracle(inp, sd, mode, torch.float64)
        assert torch.equal(torch.clamp(r, min=1e-9), lik)


def test_seeds():
    r = R.gaussian_raw(R.gaussian_inputs(), "train")
    live, floor, grey = R.classify(r)
    g = R.seed(r, "bits", "t")
    assert torch.equal(g[~live], torch.full_like(g[~live], -1.0)) and (g[live] < 0).all()
    assert torch.allclose(g[live].double() * r[live] * R.LN2, torch.full_like(r[live], -1.0), rtol=1e-6)
    m = R.seed(r, "mixed", "t", zero_grey=True)
    assert (m[grey] == 0).all() and (m[floor] > 0).any() and (m[floor] < 0).any() and m.abs().max() <= 1
