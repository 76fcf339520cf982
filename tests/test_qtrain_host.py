"""Host side of variable-rate training, no GPU: the training CLI's two flags and their refusals, the step and weight
tables a step gathers from, how ``forward(x, qstep=...)`` reads its argument, and the checkpoint key."""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "image-compression-for-machine_amd"))
import _qstep_ref as Q  # noqa: E402


def parse(*argv):
    from icm_amd import train
    return train.parse_args(["-d", "data", *argv])


def test_cli_flags():
    a = parse()
    assert a.qstep_range is None and a.qstep_lambda_exp == 2.0
    assert parse("--qstep-range", "0,16").qstep_range == (0, 16)
    assert parse("--qstep-range", "-8,16").qstep_range == (-8, 16)          # a negative LO, in either spelling
    assert parse("--qstep-range=-16,32").qstep_range == (-16, 32)
    assert parse("--qstep-range", " 4 , 4 ").qstep_range == (4, 4)
    assert parse("--qstep-range", "-16,-2", "--qstep-lambda-exp", "1.5").qstep_lambda_exp == 1.5
    assert parse("-m", "stf", "--qstep-range", "0,8").model == "stf"


@pytest.mark.parametrize("argv", [
    ("--qstep-range", "16,-8"), ("--qstep-range", "-17,0"), ("--qstep-range", "0,33"), ("--qstep-range", "4"),
    ("--qstep-range", "1,2,3"), ("--qstep-range", "a,b"), ("--qstep-range", "0.5,2"), ("--qstep-range", ""),
    ("--qstep-range", "0,8", "--metric", "ms-ssim"), ("--qstep-range", "0,8", "-m", "stf6"),
    ("--qstep-lambda-exp", "two")])
def test_cli_refusals_exit_2(argv, capsys):
    with pytest.raises(SystemExit) as e:
        parse(*argv)
    assert e.value.code == 2
    assert "qstep" in capsys.readouterr().err


def test_range_check():
    from icm_amd.trainer import check_qstep_range
    assert check_qstep_range((-16, 32)) == (-16, 32) and check_qstep_range([3, 3]) == (3, 3)
    assert check_qstep_range((np.int64(-2), np.int32(5))) == (-2, 5)
    for bad in ((5, 3), (-17, 0), (0, 33), (1,), (1, 2, 3), (1.0, 2), (True, 2), None, 7, "1,2"):
        with pytest.raises(ValueError):
            check_qstep_range(bad)


@pytest.mark.parametrize("exp", [2.0, 1.0, 0.0, 2.5])
@pytest.mark.parametrize("lmbda", [0.0067, 0.05])
def test_tables_against_float64(lmbda, exp):
    from icm_amd.bitstream import step_of
    from icm_amd.trainer import qstep_tables
    lo, hi = -16, 32
    steps, lam = qstep_tables((lo, hi), lmbda, exp)
    assert steps.dtype == torch.float32 and tuple(steps.shape) == (49, 2)
    assert lam.dtype == torch.float32 and tuple(lam.shape) == (49,)
    for i, k in enumerate(range(lo, hi + 1)):
        # the pairs are the codec's own, bit for bit (bitstream.step_of, restated in tests/_qstep_ref.py)
        assert (steps[i, 0].item(), steps[i, 1].item()) == step_of(k) == tuple(float(v) for v in Q.step_of(k))
        want = np.float64(lmbda) * np.float64(2.0) ** (-np.float64(k) * np.float64(exp) / 8.0)
        assert lam[i].item() == float(np.float32(want)), (k, lam[i].item(), want)       # float64, rounded once
        # ... which is lmbda * step^-exp up to the rounding of the step itself
        assert lam[i].item() == pytest.approx(lmbda * float(steps[i, 0]) ** -exp, rel=1e-6)
    assert lam[16].item() == float(np.float32(lmbda))                                    # k = 0: the scalar lmbda
    if exp > 0:
        assert (lam[1:] < lam[:-1]).all()                                                # a larger step, a smaller weight
    sub = qstep_tables((5, 7), lmbda, exp)
    assert torch.equal(sub[0], steps[21:24]) and torch.equal(sub[1], lam[21:24])


def test_forward_argument():
    from icm_amd.engine import qstep_indexes, qstep_per_image, qstep_steps
    assert qstep_indexes([-16, 0, 32], 3) == [-16, 0, 32] and qstep_indexes(5, 2) == [5, 5] and qstep_indexes(0, 2) is None
    assert qstep_indexes(torch.zeros(2, dtype=torch.int32), 2) == [0, 0]
    assert [qstep_per_image(q) for q in (None, 4, [4, 4], (4,), torch.tensor([4]))] == [False, False, True, True, True]
    for none in (None, 0, [0, 0, 0], (0, 0, 0), np.int64(0)):
        assert qstep_steps(none, 3, "cpu") is None
    s = qstep_steps(5, 3, "cpu")
    assert s.dtype == torch.float32 and tuple(s.shape) == (3, 2) and s.is_contiguous()
    assert torch.equal(s, torch.tensor([[float(v) for v in Q.step_of(5)]] * 3))
    s = qstep_steps([-16, 0, 32], 3, "cpu")
    assert torch.equal(s, torch.tensor([[float(v) for v in Q.step_of(k)] for k in (-16, 0, 32)]))
    assert torch.equal(qstep_steps(torch.tensor([-16, 0, 32]), 3, "cpu"), s)
    assert torch.equal(qstep_steps(torch.zeros(3, dtype=torch.int64), 3, "cpu"), torch.ones(3, 2))   # a tensor is never "no step"
    for bad in (33, -17, 2.0, True, "4", [1, 2], [1, 2, 3, 4], [1, 2.5, 3], torch.tensor([1.0, 2.0, 3.0]),
                torch.zeros(3, 1, dtype=torch.int64), torch.tensor([True, False, True])):
        with pytest.raises(ValueError):
            qstep_steps(bad, 3, "cpu")


def test_checkpoint_records_the_range(tmp_path):
    from icm_amd import train
    sd = {"w": torch.arange(4.0)}
    ck = train.checkpoint_state(3, sd, 1.25, {"m": {}}, {"m": {}}, {"best": 1.0}, (-8, 16), 1.5)
    assert ck["qstep_range"] == [-8, 16] and ck["qstep_lambda_exp"] == 1.5 and ck["epoch"] == 3 and ck["loss"] == 1.25
    assert set(ck) == {"epoch", "state_dict", "loss", "optimizer", "aux_optimizer", "lr_scheduler", "qstep_range",
                       "qstep_lambda_exp"}
    plain = train.checkpoint_state(0, sd, 2.0, {}, {}, {})
    assert plain["qstep_range"] is None
    # both load the way the CLI and the evaluation tool read checkpoints, and so does one from before the key
    for i, c in enumerate((ck, plain, {k: v for k, v in plain.items() if not k.startswith("qstep")})):
        path = tmp_path / f"{i}.ckpt"
        train.save_checkpoint(c, str(path))
        back = torch.load(str(path), map_location="cpu", weights_only=True)
        assert back.get("qstep_range") == c.get("qstep_range") and torch.equal(back["state_dict"]["w"], sd["w"])


def test_report_points():
    from icm_amd.train import qstep_test_points
    assert qstep_test_points((-8, 16)) == [-8, 0, 16]
    assert qstep_test_points((0, 16)) == [0, 16] and qstep_test_points((-8, 0)) == [-8, 0]
    assert qstep_test_points((4, 12)) == [4, 12] and qstep_test_points((5, 5)) == [5]


def test_loss_refuses_weights_it_cannot_take():
    from icm_amd.losses import RateDistortionLoss, _weights
    x = torch.zeros(2, 3, 8, 8)
    assert _weights([0.5, 0.25], x).tolist() == [0.5, 0.25]
    for bad in ([0.5], [[0.5, 0.25]], 0.5):
        with pytest.raises(ValueError):
            _weights(bad, x)
    with pytest.raises(ValueError):
        RateDistortionLoss(0.01, metric="ms-ssim")({"likelihoods": {}}, x, lmbda_n=[0.5, 0.25])
