"""CPU: what the AQ-map GPU tests rely on, and the host side of ``--qmap-aq`` / ``eval_model --aq``.  No cell of a GPU
case lies inside the zone where device and reference may round differently (so the GPU file compares every cell
exactly); every case reaches what it is named for; the 8-bit rule returns all 256 values; the host definition in
``icm_amd.codec`` gives the reference's maps; ``check_qmap_aq``, the training CLI, the checkpoint and ``eval_model``
accept and refuse as specified."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "image-compression-for-machine_amd"))
import _qmap_aq_inputs as I  # noqa: E402


@pytest.mark.parametrize("name", sorted(I.CASES))
def test_no_cell_of_a_gpu_case_lies_in_the_zone(name):
    r = I.reference(name)
    d = I.zone_distance(r["value"])
    print(f"{name}: {d.size} cells, smallest distance to a half-integer {d.min():.3e}")
    assert (d > I.ZONE).all()          # the share of cells a case may leave out is zero
    assert d.min() > 1e-6              # and by a margin that no change of the last bits can use up
    x, u8, strength, base, rects = I.case(name)
    assert r["map"].shape == (x.shape[0], x.shape[2] // 16, x.shape[3] // 16) and r["map"].dtype == np.int8
    assert r["map"].min() >= -16 and r["map"].max() <= 32


@pytest.mark.parametrize("name", sorted(I.CASES))
def test_every_case_reaches_what_it_is_named_for(name):
    want = I.CASES[name][6]
    assert want <= I.reached(name), (want, I.reached(name))


def test_the_cases_cover_the_contract_between_them():
    need = {"saturated", "clamp_lo", "clamp_hi", "flat", "rect_wins"}
    assert need <= set().union(*(c[6] for c in I.CASES.values()))
    strengths = [s for c in I.CASES.values() for s in c[3]]
    bases = [b for c in I.CASES.values() for b in c[4]]
    assert 0.0 in strengths and 4.0 in strengths and -4.0 in strengths and min(strengths) < 0
    assert -16 in bases and 32 in bases
    assert any(c[5] is None for c in I.CASES.values())
    assert {c[1] for c in I.CASES.values()} == {(3, 48, 80), (2, 64, 64), (2, 128, 192)}
    for name, c in I.CASES.items():
        assert len(set(c[3])) == len(c[3]) and len(set(c[4])) == len(c[4]), name       # they differ per image
        if c[5] is not None:                   # image 0: an empty rectangle and one the map's edge clips
            h, w = c[1][1] // 16, c[1][2] // 16
            (y0, x0, y1, x1, _), (cy0, cx0, cy1, cx1, _) = c[5][0].tolist()
            assert y1 <= y0 or x1 <= x0
            assert cy0 < h and cx0 < w and (cy1 > h or cx1 > w)
    x = I.case("floats-48x80")[0]
    assert (x < 0).mean() > 0.02 and (x > 1).mean() > 0.02


def test_the_8_bit_rule_returns_all_256_values():
    k = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1).repeat(3, axis=3)
    assert np.array_equal(I.to_u8(I.planar(k)), k)
    odd = np.array([-1.0, -0.0, 0.0, 0.999999, 1.0, 1.5, 254.9999 / 255, 0.5], dtype=np.float32).reshape(1, 1, 1, 8)
    odd = np.ascontiguousarray(np.broadcast_to(odd, (1, 3, 1, 8)))
    assert I.to_u8(odd)[0, 0, :, 0].tolist() == [0, 0, 0, 254, 255, 255, 254, 127]


@pytest.mark.parametrize("name", sorted(I.CASES))
def test_the_host_definition_gives_the_references_maps(name):
    """icm_amd/codec.py (aq_reference, aq_offsets, quality_map) on the reference's integer statistics: the maps of
    tests/_aq_ref.py, the mean within the limit the GPU file holds the device to"""
    from icm_amd import codec
    import _aq_ref as A
    _, u8, strength, base, _ = I.case(name)
    r = I.reference(name)
    for n in range(len(u8)):
        stats = A.stats_of(u8[n], (0, 0, 0, 0))
        ref = codec.aq_reference(stats)
        assert abs(ref - r["ref"][n]) <= I.REF_LIMIT
        offs = codec.aq_offsets(stats, float(strength[n]), ref)
        H, W = u8[n].shape[:2]
        I.check_maps(codec.quality_map(H, W, (0, 0, 0, 0), int(base[n]), [], offs), r["aq"][n], r["value"][n], name)


def test_check_qmap_aq():
    from icm_amd.trainer import check_qmap_aq
    from icm_amd.codec import AQ_STRENGTH_MAX
    assert AQ_STRENGTH_MAX == 4.0
    assert check_qmap_aq(None) is None and check_qmap_aq((0, 0)) is None and check_qmap_aq([0.0, -0.0]) is None
    assert check_qmap_aq((-4, 4)) == (-4.0, 4.0) and check_qmap_aq((1.5, 1.5)) == (1.5, 1.5)
    assert check_qmap_aq([0, 2]) == (0.0, 2.0) and check_qmap_aq((np.float32(-1), np.int64(0))) == (-1.0, 0.0)
    got = check_qmap_aq((-2.5, 1))
    assert got == (-2.5, 1.0) and all(type(v) is float for v in got)
    for bad in ((1, 0), (-4.01, 0), (0, 4.5), (float("nan"), 1), (0, float("inf")), (True, 1), ("1", 2), (1,), (1, 2, 3), 2.0,
                "1,2", (None, 1)):
        with pytest.raises(ValueError):
            check_qmap_aq(bad)


def test_the_trainer_refuses_before_it_touches_a_device():
    from icm_amd.trainer import Trainer
    from icm_amd.zoo import models
    net = models["cnn"]()
    with pytest.raises(ValueError, match="qmap_aq: quality-map training draws its step indexes from qstep_range"):
        Trainer(net, device="cpu", qmap_aq=(0, 1))
    with pytest.raises(ValueError, match="qmap_aq: the MS-SSIM loss takes a scalar lmbda"):
        Trainer(net, device="cpu", metric="ms-ssim", qstep_range=(-8, 16), qmap_aq=(0, 1))
    with pytest.raises(ValueError, match="qmap_aq: stf6 has no codec"):
        Trainer(models["stf6"](), device="cpu", qstep_range=(-8, 16), qmap_aq=(0, 1))
    with pytest.raises(ValueError, match="qmap_aq"):
        Trainer(net, device="cpu", qstep_range=(-8, 16), qmap_aq=(2, 1))


def test_train_arguments():
    from icm_amd import train as TR
    a = TR.parse_args(["-d", "x", "--qstep-range", "-8,16", "--qmap-aq", "-2.5,1"])
    assert a.qmap_aq == (-2.5, 1.0) and a.qmap_aq_given and a.qstep_range == (-8, 16) and a.qmap_rects is None
    a = TR.parse_args(["-d", "x", "--qstep-range=-8,16", "--qmap-aq=0.5,4", "--qmap-rects", "2", "-m", "stf"])
    assert a.qmap_aq == (0.5, 4.0) and a.qmap_rects == 2
    a = TR.parse_args(["-d", "x", "--qstep-range", "-8,16", "--qmap-aq", "0,0"])
    assert a.qmap_aq is None and a.qmap_aq_given                    # off, said so: a resumed run's maps are dropped
    a = TR.parse_args(["-d", "x", "--qstep-range", "-8,16"])
    assert a.qmap_aq is None and not a.qmap_aq_given
    for bad in (["--qmap-aq", "0,1"],                                                    # no --qstep-range
                ["--qstep-range", "-8,16", "--qmap-aq", "0,1", "--metric", "ms-ssim"],
                ["--qstep-range", "-8,16", "--qmap-aq", "0,1", "-m", "stf6"],
                ["--qstep-range", "-8,16", "--qmap-aq", "1,0"], ["--qstep-range", "-8,16", "--qmap-aq", "0,5"],
                ["--qstep-range", "-8,16", "--qmap-aq", "1"], ["--qstep-range", "-8,16", "--qmap-aq", "a,b"],
                ["--qstep-range", "-8,16", "--qmap-aq", "nan,1"]):
        with pytest.raises(SystemExit):
            TR.parse_args(["-d", "x"] + bad)
    assert TR.parse_qmap_aq("0, 2") == (0.0, 2.0) and TR.parse_qmap_aq("0,0") is None
    # the test loop's line: the background of the "0" line (LO when 0 is outside), the strength larger in magnitude
    assert TR.aq_test_point((-8, 16), (-1.0, 2.0)) == (0, 2.0)
    assert TR.aq_test_point((-8, 16), (-3.0, 2.0)) == (0, -3.0)
    assert TR.aq_test_point((4, 16), (0.0, 1.0)) == (4, 1.0)
    assert TR.aq_test_point((0, 16), (1.0, 1.0)) == (0, 1.0)
    assert TR.aq_test_point((-8, 0), (-1.0, 1.0)) == (-8, 1.0)


def test_the_checkpoint_carries_qmap_aq():
    from icm_amd import train as TR
    from icm_amd.trainer import check_qmap_aq
    ck = TR.checkpoint_state(3, {}, 1.0, {}, {}, {}, (-8, 16), 2.0, 1, (-2.5, 1.0))
    assert ck["qmap_aq"] == [-2.5, 1.0] and ck["qmap_rects"] == 1 and ck["qstep_range"] == [-8, 16]
    assert check_qmap_aq(ck["qmap_aq"]) == (-2.5, 1.0)
    assert "qmap_aq" not in TR.checkpoint_state(3, {}, 1.0, {}, {}, {}, (-8, 16), 2.0, 1)
    assert "qmap_aq" not in TR.checkpoint_state(3, {}, 1.0, {}, {}, {})
    assert check_qmap_aq({}.get("qmap_aq")) is None                 # a checkpoint without the key: off


def test_eval_model_refusals_need_no_device():
    from icm_amd import eval_model as EM
    from icm_amd import utils
    m = np.zeros((4, 4), dtype=np.int8)
    with pytest.raises(ValueError, match="aq or qmap"):
        EM.eval_model(None, ["a.png"], entropy_estimation=True, aq=1.0, qmap=m)
    with pytest.raises(ValueError, match="aq or qmap"):
        EM.eval_model(None, ["a.png"], aq=1.0, qmap=m)
    with pytest.raises(ValueError, match="qmap is for the entropy estimation"):          # as before
        EM.eval_model(None, ["a.png"], qmap=m)
    for bad in (4.5, float("nan"), True, "1"):
        with pytest.raises(ValueError):
            EM.eval_model(None, ["a.png"], aq=bad)
    with pytest.raises(ValueError):
        EM.eval_model(None, ["a.png"], aq=1.0, qstep=33)
    import torch
    with pytest.raises(ValueError, match="qstep and qmap"):
        utils.inference(None, torch.zeros(3, 64, 64), qstep=4, qmap=m)
    a = EM.setup_args().parse_args(["-d", "x", "--aq", "-2.5", "--qstep", "4"])
    assert a.aq == -2.5 and a.qstep == 4
    assert EM.setup_args().parse_args(["-d", "x"]).aq is None
