"""conv_wino8_kernel -- the four-slot V ring and the paired epilogue -- against the float64 reference of tests/_conv_ref.py
under that file's Winograd rule (bit equality on `grid` where the epilogue is exact arithmetic, the limit rule on `real`).

The planner gives the eight-wave kernel to launches of 150 workgroups and more (test_winograd_eight_wave_kernel reaches
them with 12 members on a 104 x 16 strip).  The shapes that can go wrong in the ring are small -- 1, 2, 3, 4, 5 and 9
steps of 16 channels: fewer than, equal to and not a multiple of the ring depth -- so a fresh child process per co-block
width runs them under ICM_WINO_TCO = 2 / 3 / 4, which the library reads once, and asserts that the plan is the eight-wave
kernel with that width.  Every operand sits in its own allocation between NaN guards (test_gpu_conv_numerics.Member).

  steps      Cin in {8, 24, 40, 56, 72, 136} on a 6 x 10 map, N = 1, Cout = 80 (a ragged last tile under every width)
  widths     Cout in {64, 80, 96, 128} on a 16 x 16 map, N = 3 (two pixel blocks, a batch tail in the tile index)
  epilogue   every EpiWino kind, accum, a null bias, y2 separate and in place on 6 x 10 (even W: 8-byte accesses) and on
             7 x 7 (odd W, odd planes: the scalar form); 6 x 10 again with batch strides off the natural ones
  group      two members in one launch
  twice      two identical calls agree bit for bit"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

CHILD = r"""
import sys
sys.path[:0] = %r
import torch
import test_gpu_conv_numerics as T
import _conv_ref as R
tco = int(sys.argv[1])
W = dict(algo=R.WINOGRAD, xv=True)
G = lambda N, H, Wd, Cin, Cout: R.geom(N, H, Wd, 3, 1, 1, ch=(Cin, Cout))
cases = []
for Cin in (8, 24, 40, 56, 72, 136):
    cases += T.both("steps-cin%%d" %% Cin, G(1, 6, 10, Cin, 80), **W)
for Cout in (64, 80, 96, 128):
    cases += T.both("width-cout%%d" %% Cout, G(3, 16, 16, 40, Cout), **W)
KINDS = [("none-y2", dict(epi=R.E_NONE, y2="sep")), ("res", dict(epi=R.E_RES)), ("res-y2same", dict(epi=R.E_RES, y2="same")),
         ("res_gelu-y2", dict(epi=R.E_RES_GELU, y2="sep")), ("mul_dgelu", dict(epi=R.E_MUL_DGELU)), ("lrp-y2", dict(epi=R.E_LRP, y2="sep")),
         ("lrp", dict(epi=R.E_LRP)), ("res_mul_dgelu", dict(epi=R.E_RES_MUL_DGELU)), ("accum-nobias", dict(accum=1, bias=False)),
         ("accum-res_gelu-y2same", dict(epi=R.E_RES_GELU, y2="same", accum=1)), ("accum-lrp-y2", dict(epi=R.E_LRP, y2="sep", accum=1))]
assert {kw.get("epi", R.E_NONE) for _, kw in KINDS} == set(R.EPI_WINO)
for name, kw in KINDS:
    cases += T.both("even-" + name, G(1, 6, 10, 24, 80), **W, **kw)
    cases += T.both("odd-" + name, G(3, 7, 7, 24, 80), **W, **kw)
OFF = {"y": "odd", "res": "slice", "aux": "odd", "y2": "slice"}     # batch strides off the natural ones, pairs still aligned
cases += T.both("strides-res-y2", G(3, 6, 10, 24, 80), epi=R.E_RES, y2="sep", strides=OFF, **W)
cases += T.both("strides-lrp-y2", G(3, 6, 10, 24, 80), epi=R.E_LRP, y2="sep", strides=OFF, **W)
for c in cases:
    p = R.plan(c)
    assert p.family == R.WINO8 and p.row == tco and p.ckm == R.cdiv(R.cdiv(c["g"].Cin, 8), 2), (c["id"], p)
    T.run_single(c)
for which in ("grid", "real"):
    cs = [R.case("group-%%s-m%%d" %% (which, i), G(3, 16, 16, 72, 96), inputs=which, member=i, ngroups=2, epi=R.E_RES, y2="sep", **W)
          for i in range(2)]
    assert R.plan(cs[0], 2).family == R.WINO8
    T.run_group(cs, "group of 2")
for c in (R.case("twice", G(3, 16, 16, 136, 128), inputs="real", epi=R.E_RES_GELU, y2="sep", **W),
          R.case("twice-odd", G(3, 7, 7, 56, 80), inputs="real", **W)):
    m = T.Member(c)
    assert T.transform([m]) == R.OK
    outs = []
    for _ in range(2):
        assert T.launch([m]) == R.OK
        outs.append((m.y.now(), m.y2.now() if m.y2 is not None else None))
    assert T.same_bits(outs[0][0], outs[1][0]) and (outs[0][1] is None or T.same_bits(outs[0][1], outs[1][1])), c["id"]
print("child ok", tco, len(cases))
"""


@pytest.mark.parametrize("tco", (2, 3, 4))
def test_ring_and_paired_epilogue(tco):
    env = dict(os.environ, ICM_WINO_TCO=str(tco))
    r = subprocess.run([sys.executable, "-c", CHILD % (sys.path,), str(tco)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok %d" % tco in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
