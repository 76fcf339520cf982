"""conv_wino8_kernel -- weight fragments as uncounted loads, hand-counted waits in the step loop -- against the float64
reference of tests/_conv_ref.py under that file's Winograd rule (bit equality on `grid`, the limit rule on `real`).

A wait counted one unit short, or the count of a step with DMAs used in a tail step without them, returns while the
fragment is still in flight: nothing faults, the values are wrong and may differ from call to call.  The shapes where that
shows are small, so a fresh child process per co-block width runs them under ICM_WINO_TCO = 2 / 3 / 4 (read once by the
library) and asserts that the plan is the eight-wave kernel of that width.  Every operand sits in its own allocation
between NaN guards (test_gpu_conv_numerics.Member).

  steps      Cin in {8, 24, ..., 136}: 1 to 9 steps of 16 channels, every count around the ring depth and the tail without
             DMAs; forward and input gradient on a 6 x 10 map, N = 1, Cout = 80 (a ragged last co tile under every width:
             the weight clamp); 7 x 7, N = 3 (odd planes) at 3 and 5 steps
  blocks     16 x 16, N = 3, Cin 72 -> Cout 96, two members in one launch, residual epilogue and a separate y2
  order      8 identical launches of a 9-step case and of the grouped case agree bit for bit"""
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
G = lambda N, H, Wd, Cin, Cout, tr=0: R.geom(N, H, Wd, 3, 1, 1, tr, ch=(Cin, Cout), HW=(H, Wd))
cases = []
for tr, name in ((0, "fwd"), (1, "dgrad")):     # forward (gather) and input gradient (scatter, the taps flipped)
    for steps in range(1, 10):
        cases += T.both("%%s-steps-%%d" %% (name, steps), G(1, 6, 10, 16 * steps - 8, 80, tr), **W)
    for steps in (3, 5):
        cases += T.both("%%s-odd-steps-%%d" %% (name, steps), G(3, 7, 7, 16 * steps - 8, 80, tr), **W)
for c in cases:
    p = R.plan(c)
    assert p.family == R.WINO8 and p.row == tco and p.ckm == R.cdiv(R.cdiv(c["g"].Cin, 8), 2), (c["id"], p)
    T.run_single(c)
GROUP = lambda which: [R.case("group-%%s-m%%d" %% (which, i), G(3, 16, 16, 72, 96), inputs=which, member=i, ngroups=2,
                              epi=R.E_RES, y2="sep", **W) for i in range(2)]
for which in ("grid", "real"):
    cs = GROUP(which)
    p = R.plan(cs[0], 2)
    assert p.family == R.WINO8 and p.row == tco, p
    T.run_group(cs, "group of 2")
nine = R.case("repeat-9-steps", G(1, 6, 10, 136, 80), inputs="real", **W)
assert R.plan(nine).family == R.WINO8 and R.plan(nine).row == tco and R.plan(nine).ckm == 9
for ms in ([T.Member(nine)], [T.Member(c) for c in GROUP("real")]):
    assert T.transform(ms) == R.OK
    outs = []
    for _ in range(8):
        assert T.launch(ms) == R.OK
        outs.append([(m.y.now(), m.y2.now() if m.y2 is not None else None) for m in ms])
    for o in outs[1:]:
        for (y0, s0), (y, s) in zip(outs[0], o):
            assert T.same_bits(y0, y) and (s0 is None or T.same_bits(s0, s)), ms[0].c["id"]
print("child ok", tco, len(cases))
"""


@pytest.mark.parametrize("tco", (2, 3, 4))
def test_counted_waits_and_tail(tco):
    env = dict(os.environ, ICM_WINO_TCO=str(tco))
    r = subprocess.run([sys.executable, "-c", CHILD % (sys.path,), str(tco)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok %d" % tco in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
