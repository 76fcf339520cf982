"""Emit tests/golden/wgrad_plans.npz: what the weight-gradient planner of csrc/conv_wgrad.hip decides, row by row.

Run against a library whose planner is the one to pin (the fixture was written from the planner as it stood before
its variant table existed, with only icm_debug_wgrad_plan added); tests/test_host_logic.py replays every row against
the built library and wants the same return code and the same eight plan values.  Pure host code: no GPU needed.

  args [rows, 15] int32: forced variant (-1 = automatic), n (problems per grouped launch), then the geometry
                         Ca, OH, OW, act_s, Cb, H, W, act_b, N, KH, KW, stride, pad
  plan [rows, 9]  int32: return code, then out[8] of icm_debug_wgrad_plan

Usage: python tests/golden/make_wgrad_plans.py"""
import ctypes
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
for p in (ROOT, os.path.join(ROOT, "image-compression-for-machine_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from icm_amd import _lib  # noqa: E402

GEOM_FIELDS = ("Ca", "OH", "OW", "act_s", "Cb", "H", "W", "act_b", "N", "KH", "KW", "stride", "pad")
ERR_UNSUPPORTED = 3   # ICM_ERR_UNSUPPORTED


def wgrad_args(geom):
    a = _lib.WgradArgs()
    a.gs, a.gb = 1, 1   # never dereferenced by the planner
    for f, v in zip(GEOM_FIELDS, geom):
        setattr(a, f, int(v))
    return a


def plan(L, forced, n, geom):
    """[return code, out[0..7]] of the planner for one row"""
    out = (ctypes.c_int32 * 8)()
    L.icm_debug_force_wgrad_cfg(int(forced), -1)
    try:
        rc = L.icm_debug_wgrad_plan(ctypes.byref(wgrad_args(geom)), int(n), out)
    finally:
        L.icm_debug_force_wgrad_cfg(-1, -1)
    return [rc] + list(out)


def rows():
    auto = []
    chans = (3, 32, 48, 96, 100, 192, 224, 320, 480)
    for (k, s, pad), ca, cb, (o, n_img), act_b, n in itertools.product(
            ((1, 1, 0), (3, 1, 1), (3, 2, 1), (5, 1, 2), (5, 2, 2), (2, 2, 0)), chans, chans,
            ((4, 4), (16, 16), (16, 2), (64, 16), (128, 8)), (_lib.ACT_NONE, _lib.ACT_GELU), (1, 6)):
        h = o * s
        assert o == (h + 2 * pad - k) // s + 1
        auto.append((-1, n, ca, o, o, 0, cb, h, h, act_b, n_img, k, k, s, pad))
    # the two geometries of test_host_planning_entry_points
    for n in (1, 6):
        auto.append((-1, n, 192, 64, 64, 0, 192, 128, 128, 0, 16, 5, 5, 2, 2))
        auto.append((-1, n, 1536, 16, 16, 0, 384, 16, 16, 0, 16, 1, 1, 1, 0))
    from test_gpu_ops import WG_CASES
    forced = []
    for _, N, cin, H, W, cout, k, s, tr, _ in WG_CASES:
        pad = k // 2
        if tr:    # transposed convolution: its input is the small grid, its output the big one
            geom = (cin, H, W, 0, cout, H * s, W * s, 0, N, k, k, s, pad)
        else:
            geom = (cout, (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1, 0, cin, H, W, 0, N, k, k, s, pad)
        forced += [(v, 1) + geom for v in range(15)]
    return auto, forced


def main():
    L = _lib.lib()
    auto, forced = rows()
    args = np.asarray(auto + forced, dtype=np.int32)
    res = np.asarray([plan(L, r[0], r[1], r[2:]) for r in args], dtype=np.int32)
    pa, pf = res[:len(auto)], res[len(auto):]
    # coverage (conditions on the pinned planner, checked before anything is written)
    reached = sorted(set(pa[pa[:, 0] == 0, 1].tolist()))
    assert {0, 1, 4, 5, 6, 7, 8, 10} <= set(reached) and len(set(reached) & {11, 12, 13, 14}) >= 2, reached
    assert set(pf[pf[:, 0] == 0, 1].tolist()) == set(range(15)), "a variant no forced row accepts"
    assert (pf[:, 0] == ERR_UNSUPPORTED).any(), "no forced row is refused"
    lgs = sorted(set(res[res[:, 0] == 0, 2].tolist()))
    assert {5, 6} <= set(lgs), lgs
    assert (res[res[:, 0] != 0, 1:] == 0).all()
    np.savez_compressed(os.path.join(HERE, "wgrad_plans.npz"), args=args, plan=res)
    print(f"wrote wgrad_plans.npz: {len(auto)} automatic + {len(forced)} forced rows; automatic rows reach variants "
          f"{reached}; lgNPX takes {lgs}; return codes {sorted(set(res[:, 0].tolist()))}")


if __name__ == "__main__":
    main()
