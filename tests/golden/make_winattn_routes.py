"""Emit tests/golden/winattn_routes.npz: which kernel family csrc/winattn.hip sends a window-attention call to, and
how much backward workspace it asks for, row by row.

Run against a library whose dispatch is the one to pin (the fixture was written from the dispatch as it stood before
its family table existed: three descriptors, three plan functions, nine functions between the two translation units);
tests/test_winattn_ref.py replays every row against the built library.  Pure host code: no GPU needed.

  args  [rows, 8] int32: force (icm_debug_force_winattn_valu), then N, C, H, W, heads, ws, shift
  route [rows, 2] int32: icm_debug_winattn_route forward, backward (0 VALU, 1 matrix cores 8x8, 2 matrix cores 4x4,
                         negative: the ICM_ERR_* code the call returns without launching)
  wsf   [rows]    int64: icm_winattn_bwd_workspace_floats

Usage: python tests/golden/make_winattn_routes.py"""
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
for p in (ROOT, os.path.join(ROOT, "image-compression-for-machine_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from icm_amd import _lib  # noqa: E402

ROUTE_VALU, ROUTE_MFMA, ROUTE_MFMA16 = 0, 1, 2
ERR_ARG, ERR_UNSUPPORTED = 1, 3
HEAD_DIMS = (4, 8, 10, 12, 16, 24, 32, 40, 48, 56, 64)   # every entry of the three head-dim tables, and some of none
HEADS = (1, 2, 4, 5, 8)


def record(L, row):
    """[route forward, route backward], workspace floats of one row"""
    force, N, C, H, W, heads, ws, shift = (int(v) for v in row)
    L.icm_debug_force_winattn_valu(force)
    try:
        route = [L.icm_debug_winattn_route(N, C, H, W, heads, ws, shift, b) for b in (0, 1)]
    finally:
        L.icm_debug_force_winattn_valu(0)
    return route, L.icm_winattn_bwd_workspace_floats(N, C, H, W, heads, ws)


def rows():
    out = []
    for ws in range(1, 10):
        # two maps per window size: 64 windows, a multiple of 4 * ws wide; 15 windows, five per row (a ragged group
        # of four for the 4x4 family, fewer than 16 slabs for the reduction plan)
        maps = ((2, 4 * ws, 8 * ws), (1, 3 * ws, 5 * ws))
        shifts = sorted({0, ws // 2, ws})                   # ws itself: refused as an argument error
        for (N, H, W), hd, heads, shift, force in itertools.product(maps, HEAD_DIMS, HEADS, shifts, (0, 1)):
            out.append((force, N, heads * hd, H, W, heads, ws, shift))
    # the cases of the numerics suite (reduction plans up to the capped S = 64 among them), under both hook settings
    import _winattn_ref as R
    for case, force in itertools.product(R.MATRIX + [R.LDS_CASE] + R.REDUCTION, (0, 1)):
        out.append((force,) + tuple(R.geometry(case)))
    # argument errors other than the shift: a map no multiple of the window, channels no multiple of the heads
    for force in (0, 1):
        out += [(force, 1, 8, 6, 4, 1, 4, 0), (force, 1, 8, 4, 6, 1, 4, 0), (force, 1, 10, 4, 4, 3, 4, 0),
                (force, 0, 8, 4, 4, 1, 4, 0), (force, 1, 8, 4, 4, 0, 4, 0)]
    return out


def main():
    L = _lib.lib()
    args = np.asarray(rows(), dtype=np.int32)
    rec = [record(L, r) for r in args]
    route = np.asarray([r for r, _ in rec], dtype=np.int32)
    wsf = np.asarray([w for _, w in rec], dtype=np.int64)
    # coverage (conditions on the pinned dispatch, checked before anything is written)
    for b in (0, 1):
        assert {ROUTE_VALU, ROUTE_MFMA, ROUTE_MFMA16, -ERR_ARG, -ERR_UNSUPPORTED} <= set(route[:, b].tolist()), b
    ok = (route >= 0).all(axis=1)
    split = args[ok & (route[:, 0] != route[:, 1])]
    assert any(r[0] == 0 and r[6] == 8 and r[2] // r[5] == 48 for r in split), "no row like head dim 48 at 8x8"
    lds = (args[:, 0] == 1) & (args[:, 6] == 8) & (args[:, 5] == 5) & (args[:, 2] == 5 * 48) & (args[:, 7] < 8)
    assert lds.any() and (route[lds, 0] == -ERR_UNSUPPORTED).all() and (route[lds, 1] == ROUTE_VALU).all(), \
        "no forced row refused for its LDS request"
    forced = args[:, 0] == 1
    assert not np.isin(route[forced], (ROUTE_MFMA, ROUTE_MFMA16)).any()
    assert (wsf > 0).sum() > len(wsf) // 2 and (wsf == -1).any()
    np.savez_compressed(os.path.join(HERE, "winattn_routes.npz"), args=args, route=route, wsf=wsf)
    print(f"wrote winattn_routes.npz: {len(args)} rows; forward routes {sorted(set(route[:, 0].tolist()))}, backward "
          f"{sorted(set(route[:, 1].tolist()))}; {len(split)} rows with differing directions; "
          f"workspace up to {wsf.max()} floats")


if __name__ == "__main__":
    main()
