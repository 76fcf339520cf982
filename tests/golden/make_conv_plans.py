"""Emit tests/golden/conv_plans.npz: what the forward / input-gradient convolution planner (csrc/conv_igemm.hip,
conv_1x1.hip, conv_wino.hip) decides, row by row.

Run against a library whose planner is the one to pin (the fixture was written from the planner as it stood before the
plan step existed, with only icm_debug_conv_plan added); tests/test_host_logic.py replays every row against the built
library and wants the same return code and the same sixteen plan values.  Pure host code: no GPU needed.

  args [rows, 25] int32: ARG_FIELDS below (forced cfg, forced 1x1 mode, members per launch, tap class, the geometry,
                         operand activation, epilogue kind, channel map, algo, "xv given", "x aligned to 16 bytes")
  plan [rows, 17] int64: return code, then out[16] of icm_debug_conv_plan

Usage: python tests/golden/make_conv_plans.py"""
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

ARG_FIELDS = ("cfg", "mode1x1", "ngroups", "cls", "N", "Cin", "H", "W", "Cout", "OH", "OW", "KH", "KW", "stride", "pad",
              "transposed", "pro_act", "epi", "accum", "pixel_shuffle", "x_seg_len", "x_seg_gap", "algo", "xv", "aligned")
PLANNER_ENV = ("ICM_CONV_1X1", "ICM_CONV_BOOST", "ICM_CONV_KS8", "ICM_CONV_KS8_MAXWG", "ICM_CONV_KS8_MINWG",
               "ICM_CONV_DMA", "ICM_1X1_CFG", "ICM_1X1_MIN_WAVES", "ICM_1X1_SHORT_K", "ICM_WINO_TCO", "ICM_WINO8",
               "ICM_WINO8_MINWG", "ICM_WINO_PXFAST", "ICM_WINO_DEBUG")
OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 3
STAGED, KSPLIT, DIRECT1X1, WINO44, WINO8 = range(5)   # out[1]
NCFG = 13                                             # rows of the staged tile table
PTR = 4096                                            # the planner looks at null-ness and alignment only


def conv_args(row):
    """ConvArgs member of one row (every member of a grouped launch is the same geometry)"""
    r = dict(zip(ARG_FIELDS, (int(v) for v in row)))
    a = _lib.ConvArgs()
    for f in ("N", "Cin", "H", "W", "Cout", "OH", "OW", "KH", "KW", "stride", "pad", "transposed", "pro_act", "epi",
              "accum", "pixel_shuffle", "x_seg_len", "x_seg_gap", "algo"):
        setattr(a, f, r[f])
    planes = r["Cin"] + ((r["Cin"] - 1) // r["x_seg_len"]) * r["x_seg_gap"] if r["x_seg_len"] else r["Cin"]
    a.x, a.x_bs = PTR + (0 if r["aligned"] else 4), planes * r["H"] * r["W"]
    a.wp, a.y, a.y_bs = PTR, PTR, r["Cout"] * r["OH"] * r["OW"]
    a.res = a.aux = a.aux2 = PTR   # every epilogue kind finds its operands
    a.res_bs = a.aux_bs = a.aux2_bs = a.y_bs
    a.xv = PTR if r["xv"] else None
    return r, a


def plan(L, row):
    """[return code, out[0..15]] of the planner for one row"""
    r, a = conv_args(row)
    arr = (_lib.ConvArgs * r["ngroups"])(*[a] * r["ngroups"])
    out = (ctypes.c_int64 * 16)()
    L.icm_debug_force_conv_cfg(r["cfg"])
    L.icm_debug_force_conv1x1(r["mode1x1"])
    try:
        rc = L.icm_debug_conv_plan(arr, r["ngroups"], r["cls"], out)
    finally:
        L.icm_debug_force_conv_cfg(-1)
        L.icm_debug_force_conv1x1(-1)
    return [rc] + list(out)


def class_taps(K, stride, pad, transposed, cls):
    """taps of tap class `cls` (the packed size of a class is cdiv(Cin, 8) * taps * cdiv(Cout, 32) * 256 floats)"""
    if not transposed:
        return K * K
    per_axis = [sum(1 for k in range(K) if (c + pad - k) % stride == 0) for c in range(stride)]
    return per_axis[cls // stride] * per_axis[cls % stride]


KERNELS = ((1, 1, 0), (3, 1, 1), (3, 2, 1), (5, 1, 2), (5, 2, 2), (2, 2, 0))
CHANS = (3, 8, 20, 32, 48, 96, 100, 192, 224, 320, 480, 1536, 3360)
THIN = (8, 48, 100, 192, 320, 1536)
MAPS = ((4, 4, 4), (16, 16, 2), (16, 16, 16), (64, 64, 16), (128, 128, 8), (24, 40, 1))   # output-side H, W, N
GDN, RES = _lib.EPI_GDN, _lib.EPI_RES   # outside / inside the kinds of the K-split and the Winograd kernels


def row(k, s, pad, tr, cin, cout, oh, ow, n, ngroups=1, cls=0, act=0, epi=0, seg=0, algo=0, xv=0, aligned=1, cfg=-1,
        mode=-1, ps=0):
    """a row from the small map (oh, ow): the input of a transposed launch, the output of a plain one"""
    if tr:
        h, w, OH, OW = oh, ow, oh * s, ow * s
    else:
        h, w, OH, OW = oh * s, ow * s, oh, ow
        assert OH == (h + 2 * pad - k) // s + 1 and OW == (w + 2 * pad - k) // s + 1
    seg_len = max(1, cin // 2) if seg else 0
    return (cfg, mode, ngroups, cls, n, cin, h, w, cout, OH, OW, k, k, s, pad, tr, act, epi, 0, ps, seg_len, 4 if seg else 0,
            algo, xv, aligned)


def case_rows():
    """forward and input-gradient launch of every conv shape of tests/test_gpu_ops.py, every tap class"""
    from test_gpu_ops import CONV_CASES, KS8_CASES, P1_CASES
    shapes = [c[1:] for c in CONV_CASES + KS8_CASES] + [c[1:] + (1, 1, False) for c in P1_CASES]
    shapes += [(3, 40, 20, 36, 200, 3, 1, False), (2, 13, 18, 24, 70, 1, 1, False), (2, 21, 18, 24, 33, 5, 2, False),
               (2, 8, 18, 24, 32, 3, 1, False)]   # test_conv_every_tile_config
    out = []
    for N, cin, H, W, cout, k, s, tr in shapes:
        pad = k // 2
        if tr:   # ConvTranspose2d: forward scatters, its input gradient gathers
            big = (H * s, W * s)
            pair = [(1, cin, cout, H, W, big[0], big[1]), (0, cout, cin, big[0], big[1], H, W)]
        else:
            o = ((H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1)
            pair = [(0, cin, cout, H, W, o[0], o[1]), (1, cout, cin, o[0], o[1], H, W)]
        for t, ci, co, h, w, oh, ow in pair:
            for cls in range(s * s if t else 1):
                out.append((-1, -1, 1, cls, N, ci, h, w, co, oh, ow, k, k, s, pad, t, 0, 0, 0, 0, 0, 0, 0, 0, 1))
    return out


def rows():
    auto = []
    for (k, s, pad), tr, cin, cout, (oh, ow, n), g in itertools.product(KERNELS, (0, 1), CHANS, CHANS, MAPS, (1, 2, 6)):
        auto.append(row(k, s, pad, tr, cin, cout, oh, ow, n, g))
    # operand activation, epilogue kind, channel map and operand alignment, on a thinner cross
    variants = ((1, 0, 0, 1), (0, RES, 0, 1), (0, GDN, 0, 1), (0, 0, 1, 1), (0, 0, 0, 0), (1, GDN, 1, 0), (1, RES, 0, 0),
                (0, RES, 1, 1))
    for (k, s, pad), tr, cin, cout, (oh, ow, n), g, (act, epi, seg, al) in itertools.product(
            KERNELS, (0, 1), THIN, THIN, MAPS, (1, 6), variants):
        auto.append(row(k, s, pad, tr, cin, cout, oh, ow, n, g, act=act, epi=epi, seg=seg, aligned=al))
    # the other tap classes of the transposed stride-2 launches
    for (k, s, pad), cin, cout, (oh, ow, n), g, cls in itertools.product(
            [x for x in KERNELS if x[1] == 2], THIN, THIN, MAPS, (1, 6), (1, 2, 3)):
        auto.append(row(k, s, pad, 1, cin, cout, oh, ow, n, g, cls=cls))
    # Winograd, from the raw and from the pre-transformed operand (GDN: a kind its kernels are not compiled for)
    for cin, cout, (oh, ow, n), g, xv, (act, epi) in itertools.product(CHANS, CHANS, MAPS, (1, 2, 6), (0, 1),
                                                                     ((0, 0), (1, RES), (0, GDN))):
        auto.append(row(3, 1, 1, 0, cin, cout, oh, ow, n, g, act=act, epi=epi, algo=1, xv=xv))
    # fused PixelShuffle store (no pointwise / Winograd form), and launches that validation refuses
    for cin, cout, (oh, ow, n) in itertools.product(THIN, (48, 192, 320), MAPS):
        auto.append(row(3, 1, 1, 0, cin, cout, oh, ow, n, ps=2))
        auto.append(row(1, 1, 0, 0, cin, cout, oh, ow, n, ps=2))
    bad = list(row(3, 1, 1, 0, 48, 48, 16, 16, 2))
    bad[ARG_FIELDS.index("OH")] += 1
    auto.append(tuple(bad))                                       # inconsistent geometry
    auto.append(row(3, 1, 1, 0, 48, 50, 16, 16, 2, ps=2))         # PixelShuffle needs Cout % 4 == 0
    auto.append(row(3, 1, 1, 0, 48, 48, 16, 16, 2, algo=2))       # no such algo
    auto.append(row(3, 1, 1, 1, 48, 48, 16, 16, 2, cls=1))        # a stride-1 launch has one class
    auto.append(row(5, 1, 2, 0, 48, 48, 16, 16, 2, algo=1))       # Winograd is 3x3 only
    cases = case_rows()
    auto += cases
    forced = []
    for c in cases:
        forced += [(cfg,) + c[1:] for cfg in list(range(NCFG)) + [_lib.CONV_CFG_KS8_64X64, _lib.CONV_CFG_KS8_32X128]]
        forced += [(-1, mode) + c[2:] for mode in (0, 1)]
    return auto, forced


def main():
    set_ = [v for v in PLANNER_ENV if v in os.environ]
    if set_:
        sys.exit(f"refusing to record plans with planner switches set: {set_}")
    L = _lib.lib()
    auto, forced = rows()
    args = np.asarray(auto + forced, dtype=np.int32)
    trace = getattr(L, "icm_debug_probe_flags", None) if hasattr(L, "icm_debug_probe_flags") else None
    res, flags = [], []
    for r in args:
        res.append(plan(L, r))
        flags.append(trace() if trace and res[-1][0] == OK and res[-1][2] in (STAGED, KSPLIT) else 0)
    res, flags = np.asarray(res, dtype=np.int64), np.asarray(flags)
    A = {f: args[:len(auto), i] for i, f in enumerate(ARG_FIELDS)}
    pa, pf, ff = res[:len(auto)], res[len(auto):], args[len(auto):, 0]
    ok = pa[:, 0] == OK
    fam, idx = pa[:, 2], pa[:, 3]
    # coverage (conditions on the pinned planner, checked before anything is written)
    assert set(fam[ok].tolist()) == {STAGED, KSPLIT, DIRECT1X1, WINO44, WINO8}, "a family no automatic row reaches"
    staged = sorted(set(idx[ok & (fam == STAGED) & (pa[:, 9] > 0)].tolist()))
    assert len(staged) >= 9, staged
    assert set(idx[ok & (fam == KSPLIT)].tolist()) == {2}, "the automatic K-split choice is the 64 x 64 block"
    for cfg, tco in ((_lib.CONV_CFG_KS8_64X64, 2), (_lib.CONV_CFG_KS8_32X128, 1)):
        m = (ff == cfg) & (pf[:, 0] == OK) & (pf[:, 2] == KSPLIT)
        assert m.any() and set(pf[m, 3].tolist()) == {tco}, cfg
    for cfg in range(NCFG):
        m = (ff == cfg) & (pf[:, 0] == OK)
        assert m.any() and set(pf[m, 2].tolist()) == {STAGED} and set(pf[m, 3].tolist()) == {cfg}, cfg
    # pointwise launches: the wave count does not depend on Cin, so a pair of rows that differ in Cin alone and fall on
    # the two sides is the short-K rule; rows beyond 384 channels on both sides are the wave threshold itself
    elig = ok & (A["KH"] == 1) & (A["stride"] == 1) & (A["Cin"] % 8 == 0) & (A["x_seg_len"] == 0) & (A["algo"] == 0) & \
        (A["pixel_shuffle"] == 0)
    took = elig & (fam == DIRECT1X1)
    assert (took & (A["Cin"] > 384)).any() and (elig & ~took & (A["Cin"] > 384)).any(), "wave threshold: one side only"
    assert (took & (A["Cin"] <= 384)).any() and (elig & ~took & (A["Cin"] <= 384)).any(), "wave threshold: one side only"
    key = lambda i: tuple(int(A[f][i]) for f in ARG_FIELDS if f != "Cin")   # noqa: E731
    short = {key(i) for i in np.nonzero(took & (A["Cin"] <= 384))[0]}
    assert any(key(i) in short for i in np.nonzero(elig & ~took & (A["Cin"] > 384))[0]), "short-K rule never decides"
    # single-pass rule (halo launches with >= 16 384 pixels): a tiling that covers all output channels exists for <= 6 co
    # tiles; rows that took it (ncb == 1) and rows that kept several co blocks
    halo = ok & (fam == STAGED) & (A["KH"] >= 3) & (A["transposed"] == 0) & (A["Cout"] <= 192) & \
        (A["N"].astype(np.int64) * A["OH"] * A["OW"] >= 16384)
    assert (halo & (pa[:, 8] == 1) & (A["Cout"] > 32)).any() and (halo & (pa[:, 8] > 1)).any()
    if trace:   # the recording library can say it exactly: a candidate existed (1) / replaced a different cheapest row (2)
        fa = flags[:len(auto)]
        assert ((fa & 3) == 1).any() and ((fa & 2) == 2).any(), "single-pass rule: one outcome only"
        print(f"single-pass rule: candidate kept {int(((fa & 3) == 1).sum())} rows, overriding {int(((fa & 2) == 2).sum())} rows")
    direct = ok & (fam <= KSPLIT) & (pa[:, 9] > 0)
    for col, name in ((12, "vec4"), (13, "dma")):
        assert set(pa[direct & (fam == STAGED), col].tolist()) == {0, 1}, name
    codes = set(res[:, 0].tolist())
    assert {OK, ERR_ARG, ERR_UNSUPPORTED} <= codes, codes
    assert (res[res[:, 0] != OK, 1:] == 0).all()
    np.savez_compressed(os.path.join(HERE, "conv_plans.npz"), args=args, plan=res)
    fams = {f: int((ok & (fam == f)).sum()) for f in range(5)}
    print(f"wrote conv_plans.npz: {len(auto)} automatic + {len(forced)} forced rows; automatic rows per family {fams}; "
          f"staged cfgs reached {staged}; return codes {sorted(codes)}")


if __name__ == "__main__":
    main()
