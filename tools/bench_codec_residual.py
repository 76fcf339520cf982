#!/usr/bin/env python
"""The error-bounded residual layer (``codec encode --max-error``): what its three kernels cost, and what the whole
encode and decode cost with and without it, on a large synthetic image (2048x3072).

    kernel   icm_residual_code, icm_residual_indexes and icm_residual_apply alone: microseconds per launch (HIP events
             over --iters launches of the C entry points) and achieved bytes/s.  Bytes are those the algorithm needs:
             6 in and 24 + 4 / 256 out per pixel for code, 12 out for indexes, 15 in and 3 out for apply.  Launches rotate
             over two sets of buffers, more than the 256 MiB last-level cache in all.  The yardstick printed next to each
             is a device-to-device copy that moves the same number of bytes (half of them read, half written), rotated
             and timed the same way.
    codec    encode_image / decode_image without and with max_error = --max-error in the same process, alternating,
             medians of --rounds wall times (device synchronised), the file sizes, and the bound as decoded.

With --error-roi Y0,X0,H,W:D' (repeatable; the rectangles of ``codec encode --error-roi``, D the background) the kernel
part also times icm_residual_code_map and icm_residual_apply_map under that map, which adds one byte per cell to code
and one or two per run of four pixels to apply, and the codec part also encodes the mapped file and the uniform
lossless one (max_error = 0) and reports their sizes next to the uniform D's.

The model is a randomly initialised ``cnn`` (seeded): its base reconstruction is far from the image, so the residual
dominates the file and the sizes say nothing about a trained codec.  The bound is what is verified, not the rate.  Prints
one JSON line per part.

    region   (--region, alone) decode_image with ``region`` = the central --region-size window against the whole decode,
             on a 2048x3072 untiled and a 3008x4032 tiled file of ``--max-error`` / ``--coder``, alternating, medians of
             --rounds wall times; the residual string alone (``residual.decode_residual`` with and without the window);
             the residual waves decoded of G; and the peak device memory of the region decode, and of the residual
             string's decode alone, above what was allocated before it (the allocator's peak: the decoder's own upload
             of the string, one copy of ``residual_bytes``, is not in it).  Runs unchanged on a checkout from before the ranged decode, where the window changes nothing.

    python tools/bench_codec_residual.py [--iters 100] [--rounds 3] [--kernel-only] [--coder {host,lanes}] [--max-error D]
                                          [--error-roi Y0,X0,H,W:D' ...] [--region [--region-size 512]]

--kernel-only runs the kernel part alone (the run to put under rocprofv3 --kernel-trace --stats).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "image-compression-for-machine_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_codec_tiles import HBM_PEAK, synthetic, wall  # noqa: E402

H, W = 2048, 3072
SETS = 2


def events(fn, iters, torch):
    for i in range(SETS + 2):
        fn(i)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def kernel_part(args, torch, np, R, L, dmap=None):
    dev, d = "cuda:0", args.max_error
    rng = np.random.default_rng(1)
    x = synthetic(np, H, W, 1)
    xhat = np.clip(x.astype(np.int64) + rng.integers(-12, 13, size=x.shape), 0, 255).astype(np.uint8)
    gh, gw = R.grid(H, W)
    sets = []
    for _ in range(SETS):
        s = {"x": torch.from_numpy(x).to(dev), "xhat": torch.from_numpy(xhat).to(dev),
             "sym": torch.empty((3, H, W), dtype=torch.int32, device=dev),
             "idx": torch.empty((3, H, W), dtype=torch.int32, device=dev),
             "cls": torch.empty((gh, gw), dtype=torch.int32, device=dev),
             "out": torch.empty((H, W, 3), dtype=torch.uint8, device=dev)}
        if dmap is not None:
            s["dmap"] = torch.from_numpy(dmap).to(dev)
        sets.append(s)
    lib, st = L.lib(), L.stream()
    px = H * W
    launches = {
        "icm_residual_code": (6 * px + 24 * px + 4 * gh * gw, lambda s: lib.icm_residual_code(
            s["x"].data_ptr(), s["xhat"].data_ptr(), H, W, d, s["sym"].data_ptr(), s["idx"].data_ptr(),
            s["cls"].data_ptr(), st)),
        "icm_residual_indexes": (12 * px + 4 * gh * gw, lambda s: lib.icm_residual_indexes(
            s["cls"].data_ptr(), H, W, s["idx"].data_ptr(), st)),
        "icm_residual_apply": (15 * px + 3 * px, lambda s: lib.icm_residual_apply(
            s["xhat"].data_ptr(), s["sym"].data_ptr(), H, W, 0, 0, H, W, d, s["out"].data_ptr(), st)),
    }
    if dmap is not None:
        runs = H * -(-W // 4)
        launches["icm_residual_code_map"] = (6 * px + 24 * px + 5 * gh * gw, lambda s: lib.icm_residual_code_map(
            s["x"].data_ptr(), s["xhat"].data_ptr(), H, W, s["dmap"].data_ptr(), s["sym"].data_ptr(),
            s["idx"].data_ptr(), s["cls"].data_ptr(), st))
        launches["icm_residual_apply_map"] = (15 * px + 3 * px + runs, lambda s: lib.icm_residual_apply_map(
            s["xhat"].data_ptr(), s["sym"].data_ptr(), H, W, 0, 0, H, W, s["dmap"].data_ptr(), s["out"].data_ptr(), st))
    for name, (nbytes, fn) in launches.items():
        L.check(fn(sets[0]), name)
        us = events(lambda i: fn(sets[i % SETS]), args.iters, torch)
        half = nbytes // 2
        src = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(SETS)]
        dst = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(SETS)]
        cus = events(lambda i: dst[i % SETS].copy_(src[i % SETS]), args.iters, torch)
        del src, dst
        if name.startswith("icm_residual_apply"):        # what the launches left: every sample within its cell's bound
            cells = sets[0]["dmap"].to(torch.int16) if name.endswith("_map") else \
                torch.full((gh, gw), d, dtype=torch.int16, device=dev)
            bound = cells.repeat_interleave(16, 0).repeat_interleave(16, 1)[:H, :W, None]
            err = (sets[0]["out"].to(torch.int16) - sets[0]["x"].to(torch.int16)).abs()
            assert bool((err <= bound).all()), name
        print(json.dumps({"metric": "residual_kernel", "kernel": name, "height": H, "width": W, "max_error": d,
                          "iters": args.iters, "us_per_launch": round(us, 2), "bytes": nbytes,
                          "GBps": round(nbytes / us / 1e3, 1),
                          "pct_of_hbm_peak": round(100.0 * nbytes / (us * 1e-6) / HBM_PEAK, 1),
                          "copy_same_bytes_us": round(cus, 2), "kernel_over_copy": round(us / cus, 2),
                          "note": "HIP events around back-to-back launches from Python, two rotating buffer sets: "
                                  "launch overhead is inside both figures"}), flush=True)


def codec_part(args, torch, np, codec, rois=None):
    from icm_amd.zoo import models
    torch.manual_seed(0)
    model = models["cnn"]().to("cuda:0").eval()
    model.update(force=True)
    a = synthetic(np, H, W, 1)
    variants = {"plain": {}, "bounded": {"max_error": args.max_error}}
    if rois:
        variants["mapped"] = {"max_error": args.max_error, "error_roi": rois}
        variants["lossless"] = {"max_error": 0}
    data, info, te, td = {}, {}, {k: [] for k in variants}, {k: [] for k in variants}
    for k, extra in variants.items():                                       # warm every shape up
        data[k], info[k] = codec.encode_image_info(model, a, coder=args.coder, **extra)
        codec.decode_image(model, data[k])
    for _ in range(args.rounds):                                            # alternating: drift hits both alike
        for k, extra in variants.items():
            te[k].append(wall(lambda: codec.encode_image(model, a, coder=args.coder, **extra), torch)[0])
            td[k].append(wall(lambda: codec.decode_image(model, data[k]), torch)[0])
    out, dinfo = codec.decode_image(model, data["bounded"], reference=a)
    assert dinfo["max_abs_error"] <= args.max_error
    print(json.dumps({"metric": "codec_residual", "coder": args.coder, "height": H, "width": W,
                      "max_error": args.max_error, "model": "cnn, randomly initialised (seed 0)", "rounds": args.rounds,
                      "plain_encode_s": round(statistics.median(te["plain"]), 4),
                      "bounded_encode_s": round(statistics.median(te["bounded"]), 4),
                      "plain_decode_s": round(statistics.median(td["plain"]), 4),
                      "bounded_decode_s": round(statistics.median(td["bounded"]), 4),
                      "plain_encode_s_all": [round(t, 4) for t in te["plain"]],
                      "bounded_encode_s_all": [round(t, 4) for t in te["bounded"]],
                      "plain_decode_s_all": [round(t, 4) for t in td["plain"]],
                      "bounded_decode_s_all": [round(t, 4) for t in td["bounded"]],
                      "plain_bytes": len(data["plain"]), "bounded_bytes": len(data["bounded"]),
                      "base_bytes": info["bounded"]["base_bytes"], "residual_bytes": info["bounded"]["residual_bytes"],
                      "residual_class_range": info["bounded"]["residual_class_range"],
                      "max_abs_error": dinfo["max_abs_error"], "bpp": round(dinfo["bpp"], 3)}), flush=True)
    if rois:
        out, minfo = codec.decode_image(model, data["mapped"], reference=a)
        assert minfo["bound_violations"] == 0
        print(json.dumps({"metric": "codec_residual_map", "coder": args.coder, "height": H, "width": W,
                          "max_error": args.max_error, "error_roi": [list(r) for r in rois],
                          "max_error_range": info["mapped"]["max_error_range"],
                          "error_roi_cells": info["mapped"]["error_roi_cells"], "cells": int(minfo["max_error_map"].size),
                          "mapped_bytes": len(data["mapped"]), "bounded_bytes": len(data["bounded"]),
                          "lossless_bytes": len(data["lossless"]), "base_bytes": info["mapped"]["base_bytes"],
                          "mapped_encode_s": round(statistics.median(te["mapped"]), 4),
                          "mapped_decode_s": round(statistics.median(td["mapped"]), 4),
                          "bounded_encode_s": round(statistics.median(te["bounded"]), 4),
                          "bounded_decode_s": round(statistics.median(td["bounded"]), 4),
                          "bound_violations": minfo["bound_violations"], "max_abs_error": minfo["max_abs_error"],
                          "note": "randomly initialised model: the sizes exercise the mechanism, nothing more"}),
              flush=True)


def region_part(args, torch, np, codec, R):
    import inspect
    from bench_codec_tiles import OVERLAP, TILE
    from icm_amd import bitstream as B
    from icm_amd.ans import coder_for
    from icm_amd.zoo import models
    torch.manual_seed(0)
    model = models["cnn"]().to("cuda:0").eval()
    model.update(force=True)
    ranged = "window" in inspect.signature(R.decode_residual).parameters
    n = args.region_size
    for name, (h, w), kw in (("untiled", (H, W), {}), ("tiled", (3008, 4032), {"tile": TILE, "overlap": OVERLAP})):
        a = synthetic(np, h, w, 1)
        region = ((h - n) // 2, (w - n) // 2, n, n)
        data = codec.encode_image(model, a, coder=args.coder, max_error=args.max_error, **kw)
        string = B.unpack_residual(data, R.tables().crc)[2]
        full, finfo = codec.decode_image(model, data)                       # warm both shapes up
        crop, rinfo = codec.decode_image(model, data, region=region)
        assert torch.equal(crop, full[region[0]:region[0] + n, region[1]:region[1] + n])
        del full, crop

        def residual(window):
            kwargs = {"window": window} if ranged and window is not None else {}
            return R.decode_residual(string, h, w, coder_for(args.coder), "cuda:0", **kwargs)
        t = {k: [] for k in ("whole", "region", "residual_whole", "residual_region")}
        for _ in range(args.rounds):                                        # alternating: drift hits all alike
            t["whole"].append(wall(lambda: codec.decode_image(model, data), torch)[0])
            t["region"].append(wall(lambda: codec.decode_image(model, data, region=region), torch)[0])
            t["residual_whole"].append(wall(lambda: residual(None), torch)[0])
            t["residual_region"].append(wall(lambda: residual(region), torch)[0])
        def peak_of(fn):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            before = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            return int(torch.cuda.max_memory_allocated() - before)
        peak = peak_of(lambda: codec.decode_image(model, data, region=region))
        peak_res = {"residual_region_peak_device_bytes": peak_of(lambda: residual(region)),
                    "residual_whole_peak_device_bytes": peak_of(lambda: residual(None))}
        waves = rinfo.get("residual_waves")
        res = {"metric": "codec_residual_region", "input": name, "coder": args.coder, "height": h, "width": w,
               "max_error": args.max_error, "region": list(region), "ranged_decode": ranged, "rounds": args.rounds,
               "residual_bytes": len(string), "residual_waves": waves, "tiles_decoded": rinfo.get("tiles_decoded"),
               "region_peak_device_bytes": peak, **peak_res}
        for k, v in t.items():
            res[f"{k}_decode_s"] = round(statistics.median(v), 4)
            res[f"{k}_decode_s_all"] = [round(x, 4) for x in v]
        if waves:
            res["residual_region_us_per_wave"] = round(1e6 * statistics.median(t["residual_region"]) / waves[0], 1)
            res["residual_whole_us_per_wave"] = round(1e6 * statistics.median(t["residual_whole"]) / waves[1], 1)
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--coder", default="lanes", choices=["host", "lanes"])
    ap.add_argument("--max-error", type=int, default=2)
    ap.add_argument("--error-roi", action="append", default=None, metavar="Y0,X0,H,W:D",
                    help="rectangle with its own absolute bound, repeatable: also time the map kernels and encode the "
                         "mapped file")
    ap.add_argument("--region", action="store_true",
                    help="the region part alone: a central window of an untiled and a tiled file against the whole decode")
    ap.add_argument("--region-size", type=int, default=512, metavar="N", help="side of the window of --region")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_codec_residual: no GPU (there is no CPU fallback)")
    from icm_amd import _lib as L
    from icm_amd import codec
    from icm_amd import residual as R
    if args.region:
        return region_part(args, torch, np, codec, R)
    rois = dmap = None
    if args.error_roi:
        rois = [codec._roi(t) for t in args.error_roi]
        dmap = codec.error_map(H, W, args.max_error, rois)
    kernel_part(args, torch, np, R, L, dmap)
    if not args.kernel_only:
        codec_part(args, torch, np, codec, rois)


if __name__ == "__main__":
    main()
