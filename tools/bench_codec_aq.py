#!/usr/bin/env python
"""Variance-adaptive quantisation (``codec encode --aq``): what the statistics kernel costs, and what the whole encode
costs with it, on large synthetic images.

    kernel   icm_image_cell_stats alone on the 8-bit image, grid of the image's own centre pads: microseconds per
             launch (HIP events over --iters launches of the C entry point) and achieved bytes/s against the HBM peak.
             Bytes are those the algorithm needs: the 3 H W image bytes read once (the 12 bytes per cell written are
             counted too).  Two rows per size: the same image every launch, which the 256 MiB last-level cache keeps
             (no HBM figure), and launches that rotate over copies of more than 300 MB in all, which it cannot.
    encode   encode_image without and with aq = 1 in the same process, alternating, medians of --rounds wall times
             (device synchronised), and the two file sizes: 2048x3072 untiled, 4032x3008 as 2 x 3 tiles
             (--tile 2048 --overlap 128).

The model is a randomly initialised ``cnn`` (seeded), so the file sizes say nothing about a trained codec and no
rate-distortion statement follows from them; they are there to show that the map changes the stream.  Prints one JSON
line per part.

    python tools/bench_codec_aq.py [--iters 200] [--rounds 5] [--kernel-only] [--coder {host,lanes}]

--kernel-only runs the kernel part alone (the run to put under rocprofv3 --kernel-trace --stats).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "image-compression-for-machine_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_codec_tiles import HBM_PEAK, OVERLAP, TILE, synthetic, wall  # noqa: E402

SIZES = [(2048, 3072, 1, {}), (3008, 4032, 2, {"tile": TILE, "overlap": OVERLAP})]
ROTATE_BYTES = 320 << 20     # more than the 256 MiB last-level cache


def kernel_part(args, torch, np, codec, L):
    dev = "cuda:0"
    for h, w, seed, _ in SIZES:
        a = torch.from_numpy(synthetic(np, h, w, seed)).to(dev)
        left, right, top, bottom = codec.center_pads(h, w)
        gh, gw = (top + h + bottom) // codec.CELL, (left + w + right) // codec.CELL
        out = torch.empty((gh, gw, 3), dtype=torch.int32, device=dev)
        copies = [a] + [a.clone() for _ in range(-(-ROTATE_BYTES // a.numel()) - 1)]
        fn, st = L.lib().icm_image_cell_stats, L.stream()
        nbytes = a.numel() + out.numel() * 4
        for name, imgs in (("one image, cache-resident", copies[:1]), ("rotating copies, from HBM", copies)):
            ptrs = [t.data_ptr() for t in imgs]
            for i in range(len(ptrs) + 4):
                L.check(fn(ptrs[i % len(ptrs)], h, w, top, left, gh, gw, out.data_ptr(), st))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for i in range(args.iters):
                fn(ptrs[i % len(ptrs)], h, w, top, left, gh, gw, out.data_ptr(), st)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) / args.iters * 1e3
            print(json.dumps({"metric": "cell_stats_kernel", "height": h, "width": w, "grid": [gh, gw], "input": name,
                              "copies": len(imgs), "iters": args.iters, "us_per_launch": round(us, 2), "bytes": nbytes,
                              "GBps": round(nbytes / us / 1e3, 1),
                              "pct_of_hbm_peak": round(100.0 * nbytes / (us * 1e-6) / HBM_PEAK, 1),
                              "note": "HIP events around back-to-back launches of the C entry point from Python: launch "
                                      "overhead is inside the figure"}), flush=True)
        assert np.array_equal(out.cpu().numpy(), codec.cell_stats(a, (left, right, top, bottom)))


def encode_part(args, torch, np, codec):
    from icm_amd.zoo import models
    torch.manual_seed(0)
    model = models["cnn"]().to("cuda:0").eval()
    model.update(force=True)
    for h, w, seed, kw in SIZES:
        a = synthetic(np, h, w, seed)
        kw = {**kw, "coder": args.coder}
        variants = {"plain": {}, "aq": {"aq": 1.0}}
        data, info, ts = {}, {}, {k: [] for k in variants}
        for k, extra in variants.items():                                   # warm every shape up
            data[k], info[k] = codec.encode_image_info(model, a, **kw, **extra)
        for _ in range(args.rounds):                                        # alternating: drift hits both alike
            for k, extra in variants.items():
                ts[k].append(wall(lambda: codec.encode_image(model, a, **kw, **extra), torch)[0])
        t_stats = wall(lambda: codec.cell_stats(torch.from_numpy(a).to("cuda:0"), (0, 0, 0, 0)), torch)[0]
        res = {"metric": "codec_encode_aq", "coder": args.coder, "height": h, "width": w, "tile": kw.get("tile"),
               "overlap": kw.get("overlap"), "model": "cnn, randomly initialised (seed 0)", "rounds": args.rounds,
               "plain_encode_s": round(statistics.median(ts["plain"]), 4),
               "aq_encode_s": round(statistics.median(ts["aq"]), 4),
               "plain_encode_s_all": [round(t, 4) for t in ts["plain"]],
               "aq_encode_s_all": [round(t, 4) for t in ts["aq"]],
               "plain_bytes": len(data["plain"]), "aq_bytes": len(data["aq"]),
               "aq_ref": round(info["aq"]["aq_ref"], 4), "aq_offset_range": info["aq"]["aq_offset_range"],
               "cells_off_the_background": info["aq"]["roi_cells"],
               "upload_and_anchored_stats_s": round(t_stats, 5)}
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--coder", default="host", choices=["host", "lanes"])
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_codec_aq: no GPU (there is no CPU fallback)")
    from icm_amd import _lib as L
    from icm_amd import codec
    kernel_part(args, torch, np, codec, L)
    if not args.kernel_only:
        encode_part(args, torch, np, codec)


if __name__ == "__main__":
    main()
