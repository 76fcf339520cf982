#!/usr/bin/env python
"""Tiled bit-streams: the assembly kernel alone, and tiled against untiled coding of large synthetic images.

    kernel   icm_image_tile_blend on one 2048x2048 tile with 128-pixel bands on all four sides: microseconds per launch
             (HIP events over --iters launches) and achieved bytes/s against the HBM peak.  Bytes are those the
             algorithm needs: the tile read once, the canvas window read and written, 36 h w in all.
    2048x3072   tiled (--tile 2048 --overlap 128: two tiles) against untiled: file bytes, the bpp overhead of tiling,
             PSNR of each against the original, wall time of encode and decode.
    4032x3008   the padded size of a 4000x3000 photograph, past what one compress() call addresses: tiled encode and
             decode wall time.  The untiled call on it is not made: its line says "not measured".

The model is a randomly initialised ``cnn`` (seeded), so file sizes and PSNR say nothing about a trained codec; they
are there for the tiled / untiled difference.  Prints one JSON line per part.

    python tools/bench_codec_tiles.py [--iters 200] [--rounds 3] [--kernel-only]

--kernel-only runs the kernel part alone (the run to put under rocprofv3 --kernel-trace --stats).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "image-compression-for-machine_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK = 8.0e12          # bytes/s, specification; about 6.3e12 is achievable by a copy
TILE, OVERLAP = 2048, 128


def synthetic(np, h, w, seed):
    """gradients, a coarse texture and a little noise: 8-bit [h, w, 3]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([127 + 90 * np.sin(yy / (37.0 + 9 * c)) * np.cos(xx / (53.0 - 7 * c)) + 0.02 * (xx - yy)
                    for c in range(3)], -1)
    return np.clip(img + rng.integers(-6, 7, size=(h, w, 3)), 0, 255).astype(np.uint8)


def wall(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def kernel_part(args, torch, codec, L):
    dev = "cuda:0"
    h = w = TILE
    src = torch.rand((1, 3, h, w), device=dev)
    canvas = torch.zeros((3, h + 64, w + 64), device=dev)
    ramp = torch.from_numpy(codec.blend_ramp(OVERLAP)).to(dev)

    def launch():
        codec.image_tile_blend(src, (0, 0, 0, 0), canvas, 32, 32, ramp, 15)

    for _ in range(5):
        launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(args.iters):
        launch()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / args.iters * 1e3
    nbytes = 36 * h * w
    print(json.dumps({"metric": "tile_blend_kernel", "tile": [h, w], "overlap": OVERLAP, "iters": args.iters,
                      "us_per_launch": round(us, 2), "bytes": nbytes, "GBps": round(nbytes / us / 1e3, 1),
                      "pct_of_hbm_peak": round(100.0 * nbytes / (us * 1e-6) / HBM_PEAK, 1),
                      "note": "HIP events around the Python wrapper's launches; the canvas window (50 MB) and the tile "
                              "(50 MB) fit the 256 MiB last-level cache, so this is no pure HBM figure"}), flush=True)


def codec_parts(args, torch, np, codec):
    from icm_amd.zoo import models
    torch.manual_seed(0)
    model = models["cnn"]().to("cuda:0").eval()
    model.update(force=True)

    def timed(fn):
        ts, r = [], None
        for _ in range(args.rounds):
            t, r = wall(fn, torch)
            ts.append(t)
        return round(statistics.median(ts), 3), r

    h, w = 2048, 3072
    a = synthetic(np, h, w, seed=1)
    res = {"metric": "codec_tiled_vs_untiled", "height": h, "width": w, "tile": TILE, "overlap": OVERLAP,
           "model": "cnn, randomly initialised (seed 0)", "rounds": args.rounds}
    for name, kw in (("untiled", {}), ("tiled", {"tile": TILE, "overlap": OVERLAP})):
        codec.encode_image(model, a, **kw)                                  # warm every shape up
        t_enc, data = timed(lambda: codec.encode_image(model, a, **kw))
        t_dec, (img, info) = timed(lambda: codec.decode_image(model, data, reference=a))
        res.update({f"{name}_bytes": len(data), f"{name}_bpp": round(info["bpp"], 5),
                    f"{name}_psnr": round(info["psnr"], 4), f"{name}_encode_s": t_enc, f"{name}_decode_s": t_dec})
        if name == "tiled":
            res["tiles"] = info["tiles"]
    res["bpp_overhead_of_tiling"] = round(res["tiled_bpp"] - res["untiled_bpp"], 5)
    print(json.dumps(res), flush=True)

    h, w = 3008, 4032
    a = synthetic(np, h, w, seed=2)
    res = {"metric": "codec_tiled_over_limit", "height": h, "width": w, "tile": TILE, "overlap": OVERLAP,
           "model": "cnn, randomly initialised (seed 0)", "rounds": args.rounds}
    codec.encode_image(model, a, tile=TILE, overlap=OVERLAP)
    t_enc, data = timed(lambda: codec.encode_image(model, a, tile=TILE, overlap=OVERLAP))
    t_dec, (img, info) = timed(lambda: codec.decode_image(model, data, reference=a))
    t_reg, (crop, rinfo) = timed(lambda: codec.decode_image(model, data, region=(100, 100, 512, 512)))
    assert np.array_equal(crop.numpy(), img.numpy()[100:612, 100:612])
    res.update({"tiled_bytes": len(data), "tiled_bpp": round(info["bpp"], 5), "tiled_psnr": round(info["psnr"], 4),
                "tiles": info["tiles"], "tiled_encode_s": t_enc, "tiled_decode_s": t_dec,
                "region_512x512_decode_s": t_reg, "region_tiles_decoded": rinfo["tiles_decoded"]})
    res["untiled"] = "not measured"
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_codec_tiles: no GPU (there is no CPU fallback)")
    from icm_amd import _lib as L
    from icm_amd import codec
    kernel_part(args, torch, codec, L)
    if not args.kernel_only:
        codec_parts(args, torch, np, codec)


if __name__ == "__main__":
    main()
