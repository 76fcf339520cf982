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

    python tools/bench_codec_tiles.py [--iters 200] [--rounds 3] [--kernel-only] [--coder {host,lanes}]
                                      [--symbols-per-wave N] [--coder-kernels]

--kernel-only runs the kernel part alone (the run to put under rocprofv3 --kernel-trace --stats).
--coder picks the entropy coder of the two codec parts (every result line names it); --coder-kernels replaces them by
    lanes_kernels   the lane-stream kernels alone on the symbols of the 2048x3072 image: HIP-event time and symbols/s
             of the whole-string encode (its launches, the 16-byte result copy and the wait) and of one decode_run
             (slice 0 of the y string), with both table searches of the decode kernel.
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


def lanes_kernel_part(args, torch, np, codec, L):
    from icm_amd import ans
    from icm_amd.zoo import models
    torch.manual_seed(0)
    model = models["cnn"]().to("cuda:0").eval()
    model.update(force=True)
    h, w = 2048, 3072
    x = codec.image_u8_to_f32(torch.from_numpy(synthetic(np, h, w, seed=1)).to("cuda:0"), (0, 0, 0, 0))
    dbg = {}
    model.compress(x, _debug=dbg, coder="lanes", symbols_per_wave=args.symbols_per_wave)
    gc = model.gaussian_conditional
    tabs = gc._device_tables()
    sym, idx = torch.from_numpy(dbg["symbols"]).to("cuda:0"), torch.from_numpy(dbg["indexes"]).to("cuda:0")
    n = sym.numel() // model.num_slices
    runs = [n] * model.num_slices
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def events(fn, iters):
        ts = []
        for _ in range(iters):
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)

    string = ans.lanes_encode_gpu(sym, idx, runs, *tabs, symbols_per_wave=args.symbols_per_wave)
    host_s = wall(lambda: ans.lanes_encode(dbg["symbols"], dbg["indexes"], runs, gc._tables(), args.symbols_per_wave), torch)
    assert host_s[1] == string
    res = {"metric": "lanes_kernels", "height": h, "width": w, "symbols": int(sym.numel()), "slice_symbols": n,
           "symbols_per_wave": args.symbols_per_wave, "waves": ans.lanes_waves(runs, args.symbols_per_wave),
           "y_string_bytes": len(string), "host_lanes_encode_s": round(host_s[0], 4)}
    ms = events(lambda: ans.lanes_encode_gpu(sym, idx, runs, *tabs, symbols_per_wave=args.symbols_per_wave), 10)
    res.update(encode_ms=round(ms, 3), encode_Msym_per_s=round(sym.numel() / ms / 1e3, 1),
               encode_note="workspace allocation, init + 10 run launches + pack, result copy and wait, string D2H")
    out = torch.empty(n, dtype=torch.int32, device="cuda:0")
    for centre in (1, 0):
        L.lib().icm_debug_lanes_search(centre)
        ts = []
        for _ in range(7):
            dec = ans.LanesDecoderGpu(string)
            ts.append(events(lambda: dec.decode_run(idx[:n], *tabs, out=out), 1))
            dec.close()
            assert torch.equal(out, sym[:n])
        ms = statistics.median(ts)
        key = "centre" if centre else "binary"
        res.update({f"decode_run_{key}_ms": round(ms, 3), f"decode_run_{key}_Msym_per_s": round(n / ms / 1e3, 1)})
    print(json.dumps(res), flush=True)

    # the random model puts nearly every symbol in the centre bin of the narrowest tables (the y string above holds no
    # word at all), which exercises neither the search nor the renormalisation reads.  A slice of the same size drawn
    # the way a trained model's latents are distributed: table index uniform over the scale table, symbol =
    # round(N(0, scale[index])), so the wide tables (up to ~3 100 bins) and several bits per symbol take part.
    g = torch.Generator(device="cuda:0").manual_seed(1)
    sidx = torch.randint(0, gc.scale_table.numel(), (n,), generator=g, device="cuda:0", dtype=torch.int32)
    scale = gc.scale_table.to("cuda:0", torch.float32)[sidx.long()]
    ssym = torch.round(torch.randn(n, generator=g, device="cuda:0") * scale).to(torch.int32)
    sstring = ans.lanes_encode_gpu(ssym, sidx, [n], *tabs, symbols_per_wave=args.symbols_per_wave)
    res = {"metric": "lanes_kernels_synthetic", "slice_symbols": n, "symbols_per_wave": args.symbols_per_wave,
           "waves": ans.lanes_waves([n], args.symbols_per_wave), "string_bytes": len(sstring),
           "bits_per_symbol": round(8.0 * len(sstring) / n, 3)}
    ms = events(lambda: ans.lanes_encode_gpu(ssym, sidx, [n], *tabs, symbols_per_wave=args.symbols_per_wave), 10)
    res.update(encode_ms=round(ms, 3), encode_Msym_per_s=round(n / ms / 1e3, 1))
    for centre in (1, 0):
        L.lib().icm_debug_lanes_search(centre)
        ts = []
        for _ in range(7):
            dec = ans.LanesDecoderGpu(sstring)
            ts.append(events(lambda: dec.decode_run(sidx, *tabs, out=out), 1))
            dec.finish()
            assert torch.equal(out, ssym)
        ms = statistics.median(ts)
        key = "centre" if centre else "binary"
        res.update({f"decode_run_{key}_ms": round(ms, 3), f"decode_run_{key}_Msym_per_s": round(n / ms / 1e3, 1)})
    print(json.dumps(res), flush=True)


def codec_parts(args, torch, np, codec):
    from icm_amd.zoo import models
    torch.manual_seed(0)
    model = models["cnn"]().to("cuda:0").eval()
    model.update(force=True)
    if args.coder != "host":      # the host rows stay the calls they were
        enc0 = codec.encode_image
        codec.encode_image = lambda m, a, **kw: enc0(m, a, coder=args.coder, symbols_per_wave=args.symbols_per_wave, **kw)

    def timed(fn):
        ts, r = [], None
        for _ in range(args.rounds):
            t, r = wall(fn, torch)
            ts.append(t)
        return round(statistics.median(ts), 3), r

    h, w = 2048, 3072
    a = synthetic(np, h, w, seed=1)
    res = {"metric": "codec_tiled_vs_untiled", "coder": args.coder, "height": h, "width": w, "tile": TILE, "overlap": OVERLAP,
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
    res = {"metric": "codec_tiled_over_limit", "coder": args.coder, "height": h, "width": w, "tile": TILE, "overlap": OVERLAP,
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
    ap.add_argument("--coder", default="host", choices=["host", "lanes"])
    ap.add_argument("--symbols-per-wave", type=int, default=16384)
    ap.add_argument("--coder-kernels", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_codec_tiles: no GPU (there is no CPU fallback)")
    from icm_amd import _lib as L
    from icm_amd import codec
    if args.coder_kernels:
        lanes_kernel_part(args, torch, np, codec, L)
        return
    kernel_part(args, torch, codec, L)
    if not args.kernel_only:
        codec_parts(args, torch, np, codec)


if __name__ == "__main__":
    main()
