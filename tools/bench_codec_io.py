#!/usr/bin/env python
"""The image boundary around the codec, host path against device path, on synthetic 8-bit images.

    (a) the f32 host path of eval_model / utils.inference:
          in:  ToTensor on the host -> f32 H2D -> pad_to_multiple
          out: crop -> f32 D2H -> mul(255).to(uint8) + transpose on the host
    (b) the 8-bit device path of icm_amd.codec:
          in:  8-bit H2D -> icm_image_u8_to_f32
          out: icm_image_f32_to_u8 (with the squared-error sum) -> 8-bit D2H

Per size: host wall time of each direction (perf_counter around work that ends in a synchronise, median of --rounds
interleaved rounds), the two kernels alone (HIP events over --iters launches) and their achieved bytes/s against the
HBM peak.  Bytes are those the algorithm needs: 3 H W read + 12 OH OW written on the way in, 12 H W read + 3 H W
written (+ 3 H W of the reference) on the way out.  Prints one JSON line per size.

    python tools/bench_codec_io.py [--rounds 7] [--iters 200] [--kernel-only]

--kernel-only runs the two kernels alone (the run to put under rocprofv3 --kernel-trace --stats).
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

SIZES = [(256, 256), (512, 768), (3000, 4000)]      # height, width
HBM_PEAK = 8.0e12                                    # bytes/s, specification; about 6.3e12 is achievable by a copy


def wall(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def events(fn, torch, iters):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # microseconds per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_codec_io: no GPU (there is no CPU fallback)")
    from icm_amd import codec
    from icm_amd import utils as U
    from icm_amd.datasets import ToTensor
    dev = "cuda:0"
    for h, w in SIZES:
        rng = np.random.default_rng(h + w)
        a = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        pads = codec.center_pads(h, w)
        OH, OW = h + pads[2] + pads[3], w + pads[0] + pads[1]
        a_dev = torch.from_numpy(a).to(dev)
        x_hat = torch.rand((1, 3, OH, OW), device=dev)

        def in_host():
            return U.pad_to_multiple(ToTensor()(a)[None].to(dev), 64)[0]

        def in_dev():
            return codec.image_u8_to_f32(torch.from_numpy(a).to(dev), pads)

        def out_host():
            t = U.crop(x_hat, pads)[0].to("cpu", torch.float32).mul(255.0).to(torch.uint8).numpy()
            return np.ascontiguousarray(t.transpose(1, 2, 0))

        def out_dev():
            img, sse = codec.image_f32_to_u8(x_hat, pads, a_dev)
            return img.cpu().numpy(), int(sse.item())

        # same results first (bit for bit), which also warms every path up
        assert torch.equal(in_host().view(torch.int32), in_dev().view(torch.int32))
        got, sse = out_dev()
        want = out_host()
        assert np.array_equal(got, want)
        d = want.astype(np.int64) - a.astype(np.int64)
        assert sse == int((d * d).sum())

        res = {"metric": "codec_image_io", "height": h, "width": w, "padded": [OH, OW]}
        k_in = events(lambda: codec.image_u8_to_f32(a_dev, pads), torch, args.iters)
        k_out = events(lambda: codec.image_f32_to_u8(x_hat, pads, a_dev), torch, args.iters)
        k_out_plain = events(lambda: codec.image_f32_to_u8(x_hat, pads), torch, args.iters)
        b_in, b_out = 3 * h * w + 12 * OH * OW, 12 * h * w + 3 * h * w + 3 * h * w
        res.update({"u8_to_f32_us": round(k_in, 2), "u8_to_f32_GBps": round(b_in / k_in / 1e3, 1),
                    "u8_to_f32_pct_of_hbm_peak": round(100.0 * b_in / (k_in * 1e-6) / HBM_PEAK, 1),
                    "f32_to_u8_sse_us": round(k_out, 2), "f32_to_u8_sse_GBps": round(b_out / k_out / 1e3, 1),
                    "f32_to_u8_sse_pct_of_hbm_peak": round(100.0 * b_out / (k_out * 1e-6) / HBM_PEAK, 1),
                    "f32_to_u8_us": round(k_out_plain, 2),
                    "note": "kernel figures include the wrapper's allocation and launch; at small sizes they measure that"})
        if not args.kernel_only:
            k_pad = events(lambda: U.pad_to_multiple(torch.empty((1, 3, h, w), device=dev), 64), torch, args.iters) \
                if pads != (0, 0, 0, 0) else 0.0
            times = {"in_host": [], "in_dev": [], "out_host": [], "out_dev": []}
            for _ in range(args.rounds):
                for name, fn in (("in_host", in_host), ("in_dev", in_dev), ("out_host", out_host), ("out_dev", out_dev)):
                    times[name].append(wall(fn, torch)[0])
            med = {k: statistics.median(v) for k, v in times.items()}
            res.update({f"{k}_wall_ms": round(v, 3) for k, v in med.items()})
            res.update({"pad2d_us": round(k_pad, 2), "in_speedup": round(med["in_host"] / med["in_dev"], 2),
                        "out_speedup": round(med["out_host"] / med["out_dev"], 2),
                        "wall_ms_rounds": {k: [round(x, 3) for x in v] for k, v in times.items()}})
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
