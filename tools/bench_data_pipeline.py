#!/usr/bin/env python
"""Feeding the training step: the DataLoader path of ``python -m icm_amd.train`` against the device-resident cache.

    (a) DataLoader(ImageFolder(Compose([RandomCrop(pad_if_needed), ToTensor()])), pin_memory) -> f32 H2D, per step:
        decode, crop, f32 conversion and collation on the host; measured with -n 0 and -n 4 workers
    (b) datasets.DeviceImageCache: the split decoded once to 8-bit on the device, then one launch of
        icm_image_batch_u8_to_f32 per step

The tool writes its own synthetic PNG folder (--images files of --src-size) into a temporary directory, first checks
that both paths return equal tensors for the same samples and the same crop draws, and prints one JSON line:
images/s of (a) per worker count (host clock around whole epochs that end in a synchronise), the cache fill time,
microseconds per ``batch()`` call (HIP events over --iters calls; includes the descriptor upload and the allocation
of the result) and per bare kernel launch, and the kernel's achieved bytes/s against the HBM peak.  Bytes are those the
algorithm needs: 3 CH CW read + 12 CH CW written per sample.

    python tools/bench_data_pipeline.py [--images 64] [--src-size 512 768] [--batch 16] [--patch 256 256]
                                        [--iters 200] [--epochs 3] [--kernel-only]

--kernel-only fills the cache and runs the kernel loop alone (the run to put under rocprofv3 --kernel-trace --stats).
"""
import argparse
import json
import os
import random
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "image-compression-for-machine_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK = 8.0e12                                    # bytes/s, specification; about 6.3e12 is achievable by a copy


def write_folder(folder, n, h, w):
    import numpy as np
    from PIL import Image
    os.makedirs(folder)
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:h, 0:w]
    for i in range(n):          # smooth ramps plus noise: PNG decode time between a flat image's and pure noise's
        base = np.stack([(yy * (i % 5 + 1) + xx * 2 + 40 * c) % 256 for c in range(3)], -1)
        a = np.clip(base + rng.integers(-12, 13, size=(h, w, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(a).save(os.path.join(folder, f"im{i:04d}.png"))


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
    return e0.elapsed_time(e1) / iters * 1e3          # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--src-size", type=int, nargs=2, default=(512, 768), metavar=("H", "W"))
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--patch", type=int, nargs=2, default=(256, 256))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--epochs", type=int, default=3, help="timed epochs of the DataLoader path per worker count")
    ap.add_argument("--workers", type=int, nargs="+", default=[0, 4])
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from torch.utils.data import DataLoader
    if not torch.cuda.is_available():
        sys.exit("bench_data_pipeline: no GPU (there is no CPU fallback)")
    from icm_amd import _lib as L
    from icm_amd import datasets as D
    dev = "cuda:0"
    ch, cw = args.patch
    B = args.batch
    with tempfile.TemporaryDirectory() as root:
        write_folder(os.path.join(root, "train"), args.images, *args.src_size)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cache = D.DeviceImageCache(root, "train", dev, 10 ** 10, num_workers=max(args.workers))
        torch.cuda.synchronize()
        fill_s = time.perf_counter() - t0
        tf = D.Compose([D.RandomCrop((ch, cw), pad_if_needed=True), D.ToTensor()])
        ds = D.ImageFolder(root, transform=tf, split="train")

        # equal tensors first: the same samples, the same crop draws
        idx = list(range(min(B, len(ds))))
        random.seed(1)
        want = torch.stack([ds[i] for i in idx]).to(dev)
        random.seed(1)
        windows = [D.crop_window("random", *cache.sizes[i], ch, cw) for i in idx]
        got = cache.batch(idx, windows, ch, cw)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "the two paths differ"

        idx = [i % len(cache) for i in range(B)]
        windows = [D.crop_window("random", *cache.sizes[i], ch, cw) for i in idx]
        out = torch.empty((B, 3, ch, cw), dtype=torch.float32, device=dev)
        desc = torch.from_numpy(D.crop_descriptors(cache.offsets, cache.sizes, idx, windows, ch, cw).view(np.uint8)).to(dev)

        def kernel():
            L.check(L.lib().icm_image_batch_u8_to_f32(cache.arena.data_ptr(), desc.data_ptr(), B, out.data_ptr(), ch, cw,
                                                      L.stream()))

        k_us = events(kernel, torch, args.iters)
        nbytes = B * ch * cw * (3 + 12)
        res = {"metric": "data_pipeline", "images": len(cache), "src_size": list(args.src_size), "batch": B,
               "patch": [ch, cw], "cache_bytes": cache.nbytes, "cache_fill_s": round(fill_s, 3),
               "cache_fill_images_per_s": round(len(cache) / fill_s, 1), "kernel_us": round(k_us, 2),
               "kernel_bytes": nbytes, "kernel_GBps": round(nbytes / k_us / 1e3, 1),
               "kernel_pct_of_hbm_peak": round(100.0 * nbytes / (k_us * 1e-6) / HBM_PEAK, 1),
               "note": "kernel_us = HIP events over back-to-back launches of a 15.7 MB working set (cache-resident)"}
        if not args.kernel_only:
            b_us = events(lambda: cache.batch(idx, windows, ch, cw), torch, args.iters)
            res.update({"batch_call_us": round(b_us, 2), "cache_images_per_s": round(B / (b_us * 1e-6), 0)})
            for nw in args.workers:
                loader = DataLoader(ds, batch_size=B, num_workers=nw, shuffle=True, pin_memory=True)
                rates = []
                for e in range(args.epochs + 1):           # the first epoch warms the workers and the page cache
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    n = 0
                    for d in loader:
                        n += len(d.to(dev, non_blocking=True))
                    torch.cuda.synchronize()
                    if e:
                        rates.append(n / (time.perf_counter() - t0))
                res[f"dataloader_n{nw}_images_per_s"] = round(sorted(rates)[len(rates) // 2], 1)
                res[f"dataloader_n{nw}_rounds"] = [round(r, 1) for r in rates]
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
