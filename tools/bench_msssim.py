#!/usr/bin/env python
"""MS-SSIM cost on the flagship workload: the `cnn` training step at batch 16, 256x256 (bench.py's workload) with
Trainer(metric="mse") against Trainer(metric="ms-ssim"), interleaved A/B in one process, plus the ms_ssim forward +
backward alone (HIP events).  Prints one JSON line.

    python tools/bench_msssim.py [--rounds 5] [--steps 10] [--kernel-only]

--kernel-only runs only the isolated forward + backward (the run to put under rocprofv3 --kernel-trace --stats).
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

BATCH = 16


def kernel_alone(torch, iters=50):
    from icm_amd.ops import ms_ssim
    g = torch.Generator(device="cuda").manual_seed(1234)
    t = torch.rand(BATCH, 3, 256, 256, generator=g, device="cuda")
    x = (t + 0.05 * torch.randn(t.shape, generator=g, device="cuda")).clamp(0, 1).requires_grad_(True)
    for _ in range(5):
        ms_ssim(x, t).backward()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        x.grad = None
        ms_ssim(x, t).backward()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_msssim: no GPU (there is no CPU fallback)")
    res = {"metric": "ms_ssim_step_overhead", "batch": BATCH,
           "ms_ssim_fwd_bwd_ms": round(kernel_alone(torch), 4)}
    if not args.kernel_only:
        from icm_amd.trainer import Trainer
        from icm_amd.zoo import models
        g = torch.Generator(device="cuda").manual_seed(1234)
        x = torch.rand(BATCH, 3, 256, 256, generator=g, device="cuda")
        trainers = {}
        for metric in ("mse", "ms-ssim"):
            torch.manual_seed(0)
            trainers[metric] = Trainer(models["cnn"](), lmbda=0.0067, device="cuda:0", seed=4321, metric=metric)
        for tr in trainers.values():
            for _ in range(4):
                tr.step(x)
        torch.cuda.synchronize()
        times = {m: [] for m in trainers}
        for _ in range(args.rounds):
            for m, tr in trainers.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    tr.step(x)
                torch.cuda.synchronize()
                times[m].append((time.perf_counter() - t0) / args.steps * 1e3)
        med = {m: statistics.median(v) for m, v in times.items()}
        res.update({"mse_step_ms": round(med["mse"], 3), "ms_ssim_step_ms": round(med["ms-ssim"], 3),
                    "mse_step_ms_rounds": [round(v, 3) for v in times["mse"]],
                    "ms_ssim_step_ms_rounds": [round(v, 3) for v in times["ms-ssim"]],
                    "delta_ms": round(med["ms-ssim"] - med["mse"], 3),
                    "delta_pct": round(100.0 * (med["ms-ssim"] - med["mse"]) / med["mse"], 2)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
