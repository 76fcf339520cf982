#!/usr/bin/env python
"""What variable-rate training costs: the ``cnn`` training step at batch 16 x 256 x 256, eager, with and without
``Trainer(qstep_range=(-16, 32))``, in one process on one GPU.

The stepped step draws one more tensor, gathers twice from two small device tables and swaps two element-wise kernels
per slice and the loss pair for their stepped / weighted forms; it should cost what the plain step costs.  The margin a
difference is read against is the plain step's own run-to-run spread, so the plain step is timed in several windows
that alternate with the stepped one's:

    plain_ms / stepped_ms   median over --rounds windows of --steps steps each (host clock around a device synchronise)
    plain_spread_ms         max - min of the plain windows: the run-to-run spread of the SAME code in this session
    delta_ms                stepped_ms - plain_ms

Two trainers, randomly initialised (seeded), the same batch; each is warmed for --warmup steps first.  Run it on the
parent commit (where ``qstep_range`` does not exist: only the plain figures are printed) and on this one, same day, same
machine.  ``--kernels`` prints instead the per-kernel device times of the kernels that differ between the two steps,
from HIP events around single launches on training-sized operands.  Prints one JSON line.

    python tools/bench_qtrain.py [--steps 10] [--warmup 4] [--rounds 5] [--kernels]
"""
import argparse
import inspect
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "image-compression-for-machine_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

BATCH, SIDE, RANGE = 16, 256, (-16, 32)


def window(torch, tr, x, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.step(x)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def step_times(args, torch):
    from icm_amd.trainer import Trainer
    from icm_amd.zoo import models
    has_range = "qstep_range" in inspect.signature(Trainer.__init__).parameters
    torch.manual_seed(0)
    x = torch.rand(BATCH, 3, SIDE, SIDE, device="cuda")
    kinds = {"plain": {}}
    if has_range:
        kinds["stepped"] = {"qstep_range": RANGE}
    trainers = {}
    for kind, kw in kinds.items():
        torch.manual_seed(1)
        trainers[kind] = Trainer(models["cnn"](), device="cuda:0", seed=3, **kw)
        window(torch, trainers[kind], x, args.warmup)
    times = {kind: [] for kind in kinds}
    for _ in range(args.rounds):
        for kind in kinds:                       # alternate: both see the same minutes of the shared machine
            times[kind].append(window(torch, trainers[kind], x, args.steps))
    out = {"bench": "qtrain_step", "batch": BATCH, "side": SIDE, "steps": args.steps, "rounds": args.rounds,
           "plain_ms": round(statistics.median(times["plain"]), 3),
           "plain_windows_ms": [round(t, 3) for t in times["plain"]],
           "plain_spread_ms": round(max(times["plain"]) - min(times["plain"]), 3),
           "plain_img_s": round(BATCH / statistics.median(times["plain"]) * 1e3, 1)}
    if has_range:
        out.update(qstep_range=list(RANGE), stepped_ms=round(statistics.median(times["stepped"]), 3),
                   stepped_windows_ms=[round(t, 3) for t in times["stepped"]],
                   delta_ms=round(statistics.median(times["stepped"]) - statistics.median(times["plain"]), 3))
    return out


def kernel_times(args, torch):
    """microseconds per launch: the Gaussian step of one slice ([16, 32, 16 x 16] out of [16, 320, ...] buffers, the
    slice loop's operands) and the loss pair on the 16 x 3 x 256 x 256 batch, plain against stepped / weighted"""
    from icm_amd import _lib as L
    from icm_amd.trainer import qstep_tables
    lib, st, dev = L.lib(), L.stream(), "cuda:0"
    B, M, c, h = BATCH, 320, 32, SIDE // 16
    torch.manual_seed(0)
    wide = lambda: torch.randn(B, M, h, h, device=dev)
    Y, MU, NZ, LIK, YH, DL, DY, DMU, DSC = (wide() for _ in range(9))
    SC = wide().abs() + 0.05
    sl = lambda t: t[:, 64:64 + c]
    steps_t, lam_t = qstep_tables(RANGE, 0.0067)
    rows = torch.randint(0, lam_t.numel(), (B,))
    steps, lam = steps_t[rows].to(dev).contiguous(), lam_t[rows].to(dev).contiguous()
    a = lambda t: (L.ptr(sl(t)), L.bs(sl(t)))
    x = torch.rand(B, 3, SIDE, SIDE, device=dev)
    xh = (x + 0.05 * torch.randn_like(x)).contiguous()
    ly = torch.rand(B * M * h * h, device=dev).clamp_min(1e-9)
    lz = torch.rand(B * 192 * (h // 4) ** 2, device=dev).clamp_min(1e-9)
    out, ws = torch.empty(5, device=dev), torch.empty(L.REDUCE_WS_FLOATS, device=dev)
    dxh, dly, dlz = torch.empty_like(x), torch.empty_like(ly), torch.empty_like(lz)
    npix, per = B * SIDE * SIDE, 3 * SIDE * SIDE
    gc = (B, c, h * h, 0.11, 1e-9)
    calls = {
        "gc_fwd": lambda: lib.icm_gc_likelihood_ste_fwd(*a(Y), *a(MU), *a(SC), *a(NZ), *a(LIK), *a(YH), 0, 0, *gc, st),
        "gc_qs_fwd": lambda: lib.icm_gc_likelihood_ste_qs_fwd(*a(Y), *a(MU), *a(SC), *a(NZ), L.ptr(steps), *a(LIK), *a(YH),
                                                              0, 0, *gc, st),
        "gc_bwd": lambda: lib.icm_gc_likelihood_ste_bwd(*a(Y), *a(MU), *a(SC), *a(NZ), *a(DL), *a(YH), *a(DY), *a(DMU),
                                                        *a(DSC), *gc, 1, st),
        "gc_qs_bwd": lambda: lib.icm_gc_likelihood_ste_qs_bwd(*a(Y), *a(MU), *a(SC), *a(NZ), L.ptr(steps), *a(DL), *a(YH),
                                                              *a(DY), *a(DMU), *a(DSC), *gc, 1, st),
        "rd_loss_fwd": lambda: lib.icm_rd_loss_fwd(L.ptr(x), L.ptr(xh), x.numel(), L.ptr(ly), ly.numel(), L.ptr(lz),
                                                   lz.numel(), npix, 0.0067, L.ptr(out), L.ptr(ws), st),
        "rd_loss_w_fwd": lambda: lib.icm_rd_loss_w_fwd(L.ptr(x), L.ptr(xh), B, per, L.ptr(ly), ly.numel(), L.ptr(lz),
                                                       lz.numel(), npix, L.ptr(lam), L.ptr(out), L.ptr(ws), st),
        "rd_loss_bwd": lambda: lib.icm_rd_loss_bwd(L.ptr(x), L.ptr(xh), x.numel(), L.ptr(ly), ly.numel(), L.ptr(lz),
                                                   lz.numel(), npix, 0.0067, 1.0, L.ptr(dxh), L.ptr(dly), L.ptr(dlz), st),
        "rd_loss_w_bwd": lambda: lib.icm_rd_loss_w_bwd(L.ptr(x), L.ptr(xh), B, per, L.ptr(ly), ly.numel(), L.ptr(lz),
                                                       lz.numel(), npix, L.ptr(lam), 1.0, L.ptr(dxh), L.ptr(dly),
                                                       L.ptr(dlz), st),
    }
    res = {"bench": "qtrain_kernels", "iters": args.iters}
    for name, fn in calls.items():
        for _ in range(5):
            L.check(fn(), name)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        res[name + "_us"] = round(e0.elapsed_time(e1) / args.iters * 1e3, 2)
    return res


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--kernels", action="store_true", help="per-kernel times of the kernels that differ, not the step")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        print("Error: no GPU (a time measured elsewhere says nothing about the MI355X).", file=sys.stderr)
        return 3
    print(json.dumps(kernel_times(args, torch) if args.kernels else step_times(args, torch)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
