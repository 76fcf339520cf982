#!/usr/bin/env python
"""What quality-map training costs: the ``cnn`` training step at batch 16 x 256 x 256, eager, plain, with
``Trainer(qstep_range=(-16, 32))`` and with ``qmap_rects=2`` on top, in one process on one GPU.

The map step makes one more draw, paints the maps with one small launch and swaps the per-image kernels of the
``qstep_range`` step (two element-wise kernels per slice, the loss pair) for their per-position / per-cell forms: the
same operand bytes plus a map byte per position.  It should cost what the per-image step costs.  The margin a
difference is read against is the run-to-run spread of one and the same code, so the three steps are timed in windows
that alternate:

    plain_ms / stepped_ms / map_ms   median over --rounds windows of --steps steps each (host clock around a device
                                     synchronise)
    *_spread_ms                      max - min of that step's windows
    map_minus_stepped_ms             map_ms - stepped_ms

Three trainers, randomly initialised (seeded), the same batch; each is warmed for --warmup steps first.  On a commit
without ``qmap_rects`` only the first two are timed: run it there and here, same day, same machine.  ``--kernels``
prints instead the per-kernel device times of the kernels that differ between the per-image and the map step, from HIP
events around single launches on training-sized operands.  Prints one JSON line.

    python tools/bench_qmap_train.py [--steps 10] [--warmup 4] [--rounds 5] [--kernels]
"""
import argparse
import inspect
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "image-compression-for-machine_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_qtrain import BATCH, RANGE, SIDE, window  # noqa: E402

RECTS = 2


def step_times(args, torch):
    from icm_amd.trainer import Trainer
    from icm_amd.zoo import models
    has_maps = "qmap_rects" in inspect.signature(Trainer.__init__).parameters
    torch.manual_seed(0)
    x = torch.rand(BATCH, 3, SIDE, SIDE, device="cuda")
    kinds = {"plain": {}, "stepped": {"qstep_range": RANGE}}
    if has_maps:
        kinds["map"] = {"qstep_range": RANGE, "qmap_rects": RECTS}
    trainers = {}
    for kind, kw in kinds.items():
        torch.manual_seed(1)
        trainers[kind] = Trainer(models["cnn"](), device="cuda:0", seed=3, **kw)
        window(torch, trainers[kind], x, args.warmup)
    times = {kind: [] for kind in kinds}
    for _ in range(args.rounds):
        for kind in kinds:                       # alternate: all see the same minutes of the shared machine
            times[kind].append(window(torch, trainers[kind], x, args.steps))
    out = {"bench": "qmap_train_step", "batch": BATCH, "side": SIDE, "steps": args.steps, "rounds": args.rounds,
           "qstep_range": list(RANGE)}
    for kind, ts in times.items():
        out[kind + "_ms"] = round(statistics.median(ts), 3)
        out[kind + "_windows_ms"] = [round(t, 3) for t in ts]
        out[kind + "_spread_ms"] = round(max(ts) - min(ts), 3)
    if has_maps:
        out.update(qmap_rects=RECTS, map_minus_stepped_ms=round(out["map_ms"] - out["stepped_ms"], 3))
    return out


def kernel_times(args, torch):
    """microseconds per launch: the Gaussian step of one slice ([16, 32, 16 x 16] out of [16, 320, ...] buffers, the
    slice loop's operands) and the loss pair on the 16 x 3 x 256 x 256 batch, per image against per position / per
    cell; and the painter on the step's 16 maps of 16 x 16 cells"""
    from icm_amd import _lib as L
    from icm_amd import engine as E
    from icm_amd.losses import qmap_lmbda_table
    from icm_amd.trainer import qmap_rects_of, qstep_tables
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
    base = (rows + RANGE[0]).to(torch.int8).to(dev)
    rects = qmap_rects_of(torch.rand(B, RECTS, 5), h, h, *RANGE).to(dev).contiguous()
    qmap = torch.empty((B, h, h), dtype=torch.int8, device=dev)
    L.check(lib.icm_qmap_paint(L.ptr(base), L.ptr(rects), RECTS, L.ptr(qmap), B, h, h, st), "qmap_paint")
    table, lam_tab = E.qmap_step_table(torch.device(dev)), qmap_lmbda_table(0.0067).to(dev)
    a = lambda t: (L.ptr(sl(t)), L.bs(sl(t)))
    x = torch.rand(B, 3, SIDE, SIDE, device=dev)
    xh = (x + 0.05 * torch.randn_like(x)).contiguous()
    ly = torch.rand(B * M * h * h, device=dev).clamp_min(1e-9)
    lz = torch.rand(B * 192 * (h // 4) ** 2, device=dev).clamp_min(1e-9)
    out, ws = torch.empty(5, device=dev), torch.empty(L.REDUCE_WS_FLOATS, device=dev)
    dxh, dly, dlz = torch.empty_like(x), torch.empty_like(ly), torch.empty_like(lz)
    npix, per = B * SIDE * SIDE, 3 * SIDE * SIDE
    gc = (B, c, h * h, 0.11, 1e-9)
    lik = (L.ptr(ly), ly.numel(), L.ptr(lz), lz.numel(), npix)
    calls = {
        "gc_qs_fwd": lambda: lib.icm_gc_likelihood_ste_qs_fwd(*a(Y), *a(MU), *a(SC), *a(NZ), L.ptr(steps), *a(LIK), *a(YH),
                                                              0, 0, *gc, st),
        "gc_qm_fwd": lambda: lib.icm_gc_likelihood_ste_qm_fwd(*a(Y), *a(MU), *a(SC), *a(NZ), L.ptr(qmap), L.ptr(table),
                                                              *a(LIK), *a(YH), 0, 0, *gc, st),
        "gc_qs_bwd": lambda: lib.icm_gc_likelihood_ste_qs_bwd(*a(Y), *a(MU), *a(SC), *a(NZ), L.ptr(steps), *a(DL), *a(YH),
                                                              *a(DY), *a(DMU), *a(DSC), *gc, 1, st),
        "gc_qm_bwd": lambda: lib.icm_gc_likelihood_ste_qm_bwd(*a(Y), *a(MU), *a(SC), *a(NZ), L.ptr(qmap), L.ptr(table),
                                                              *a(DL), *a(YH), *a(DY), *a(DMU), *a(DSC), *gc, 1, st),
        "rd_loss_w_fwd": lambda: lib.icm_rd_loss_w_fwd(L.ptr(x), L.ptr(xh), B, per, *lik, L.ptr(lam), L.ptr(out),
                                                       L.ptr(ws), st),
        "rd_loss_m_fwd": lambda: lib.icm_rd_loss_m_fwd(L.ptr(x), L.ptr(xh), B, 3, SIDE, SIDE, 16, L.ptr(qmap),
                                                       L.ptr(lam_tab), *lik, L.ptr(out), L.ptr(ws), st),
        "rd_loss_w_bwd": lambda: lib.icm_rd_loss_w_bwd(L.ptr(x), L.ptr(xh), B, per, *lik, L.ptr(lam), 1.0, L.ptr(dxh),
                                                       L.ptr(dly), L.ptr(dlz), st),
        "rd_loss_m_bwd": lambda: lib.icm_rd_loss_m_bwd(L.ptr(x), L.ptr(xh), B, 3, SIDE, SIDE, 16, L.ptr(qmap),
                                                       L.ptr(lam_tab), *lik, 1.0, L.ptr(dxh), L.ptr(dly), L.ptr(dlz), st),
        "qmap_paint": lambda: lib.icm_qmap_paint(L.ptr(base), L.ptr(rects), RECTS, L.ptr(qmap), B, h, h, st),
    }
    res = {"bench": "qmap_train_kernels", "iters": args.iters}
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
