#!/usr/bin/env python
"""What AQ-map training costs: the ``cnn`` training step at batch 16 x 256 x 256, eager, with
``Trainer(qstep_range=(-16, 32), qmap_rects=1)`` (the rectangle step, whose launches this feature leaves alone: the
baseline) and with ``qmap_aq=(-2, 2)`` on top, in one process on one GPU.

The AQ step makes one more draw ([B] strengths) and replaces the painter's launch by the two of ``icm_qmap_aq``: one
pass over the batch (3 MB) and one small workgroup per image.  Everything downstream is the map path of the baseline.
The margin a difference is read against is the run-to-run spread of one and the same code, so the two steps are timed
in windows that alternate:

    rects_ms / aq_ms          median over --rounds windows of --steps steps each (host clock around a device synchronise)
    *_spread_ms               max - min of that step's windows
    aq_minus_rects_ms         aq_ms - rects_ms

Two trainers, randomly initialised (seeded), the same batch; each is warmed for --warmup steps first.

``--kernels`` launches ``icm_qmap_aq`` alone, --iters times on a training-sized batch, and reports the pair's time per
call from HIP events.  Run under a kernel trace it leaves the two kernels' own times there:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_aq_train.py --kernels
    python tools/bench_aq_train.py --trace DIR          # the two kernels' rows of the kernel_stats.csv under DIR

Prints one JSON line.

    python tools/bench_aq_train.py [--steps 10] [--warmup 4] [--rounds 5] [--kernels] [--trace DIR]
"""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "image-compression-for-machine_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_qtrain import BATCH, RANGE, SIDE, window  # noqa: E402

RECTS = 1
AQ = (-2.0, 2.0)
KERNELS = ("qmap_aq_activity_kernel", "qmap_aq_map_kernel")


def step_times(args, torch):
    from icm_amd.trainer import Trainer
    from icm_amd.zoo import models
    torch.manual_seed(0)
    x = torch.rand(BATCH, 3, SIDE, SIDE, device="cuda")
    kinds = {"rects": {"qstep_range": RANGE, "qmap_rects": RECTS},
             "aq": {"qstep_range": RANGE, "qmap_rects": RECTS, "qmap_aq": AQ}}
    trainers = {}
    for kind, kw in kinds.items():
        torch.manual_seed(1)
        trainers[kind] = Trainer(models["cnn"](), device="cuda:0", seed=3, **kw)
        window(torch, trainers[kind], x, args.warmup)
    times = {kind: [] for kind in kinds}
    for _ in range(args.rounds):
        for kind in kinds:                       # alternate: both see the same minutes of the shared machine
            times[kind].append(window(torch, trainers[kind], x, args.steps))
    out = {"bench": "aq_train_step", "batch": BATCH, "side": SIDE, "steps": args.steps, "rounds": args.rounds,
           "qstep_range": list(RANGE), "qmap_rects": RECTS, "qmap_aq": list(AQ)}
    for kind, ts in times.items():
        out[kind + "_ms"] = round(statistics.median(ts), 3)
        out[kind + "_windows_ms"] = [round(t, 3) for t in ts]
        out[kind + "_spread_ms"] = round(max(ts) - min(ts), 3)
    out["aq_minus_rects_ms"] = round(out["aq_ms"] - out["rects_ms"], 3)
    return out


def kernel_times(args, torch):
    """microseconds per call of icm_qmap_aq (both launches) on the step's 16 x 3 x 256 x 256 batch with one rectangle
    per image, from HIP events; under rocprofv3 the trace holds the two kernels apart"""
    from icm_amd import engine as E
    from icm_amd.trainer import qmap_rects_of
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    x = torch.rand(BATCH, 3, SIDE, SIDE, device=dev)
    h = SIDE // 16
    base = torch.randint(RANGE[0], RANGE[1] + 1, (BATCH,)).to(torch.int8).to(dev)
    strength = (AQ[0] + (AQ[1] - AQ[0]) * torch.rand(BATCH)).to(dev)
    rects = qmap_rects_of(torch.rand(BATCH, RECTS, 5), h, h, *RANGE).to(dev).contiguous()
    out = torch.empty((BATCH, h, h), dtype=torch.int8, device=dev)
    ref = torch.empty((BATCH,), dtype=torch.float64, device=dev)
    ws = E.qmap_aq_workspace(BATCH, SIDE, SIDE, dev)
    fn = lambda: E.qmap_aq(x, base, strength, rects, out=out, ref=ref, ws=ws)   # noqa: E731
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(args.iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return {"bench": "aq_train_kernels", "iters": args.iters, "batch": BATCH, "side": SIDE,
            "qmap_aq_pair_us": round(e0.elapsed_time(e1) / args.iters * 1e3, 2), "bytes_read": x.numel() * 4}


def trace_times(root):
    """the two kernels' rows of the kernel_stats.csv files below ``root`` (rocprofv3 --kernel-trace --stats)"""
    res = {"bench": "aq_train_kernel_trace"}
    for d, _, files in os.walk(root):
        for f in files:
            if not f.endswith("kernel_stats.csv"):
                continue
            for r in csv.DictReader(open(os.path.join(d, f))):
                for k in KERNELS:
                    if k in r["Name"]:
                        res[k] = {"calls": int(r["Calls"]),
                                  "avg_us": round(float(r["TotalDurationNs"]) / int(r["Calls"]) / 1e3, 2)}
                        for col in ("MinNs", "MaxNs"):
                            if r.get(col):
                                res[k][col[:3].lower() + "_us"] = round(float(r[col]) / 1e3, 2)
    missing = [k for k in KERNELS if k not in res]
    if missing:
        raise SystemExit(f"no kernel_stats.csv row under {root} for {missing}")
    return res


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--kernels", action="store_true", help="icm_qmap_aq alone, not the step")
    ap.add_argument("--trace", type=str, default=None, metavar="DIR", help="read a kernel trace's statistics instead")
    args = ap.parse_args(argv)
    if args.trace:
        print(json.dumps(trace_times(args.trace)))
        return 0
    import torch
    if not torch.cuda.is_available():
        print("Error: no GPU (a time measured elsewhere says nothing about the MI355X).", file=sys.stderr)
        return 3
    print(json.dumps(kernel_times(args, torch) if args.kernels else step_times(args, torch)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
