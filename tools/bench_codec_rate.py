#!/usr/bin/env python
"""The codec's quantiser step and its rate search on one 2048x3072 synthetic image, randomly initialised ``cnn``.

    step_vs_plain   encode wall time at qstep 0 (the path without a step: likelihood + quantise + index launches per
                    slice) and at qstep 8 (one fused launch per slice), alternated within one run, median of --rounds.
    slice_kernels   the per-slice encoder work alone on one slice of this image ([1, 32, 128 x 192] out of the wide
                    buffers): today's three launches (and the copy ``build_indexes`` makes of a strided scale) against
                    the one fused launch, microseconds per slice from HIP events over --iters repetitions.
    rate_points     file bytes and PSNR of the decoded 8-bit image at qstep -16, -8, 0, 8, 16, 24, 32.
    target_bpp      encode wall time and probe count of an encode to size at two budgets, the size of the qstep -8
                    file and the middle between it and the qstep 0 file (where this model's sizes still move; a budget
                    the coarsest step misses is reported as such), with the wall time of the analysis transform alone
                    and of one probe (``compress_latent`` + container) next to them.
    roi_encode      encode wall time at qstep 8 against the same encode with one centred region of interest (a quarter
                    of the image at offset -16: a quality map, the map-reading kernel per slice), alternated, with both
                    file sizes.

    rdoq_kernel     the encoder's rate-distortion optimised quantisation kernel (``icm_gc_code_rdo``) on that same
                    slice against the scalar fused kernel (``icm_gc_code_q``, k = 8) in the same run, the forms
                    alternated: with the scalar pair, with the centred region's map and with the busy map, at weight
                    0.25, microseconds per slice.
    rdoq_points     file bytes and latent squared error sum((y - y_hat)^2) without RDOQ and at the weights 4 and
                    0.25, at qstep -16 and -8 (``analysis()`` once, ``compress_latent`` with ``_debug`` per point).

``slice_kernels`` also times the map-reading fused kernel (``icm_gc_code_qmap``) against the scalar one
(``icm_gc_code_q``) on the same operands in the same run, with the map of that centred region and with a map that
changes its step at every position.

Every part runs for both coders, warmed, with the host clock around a device synchronise.  The model is randomly
initialised (seeded): bytes and PSNR exercise the mechanism and say nothing about a trained codec's rate-distortion.
Prints one JSON line per part and coder.

    python tools/bench_codec_rate.py [--rounds 5] [--iters 100] [--coder {host,lanes,both}] [--parts a,b,...]
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

H, W = 2048, 3072
RATE_POINTS = (-16, -8, 0, 8, 16, 24, 32)
PARTS = ("slice_kernels", "step_vs_plain", "rate_points", "target_bpp", "roi_encode", "rdoq_kernel", "rdoq_points")
RDOQ_WEIGHTS = (4.0, 0.25)
RDOQ_STEPS = (-16, -8)
ROI = (H // 4, W // 4, H // 2, W // 2, -16)        # the centred quarter of the image, two octaves finer


def synthetic(np, h, w, seed):
    """gradients, a coarse texture and a little noise: 8-bit [h, w, 3] (the image of tools/bench_codec_tiles.py)"""
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


def slice_kernels(args, torch, np):
    from icm_amd import _lib as L
    from icm_amd import codec
    from icm_amd import engine as E
    from icm_amd.zoo import models
    model = models["cnn"]().to("cuda:0").eval()
    model.update(force=True)
    gc = model.gaussian_conditional
    g = torch.Generator(device="cuda:0").manual_seed(0)
    N, M, c, h, w = 1, 320, 32, H // 16, W // 16
    Y, MU, YP, LIK = (torch.randn((N, M, h, w), generator=g, device="cuda:0") for _ in range(4))
    SC = torch.rand((N, M, h, w), generator=g, device="cuda:0") * 2
    s1 = slice(64, 96)
    tape = E.Tape(need_grad=False)
    args_ = (L.stream(), Y[:, s1], MU[:, s1], SC[:, s1], YP[:, s1])
    q0, q8 = E.Quantiser(gc), E.Quantiser(gc, 8)

    def plain():
        E.gc_likelihood_ste(tape, Y[:, s1], MU[:, s1], SC[:, s1], None, LIK[:, s1], YP[:, s1])
        return q0.code(*args_)

    def fused():
        return q8.code(*args_)

    roi = torch.from_numpy(codec.roi_map(H, W, codec.center_pads(H, W), 8, [ROI])).to("cuda:0")
    busy = torch.from_numpy(np.array([-16, -3, 0, 5, 8, 32], dtype=np.int8)[(5 * np.arange(h * w)) % 6].reshape(h, w))
    busy = busy.to("cuda:0")

    def mapped(qmap):
        q = E.Quantiser(gc, 0, qmap)
        return lambda: q.code(*args_)

    res = {"metric": "slice_kernels", "slice": [N, c, h, w], "iters": args.iters}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, fn in (("plain_three_launches_us", plain), ("fused_one_launch_us", fused), ("plain_again_us", plain),
                     ("fused_again_us", fused), ("map_roi_us", mapped(roi)), ("fused_third_us", fused),
                     ("map_busy_us", mapped(busy)), ("fused_fourth_us", fused), ("map_roi_again_us", mapped(roi)),
                     ("map_busy_again_us", mapped(busy))):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        res[name] = round(e0.elapsed_time(e1) / args.iters * 1e3, 2)
    print(json.dumps(res), flush=True)


def rdoq_kernel(args, torch, np):
    """``icm_gc_code_rdo`` against ``icm_gc_code_q`` on the slice of ``slice_kernels``, the forms alternated"""
    from icm_amd import _lib as L
    from icm_amd import codec
    from icm_amd import engine as E
    from icm_amd.zoo import models
    model = models["cnn"]().to("cuda:0").eval()
    model.update(force=True)
    gc = model.gaussian_conditional
    g = torch.Generator(device="cuda:0").manual_seed(0)
    N, M, c, h, w = 1, 320, 32, H // 16, W // 16
    Y, MU, YP = (torch.randn((N, M, h, w), generator=g, device="cuda:0") for _ in range(3))
    SC = torch.rand((N, M, h, w), generator=g, device="cuda:0") * 2
    s1 = slice(64, 96)
    args_ = (L.stream(), Y[:, s1], MU[:, s1], SC[:, s1], YP[:, s1])
    roi = torch.from_numpy(codec.roi_map(H, W, codec.center_pads(H, W), 8, [ROI])).to("cuda:0")
    busy = torch.from_numpy(np.array([-16, -3, 0, 5, 8, 32], dtype=np.int8)[(5 * np.arange(h * w)) % 6].reshape(h, w))
    busy = busy.to("cuda:0")
    weight = RDOQ_WEIGHTS[1]
    qs = {"scalar": E.Quantiser(gc, 8), "rdo": E.Quantiser(gc, 8, rdoq=weight),
          "rdo_roi": E.Quantiser(gc, 0, roi, rdoq=weight), "rdo_busy": E.Quantiser(gc, 0, busy, rdoq=weight),
          "rdo_huge": E.Quantiser(gc, 8, rdoq=1e30)}
    sym0, sym1 = qs["scalar"].code(*args_)[0], qs["rdo"].code(*args_)[0]
    res = {"metric": "rdoq_kernel", "slice": [N, c, h, w], "iters": args.iters, "weight": weight,
           "symbols_moved": int((sym0 != sym1).sum().item()), "symbols_nonzero": int((sym0 != 0).sum().item())}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    order = ("scalar", "rdo", "scalar", "rdo", "scalar", "rdo_roi", "scalar", "rdo_busy", "scalar", "rdo_huge", "scalar",
             "rdo", "rdo_roi", "rdo_busy")
    for name in order:
        fn = (lambda q: lambda: q.code(*args_))(qs[name])
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        res.setdefault(name + "_us", []).append(round(e0.elapsed_time(e1) / args.iters * 1e3, 2))
    print(json.dumps(res), flush=True)


def rdoq_points(args, coder, torch, np, codec, B, model, a, base):
    """bytes and latent squared error with and without RDOQ: the mechanism on a randomly initialised model"""
    pads = codec.center_pads(H, W)
    y = model.analysis(codec.image_u8_to_f32(torch.from_numpy(a).to("cuda:0"), pads))
    arch, fp = codec.arch_of(model), B.fingerprint(model)
    pts = []
    for k in RDOQ_STEPS:
        for weight in (None,) + RDOQ_WEIGHTS:
            d = {}
            enc = model.compress_latent(y, _debug=d, coder=coder, qstep=k, **({} if weight is None else {"rdoq": weight}))
            data = codec._pack_one(arch, fp, H, W, pads, enc, coder)
            sse = float(((y.double() - d["y_hat"].double()) ** 2).sum().item())
            pts.append({"qstep": k, "rdoq": weight, "bytes": len(data), "latent_sse": round(sse, 1),
                        "symbols_nonzero": int((d["symbols"] != 0).sum())})
    print(json.dumps({"metric": "rdoq_points", **base, "latent_elements": int(y.numel()), "points": pts}), flush=True)


def run(args, coder, torch, np, codec, B):
    from icm_amd.zoo import models
    torch.manual_seed(0)
    model = models["cnn"]().to("cuda:0").eval()
    model.update(force=True)
    a = synthetic(np, H, W, seed=1)
    base = {"coder": coder, "height": H, "width": W, "model": "cnn, randomly initialised (seed 0)", "rounds": args.rounds}

    def encode(**kw):
        return codec.encode_image_info(model, a, coder=coder, **kw)

    if "rdoq_points" in args.parts:
        rdoq_points(args, coder, torch, np, codec, B, model, a, base)

    # ---- (d) one centred region of interest against the scalar step, alternated
    if "roi_encode" in args.parts:
        kws = {"scalar": dict(qstep=8), "roi": dict(qstep=8, roi=[ROI])}
        for kw in kws.values():
            encode(**kw)
        ts = {name: [] for name in kws}
        for _ in range(args.rounds):
            for name, kw in kws.items():
                ts[name].append(wall(lambda: encode(**kw), torch)[0])
        out = {name: encode(**kw) for name, kw in kws.items()}
        print(json.dumps({"metric": "roi_encode", **base, "roi": list(ROI),
                          "qstep8_encode_s": round(statistics.median(ts["scalar"]), 4),
                          "qstep8_roi_encode_s": round(statistics.median(ts["roi"]), 4),
                          "qstep8_all_s": [round(t, 4) for t in ts["scalar"]],
                          "qstep8_roi_all_s": [round(t, 4) for t in ts["roi"]],
                          "qstep8_bytes": len(out["scalar"][0]), "qstep8_roi_bytes": len(out["roi"][0]),
                          "roi_cells": out["roi"][1]["roi_cells"], "qmap_range": out["roi"][1]["qmap_range"]}),
              flush=True)
    if not {"step_vs_plain", "rate_points", "target_bpp"} & set(args.parts):
        return

    # ---- (a) the fused launch against today's three, alternated
    for k in (0, 8):
        encode(qstep=k)
    ts = {0: [], 8: []}
    for _ in range(args.rounds):
        for k in (0, 8):
            ts[k].append(wall(lambda: encode(qstep=k), torch)[0])
    plain = len(encode(qstep=0)[0])
    print(json.dumps({"metric": "step_vs_plain", **base, "qstep0_encode_s": round(statistics.median(ts[0]), 4),
                      "qstep8_encode_s": round(statistics.median(ts[8]), 4),
                      "qstep0_all_s": [round(t, 4) for t in ts[0]], "qstep8_all_s": [round(t, 4) for t in ts[8]]}),
          flush=True)

    # ---- (c) the rate points of one checkpoint
    pts = []
    for k in RATE_POINTS:
        data, _ = encode(qstep=k)
        _, info = codec.decode_image(model, data, reference=a)
        assert info["qstep"] == k
        pts.append({"qstep": k, "step": B.step_of(k)[0], "bytes": len(data), "bpp": round(info["bpp"], 5),
                    "psnr": round(info["psnr"], 4)})
    print(json.dumps({"metric": "rate_points", **base, "points": pts}), flush=True)
    sizes = {p_["qstep"]: p_["bytes"] for p_ in pts}

    # ---- (b) encode to size
    pads = codec.center_pads(H, W)
    u8 = torch.from_numpy(a).to("cuda:0")
    x = codec.image_u8_to_f32(u8, pads)
    y = model.analysis(x)
    t_ana = statistics.median(wall(lambda: model.analysis(x), torch)[0] for _ in range(args.rounds))
    arch, fp = codec.arch_of(model), B.fingerprint(model)
    t_probe = statistics.median(
        wall(lambda: codec._pack_one(arch, fp, H, W, pads, model.compress_latent(y, coder=coder, qstep=8), coder), torch)[0]
        for _ in range(args.rounds))
    res = {"metric": "target_bpp", **base, "qstep0_bytes": plain, "analysis_s": round(t_ana, 4),
           "one_probe_s": round(t_probe, 4), "budgets": []}
    for budget in (sizes[-8], (sizes[-8] + sizes[0]) // 2):
        bpp = 8.0 * (budget + 0.5) / (H * W)
        if sizes[B.QSTEP_MAX] > budget:
            res["budgets"].append({"target_bpp": round(bpp, 5), "budget_bytes": budget, "result": "out of reach: the "
                                   f"file at qstep {B.QSTEP_MAX} has {sizes[B.QSTEP_MAX]} bytes"})
            continue
        encode(max_bytes=budget)
        t = []
        for _ in range(args.rounds):
            dt, (data, found) = wall(lambda: encode(max_bytes=budget), torch)
            t.append(dt)
        res["budgets"].append({"target_bpp": round(bpp, 5), "budget_bytes": budget, "bytes": len(data), **found,
                               "encode_s": round(statistics.median(t), 4)})
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--coder", default="both", choices=["host", "lanes", "both"])
    ap.add_argument("--parts", default=",".join(PARTS),
                    help=f"comma-separated parts to run, of {', '.join(PARTS)} (step_vs_plain, rate_points and "
                         f"target_bpp build on one another and run together)")
    args = ap.parse_args()
    args.parts = [p for p in args.parts.split(",") if p]
    if set(args.parts) - set(PARTS):
        ap.error(f"unknown part in --parts; choose from {', '.join(PARTS)}")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_codec_rate: no GPU (there is no CPU fallback)")
    from icm_amd import bitstream as B
    from icm_amd import codec
    if "slice_kernels" in args.parts:
        slice_kernels(args, torch, np)
    if "rdoq_kernel" in args.parts:
        rdoq_kernel(args, torch, np)
    if not set(args.parts) - {"slice_kernels", "rdoq_kernel"}:
        return
    for coder in (("host", "lanes") if args.coder == "both" else (args.coder,)):
        run(args, coder, torch, np, codec, B)


if __name__ == "__main__":
    main()
