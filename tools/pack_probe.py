"""Pack-only launches of a training step's real job list (measurement tool).

One step of the bench workload records the trainer's packing sequence; the probe replays it the way the trainer does,
one icm_pack_weights_batch call per window of 24 entries, with nothing else on the GPU.  Bytes are counted from the job
descriptors: every source element read once (Cout * Cin * KH * KW floats per job) and every float of the packed
buffers written once.  Prints per-step microseconds and bytes/s, and with --digest FILE writes a SHA-256 per window of
the packed buffers (compare two library builds: ICM_LIB=<other libicm_hip.so>).

    python tools/pack_probe.py [--reps 20] [--digest FILE]"""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "image-compression-for-machine_amd")]
import bench  # noqa: E402
from icm_amd import _lib as L  # noqa: E402

COPY_BYTES_PER_S = 6.29e12   # plain copy on MI355X


def windows(seq, window):
    """[(PackJob array, buffers, bytes read, bytes written)] per window of the recorded miss sequence"""
    out = []
    lib = L.lib()
    for i in range(0, len(seq), window):
        flat, bufs, rd, wr = [], [], 0, 0
        for _, floats, jobs in seq[i:i + window]:
            buf = torch.full((floats,), float("nan"), dtype=torch.float32, device=jobs[0][0].device)
            bufs.append(buf)
            for w, a, off in jobs:
                flat.append((w, a, buf.data_ptr() + 4 * off))
                rd += 4 * a[0] * a[1] * a[2] * a[3]
                wr += 4 * (lib.icm_packed_weight_floats(a[0], a[1], 4, 4) if a[15] else
                           lib.icm_packed_weight_floats(a[0], a[1], a[2], a[3]))
        arr = (L.PackJob * len(flat))()
        for j, (w, a, wp) in zip(arr, flat):
            j.w, j.wp, j.Cout, j.Cin, j.KH, j.KW = w.data_ptr(), wp, a[0], a[1], a[2], a[3]
            (j.src_out_major, j.transposed, j.stride, j.pad, j.nonneg, j.bound, j.pedestal, j.src_ld, j.src_off,
             j.dst_ncot, j.dst_cot_off, j.wino) = a[4:16]
        out.append((arr, bufs, rd, wr))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--digest", metavar="FILE")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    tr, x, _ = bench.make_workload("cnn", dev)
    tr.step(x)
    torch.cuda.synchronize()
    wins = windows(tr._pack_seq, tr.pack_window)
    lib, st = L.lib(), L.stream()

    def run():
        for arr, _, _, _ in wins:
            L.check(lib.icm_pack_weights_batch(arr, len(arr), st), "pack_weights_batch")

    for _ in range(3):
        run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(args.reps):
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    times.sort()
    rd, wr = sum(w[2] for w in wins), sum(w[3] for w in wins)
    us = times[len(times) // 2]
    res = {"lib": L.LIB_PATH, "calls_per_step": len(wins), "jobs_per_step": sum(len(w[0]) for w in wins),
           "MB_read": round(rd / 1e6, 1), "MB_written": round(wr / 1e6, 1), "us_per_step_median": round(us, 1),
           "us_min": round(times[0], 1), "us_max": round(times[-1], 1), "TB_per_s": round((rd + wr) / us / 1e6, 3),
           "share_of_copy_rate": round((rd + wr) / us / 1e6 / (COPY_BYTES_PER_S / 1e12), 3)}
    print(json.dumps(res), flush=True)
    if args.digest:
        dig = []
        for _, bufs, _, _ in wins:
            h = hashlib.sha256()
            for b in bufs:
                h.update(b.cpu().numpy().tobytes())
            dig.append(h.hexdigest())
        with open(args.digest, "w") as fh:
            json.dump(dig, fh)


if __name__ == "__main__":
    main()
