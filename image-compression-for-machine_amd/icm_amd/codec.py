"""``python -m icm_amd.codec`` -- image file to bit-stream file and back, in two processes that share a checkpoint.

    python -m icm_amd.codec encode IMAGE -o FILE -a cnn -p CKPT
    python -m icm_amd.codec decode FILE -o IMAGE.png -p CKPT [--reference IMAGE]

Parity unpinned: no counterpart in the reference (upstream CompressAI's ``examples/codec.py`` is not in its tree).  The
conventions are those of ``icm_amd.eval_model``: ``-a`` architecture, ``-p`` checkpoint (``weights_only=True``), exit
codes 2 = argument error, 3 = no GPU, 4 = bad input.  ``decode`` takes the architecture from the stream (``-a``, if
given, must agree) and refuses, before it touches the payload, a stream whose model fingerprint is not the
checkpoint's.  Both commands print one JSON line.

The image boundary runs on the device: the 8-bit image crosses PCIe as bytes, ``icm_image_u8_to_f32`` converts and
pads in one pass (``ToTensor`` + ``utils.pad_to_multiple``, bit for bit), and ``icm_image_f32_to_u8`` crops, quantises
(``datasets.to_pil_image``) and, given the original, sums the squared 8-bit differences that the PSNR is formed from.
The container is ``icm_amd.bitstream``; one image per stream."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from . import bitstream as B
from ._lib import check

PAD_MULTIPLE = 64      # six stride-2 stages (utils.pad_to_multiple)


def arch_of(model) -> str:
    """name of the model's class in ``zoo.models``; ValueError unless the bit-stream format knows it (``stf6`` has no
    entropy coder loop: its ``compress`` raises NotImplementedError).  Host-only: no GPU work."""
    from .zoo import models
    name = next((k for k, cls in models.items() if type(model) is cls), None)
    if name is None:
        raise ValueError(f"codec: {type(model).__name__} is not an architecture of icm_amd.zoo.models")
    if name not in B.ARCHS:
        raise ValueError(f"codec: architecture {name!r} has no bit-stream codec (compress() is not implemented); "
                         f"choose from {list(B.ARCHS)}")
    return name


def center_pads(h: int, w: int, p: int = PAD_MULTIPLE) -> Tuple[int, int, int, int]:
    """(left, right, top, bottom) of ``utils.pad_to_multiple``: centre padding, the extra pixel right / bottom"""
    new_h, new_w = (h + p - 1) // p * p, (w + p - 1) // p * p
    left, top = (new_w - w) // 2, (new_h - h) // 2
    return left, new_w - w - left, top, new_h - h - top


def _as_u8_image(img, device, what: str = "image") -> torch.Tensor:
    """8-bit [H, W, 3] on ``device``, contiguous; the copy to the device moves bytes"""
    if isinstance(img, torch.Tensor):
        t = img
    else:
        a = np.asarray(img)
        if not (a.flags.writeable and a.flags.c_contiguous):     # PIL hands out read-only views
            a = np.array(a, order="C")
        t = torch.from_numpy(a)
    if t.dtype != torch.uint8 or t.dim() != 3 or t.size(2) != 3 or t.size(0) < 1 or t.size(1) < 1:
        raise ValueError(f"codec: {what} must be 8-bit [H, W, 3], got {t.dtype} {tuple(t.shape)}")
    return t.to(device).contiguous()


def image_u8_to_f32(img: torch.Tensor, pads: Tuple[int, int, int, int]) -> torch.Tensor:
    """device 8-bit [H, W, 3] -> f32 [1, 3, top + H + bottom, left + W + right], zeros around the image"""
    H, W = img.size(0), img.size(1)
    left, right, top, bottom = pads
    out = torch.empty((1, 3, top + H + bottom, left + W + right), dtype=torch.float32, device=img.device)
    check(L.lib().icm_image_u8_to_f32(img.data_ptr(), H, W, out.data_ptr(), out.size(2), out.size(3), top, left,
                                      L.stream()), "image_u8_to_f32")
    return out


def image_f32_to_u8(x: torch.Tensor, pads: Tuple[int, int, int, int],
                    reference: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """device f32 [1, 3, PH, PW] -> (8-bit [H, W, 3] of the window inside ``pads``, sum of squared 8-bit differences to
    ``reference`` as a device int64 scalar, or None)"""
    if x.dim() != 4 or x.size(0) != 1 or x.size(1) != 3 or x.dtype != torch.float32:
        raise ValueError(f"codec: expected f32 [1, 3, H, W], got {x.dtype} {tuple(x.shape)}")
    x = x.contiguous()
    left, right, top, bottom = pads
    H, W = x.size(2) - top - bottom, x.size(3) - left - right
    if H < 1 or W < 1:
        raise ValueError(f"codec: pads {pads} leave nothing of {tuple(x.shape)}")
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=x.device)
    sse = ws = None
    ws_bytes = 0
    if reference is not None:
        if tuple(reference.shape) != (H, W, 3) or reference.dtype != torch.uint8:
            raise ValueError(f"codec: reference must be 8-bit {(H, W, 3)}, got {reference.dtype} {tuple(reference.shape)}")
        reference = reference.to(x.device).contiguous()
        ws_bytes = int(L.lib().icm_image_workspace_bytes(H, W))
        ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=x.device)
        sse = torch.empty((), dtype=torch.int64, device=x.device)
    check(L.lib().icm_image_f32_to_u8(x.data_ptr(), x.size(2), x.size(3), top, left, out.data_ptr(), H, W,
                                      L.ptr(reference), L.ptr(sse), L.ptr(ws), ws_bytes, L.stream()), "image_f32_to_u8")
    return out, sse


def _ready(model) -> str:
    arch = arch_of(model)                      # refuses before any GPU work
    if model.training:
        raise ValueError("codec: the model must be in eval mode")
    if model.entropy_bottleneck._offset.numel() == 0:
        model.update(force=True)
    return arch


@torch.no_grad()
def encode_image(model, img) -> bytes:
    """8-bit [H, W, 3] image (tensor on any device, or anything ``numpy.asarray`` accepts) -> one bit-stream"""
    arch = _ready(model)
    device = next(model.parameters()).device
    u8 = _as_u8_image(img, device)
    H, W = u8.size(0), u8.size(1)
    pads = center_pads(H, W)
    enc = model.compress(image_u8_to_f32(u8, pads))
    header = {"arch": arch, "height": H, "width": W, "pads": pads, "shape": tuple(int(s) for s in enc["shape"]),
              "fingerprint": B.fingerprint(model)}
    return B.pack(header, [s for part in enc["strings"] for s in part])


@torch.no_grad()
def decode_image(model, data: bytes, reference=None) -> Tuple[torch.Tensor, Dict]:
    """one bit-stream -> (8-bit [H, W, 3] host tensor, info); ``info``: "bpp" = 8 x the whole stream length / (H W),
    header included, and, given ``reference`` (the original 8-bit image), "psnr" of the two 8-bit images"""
    arch = _ready(model)
    header, strings = B.unpack(data)
    if header["arch"] != arch:
        raise ValueError(f"codec: the stream was written by architecture {header['arch']!r}, the model is {arch!r}")
    fp = B.fingerprint(model)
    if header["fingerprint"] != fp:
        raise ValueError(f"codec: model fingerprint mismatch: the stream was written with entropy tables "
                         f"{header['fingerprint']:#010x}, this checkpoint has {fp:#010x}")
    H, W, pads = header["height"], header["width"], header["pads"]
    if len(strings) != 2:
        raise ValueError(f"codec: {arch} streams hold two strings, this one holds {len(strings)}")
    device = next(model.parameters()).device
    ref = None if reference is None else _as_u8_image(reference, device, "reference")
    if ref is not None and tuple(ref.shape) != (H, W, 3):
        raise ValueError(f"codec: the reference is {ref.size(0)}x{ref.size(1)}, the stream holds a {H}x{W} image")
    x_hat = model.decompress([[strings[0]], [strings[1]]], header["shape"])["x_hat"]
    left, right, top, bottom = pads
    if tuple(x_hat.shape) != (1, 3, top + H + bottom, left + W + right):
        raise ValueError(f"codec: latent shape {header['shape']} decodes to {tuple(x_hat.shape)}, not to a padded "
                         f"{H}x{W} image")
    out, sse = image_f32_to_u8(x_hat, pads, ref)
    info = {"arch": arch, "height": H, "width": W, "bytes": len(data), "bpp": 8.0 * len(data) / (H * W)}
    if sse is not None:
        info["sse"] = int(sse.item())
        info["psnr"] = 10.0 * math.log10(255.0 ** 2 / (info["sse"] / (H * W * 3))) if info["sse"] else math.inf
    return out.cpu(), info


# ------------------------------------------------------------------------------------------------------------ CLI
def read_image_u8(path: str) -> np.ndarray:
    from PIL import Image
    if not os.path.isfile(path):
        raise ValueError(f"{path}: no such file")
    try:
        return np.asarray(Image.open(path).convert("RGB"))
    except OSError as e:       # PIL.UnidentifiedImageError is one
        raise ValueError(f"{path}: not an image ({e})")


def setup_args() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="icm_amd.codec")
    sub = p.add_subparsers(dest="command", required=True)
    enc = sub.add_parser("encode", help="image file -> bit-stream file")
    enc.add_argument("input", help="image file")
    enc.add_argument("-a", "--architecture", default="cnn", type=str, help="model architecture")
    dec = sub.add_parser("decode", help="bit-stream file -> image file")
    dec.add_argument("input", help="bit-stream file")
    dec.add_argument("-a", "--architecture", default=None, type=str,
                     help="model architecture (default: the stream's; must agree with it)")
    dec.add_argument("--reference", default=None, help="the original image: report the PSNR of the reconstruction")
    for s in (enc, dec):
        s.add_argument("-o", "--output", required=True, help="file to write")
        s.add_argument("-p", "--path", dest="paths", required=True, type=str, help="checkpoint path")
    return p


def _load(arch: str, path: str):
    from .eval_model import load_checkpoint
    model = load_checkpoint(arch, path).to("cuda")
    model.update(force=True)
    return model


def main(argv) -> int:
    from .zoo import models
    args = setup_args().parse_args(argv)
    arch = args.architecture
    if arch is not None and (arch not in models or arch not in B.ARCHS):
        known = f"choose from {list(B.ARCHS)}"
        why = "has no bit-stream codec" if arch in models else "is not an architecture"
        print(f"Error: -a {arch}: {why}; {known}.", file=sys.stderr)
        return 2
    try:
        if args.command == "encode":
            payload = read_image_u8(args.input)
        else:
            if not os.path.isfile(args.input):
                raise ValueError(f"{args.input}: no such file")
            with open(args.input, "rb") as f:
                payload = f.read()
            header, _ = B.unpack(payload)
            if arch is not None and arch != header["arch"]:
                print(f"Error: -a {arch} disagrees with the stream, written by {header['arch']!r}.", file=sys.stderr)
                return 2
            arch = header["arch"]
            reference = read_image_u8(args.reference) if args.reference else None
    except ValueError as e:
        print(f"Error: {e}", file=sys.stderr)
        return 4
    if not torch.cuda.is_available():
        print("Error: no GPU (the HIP path has no CPU fallback).", file=sys.stderr)
        return 3
    try:
        model = _load(arch, args.paths)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if args.command == "encode":
            data = encode_image(model, payload)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            h, w = payload.shape[:2]
            with open(args.output, "wb") as f:
                f.write(data)
            report = {"command": "encode", "arch": arch, "height": h, "width": w, "bytes": len(data),
                      "bpp": 8.0 * len(data) / (h * w), "encode_time": dt}
        else:
            img, info = decode_image(model, payload, reference)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            from PIL import Image
            Image.fromarray(img.numpy()).save(args.output)
            report = {"command": "decode", **{k: v for k, v in info.items() if k != "sse"}, "decode_time": dt}
    except (ValueError, FileNotFoundError) as e:
        print(f"Error: {e}", file=sys.stderr)
        return 4
    print(json.dumps(report))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
