"""``python -m icm_amd.eval_model`` -- the image-compression branch of the reference's evaluation CLI
(compressai/utils/eval_model/__main__.py:627-671: collect images, load a checkpoint, ``update(force=True)``, run every
image through ``inference`` (real rANS bit-streams) or ``inference_entropy_estimation`` (forward pass), average the
metrics and print the JSON report) on the HIP path.  Same flags (-d/-r/-a/-c/-p/--entropy-estimation/--half/-v), same
report layout (``--metric psnr,ms-ssim`` adds the "ms-ssim" entry the reference has commented out, :135); the task-model
branches of the reference (detectron2 / segmentation, :553-625) are out of scope.

Differences kept deliberate: ``--entropy-estimation`` and ``--cuda`` are real booleans (the reference declares them
without ``type``/``action``, so any string is truthy); ``--half`` is refused (the HIP path is f32 end to end, like the
training path it mirrors); the reference's hard-coded default paths are replaced by required arguments."""
from __future__ import annotations

import argparse
import json
import os
import sys
from collections import defaultdict
from typing import Dict, List

import torch

from . import codec
from . import utils as U
from .bitstream import check_qstep, check_rdoq
from .datasets import IMG_EXTENSIONS, ToTensor, to_pil_image
from .zoo import models


def collect_images(rootpath: str) -> List[str]:
    """eval_model/__main__.py:70-75"""
    return sorted(os.path.join(rootpath, f) for f in os.listdir(rootpath)
                  if os.path.splitext(f)[-1].lower() in IMG_EXTENSIONS)


def read_image(filepath: str) -> torch.Tensor:
    """eval_model/__main__.py:83-86"""
    from PIL import Image
    if not os.path.isfile(filepath):
        raise FileNotFoundError(filepath)
    return ToTensor()(Image.open(filepath).convert("RGB"))


def reconstruct(reconstruction: torch.Tensor, filename: str, recon_path: str) -> None:
    """eval_model/__main__.py:89-94: clamp to [0,1] and save next to the metrics"""
    os.makedirs(recon_path, exist_ok=True)
    to_pil_image(reconstruction.squeeze(0).clamp(0, 1)).save(os.path.join(recon_path, filename))


def load_checkpoint(arch: str, checkpoint_path: str) -> torch.nn.Module:
    """eval_model/__main__.py:250-253: ``models[arch]()`` + the "state_dict" entry of a training checkpoint.  Only
    tensors are unpickled (``weights_only=True``); a bare state-dict file is accepted as well."""
    ck = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
    sd = ck["state_dict"] if isinstance(ck, dict) and "state_dict" in ck else ck
    net = models[arch]()
    net.load_state_dict(sd)
    return net.eval()


def aq_quality_map(filepath: str, device, aq: float, qstep: int = 0):
    """the quality map ``codec.encode_image(model, img, aq=aq, qstep=qstep)`` builds for the image of a file, untiled:
    the luma statistics of the 8-bit image on the grid of its centre pads, against the reference of the grid anchored
    at its first pixel -> int8 [h, w] of the padded latent's size (host)"""
    u8 = codec._as_u8_image(codec.read_image_u8(filepath), device)
    H, W = u8.size(0), u8.size(1)
    pads = codec.center_pads(H, W)
    ref = codec.aq_reference(codec.cell_stats(u8, (0, 0, 0, 0)))
    return codec.quality_map(H, W, pads, qstep, [], codec.aq_offsets(codec.cell_stats(u8, pads), aq, ref))


@torch.no_grad()
def eval_model(model, filepaths: List[str], entropy_estimation: bool = False, recon_path: str = "",
               metric_names=None, qstep: int = 0, qmap=None, rdoq=None, aq=None) -> Dict[str, float]:
    """eval_model/__main__.py:472-487 (per-image metrics averaged over the folder); ``qstep``: the codec's quantiser
    step index, for the real codec (``utils.inference``) and for the estimate
    (``utils.inference_entropy_estimation``) alike; ``qmap`` (with ``entropy_estimation``, instead of ``qstep``): a
    quality map of the padded latent's size of every image, the rate estimate under that map; ``rdoq`` (real codec
    only): weight of the encoder's rate-distortion optimised quantisation (``utils.inference``); ``aq`` (instead of
    ``qmap``; real codec and estimate alike): strength of variance-adaptive quantisation (``codec.check_aq``; None or
    0: off) -- every image is coded under the map ``codec.encode_image(aq=aq, qstep=qstep)`` derives from it
    (``aq_quality_map``), ``qstep`` being the map's background"""
    rdoq = check_rdoq(rdoq, "eval_model: ")
    aq = codec.check_aq(aq, "eval_model: ")
    if aq is not None and qmap is not None:
        raise ValueError("eval_model: aq derives a quality map from every image; give aq or qmap, not both")
    if aq is not None:
        qstep = check_qstep(qstep, "eval_model: ")
    if rdoq is not None and entropy_estimation:
        raise ValueError("eval_model: rdoq needs the real codec: the entropy estimation's kernels know no RDOQ")
    if qmap is not None and not entropy_estimation:
        raise ValueError("eval_model: qmap is for the entropy estimation (the codec's map comes from codec.py --roi)")
    device = next(model.parameters()).device
    metrics: Dict[str, float] = defaultdict(float)
    for f in filepaths:
        x = read_image(f).to(device)
        fn = U.inference_entropy_estimation if entropy_estimation else U.inference
        if metric_names is not None and "ms-ssim" in metric_names and min(x.shape[-2:]) <= 160:
            raise ValueError(f"{f}: {x.shape[-1]}x{x.shape[-2]} is too small for MS-SSIM (both sides must exceed 160 "
                             "pixels: five levels of an 11-tap window)")
        quality = {"qmap": aq_quality_map(f, device, aq, qstep)} if aq is not None else \
            {**({"qstep": qstep} if qstep else {}), **({} if qmap is None else {"qmap": qmap})}
        rv = fn(model, x, recon=(lambda xh, name=os.path.basename(f): reconstruct(xh, name, recon_path)) if recon_path else None,
                **({} if metric_names is None else {"metrics": metric_names}), **quality,
                **({} if rdoq is None else {"rdoq": rdoq}))
        for k, v in rv.items():
            metrics[k] += v
    return {k: v / len(filepaths) for k, v in metrics.items()}


def parse_metrics(values) -> List[str]:
    """--metric may be repeated and / or comma-separated; no flag = ["psnr"]"""
    if not values:
        return ["psnr"]
    names = [m.strip() for v in values for m in v.split(",") if m.strip()]
    unknown = [m for m in names if m not in U.EVAL_METRICS]
    if unknown or not names:
        raise ValueError(f"--metric: unknown metric(s) {unknown}; choose from {list(U.EVAL_METRICS)}")
    return [m for m in U.EVAL_METRICS if m in names]


def setup_args() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="icm_amd.eval_model")
    p.add_argument("-d", "--dataset", type=str, required=True, help="dataset path (a folder of images)")
    p.add_argument("-r", "--recon_path", type=str, default="", help="where to save reconstructed images (empty: do not save)")
    p.add_argument("-a", "--architecture", default="cnn", type=str, choices=sorted(models.keys()), help="model architecture")
    p.add_argument("-c", "--entropy-coder", choices=["ans"], default="ans", help="entropy coder (default: %(default)s)")
    p.add_argument("--cuda", dest="cuda", action="store_true", default=True, help="run on the GPU (required by the HIP path)")
    p.add_argument("--half", action="store_true", default=False, help="refused: the HIP path is f32")
    p.add_argument("--entropy-estimation", action="store_true", default=False,
                   help="use evaluated entropy estimation (no entropy coding)")
    p.add_argument("-v", "--verbose", action="store_true", help="verbose mode")
    p.add_argument("-p", "--path", dest="paths", type=str, default=None,
                   help="checkpoint path (default: the architecture's initial weights)")
    p.add_argument("--metric", dest="metric", action="append", default=None, metavar="{psnr,ms-ssim}",
                   help="quality metric(s) of the report; repeat the flag or separate by commas (default: psnr)")
    p.add_argument("--qstep", type=int, default=0, metavar="K",
                   help="quantiser step 2^(K/8) on the latent of the real codec, K in -16..32 (default 0: none)")
    p.add_argument("--rdoq", type=float, default=None, metavar="W",
                   help="rate-distortion optimised quantisation in the real codec's encoder, weight W > 0 (default: off)")
    p.add_argument("--aq", type=float, default=None, metavar="S",
                   help="variance-adaptive quantisation as `codec encode --aq S`: every image under the quality map "
                        "derived from it, --qstep its background; with --entropy-estimation the estimate under that map "
                        "(0 < |S| <= 4; default: off)")
    p.add_argument("--limit", type=int, default=0, help="evaluate only the first N images (0 = all)")
    return p


def main(argv) -> int:
    args = setup_args().parse_args(argv)
    try:
        metric_names = parse_metrics(args.metric)
    except ValueError as e:
        print(f"Error: {e}", file=sys.stderr)
        return 2
    if args.half:
        print("Error: --half is not supported (f32 path).", file=sys.stderr)
        return 2
    try:
        check_qstep(args.qstep, "--")
        codec.check_aq(args.aq, "--")
        if args.qstep and args.entropy_estimation and not args.aq:
            raise ValueError("--qstep needs the real codec: the entropy estimation has no quantiser step")
        check_rdoq(args.rdoq, "--")
        if args.rdoq is not None and args.entropy_estimation:
            raise ValueError("--rdoq needs the real codec: the entropy estimation's kernels know no RDOQ")
    except ValueError as e:
        print(f"Error: {e}", file=sys.stderr)
        return 2
    filepaths = collect_images(args.dataset)
    if args.limit > 0:
        filepaths = filepaths[:args.limit]
    if len(filepaths) == 0:
        print("Error: no images found in directory.", file=sys.stderr)
        return 1
    if not torch.cuda.is_available():
        print("Error: no GPU (the HIP path has no CPU fallback).", file=sys.stderr)
        return 3
    model = load_checkpoint(args.architecture, args.paths) if args.paths else models[args.architecture]().eval()
    model = model.to("cuda")
    model.update(force=True)
    if args.verbose:
        sys.stderr.write(f"Evaluating {args.paths or '<initial weights>'} on {len(filepaths)} images\n")
    try:
        metrics = eval_model(model, filepaths, args.entropy_estimation, args.recon_path,
                             metric_names=metric_names if args.metric else None, qstep=args.qstep,
                             rdoq=args.rdoq, aq=args.aq)
    except ValueError as e:
        print(f"Error: {e}", file=sys.stderr)
        return 4
    results = defaultdict(list)
    for k, v in metrics.items():
        results[k].append(v)
    description = "entropy estimation" if args.entropy_estimation else args.entropy_coder
    print(json.dumps({"name": args.architecture, "description": f"Inference ({description})", "results": results}, indent=2))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
