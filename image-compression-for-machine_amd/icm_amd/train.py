"""``python -m icm_amd.train`` -- the reference's training script (train.py:170-530) driving the HIP hot path.

Same flags (-m/-d/-e/-lr/-n/--lambda/--batch-size/--test-batch-size/--aux-learning-rate/--patch-size/--save/
--save_path/--seed/--clip_max_norm/--checkpoint), same epoch structure: ``train_one_epoch`` (train.py:170-232),
``test_epoch`` every fifth epoch (:235-283, :505-507), ``ReduceLROnPlateau(min, factor 0.6, patience 6)`` on the test
loss (:438), best-only checkpoints ``<save_path><epoch>.ckpt`` holding epoch / state_dict / loss / optimizer state
(:512-527).  What differs, on purpose:

* one optimisation step is ``icm_amd.trainer.Trainer.step`` -- forward, R-D loss, backward, clip, Adam, aux loss and aux
  Adam as fused HIP launches on flat buffers -- instead of five Python-level calls (identical arithmetic; parity with the
  reference loop is a GPU test); the learning rate of ReduceLROnPlateau is applied through ``Trainer.lr``;
* ``--split``/``--test-split`` replace the hard-coded ``val2017`` folder name (:404-405); ``--random-crop`` selects the
  ``RandomCrop(pad_if_needed)`` transform the reference has commented out (:393-395) instead of ``CenterCrop``;
* the loss is the published ``lmbda * 255^2 * mse + bpp`` (train_czigzag.py:63,71; default 0.0067); ``--metric ms-ssim``
  selects ``lmbda * (1 - ms_ssim) + bpp`` instead (upstream CompressAI's ``RateDistortionLoss(metric="ms-ssim")``);
* under ``torch.distributed.run`` (WORLD_SIZE > 1) every rank trains on its shard of each batch (DistributedSampler)
  and gradients are all-reduced over RCCL by the Trainer; the reference is single-process;
* ``--device-cache GB`` keeps both splits on the device as 8-bit images (decoded once, ``datasets.DeviceImageCache``)
  and cuts every batch there with one kernel launch; the per-step host work left is drawing the crop positions.  The
  crops are the transforms' own (same ``random`` draws); the epoch order comes from ``datasets.EpochSampler``;
* ``--qstep-range LO,HI`` trains one model across the codec's quantiser steps (``Trainer(qstep_range=...)``: a step per
  image and iteration, distortion weight ``lambda * step^-E``, ``--qstep-lambda-exp E``); the test loop then reports
  loss, bpp and mse at K = LO, 0 (if inside the range) and HI, and the checkpoint records ``qstep_range``;
* ``--qmap-rects R`` (with ``--qstep-range``) trains with a quality map per image and iteration
  (``Trainer(qmap_rects=R)``: R random rectangles over the drawn background, a step per latent position, a distortion
  weight per 16 x 16 cell); the test loop adds one fixed pattern labelled ``roi`` (``roi_test_map``), the checkpoint
  records ``qmap_rects`` and a resumed run without the flag keeps the checkpoint's;
* ``--qmap-aq SLO,SHI`` (with ``--qstep-range``, with or without ``--qmap-rects``) trains on the maps ``codec encode
  --aq S`` would make for the crops themselves (``Trainer(qmap_aq=(SLO, SHI))``: S uniform on SLO..SHI per image and
  iteration, the maps computed on the device inside the step); the test loop adds one line labelled ``aq``
  (``aq_test_point``), the checkpoint records ``qmap_aq`` and a resumed run without the flag keeps the checkpoint's;
* checkpoints are read with ``weights_only=True``."""
from __future__ import annotations

import argparse
import os
import random
import sys
import time

import torch
from torch.utils.data import DataLoader

from .datasets import (CenterCrop, Compose, DeviceCacheLoader, DeviceImageCache, EpochSampler, ImageFolder, RandomCrop,
                       ToTensor)
from .losses import METRICS, RateDistortionLoss
from . import engine as E
from .trainer import Trainer, check_qmap_aq, check_qmap_rects, check_qstep_range, qstep_tables
from .zoo import models


class AverageMeter:
    """train.py:79-92"""

    def __init__(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


class PlateauLR:
    """optim.lr_scheduler.ReduceLROnPlateau(mode="min", factor, patience) with torch's defaults (relative threshold 1e-4,
    no cooldown, min_lr 0, eps 1e-8) acting on ``Trainer.lr`` (train.py:438,507)"""

    def __init__(self, trainer: Trainer, factor: float = 0.6, patience: int = 6, threshold: float = 1e-4):
        self.trainer, self.factor, self.patience, self.threshold = trainer, factor, patience, threshold
        self.best, self.num_bad = float("inf"), 0

    def step(self, metric: float) -> None:
        if metric < self.best * (1.0 - self.threshold):
            self.best, self.num_bad = metric, 0
        else:
            self.num_bad += 1
        if self.num_bad > self.patience:
            new_lr = self.trainer.lr * self.factor
            if self.trainer.lr - new_lr > 1e-8:
                self.trainer.lr = new_lr
            self.num_bad = 0

    def state_dict(self):
        return {"best": self.best, "num_bad_epochs": self.num_bad, "factor": self.factor, "patience": self.patience}

    def load_state_dict(self, sd):
        self.best, self.num_bad = float(sd["best"]), int(sd["num_bad_epochs"])


def train_one_epoch(trainer: Trainer, train_dataloader, epoch: int, log_every: int = 600) -> None:
    """train.py:170-232"""
    start = time.time()
    for i, d in enumerate(train_dataloader):
        x = d.to(trainer.device, non_blocking=True).contiguous()
        s = trainer.step(x)
        if i % log_every == 0 and trainer.rank == 0:
            v = s.tolist()   # the only host sync of the loop
            dt, start = time.time() - start, time.time()
            dist = f"MS-SSIM loss: {v[7]:.4f}" if trainer.metric == "ms-ssim" else f"MSE loss: {v[1]:.3f}"
            print(f"Train epoch {epoch}: [{i * len(x)}/{len(train_dataloader.dataset)} "
                  f"({100. * i / len(train_dataloader):.0f}%)]\tLoss: {v[2]:.3f} |\t{dist} |"
                  f"\tBpp loss: {v[0]:.2f} |\tAux loss: {v[6]:.2f} |\ttime: {dt:.1f}", flush=True)


def parse_qstep_range(text):
    """--qstep-range LO,HI -> (lo, hi), two step indexes with lo <= hi (ValueError otherwise)"""
    parts = [p.strip() for p in str(text).split(",")]
    try:
        lo, hi = (int(p) for p in parts)
    except ValueError:
        raise ValueError(f"--qstep-range: expected LO,HI (two integers), got {text!r}")
    return check_qstep_range((lo, hi))


def qstep_test_points(qstep_range):
    """the step indexes the test loop reports of a variable-rate run: LO, 0 (if inside the range) and HI"""
    lo, hi = qstep_range
    return sorted({lo, hi} | ({0} if lo < 0 < hi else set()))


def parse_qmap_aq(text):
    """--qmap-aq SLO,SHI -> (slo, shi) or None for off (``trainer.check_qmap_aq``; ValueError otherwise)"""
    parts = [p.strip() for p in str(text).split(",")]
    try:
        slo, shi = (float(p) for p in parts)
    except ValueError:
        raise ValueError(f"--qmap-aq: expected SLO,SHI (two numbers), got {text!r}")
    return check_qmap_aq((slo, shi))


def aq_test_point(qstep_range, qmap_aq):
    """(K, S) of the line the test loop of an AQ-map run reports as ``aq``: the background of the ``0`` line (LO when 0
    is outside the range) and whichever of SLO, SHI is larger in magnitude"""
    lo, hi = qstep_range
    slo, shi = qmap_aq
    return (0 if lo < 0 < hi else lo), (shi if abs(shi) >= abs(slo) else slo)


def roi_test_map(h: int, w: int, lo: int, hi: int):
    """the fixed pattern the test loop of a quality-map run reports as ``roi``: background HI, and at LO a centred
    rectangle of half the map's height and width (rounded down, one cell at least) -> int8 [h, w] host array"""
    import numpy as np
    m = np.full((h, w), hi, dtype=np.int8)
    rh, rw = max(h // 2, 1), max(w // 2, 1)
    y0, x0 = (h - rh) // 2, (w - rw) // 2
    m[y0:y0 + rh, x0:x0 + rw] = lo
    return m


@torch.no_grad()
def qstep_test_epoch(epoch: int, test_dataloader, model, criterion, lmbda: float, lmbda_exp: float, qstep_range,
                     verbose: bool = True, qmap_rects: int = 0, qmap_aq=None) -> float:
    """``test_epoch`` of a variable-rate run: loss, bpp and mse at every step index of ``qstep_test_points``, each with the
    weight training gives that step (``trainer.qstep_tables``); returns the mean of the points' losses, which is what
    the learning-rate schedule and the best-checkpoint choice then see.  With ``qmap_rects`` one more line, ``roi``: the
    pattern of ``roi_test_map`` under the per-cell loss (it is reported, and stays out of the returned mean, so runs
    with and without maps are compared by the same figure).  With ``qmap_aq`` one more line, ``aq``, reported the same
    way: every test image under the map variance-adaptive quantisation makes for it (``engine.qmap_aq``, the entry point
    the training step uses) at the background and strength of ``aq_test_point``"""
    model.eval()
    device = next(model.parameters()).device
    points = qstep_test_points(qstep_range)
    meters = {k: (AverageMeter(), AverageMeter(), AverageMeter()) for k in points}
    lam = {k: float(qstep_tables((k, k), lmbda, lmbda_exp)[1][0]) for k in points}
    roi_meters = (AverageMeter(), AverageMeter(), AverageMeter())
    aq_meters = (AverageMeter(), AverageMeter(), AverageMeter())
    for d in test_dataloader:
        x = d.to(device)
        for k in points:
            out = criterion(model(x, qstep=k), x, lmbda_n=[lam[k]] * x.shape[0])
            for m, name in zip(meters[k], ("loss", "bpp_loss", "mse_loss")):
                m.update(float(out[name]))
        if qmap_rects:
            roi = roi_test_map(x.shape[2] // 16, x.shape[3] // 16, qstep_range[0], qstep_range[1])
            out = criterion(model(x, qmap=roi), x, qmap=roi, lmbda_exp=lmbda_exp)
            for m, name in zip(roi_meters, ("loss", "bpp_loss", "mse_loss")):
                m.update(float(out[name]))
        if qmap_aq is not None:
            k, s = aq_test_point(qstep_range, qmap_aq)
            n = x.shape[0]
            maps = E.qmap_aq(x.contiguous(), torch.full((n,), k, dtype=torch.int8, device=device),
                             torch.full((n,), s, dtype=torch.float32, device=device))[0].cpu().numpy()
            out = criterion(model(x, qmap=maps), x, qmap=maps, lmbda_exp=lmbda_exp)
            for m, name in zip(aq_meters, ("loss", "bpp_loss", "mse_loss")):
                m.update(float(out[name]))
    model.train()
    if verbose:
        for k in points:
            loss, bpp, mse = meters[k]
            print(f"Test epoch {epoch}: qstep {k}:\tLoss: {loss.avg:.3f} |\tMSE loss: {mse.avg * 255 ** 2:.3f} |"
                  f"\tBpp loss: {bpp.avg:.2f}", flush=True)
        if qmap_rects:
            loss, bpp, mse = roi_meters
            print(f"Test epoch {epoch}: qstep roi:\tLoss: {loss.avg:.3f} |\tMSE loss: {mse.avg * 255 ** 2:.3f} |"
                  f"\tBpp loss: {bpp.avg:.4f}", flush=True)
        if qmap_aq is not None:
            loss, bpp, mse = aq_meters
            print(f"Test epoch {epoch}: qstep aq:\tLoss: {loss.avg:.3f} |\tMSE loss: {mse.avg * 255 ** 2:.3f} |"
                  f"\tBpp loss: {bpp.avg:.4f}", flush=True)
    return sum(meters[k][0].avg for k in points) / len(points)


def checkpoint_state(epoch, state_dict, loss, optimizer, aux_optimizer, lr_scheduler, qstep_range=None,
                     qstep_lmbda_exp=2.0, qmap_rects=0, qmap_aq=None) -> dict:
    """what a checkpoint holds (train.py:512-527); "qstep_range" is [lo, hi] of a variable-rate run and None otherwise
    (a checkpoint without the key is a fixed-rate one); "qmap_rects" is the rectangle count of a quality-map run, and
    only such a run has the key; likewise "qmap_aq", [slo, shi] of an AQ-map run"""
    ck = {"epoch": epoch, "state_dict": state_dict, "loss": loss, "optimizer": optimizer,
          "aux_optimizer": aux_optimizer, "lr_scheduler": lr_scheduler,
          "qstep_range": None if qstep_range is None else [int(k) for k in qstep_range],
          "qstep_lambda_exp": float(qstep_lmbda_exp)}
    if qmap_rects:
        ck["qmap_rects"] = int(qmap_rects)
    if qmap_aq is not None:
        ck["qmap_aq"] = [float(v) for v in qmap_aq]
    return ck


@torch.no_grad()
def test_epoch(epoch: int, test_dataloader, model, criterion, verbose: bool = True) -> float:
    """train.py:235-283"""
    model.eval()
    device = next(model.parameters()).device
    loss, bpp_loss, mse_loss, aux_loss = AverageMeter(), AverageMeter(), AverageMeter(), AverageMeter()
    ms_ssim_loss = AverageMeter()
    for d in test_dataloader:
        x = d.to(device)
        out = criterion(model(x), x)
        aux_loss.update(float(model.aux_loss()))
        bpp_loss.update(float(out["bpp_loss"]))
        loss.update(float(out["loss"]))
        if "ms_ssim_loss" in out:
            ms_ssim_loss.update(float(out["ms_ssim_loss"]))
        else:
            mse_loss.update(float(out["mse_loss"]))
    model.train()
    if verbose:
        dist = (f"MS-SSIM loss: {ms_ssim_loss.avg:.4f}" if ms_ssim_loss.count
                else f"MSE loss: {mse_loss.avg * 255 ** 2:.3f}")
        print(f"Test epoch {epoch}: Average losses:\tLoss: {loss.avg:.3f} |\t{dist} |"
              f"\tBpp loss: {bpp_loss.avg:.2f} |\tAux loss: {aux_loss.avg:.2f}\n", flush=True)
    return loss.avg


def save_checkpoint(state, filename: str) -> None:
    """train.py:286-289"""
    os.makedirs(os.path.dirname(filename) or ".", exist_ok=True)
    torch.save(state, filename)


def parse_args(argv):
    p = argparse.ArgumentParser(description="Training script (HIP path).")
    p.add_argument("-m", "--model", default="cnn", choices=sorted(models.keys()), help="Model architecture (default: %(default)s)")
    p.add_argument("-d", "--dataset", type=str, required=True, help="Training dataset (root of the split folders)")
    p.add_argument("--split", type=str, default="train", help="training split folder (default: %(default)s)")
    p.add_argument("--test-split", type=str, default="test", help="test split folder (default: %(default)s)")
    p.add_argument("-e", "--epochs", default=100, type=int, help="Number of epochs (default: %(default)s)")
    p.add_argument("-lr", "--learning-rate", default=1e-4, type=float, help="Learning rate (default: %(default)s)")
    p.add_argument("-n", "--num-workers", type=int, default=4, help="Dataloaders threads (default: %(default)s)")
    p.add_argument("--lambda", dest="lmbda", type=float, default=0.0067, help="Bit-rate distortion parameter (default: %(default)s)")
    p.add_argument("--metric", type=str, default="mse", choices=list(METRICS),
                   help="Distortion of the loss: mse = lmbda*255^2*mse + bpp, ms-ssim = lmbda*(1 - ms_ssim) + bpp "
                        "(default: %(default)s)")
    p.add_argument("--batch-size", type=int, default=16, help="Batch size per GPU (default: %(default)s)")
    p.add_argument("--test-batch-size", type=int, default=16, help="Test batch size (default: %(default)s)")
    p.add_argument("--aux-learning-rate", default=1e-4, type=float, help="Auxiliary loss learning rate (default: %(default)s)")
    p.add_argument("--patch-size", type=int, nargs=2, default=(256, 256), help="Size of the patches to be cropped (default: %(default)s)")
    p.add_argument("--random-crop", action="store_true", help="RandomCrop(pad_if_needed) instead of CenterCrop for training")
    p.add_argument("--save", action="store_true", default=False, help="Save model to disk")
    p.add_argument("--save_path", type=str, default="./checkpoints/", help="Where to Save model")
    p.add_argument("--seed", type=float, help="Set random seed for reproducibility")
    p.add_argument("--clip_max_norm", default=1.0, type=float, help="gradient clipping max norm (default: %(default)s)")
    p.add_argument("--checkpoint", type=str, default=None, help="Path to a checkpoint")
    p.add_argument("--test-every", type=int, default=5, help="test / checkpoint every N epochs (train.py:505; default: %(default)s)")
    p.add_argument("--max-steps", type=int, default=0, help="stop each epoch after N iterations (0 = full epoch)")
    p.add_argument("--device-cache", type=float, default=0.0, metavar="GB",
                   help="keep both splits on the device as 8-bit images, at most GB gigabytes (10^9 bytes), and crop "
                        "batches there (default: 0 = off, DataLoader workers decode every step)")
    p.add_argument("--qstep-range", type=str, default=None, metavar="LO,HI",
                   help="variable-rate training: draw a quantiser step 2^(K/8) per image, K uniform on LO..HI "
                        "(integers in -16..32, LO <= HI), and weight its distortion by lambda * step^-E (default: off)")
    p.add_argument("--qstep-lambda-exp", type=float, default=2.0, metavar="E",
                   help="exponent E of the per-step distortion weight (default: %(default)s, the high-rate "
                        "approximation D ~ step^2)")
    p.add_argument("--qmap-rects", type=int, default=None, metavar="R",
                   help="quality-map training (needs --qstep-range): R random rectangles per image, 0..8, each with its "
                        "own step, over the drawn background; distortion weight per 16x16 cell (default: 0 = off, or "
                        "what the --checkpoint resumed from records)")
    p.add_argument("--qmap-aq", type=str, default=None, metavar="SLO,SHI",
                   help="AQ-map training (needs --qstep-range): the quality map of every crop is the one `codec encode "
                        "--aq S` would make for it, S uniform on SLO..SHI per image (-4 <= SLO <= SHI <= 4); with "
                        "--qmap-rects the rectangles win (default: off, or what the --checkpoint resumed from records; "
                        "0,0 = off)")
    # "--qstep-range -8,16": argparse takes a value that begins with "-" and is no number for an option; hand it the
    # "--qstep-range=-8,16" form (--qmap-aq likewise)
    argv = list(argv)
    for flag in ("--qstep-range", "--qmap-aq"):
        for i in range(len(argv) - 1):
            if argv[i] == flag and argv[i + 1][:1] == "-" and argv[i + 1][1:2] in tuple("0123456789."):
                argv[i:i + 2] = [f"{flag}={argv[i + 1]}"]
                break
    args = p.parse_args(argv)
    try:
        args.qstep_range = None if args.qstep_range is None else parse_qstep_range(args.qstep_range)
        if args.qstep_range is not None and args.metric == "ms-ssim":
            raise ValueError("--qstep-range: the MS-SSIM loss takes a scalar lambda (use --metric mse)")
        if args.qstep_range is not None and args.model == "stf6":
            raise ValueError("--qstep-range: stf6 has no codec and so no quantiser step")
        if args.qmap_rects is not None and check_qmap_rects(args.qmap_rects) and args.qstep_range is None:
            raise ValueError("--qmap-rects: quality-map training draws its step indexes from --qstep-range; give one")
        args.qmap_aq_given = args.qmap_aq is not None   # "0,0" turns a resumed run's maps off; no flag keeps them
        args.qmap_aq = None if args.qmap_aq is None else parse_qmap_aq(args.qmap_aq)
        if args.qmap_aq is not None:
            if args.qstep_range is None:
                raise ValueError("--qmap-aq: quality-map training draws its step indexes from --qstep-range; give one")
            if args.metric == "ms-ssim":
                raise ValueError("--qmap-aq: the MS-SSIM loss takes a scalar lambda (use --metric mse)")
            if args.model == "stf6":
                raise ValueError("--qmap-aq: stf6 has no codec and so no quantiser step")
    except ValueError as e:
        p.error(str(e))   # exit 2, like every other bad argument
    return args


class _Limited:
    def __init__(self, loader, n):
        self.loader, self.n, self.dataset = loader, n, loader.dataset

    def __len__(self):
        return min(self.n, len(self.loader))

    def __iter__(self):
        for i, d in enumerate(self.loader):
            if i >= self.n:
                return
            yield d


def main(argv) -> int:
    args = parse_args(argv)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if rank == 0:
        print(args)
    if not torch.cuda.is_available():
        print("Error: no GPU (the HIP path has no CPU fallback).", file=sys.stderr)
        return 3
    if args.seed is not None:
        torch.manual_seed(args.seed)
        random.seed(args.seed)
    device = f"cuda:{local}"
    torch.cuda.set_device(local)
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=torch.device(device))

    sampler = None
    if args.device_cache > 0:
        budget = int(args.device_cache * 1e9)
        seed = int(args.seed or 0)
        try:
            train_cache = DeviceImageCache(args.dataset, args.split, device, budget, num_workers=args.num_workers)
            test_cache = DeviceImageCache(args.dataset, args.test_split, device, budget - train_cache.nbytes,
                                          num_workers=args.num_workers)
        except ValueError as e:
            print(f"Error: {e}", file=sys.stderr)
            if world > 1:
                dist.destroy_process_group()
            return 2
        if rank == 0:
            print(f"device cache: {len(train_cache) + len(test_cache)} images, "
                  f"{(train_cache.nbytes + test_cache.nbytes) / 1e9:.2f} GB", flush=True)
        sampler = EpochSampler(len(train_cache), args.batch_size, seed, rank=rank, world=world)
        train_dataloader = DeviceCacheLoader(train_cache, sampler, "random" if args.random_crop else "center", args.patch_size)
        test_dataloader = DeviceCacheLoader(test_cache, EpochSampler(len(test_cache), args.test_batch_size, seed, shuffle=False),
                                            "center", args.patch_size)
    else:
        crop = RandomCrop(args.patch_size, pad_if_needed=True) if args.random_crop else CenterCrop(args.patch_size)
        train_dataset = ImageFolder(args.dataset, split=args.split, transform=Compose([crop, ToTensor()]))
        test_dataset = ImageFolder(args.dataset, split=args.test_split, transform=Compose([CenterCrop(args.patch_size), ToTensor()]))
        if world > 1:
            from torch.utils.data.distributed import DistributedSampler
            sampler = DistributedSampler(train_dataset, num_replicas=world, rank=rank, shuffle=True, drop_last=True)
        train_dataloader = DataLoader(train_dataset, batch_size=args.batch_size, num_workers=args.num_workers,
                                      shuffle=sampler is None, sampler=sampler, pin_memory=True, drop_last=world > 1)
        test_dataloader = DataLoader(test_dataset, batch_size=args.test_batch_size, num_workers=args.num_workers,
                                     shuffle=False, pin_memory=True)
    if args.max_steps > 0:
        train_dataloader = _Limited(train_dataloader, args.max_steps)

    net = models[args.model]()
    last_epoch = 0
    ck = None
    if args.checkpoint:   # train.py:453-485
        if rank == 0:
            print("Loading", args.checkpoint)
        ck = torch.load(args.checkpoint, map_location="cpu", weights_only=True)
        last_epoch = int(ck["epoch"]) + 1
        net.load_state_dict(ck["state_dict"])
    if args.qmap_rects is None:   # a resumed quality-map run keeps its rectangle count
        args.qmap_rects = int(ck.get("qmap_rects", 0) or 0) if ck is not None and args.qstep_range is not None else 0
    if not args.qmap_aq_given and ck is not None and args.qstep_range is not None:   # ... and its AQ strengths
        args.qmap_aq = check_qmap_aq(ck.get("qmap_aq"))
    trainer = Trainer(net, lr=args.learning_rate, aux_lr=args.aux_learning_rate, lmbda=args.lmbda,
                      clip_max_norm=args.clip_max_norm, device=device, seed=int(args.seed or 0), metric=args.metric,
                      qstep_range=args.qstep_range, qstep_lmbda_exp=args.qstep_lambda_exp, qmap_rects=args.qmap_rects,
                      qmap_aq=args.qmap_aq)
    lr_scheduler = PlateauLR(trainer, factor=0.6, patience=6)
    criterion = RateDistortionLoss(lmbda=args.lmbda, metric=args.metric)
    if ck is not None and "optimizer" in ck and isinstance(ck["optimizer"], dict) and "m" in ck["optimizer"]:
        trainer.load_optimizer_state(ck["optimizer"], ck.get("aux_optimizer"))
        if "lr_scheduler" in ck:
            lr_scheduler.load_state_dict(ck["lr_scheduler"])

    best_loss = float("inf")
    for epoch in range(last_epoch, args.epochs):
        if rank == 0:
            print(f"Learning rate: {trainer.lr}")
        if sampler is not None:
            sampler.set_epoch(epoch)
        train_one_epoch(trainer, train_dataloader, epoch)
        if epoch % args.test_every == 0:
            if args.qstep_range is not None:
                loss = qstep_test_epoch(epoch, test_dataloader, trainer.model, criterion, args.lmbda,
                                        args.qstep_lambda_exp, args.qstep_range, verbose=rank == 0,
                                        qmap_rects=args.qmap_rects, qmap_aq=args.qmap_aq)
            else:
                loss = test_epoch(epoch, test_dataloader, trainer.model, criterion, verbose=rank == 0)
            lr_scheduler.step(loss)
            is_best = loss < best_loss
            best_loss = min(loss, best_loss)
            if args.save and is_best and rank == 0:
                opt, aux = trainer.optimizer_state()
                save_checkpoint(checkpoint_state(epoch, trainer.model.state_dict(), loss, opt, aux,
                                                 lr_scheduler.state_dict(), args.qstep_range, args.qstep_lambda_exp,
                                                 args.qmap_rects, args.qmap_aq),
                                os.path.join(args.save_path, f"{epoch}.ckpt"))
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
