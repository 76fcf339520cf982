"""compressai.datasets mirror (compressai/datasets/utils.py:23-89): the image-folder dataset the reference's training
script feeds the hot path with (train.py:404-425), plus the three torchvision transforms that script composes
(``CenterCrop`` / ``RandomCrop(pad_if_needed)`` / ``ToTensor``, train.py:393-402) -- torchvision is not a dependency
here, so they are restated on PIL + numpy with torchvision's semantics (centre offset rounding, zero padding, CHW f32
in [0, 1]).  That part is host-side data plumbing.

The second half keeps a split resident on the device instead: ``DeviceImageCache`` decodes every sample once to 8-bit
RGB, packs the bytes into one device tensor and cuts each training batch out of it with one launch of
``icm_image_batch_u8_to_f32`` (csrc/imageio.hip); ``crop_window`` gives the window the two crop transforms would cut,
``EpochSampler`` the order of an epoch, ``DeviceCacheLoader`` the object the training loop iterates over."""
from __future__ import annotations

import math
import random
from pathlib import Path
from typing import Callable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from PIL import Image
from torch.utils.data import Dataset

IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")   # eval_model/__main__.py:56-67


class ImageFolder(Dataset):
    """``rootdir/<split>/*``: every regular file of the split directory is a sample (datasets/utils.py:46-55);
    ``__getitem__`` opens it as RGB and applies ``transform`` (:57-86)."""

    def __init__(self, root, transform: Optional[Callable] = None, split: str = "train"):
        splitdir = Path(root) / split
        if not splitdir.is_dir():
            raise RuntimeError(f'Invalid directory "{root}"')
        self.samples = sorted(f for f in splitdir.iterdir() if f.is_file())
        self.transform = transform

    def __getitem__(self, index):
        img = Image.open(self.samples[index]).convert("RGB")
        if self.transform:
            return self.transform(img)
        return img

    def __len__(self):
        return len(self.samples)


def _size2(size) -> Tuple[int, int]:
    if isinstance(size, (int, float)):
        return int(size), int(size)
    if len(size) == 1:
        return int(size[0]), int(size[0])
    return int(size[0]), int(size[1])


def _pad(img: Image.Image, left: int, top: int, right: int, bottom: int) -> Image.Image:
    if not (left or top or right or bottom):
        return img
    out = Image.new(img.mode, (img.width + left + right, img.height + top + bottom), 0)
    out.paste(img, (left, top))
    return out


class Compose:
    def __init__(self, transforms: Sequence[Callable]):
        self.transforms = list(transforms)

    def __call__(self, img):
        for t in self.transforms:
            img = t(img)
        return img


class ToTensor:
    """PIL RGB (or HxWxC uint8 array) -> f32 [C,H,W] in [0, 1]"""

    def __call__(self, img) -> torch.Tensor:
        a = np.asarray(img)
        if a.ndim == 2:
            a = a[:, :, None]
        t = torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))
        return t.to(torch.float32).div_(255.0) if t.dtype == torch.uint8 else t.to(torch.float32)


class CenterCrop:
    """torchvision semantics: images smaller than the crop are zero-padded symmetrically first (extra pixel on the
    right / bottom), the crop offset is ``round((size - crop) / 2)``"""

    def __init__(self, size):
        self.size = _size2(size)

    def __call__(self, img: Image.Image) -> Image.Image:
        ch, cw = self.size
        w, h = img.size
        if cw > w or ch > h:
            pl, pt = max((cw - w) // 2, 0), max((ch - h) // 2, 0)
            pr, pb = max((cw - w + 1) // 2, 0), max((ch - h + 1) // 2, 0)
            img = _pad(img, pl, pt, pr, pb)
            w, h = img.size
            if (cw, ch) == (w, h):
                return img
        top, left = int(round((h - ch) / 2.0)), int(round((w - cw) / 2.0))
        return img.crop((left, top, left + cw, top + ch))


class RandomCrop:
    """uniform crop position (Python ``random``: seeded by train.py:388-390's ``random.seed``); ``pad_if_needed`` zero-pads
    both sides of a too-small axis like torchvision"""

    def __init__(self, size, pad_if_needed: bool = False):
        self.size = _size2(size)
        self.pad_if_needed = pad_if_needed

    def __call__(self, img: Image.Image) -> Image.Image:
        ch, cw = self.size
        w, h = img.size
        if self.pad_if_needed and w < cw:
            img = _pad(img, cw - w, 0, cw - w, 0)
        if self.pad_if_needed and h < ch:
            img = _pad(img, 0, ch - h, 0, ch - h)
        w, h = img.size
        if w < cw or h < ch:
            raise ValueError(f"Required crop size {(ch, cw)} is larger than input image size {(h, w)}")
        top = random.randint(0, h - ch)
        left = random.randint(0, w - cw)
        return img.crop((left, top, left + cw, top + ch))


def to_pil_image(x: torch.Tensor) -> Image.Image:
    """f32 [3,H,W] in [0,1] -> PIL RGB (torchvision ToPILImage: x*255 truncated to uint8; eval_model/__main__.py:89-94)"""
    a = x.detach().to("cpu", torch.float32).mul(255.0).to(torch.uint8).numpy()
    return Image.fromarray(np.ascontiguousarray(a.transpose(1, 2, 0)), mode="RGB")


# ---- device-resident training data ------------------------------------------------------------------------------

ARENA_ALIGN = 16          # every image starts on a 16-byte boundary of the arena
MAX_SIDE = 32768          # csrc/imageio.hip
CROP_DESC = np.dtype([("offset", "<i8"), ("H", "<i4"), ("W", "<i4"), ("y0", "<i4"), ("x0", "<i4")])   # icm_crop_desc
assert CROP_DESC.itemsize == 24


def crop_window(kind: str, h: int, w: int, ch: int, cw: int, rng=random) -> Tuple[int, int]:
    """``(y0, x0)`` of the ``ch x cw`` window that ``CenterCrop`` (kind "center") or ``RandomCrop(pad_if_needed=True)``
    (kind "random") cuts from an ``h x w`` image, in the coordinates of the unpadded image: zero padding shows as
    negative ``y0`` / ``x0`` or a window that runs past the image.  "random" draws ``rng.randint`` for the row, then
    for the column, with the transform's own bounds, so ``rng=random`` under one seed gives the transform's window."""
    if kind == "center":
        pt, pl = max((ch - h) // 2, 0), max((cw - w) // 2, 0)            # the extra pixel goes right / bottom
        hp, wp = max(h, ch), max(w, cw)
        return int(round((hp - ch) / 2.0)) - pt, int(round((wp - cw) / 2.0)) - pl
    if kind == "random":
        pl = cw - w if w < cw else 0                                       # both sides of a too-small axis
        pt = ch - h if h < ch else 0
        top = rng.randint(0, h + 2 * pt - ch)
        left = rng.randint(0, w + 2 * pl - cw)
        return top - pt, left - pl
    raise ValueError(f"unknown crop kind {kind!r}")


def arena_layout(sizes: Sequence[Tuple[int, int]], budget_bytes: Optional[int] = None) -> Tuple[np.ndarray, int]:
    """byte offset of every ``[h, w, 3]`` image packed in order, each on a 16-byte boundary, and the arena's size;
    ``ValueError`` naming the bytes needed when that exceeds ``budget_bytes``"""
    offsets = np.zeros(len(sizes), dtype=np.int64)
    total = 0
    for i, (h, w) in enumerate(sizes):
        if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
            raise ValueError(f"image {i}: size {h}x{w} outside 1..{MAX_SIDE}")
        offsets[i] = total
        total += -(-3 * h * w // ARENA_ALIGN) * ARENA_ALIGN
    if budget_bytes is not None and total > budget_bytes:
        raise ValueError(f"device cache needs {total} bytes for {len(sizes)} images, budget is {int(budget_bytes)} bytes")
    return offsets, total


def crop_descriptors(offsets: np.ndarray, sizes: Sequence[Tuple[int, int]], indices: Sequence[int],
                     windows: Sequence[Tuple[int, int]], ch: int, cw: int) -> np.ndarray:
    """the ``icm_crop_desc`` records of one batch, every index and window checked against the table (the kernel trusts
    them): indices in ``0..n-1``, window origins within ``MAX_SIDE`` of the image, crop sides in ``1..MAX_SIDE``"""
    n = len(offsets)
    if len(indices) < 1 or len(indices) != len(windows):
        raise ValueError(f"{len(indices)} indices for {len(windows)} windows")
    if not (1 <= ch <= MAX_SIDE and 1 <= cw <= MAX_SIDE):
        raise ValueError(f"crop {ch}x{cw} outside 1..{MAX_SIDE}")
    desc = np.zeros(len(indices), dtype=CROP_DESC)
    for k, (i, (y0, x0)) in enumerate(zip(indices, windows)):
        if not (isinstance(i, (int, np.integer)) and 0 <= i < n):
            raise IndexError(f"sample index {i!r} outside 0..{n - 1}")
        if not (-MAX_SIDE <= y0 <= MAX_SIDE and -MAX_SIDE <= x0 <= MAX_SIDE):
            raise ValueError(f"window origin ({y0}, {x0}) outside +-{MAX_SIDE}")
        h, w = sizes[i]
        desc[k] = (offsets[i], h, w, y0, x0)
    return desc


class _DecodedBytes(Dataset):
    """sample i of an ``ImageFolder(transform=None)`` as a flat uint8 tensor plus its (h, w)"""

    def __init__(self, folder: ImageFolder):
        self.folder = folder

    def __len__(self):
        return len(self.folder)

    def __getitem__(self, index):
        a = np.array(self.folder[index])          # a writable copy: PIL's buffer is read-only
        return torch.from_numpy(a.reshape(-1)), a.shape[0], a.shape[1]


class DeviceImageCache:
    """A split decoded once to 8-bit RGB and kept on the device as one packed uint8 tensor.

    Samples are listed and opened exactly as ``ImageFolder`` does (``.convert("RGB")``); sizes come from the image
    headers first, so a split that does not fit ``budget_bytes`` raises ``ValueError`` before anything is allocated.
    The decode pass runs through a DataLoader with ``num_workers`` workers and fills the arena through one pinned
    staging buffer.  ``batch`` cuts ``[B, 3, ch, cw]`` f32 out of it in one kernel launch."""

    STAGING_BYTES = 64 << 20

    def __init__(self, root, split: str, device, budget_bytes: int, num_workers: int = 0):
        self.folder = ImageFolder(root, transform=None, split=split)
        if len(self.folder) == 0:
            raise RuntimeError(f'Invalid directory "{root}"')
        self.device = torch.device(device)
        self.sizes: List[Tuple[int, int]] = []
        for f in self.folder.samples:
            with Image.open(f) as im:
                self.sizes.append((im.height, im.width))
        self.offsets, self.nbytes = arena_layout(self.sizes, budget_bytes)
        self.arena = torch.empty(self.nbytes, dtype=torch.uint8, device=self.device)
        self._fill(num_workers)

    def __len__(self):
        return len(self.sizes)

    def _fill(self, num_workers: int) -> None:
        from torch.utils.data import DataLoader
        padded = np.diff(np.append(self.offsets, self.nbytes))
        stage = torch.zeros(max(self.STAGING_BYTES, int(padded.max())), dtype=torch.uint8).pin_memory()
        base = used = 0          # the staging buffer holds arena[base : base + used]

        def flush():
            self.arena[base:base + used].copy_(stage[:used], non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()     # the buffer is refilled next

        loader = DataLoader(_DecodedBytes(self.folder), batch_size=None, shuffle=False, num_workers=num_workers)
        for i, (data, h, w) in enumerate(loader):
            if (int(h), int(w)) != self.sizes[i] or data.numel() != 3 * int(h) * int(w):
                raise RuntimeError(f"{self.folder.samples[i]}: decoded size {int(h)}x{int(w)} differs from its header")
            if used + int(padded[i]) > stage.numel():
                flush()
                base, used = int(self.offsets[i]), 0
            stage[used:used + data.numel()] = data
            stage[used + data.numel():used + int(padded[i])] = 0
            used += int(padded[i])
        flush()

    def batch(self, indices: Sequence[int], windows: Sequence[Tuple[int, int]], ch: int, cw: int,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``out[b, c, y, x] = image[indices[b]][y0 + y, x0 + x, c] / 255`` with ``(y0, x0) = windows[b]`` and +0.0
        outside the image (ToTensor of the zero-padded crop, bit for bit)"""
        from . import _lib as L
        desc = crop_descriptors(self.offsets, self.sizes, indices, windows, ch, cw)
        B = len(desc)
        if out is None:
            out = torch.empty((B, 3, ch, cw), dtype=torch.float32, device=self.device)
        elif not (out.dtype == torch.float32 and out.device == self.arena.device and out.is_contiguous()
                  and tuple(out.shape) == (B, 3, ch, cw)):
            raise ValueError(f"out must be a contiguous f32 [{B}, 3, {ch}, {cw}] tensor on {self.arena.device}")
        host = torch.from_numpy(desc.view(np.uint8)).pin_memory()
        with torch.cuda.device(self.arena.device):
            dev = host.to(self.arena.device, non_blocking=True)
            L.check(L.lib().icm_image_batch_u8_to_f32(self.arena.data_ptr(), dev.data_ptr(), B, out.data_ptr(), ch, cw,
                                                      L.stream()), "image_batch_u8_to_f32")
        return out


class EpochSampler:
    """Batches of sample indices for one rank.  Epoch ``e`` is a permutation of ``0..n-1`` from a generator seeded by
    ``(seed, e)`` (the identity without ``shuffle``).  ``world > 1``: rank ``r`` takes every ``world``-th index from
    ``r``, truncated to ``n // world`` -- disjoint, equal-sized ranks, as ``DistributedSampler(drop_last=True)`` -- and
    a last partial batch is dropped like the DataLoader it stands in for; ``world == 1``: all ``n``, the last partial
    batch kept."""

    def __init__(self, n: int, batch_size: int, seed: int, rank: int = 0, world: int = 1, shuffle: bool = True):
        if n < 1 or batch_size < 1 or not 0 <= rank < world:
            raise ValueError(f"EpochSampler(n={n}, batch_size={batch_size}, rank={rank}, world={world})")
        self.n, self.batch_size, self.seed, self.rank, self.world, self.shuffle = n, batch_size, int(seed), rank, world, shuffle
        self.epoch = 0

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def indices(self, epoch: Optional[int] = None) -> List[int]:
        e = self.epoch if epoch is None else int(epoch)
        order = np.random.default_rng([self.seed, e]).permutation(self.n) if self.shuffle else np.arange(self.n)
        if self.world > 1:
            order = order[self.rank::self.world][:self.n // self.world]
        return [int(i) for i in order]

    def __len__(self):
        if self.world > 1:
            return self.n // self.world // self.batch_size
        return math.ceil(self.n / self.batch_size)

    def __iter__(self):
        idx = self.indices()
        for k in range(len(self)):
            yield idx[k * self.batch_size:(k + 1) * self.batch_size]


class DeviceCacheLoader:
    """what ``train_one_epoch`` / ``test_epoch`` iterate over when the split is device-resident: yields ``[B, 3, ch, cw]``
    device batches; the only host work per step is drawing the crop windows (``random``, like the transforms)"""

    def __init__(self, cache: DeviceImageCache, sampler: EpochSampler, kind: str, patch_size):
        self.dataset, self.sampler, self.kind = cache, sampler, kind
        self.ch, self.cw = _size2(patch_size)

    def __len__(self):
        return len(self.sampler)

    def __iter__(self):
        sizes = self.dataset.sizes
        for idx in self.sampler:
            windows = [crop_window(self.kind, *sizes[i], self.ch, self.cw) for i in idx]
            yield self.dataset.batch(idx, windows, self.ch, self.cw)
