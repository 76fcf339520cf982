"""CPU: the host side of the device-resident training data (icm_amd/datasets.py): ``crop_window`` against the crop
transforms themselves, the arena layout and the descriptor checks of ``DeviceImageCache``, ``EpochSampler``, and the
``--device-cache`` flag.  Nothing here needs a device: the layout and the descriptors are plain functions."""
import itertools
import os
import random
import sys

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "image-compression-for-machine_amd"))
from icm_amd import datasets as D  # noqa: E402

CROPS = [(48, 64), (17, 19)]


def _coded(h, w):
    """R = x + 1, G = y + 1 (sides <= 250): every pixel names its own position and differs from padding zeros"""
    a = np.zeros((h, w, 3), np.uint8)
    a[:, :, 0] = np.arange(1, w + 1, dtype=np.uint8)[None, :]
    a[:, :, 1] = np.arange(1, h + 1, dtype=np.uint8)[:, None]
    a[:, :, 2] = 200
    return a


def _window(a, y0, x0, ch, cw):
    """the numpy crop of a window: zeros outside the image"""
    h, w = a.shape[:2]
    out = np.zeros((ch, cw, 3), np.uint8)
    ys, ye, xs, xe = max(y0, 0), min(y0 + ch, h), max(x0, 0), min(x0 + cw, w)
    if ys < ye and xs < xe:
        out[ys - y0:ye - y0, xs - x0:xe - x0] = a[ys:ye, xs:xe]
    return out


def _sides(c):
    """smaller than, equal to and larger than the crop side c, with odd and even differences"""
    return [c - 6, c - 3, c - 1, c, c + 1, c + 2, c + 7, c + 40]


def _cases():
    for ch, cw in CROPS:
        for h, w in itertools.product(_sides(ch), _sides(cw)):     # each axis independently
            yield h, w, ch, cw


@pytest.mark.parametrize("ch,cw", CROPS)
def test_crop_window_is_center_crop(ch, cw):
    n = 0
    for h, w, c1, c2 in _cases():
        if (c1, c2) != (ch, cw):
            continue
        a = _coded(h, w)
        want = np.asarray(D.CenterCrop((ch, cw))(Image.fromarray(a)))
        y0, x0 = D.crop_window("center", h, w, ch, cw)
        assert np.array_equal(_window(a, y0, x0, ch, cw), want), (h, w, y0, x0)
        n += 1
    assert n == 64


@pytest.mark.parametrize("ch,cw", CROPS)
def test_crop_window_is_random_crop_under_the_same_seed(ch, cw):
    t = D.RandomCrop((ch, cw), pad_if_needed=True)
    for h, w, c1, c2 in _cases():
        if (c1, c2) != (ch, cw):
            continue
        a = _coded(h, w)
        im = Image.fromarray(a)
        for s in (0, 1, 5, 1234):
            random.seed(s)
            want = [np.asarray(t(im)) for _ in range(3)]
            after_t = random.random()
            random.seed(s)
            wins = [D.crop_window("random", h, w, ch, cw) for _ in range(3)]
            assert random.random() == after_t                       # the same number of draws, in the same order
            for (y0, x0), wnt in zip(wins, want):
                assert np.array_equal(_window(a, y0, x0, ch, cw), wnt), (h, w, s, y0, x0)
    # a private generator is used when one is given, and the global one is left alone
    random.seed(3)
    state = random.getstate()
    r1, r2 = random.Random(9), random.Random(9)
    assert D.crop_window("random", 100, 90, ch, cw, rng=r1) == D.crop_window("random", 100, 90, ch, cw, rng=r2)
    assert random.getstate() == state
    with pytest.raises(ValueError):
        D.crop_window("middle", 10, 10, 4, 4)


def test_arena_layout():
    sizes = [(37, 53), (64, 48), (1, 1), (130, 70), (16, 16)]
    off, total = D.arena_layout(sizes)
    assert off.dtype == np.int64 and list(off % 16) == [0] * 5 and off[0] == 0
    need = [-(-3 * h * w // 16) * 16 for h, w in sizes]
    assert list(off) == list(np.cumsum([0] + need[:-1])) and total == sum(need)
    assert all(off[i] + 3 * h * w <= (off[i + 1] if i + 1 < len(sizes) else total) for i, (h, w) in enumerate(sizes))
    assert D.arena_layout(sizes, budget_bytes=total)[1] == total           # exactly at the budget fits
    with pytest.raises(ValueError, match=str(total)):                      # the message names the bytes needed
        D.arena_layout(sizes, budget_bytes=total - 1)
    with pytest.raises(ValueError):
        D.arena_layout([(0, 5)])
    with pytest.raises(ValueError):
        D.arena_layout([(5, 40000)])


def test_crop_descriptors_are_checked_against_the_table():
    sizes = [(37, 53), (64, 48), (1, 1)]
    off, _ = D.arena_layout(sizes)
    d = D.crop_descriptors(off, sizes, [2, 0, 0], [(-3, 4), (0, 0), (30, -60)], 48, 64)
    assert d.dtype.itemsize == 24 and d.tobytes() == b"".join(
        np.array([o], "<i8").tobytes() + np.array(r, "<i4").tobytes()
        for o, r in [(off[2], (1, 1, -3, 4)), (0, (37, 53, 0, 0)), (0, (37, 53, 30, -60))])
    for bad in ([3], [-1], [1.0], ["0"]):
        with pytest.raises(IndexError):
            D.crop_descriptors(off, sizes, bad, [(0, 0)], 8, 8)
    with pytest.raises(ValueError):
        D.crop_descriptors(off, sizes, [], [], 8, 8)
    with pytest.raises(ValueError):
        D.crop_descriptors(off, sizes, [0, 1], [(0, 0)], 8, 8)
    with pytest.raises(ValueError):
        D.crop_descriptors(off, sizes, [0], [(2 ** 31 - 5, 0)], 8, 8)       # would overflow the kernel's 32-bit sums
    with pytest.raises(ValueError):
        D.crop_descriptors(off, sizes, [0], [(0, -40000)], 8, 8)
    for ch, cw in ((0, 8), (8, 32769)):
        with pytest.raises(ValueError):
            D.crop_descriptors(off, sizes, [0], [(0, 0)], ch, cw)


def test_cache_refuses_an_over_budget_or_empty_split_before_touching_a_device(tmp_path):
    d = tmp_path / "train"
    d.mkdir()
    (tmp_path / "empty").mkdir()
    for i, (h, w) in enumerate([(20, 30), (9, 7)]):
        Image.fromarray(_coded(h, w)).save(d / f"i{i}.png")
    need = 1808 + 192
    with pytest.raises(ValueError, match=f"{need} bytes"):
        D.DeviceImageCache(str(tmp_path), "train", "cuda:0", need - 1)     # raised from the headers alone
    with pytest.raises(RuntimeError) as missing:
        D.ImageFolder(str(tmp_path), split="nope")
    for split in ("nope", "empty"):
        with pytest.raises(RuntimeError) as ei:
            D.DeviceImageCache(str(tmp_path), split, "cuda:0", 10 ** 9)
        assert str(ei.value) == str(missing.value)


def test_epoch_sampler():
    n = 10
    s = D.EpochSampler(n, 4, seed=7)
    a = s.indices(0)
    assert a == D.EpochSampler(n, 4, seed=7).indices(0) and sorted(a) == list(range(n))
    assert s.indices(1) != a and sorted(s.indices(1)) == list(range(n))
    assert D.EpochSampler(n, 4, seed=8).indices(0) != a
    batches = list(s)
    assert len(s) == 3 and [len(b) for b in batches] == [4, 4, 2] and sum(batches, []) == a    # short last batch kept
    s.set_epoch(1)
    assert sum(list(s), []) == s.indices(1)
    assert D.EpochSampler(n, 4, seed=7, shuffle=False).indices(3) == list(range(n))
    for world in (1, 2, 3):
        ranks = [D.EpochSampler(n, 2, seed=7, rank=r, world=world) for r in range(world)]
        got = [r.indices(2) for r in ranks]
        assert all(len(g) == n // world for g in got)
        flat = sum(got, [])
        assert len(set(flat)) == len(flat) and set(flat) <= set(range(n))                      # disjoint
        assert all(all(len(b) == 2 for b in r) or world == 1 for r in ranks)
        assert len({len(r) for r in ranks}) == 1 and all(len(list(r)) == len(r) for r in ranks)
    with pytest.raises(ValueError):
        D.EpochSampler(n, 2, seed=0, rank=2, world=2)


def test_train_cli_has_the_flag():
    from icm_amd import train as T
    assert T.parse_args(["-d", "root"]).device_cache == 0
    assert T.parse_args(["-d", "root", "--device-cache", "1.5"]).device_cache == 1.5
