"""GPU: the 8-bit image boundary kernels (csrc/imageio.hip) against the host path they stand in for -- ToTensor +
pad_to_multiple on the way in, crop + clamp + x255 + truncation on the way out -- and against numpy.  Everything here
is bit-exact: the quotient v / 255 is the correctly rounded one, the squared-error sum is integer work.

NaN input to icm_image_f32_to_u8 is unspecified and not tested."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SIZES = [(256, 256), (175, 201), (64, 63), (1, 1), (161, 500)]


def _image(h, w, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    n = min(a.size, 768)
    a.reshape(-1)[:n] = np.repeat(np.arange(256, dtype=np.uint8), 3)[:n]      # every byte value in every channel
    return a


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _host_in(a):
    """the path the kernel replaces: ToTensor on the host, f32 to the device, pad_to_multiple"""
    from icm_amd.datasets import ToTensor
    from icm_amd.utils import pad_to_multiple
    return pad_to_multiple(ToTensor()(a)[None].to(DEV), 64)


def _u8_to_f32_raw(src_ptr, h, w, out, top, left):
    from icm_amd import _lib as L
    return L.lib().icm_image_u8_to_f32(src_ptr, h, w, out.data_ptr(), out.size(2), out.size(3), top, left, L.stream())


@pytest.mark.parametrize("h,w", SIZES)
def test_u8_to_f32_equals_totensor_and_pad_bit_for_bit(h, w):
    from icm_amd import codec
    a = _image(h, w, 7 * h + w)
    want, pads = _host_in(a)
    assert pads == codec.center_pads(h, w)
    got = codec.image_u8_to_f32(torch.from_numpy(a).to(DEV), pads)
    assert got.shape == want.shape and torch.equal(_bits(got), _bits(want))
    # every element is written: a buffer of NaNs comes back with +0.0 (all bits clear) around the image
    left, right, top, bottom = pads
    out = torch.full_like(want, float("nan"))
    assert _u8_to_f32_raw(torch.from_numpy(a).to(DEV).data_ptr(), h, w, out, top, left) == 0
    assert torch.equal(_bits(out), _bits(want))
    mask = torch.ones(out.shape[-2:], dtype=torch.bool)
    mask[top:top + h, left:left + w] = False
    assert (_bits(out)[0, :, mask] == 0).all()


@pytest.mark.parametrize("h,w,off,OH,OW,top,left", [
    (37, 53, 1, 64, 64, 13, 5),       # source one byte past an aligned allocation: no run is 16-byte aligned
    (37, 48, 1, 64, 64, 0, 16),
    (20, 40, 0, 23, 45, 2, 3),        # output width not a multiple of 4: scalar stores, a 13-pixel run at the row end
    (9, 16, 0, 9, 16, 0, 0),          # no padding at all, one full aligned run per row
    (5, 100, 3, 8, 108, 3, 8),
])
def test_u8_to_f32_tail_paths(h, w, off, OH, OW, top, left):
    a = _image(h, w, h * 1000 + w + off)
    buf = torch.zeros(off + a.size + 64, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    buf[off:off + a.size] = torch.from_numpy(a).to(DEV).reshape(-1)
    out = torch.full((1, 3, OH, OW), float("nan"), dtype=torch.float32, device=DEV)
    assert _u8_to_f32_raw(buf.data_ptr() + off, h, w, out, top, left) == 0
    want = np.zeros((3, OH, OW), dtype=np.float32)
    want[:, top:top + h, left:left + w] = a.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0)
    assert np.array_equal(out[0].cpu().numpy().view(np.int32), want.view(np.int32))


def _adversarial_planes(PH, PW, seed):
    """values around every quantisation boundary: exact 0 and 1, k/255 and its f32 neighbours, negatives, > 1"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 256, size=(3, PH, PW)).astype(np.float32)
    x = k / np.float32(255.0)
    step = rng.integers(-2, 3, size=x.shape)
    for s in (-2, -1, 1, 2):
        m = step == s
        y = x.copy()
        for _ in range(abs(s)):
            y = np.nextafter(y, np.float32(-9.0 if s < 0 else 9.0), dtype=np.float32)
        x[m] = y[m]
    noise = rng.random(size=x.shape, dtype=np.float32)
    pick = rng.integers(0, 8, size=x.shape)
    x[pick == 0] = noise[pick == 0]
    x[pick == 1] = (noise[pick == 1] - 0.5) * 4.0          # negatives and values above 1
    flat = x.reshape(-1)
    special = np.array([0.0, -0.0, 1.0, np.nextafter(np.float32(1.0), np.float32(0.0)), 1.0 + 2.0 ** -23, -1e-30, 1e-30,
                        -5.0, 7.5, 0.5, 254.0 / 255.0, 1.0 / 255.0], dtype=np.float32)
    flat[:min(flat.size, special.size)] = special[:flat.size]
    return x


def _want_u8(xs, pads):
    from icm_amd.utils import crop
    c = crop(xs, pads)
    return (c.clamp(0, 1) * 255.0).to(torch.uint8)[0].permute(1, 2, 0).contiguous().cpu().numpy()


@pytest.mark.parametrize("h,w", SIZES)
def test_f32_to_u8_equals_crop_clamp_scale_truncate(h, w):
    from icm_amd import codec
    pads = codec.center_pads(h, w)
    PH, PW = h + pads[2] + pads[3], w + pads[0] + pads[1]
    xs = torch.from_numpy(_adversarial_planes(PH, PW, 3 * h + w))[None].to(DEV)
    want = _want_u8(xs, pads)
    # the reference value restated in numpy: f32 product, truncation
    xc = xs[0].cpu().numpy()[:, pads[2]:pads[2] + h, pads[0]:pads[0] + w]
    assert np.array_equal(want, (np.clip(xc, 0, 1) * np.float32(255.0)).astype(np.uint8).transpose(1, 2, 0))
    got, sse = codec.image_f32_to_u8(xs, pads)
    assert sse is None and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    # with a reference: same bytes, and the exact int64 sum of squared differences
    ref = _image(h, w, 11 * h + w)
    got2, sse = codec.image_f32_to_u8(xs, pads, torch.from_numpy(ref).to(DEV))
    assert np.array_equal(got2.cpu().numpy(), want)
    d = want.astype(np.int64) - ref.astype(np.int64)
    assert sse.dtype == torch.int64 and int(sse.item()) == int((d * d).sum())


@pytest.mark.parametrize("h,w,PH,PW,top,left,off", [
    (30, 50, 40, 61, 3, 7, 1),       # odd plane size, odd window origin, dst / ref one byte past an aligned allocation
    (16, 64, 16, 64, 0, 0, 0),       # everything aligned: the 16-byte paths on all three sides
    (16, 64, 17, 67, 1, 3, 0),       # aligned bytes, unaligned floats
    (7, 33, 8, 36, 0, 0, 16),        # a one-pixel run at the row end
])
def test_f32_to_u8_tail_paths(h, w, PH, PW, top, left, off):
    from icm_amd import _lib as L
    x = _adversarial_planes(PH, PW, PH * 100 + PW)
    xs = torch.from_numpy(x).to(DEV)
    ref = _image(h, w, h + w + off)
    n = h * w * 3
    dbuf = torch.full((off + n + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    rbuf = torch.zeros(off + n + 64, dtype=torch.uint8, device=DEV)
    rbuf[off:off + n] = torch.from_numpy(ref).to(DEV).reshape(-1)
    nws = int(L.lib().icm_image_workspace_bytes(h, w))
    assert nws > 0 and nws % 8 == 0
    ws = torch.zeros(nws // 8, dtype=torch.int64, device=DEV)
    sse = torch.zeros((), dtype=torch.int64, device=DEV)
    rc = L.lib().icm_image_f32_to_u8(xs.data_ptr(), PH, PW, top, left, dbuf.data_ptr() + off, h, w, rbuf.data_ptr() + off,
                                     sse.data_ptr(), ws.data_ptr(), nws, L.stream())
    assert rc == 0
    want = (np.clip(x[:, top:top + h, left:left + w], 0, 1) * np.float32(255.0)).astype(np.uint8).transpose(1, 2, 0)
    got = dbuf.cpu().numpy()
    assert np.array_equal(got[off:off + n].reshape(h, w, 3), want)
    assert (got[:off] == 0xAB).all() and (got[off + n:] == 0xAB).all()      # nothing written outside the image
    d = want.astype(np.int64) - ref.astype(np.int64)
    assert int(sse.item()) == int((d * d).sum())


def test_squared_error_sum_beyond_32_bits_and_repeatable():
    from icm_amd import codec
    h, w = 301, 257                                   # 301 * 257 * 3 * 255^2 = 1.5e10 > 2^32
    xs = torch.zeros((1, 3, h, w), dtype=torch.float32, device=DEV)
    ref = torch.full((h, w, 3), 255, dtype=torch.uint8, device=DEV)
    out, sse = codec.image_f32_to_u8(xs, (0, 0, 0, 0), ref)
    assert int(out.max().item()) == 0
    assert int(sse.item()) == h * w * 3 * 255 * 255 > 2 ** 32
    x = torch.from_numpy(_adversarial_planes(h, w, 5))[None].to(DEV)
    r = torch.from_numpy(_image(h, w, 6)).to(DEV)
    a, sa = codec.image_f32_to_u8(x, (0, 0, 0, 0), r)
    b, sb = codec.image_f32_to_u8(x, (0, 0, 0, 0), r)
    assert torch.equal(a, b) and int(sa.item()) == int(sb.item())
    d = a.cpu().numpy().astype(np.int64) - r.cpu().numpy().astype(np.int64)
    assert int(sa.item()) == int((d * d).sum())


def test_argument_errors_return_the_code_and_launch_nothing():
    from icm_amd import _lib as L
    lib = L.lib()
    st = L.stream()
    src = torch.full((8, 8, 3), 9, dtype=torch.uint8, device=DEV)
    dst = torch.full((1, 3, 16, 16), -7.0, dtype=torch.float32, device=DEV)
    out = torch.full((8, 8, 3), 0xCD, dtype=torch.uint8, device=DEV)
    ws = torch.full((4,), -1, dtype=torch.int64, device=DEV)
    sse = torch.full((), -1, dtype=torch.int64, device=DEV)
    s, d, o = src.data_ptr(), dst.data_ptr(), out.data_ptr()
    ERR = 1
    bad_in = [(0, 8, 8, d, 16, 16, 4, 4), (s, 8, 8, 0, 16, 16, 4, 4), (s, 0, 8, d, 16, 16, 4, 4), (s, 8, -1, d, 16, 16, 4, 4),
              (s, 8, 8, d, 0, 16, 0, 0), (s, 8, 8, d, 16, 16, 9, 4), (s, 8, 8, d, 16, 16, 4, 9), (s, 8, 8, d, 16, 16, -1, 4),
              (s, 8, 8, d, 16, 16, 4, -1), (s, 40000, 8, d, 40008, 16, 4, 4)]
    for a in bad_in:
        assert lib.icm_image_u8_to_f32(*a, st) == ERR, a
    r = src.data_ptr()
    w, q, nb = ws.data_ptr(), sse.data_ptr(), 32
    bad_out = [(0, 16, 16, 4, 4, o, 8, 8, 0, 0, 0, 0), (d, 16, 16, 4, 4, 0, 8, 8, 0, 0, 0, 0),
               (d, 16, 16, 4, 4, o, 0, 8, 0, 0, 0, 0), (d, 16, 16, 4, 4, o, 8, -3, 0, 0, 0, 0),
               (d, 0, 16, 0, 0, o, 8, 8, 0, 0, 0, 0),
               (d, 16, 16, 9, 4, o, 8, 8, 0, 0, 0, 0), (d, 16, 16, 4, 9, o, 8, 8, 0, 0, 0, 0),    # window outside the source
               (d, 16, 16, -1, 4, o, 8, 8, 0, 0, 0, 0), (d, 16, 16, 4, -1, o, 8, 8, 0, 0, 0, 0),
               (d, 16, 16, 4, 4, o, 8, 8, r, q, w, 7),                                            # short workspace
               (d, 16, 16, 4, 4, o, 8, 8, r, q, 0, nb), (d, 16, 16, 4, 4, o, 8, 8, r, 0, w, nb)]  # ref without ws / sse
    for a in bad_out:
        assert lib.icm_image_f32_to_u8(*a, st) == ERR, a
    assert lib.icm_image_workspace_bytes(0, 8) == 0 and lib.icm_image_workspace_bytes(8, -1) == 0
    assert lib.icm_image_workspace_bytes(8, 8) == 8 and lib.icm_image_workspace_bytes(3000, 4000) == 8 * 2930
    torch.cuda.synchronize()
    assert (dst == -7.0).all() and (out == 0xCD).all() and (ws == -1).all() and int(sse.item()) == -1
    # and the wrappers turn the code into ValueError
    from icm_amd import codec
    with pytest.raises(ValueError):
        codec.image_f32_to_u8(dst, (8, 8, 0, 0))
    with pytest.raises(ValueError):
        codec.image_f32_to_u8(dst, (4, 4, 4, 4), torch.zeros((8, 9, 3), dtype=torch.uint8, device=DEV))
