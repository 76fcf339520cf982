"""MI355X: ``icm_qmap_aq`` through the C ABI against the float64 reference of tests/_aq_ref.py (inputs and references:
tests/_qmap_aq_inputs.py).

Exactness.  The integer statistics are exact on both sides, so device and reference can differ only through the last
bits of log2 and of the mean: L <= log2(16257) < 14, one ulp is below 2e-15; a fixed-order sum of at most 256 such terms
is off by less than 1e-12; times 4 |S| <= 16 that is below 2e-11 on the value that is rounded.  So the map must equal
the reference EXACTLY on every cell whose reference value 4 S (L - mean) lies more than 1e-9 (50 times the bound) from
a half-integer, and tests/test_qmap_aq_ref.py asserts that no cell of any case here lies closer: every cell is
compared.  ``ref`` is held to 1e-12 absolutely.

The shapes are the smallest at which the kernels can go wrong: 3 x 5 cells (h != w, a cell count that is no multiple
of a wave or a workgroup), 4 x 4, and 8 x 12 with two images."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "image-compression-for-machine_amd"))
import _qmap_aq_inputs as I  # noqa: E402
import _qmtrain_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = 1
GARBAGE = 0x7f


def lib():
    from icm_amd import _lib
    return _lib


def ws_bytes(N, H, W):
    return int(lib().lib().icm_qmap_aq_workspace_bytes(N, H, W))


def run(x, strength, base, rects):
    """one call on numpy inputs with ``qmap``, ``ref`` and ``ws`` pre-filled with garbage and guard bytes around the
    map -> (maps int8 [N, h, w], ref float64 [N])"""
    L = lib()
    N, _, H, W = x.shape
    h, w = H // 16, W // 16
    xd = torch.from_numpy(x).to(DEV).contiguous()
    sd, bd = torch.from_numpy(strength).to(DEV), torch.from_numpy(base).to(DEV)
    R = 0 if rects is None else rects.shape[1]
    rd = None if rects is None else torch.from_numpy(rects).to(DEV).contiguous()
    buf = torch.full((N * h * w + 64,), GARBAGE, dtype=torch.int8, device=DEV)
    ref = torch.full((N,), float("nan"), dtype=torch.float64, device=DEV)
    nb = ws_bytes(N, H, W)
    assert nb == N * h * w * 8
    ws = torch.full((nb // 8,), float("nan"), dtype=torch.float64, device=DEV)
    L.check(L.lib().icm_qmap_aq(xd.data_ptr(), N, H, W, bd.data_ptr(), sd.data_ptr(), L.ptr(rd), R, buf.data_ptr() + 32,
                                ref.data_ptr(), ws.data_ptr(), nb, L.stream()), "qmap_aq")
    got = buf.cpu().numpy()
    assert (got[:32] == GARBAGE).all() and (got[32 + N * h * w:] == GARBAGE).all(), "written outside the maps"
    return got[32:32 + N * h * w].reshape(N, h, w).copy(), ref.cpu().numpy()


@pytest.fixture(scope="module")
def results():
    """every case run once, shared by the tests below and left unchanged"""
    return {name: run(*(I.case(name)[k] for k in (0, 2, 3, 4))) for name in I.CASES}


@pytest.mark.parametrize("name", sorted(I.CASES))
def test_maps_and_means_against_float64(results, name):
    maps, ref = results[name]
    r = I.reference(name)
    err = np.abs(ref - r["ref"]).max()
    print(f"{name}: mean activity {r['ref'].tolist()}, largest error {err:.3e} (limit {I.REF_LIMIT:.0e}); "
          f"map range {maps.min()} .. {maps.max()}")
    assert err <= I.REF_LIMIT
    assert I.check_maps(maps, r["map"], r["value"], name) == 0       # no cell was inside the zone: all were compared
    assert np.array_equal(maps, r["map"])


@pytest.mark.parametrize("name", sorted(I.CASES))
def test_two_runs_agree_bit_for_bit(results, name):
    maps, ref = run(*(I.case(name)[k] for k in (0, 2, 3, 4)))
    assert np.array_equal(maps, results[name][0])
    assert np.array_equal(ref.view(np.int64), results[name][1].view(np.int64))


@pytest.mark.parametrize("name", sorted(I.CASES))
def test_an_image_alone_gives_its_rows_of_the_batch(results, name):
    x, _, strength, base, rects = I.case(name)
    for n in range(x.shape[0]):
        maps, ref = run(x[n:n + 1], strength[n:n + 1], base[n:n + 1], None if rects is None else rects[n:n + 1])
        assert np.array_equal(maps[0], results[name][0][n]), f"{name}: image {n}"
        assert ref.view(np.int64)[0] == results[name][1].view(np.int64)[n], f"{name}: image {n}"


@pytest.mark.parametrize("name", sorted(n for n, c in I.CASES.items() if c[5] is not None))
def test_strength_zero_is_the_painter_byte_for_byte(name):
    L = lib()
    x, _, strength, base, rects = I.case(name)
    N, _, H, W = x.shape
    h, w = H // 16, W // 16
    maps, _ = run(x, np.zeros_like(strength), base, rects)
    painted = torch.full((N, h, w), GARBAGE, dtype=torch.int8, device=DEV)
    bd, rd = torch.from_numpy(base).to(DEV), torch.from_numpy(rects).to(DEV).contiguous()     # alive over the launch
    L.check(L.lib().icm_qmap_paint(bd.data_ptr(), rd.data_ptr(), rects.shape[1], painted.data_ptr(), N, h, w, L.stream()),
            "qmap_paint")
    assert np.array_equal(maps, painted.cpu().numpy())
    assert np.array_equal(maps, M.paint(base, rects, h, w))


def test_the_engine_form(results):
    from icm_amd import engine as E
    name = "mixed-64x64"
    x, _, strength, base, rects = I.case(name)
    t = lambda a: torch.from_numpy(a).to(DEV)   # noqa: E731
    maps, ref = E.qmap_aq(t(x), t(base), t(strength), t(rects))
    assert maps.dtype == torch.int8 and ref.dtype == torch.float64
    assert np.array_equal(maps.cpu().numpy(), results[name][0]) and np.array_equal(ref.cpu().numpy(), results[name][1])
    plain, _ = E.qmap_aq(t(x), t(base), t(strength))
    assert np.array_equal(plain.cpu().numpy(), I.reference(name)["aq"])
    none, _ = E.qmap_aq(t(x), t(base), t(strength), t(rects)[:, :0].contiguous())
    assert torch.equal(none, plain)
    out, rbuf = torch.zeros_like(maps), torch.zeros_like(ref)
    ws = E.qmap_aq_workspace(2, 64, 64, torch.device(DEV))
    got = E.qmap_aq(t(x), t(base), t(strength), t(rects), out=out, ref=rbuf, ws=ws)
    assert got[0] is out and got[1] is rbuf and torch.equal(out, maps) and torch.equal(rbuf, ref)
    bad = [lambda: E.qmap_aq(t(x).double(), t(base), t(strength)), lambda: E.qmap_aq(t(x)[:, :2], t(base), t(strength)),
           lambda: E.qmap_aq(t(x)[:, :, :40].contiguous(), t(base), t(strength)),
           lambda: E.qmap_aq(t(x), t(base).to(torch.int32), t(strength)), lambda: E.qmap_aq(t(x), t(base)[:1], t(strength)),
           lambda: E.qmap_aq(t(x), t(base), t(strength).double()), lambda: E.qmap_aq(t(x), t(base), t(strength), t(rects)[:1]),
           lambda: E.qmap_aq(t(x), t(base), t(strength), t(rects).to(torch.int64)),
           lambda: E.qmap_aq(t(x).cpu(), t(base), t(strength)), lambda: E.qmap_aq(t(x), t(base), t(strength), out=out[:1]),
           lambda: E.qmap_aq(t(x), t(base), t(strength), ws=ws[:8]), lambda: E.qmap_aq_workspace(2, 64, 72, torch.device(DEV))]
    for f in bad:
        with pytest.raises(ValueError):
            f()


def test_refused_calls_write_nothing():
    L = lib().lib()
    st = lib().stream()
    N, H, W = 2, 64, 64
    x = torch.zeros((N, 3, H, W), dtype=torch.float32, device=DEV)
    base = torch.zeros(N, dtype=torch.int8, device=DEV)
    strength = torch.ones(N, dtype=torch.float32, device=DEV)
    rects = torch.zeros((N, 1, 5), dtype=torch.int32, device=DEV)
    out = torch.full((N * 16,), GARBAGE, dtype=torch.int8, device=DEV)
    ref = torch.full((N,), -1.0, dtype=torch.float64, device=DEV)
    nb = ws_bytes(N, H, W)
    ws = torch.zeros(nb // 8, dtype=torch.float64, device=DEV)

    def call(x_=x.data_ptr(), N_=N, H_=H, W_=W, b=base.data_ptr(), s=strength.data_ptr(), r=rects.data_ptr(), R=1,
             o=out.data_ptr(), f=ref.data_ptr(), w=ws.data_ptr(), wb=nb):
        return L.icm_qmap_aq(x_, N_, H_, W_, b, s, r, R, o, f, w, wb, st)
    rcs = [call(x_=0), call(b=0), call(s=0), call(o=0), call(f=0), call(w=0), call(r=0), call(N_=0), call(H_=0), call(W_=0),
           call(H_=-16), call(H_=72), call(W_=40), call(R=-1), call(wb=nb - 8), call(wb=0), call(N_=65536),
           call(x_=x.data_ptr() + 4), call(f=ref.data_ptr() + 4), call(w=ws.data_ptr() + 4)]
    torch.cuda.synchronize()
    assert rcs == [ERR_ARG] * len(rcs), rcs
    assert (out == GARBAGE).all() and (ref == -1.0).all(), "a refused call wrote"
    assert [ws_bytes(0, 64, 64), ws_bytes(2, 0, 64), ws_bytes(2, 64, 0), ws_bytes(2, 72, 64), ws_bytes(2, 64, 8),
            ws_bytes(65536, 64, 64), ws_bytes(-1, 64, 64)] == [0] * 7
    assert ws_bytes(3, 48, 80) == 3 * 15 * 8 and ws_bytes(1, 16, 16) == 8
    assert call() == 0 and call(r=0, R=0) == 0                      # complete arguments; no rectangles, rects null
    torch.cuda.synchronize()
    assert (out == 0).all() and (ref == 0.0).all()                  # black images: flat cells, mean 0, base 0
