"""The weight-packing kernels (icm_pack_weights_batch, icm_pack_weights) against a restatement of the packed layout.

Layout (csrc/conv_igemm.hip): per tap class, in build_classes order, a block of nchunks * ntaps * dst_ncot fragment
tiles of 64 lanes x 4 floats,
    wp[((chunk * ntaps + t) * dst_ncot + dst_cot_off + cot) * 64 + lane][j] = W[co = cot * 32 + (lane & 31)]
                                                                               [ci = chunk * 8 + 2 j + (lane >> 5)][tap t]
with exact +0.0 where co >= Cout or ci >= Cin; wino = 1 / 2 packs the 16 points of G g G^T (2: of the rotated kernel) as
taps.  `expected` writes that into a NaN-filled copy of the destination, so a whole-buffer comparison of bit patterns
also shows that the guard floats around the destination and the tiles of other members keep their NaN.

  wino = 0, nonneg = 0   bit for bit (a copy)
  wino = 1 / 2           `grid` weights (integers in [-2, 2]): G g G^T is a multiple of 1/4 below 2^24, exact in float32,
                         bit for bit; `real`: the rule of tests/_conv_ref.py applied to the packed tensor,
                         FACTOR * |U32 - U64|_max + FACTOR * 2^-24 * |U64|_max, U32 the float32 evaluation
  nonneg                 the same rule with make_inputs' float32 and float64 evaluations of max(w, bound)^2 - pedestal
  padded rows / channels exact +0.0 in every mode
Shapes: Cout in {1, 31, 32, 33, 80} x Cin in {1, 7, 8, 9, 40}: below, at and above a 32-row tile and an 8-channel chunk
(Cin = 40 is a 1x1 item of four chunks plus one of one); each is a few hundred floats to a few thousand."""
import pytest
import torch

import _conv_ref as R
import test_gpu_conv_numerics as T
from test_gpu_conv_numerics import Buf, NAN, TAIL, dense, pack_job, run_pack, same_bits

pytestmark = pytest.mark.gpu

COUTS, CINS = (1, 31, 32, 33, 80), (1, 7, 8, 9, 40)
# kernel, stride, pad, transposed: one tap class in raster order; four parity classes of 1-4 and of 4-9 taps; the
# stride-1 scatter; a 25-tap gather
ORDERS = [(1, 1, 0, 0), (3, 1, 1, 0), (5, 2, 2, 0), (3, 2, 1, 1), (5, 2, 2, 1), (3, 1, 1, 1), (5, 1, 2, 0)]


def G(Cout, Cin, k=3, stride=1, pad=None, transposed=0):
    return R.geom(1, 8, 8, k, stride, k // 2 if pad is None else pad, transposed, ch=(Cin, Cout))


def weights(g, which="grid", member=0):
    return R.make_inputs(R.case("pack", g, inputs=which, member=member))["w"]          # [Cout, Cin, KH, KW]


def wino_points(w, wino, dt):
    """[Cout, Cin, 16]: G g G^T, point 4 a + b; wino = 2 takes the kernel rotated by 180 degrees"""
    k = w.to(dt).flip(2, 3) if wino == 2 else w.to(dt)
    Gm = R.WINO_G.to(dt)
    return torch.einsum("ap,oipq,bq->oiab", Gm, k, Gm).reshape(w.shape[0], w.shape[1], 16)


def class_taps(g, wino):
    if wino:
        return [list(range(16))]
    return [[t.kidx for t in cl.taps] for cl in R.build_classes(g) if cl.taps]


def packed_floats(g, wino=0, dst_ncot=0):
    ncot = dst_ncot or R.cdiv(g.Cout, 32)
    return sum(R.cdiv(g.Cin, 8) * len(taps) * ncot * 256 for taps in class_taps(g, wino))


def expected(buf, off, values, g, wino=0, dst_ncot=0, dst_cot_off=0):
    """write the packed form of values [Cout, Cin, taps of the canonical weight or 16 points] into the float32 vector
    buf from float offset off on; returns the mask of the floats that hold padding"""
    Co, Ci = g.Cout, g.Cin
    ncot, nch = R.cdiv(Co, 32), R.cdiv(Ci, 8)
    dn = dst_ncot or ncot
    Wp = torch.zeros((ncot * 32, nch * 8, values.shape[2]), dtype=torch.float32)
    Wp[:Co, :Ci] = values
    real = torch.zeros((ncot * 32, nch * 8), dtype=torch.bool)
    real[:Co, :Ci] = True
    pad_mask = torch.zeros_like(buf, dtype=torch.bool)
    for taps in class_taps(g, wino):
        nt = len(taps)
        A = Wp[:, :, taps].reshape(ncot, 32, nch, 4, 2, nt).permute(2, 5, 0, 4, 1, 3)      # [chunk, t, cot, hh, col, j]
        P = (~real)[:, :, None].expand(-1, -1, nt).reshape(ncot, 32, nch, 4, 2, nt).permute(2, 5, 0, 4, 1, 3)
        n = nch * nt * dn * 256
        buf[off:off + n].view(nch, nt, dn, 2, 32, 4)[:, :, dst_cot_off:dst_cot_off + ncot] = A
        pad_mask[off:off + n].view(nch, nt, dn, 2, 32, 4)[:, :, dst_cot_off:dst_cot_off + ncot] = P
        off += n
    return pad_mask


class Dest:
    """a guarded NaN destination and what it has to hold after the jobs written into it"""

    def __init__(self, floats):
        self.buf = Buf(floats)
        self.want = self.buf.cpu0.clone()
        self.pad = torch.zeros_like(self.want, dtype=torch.bool)

    def expect(self, off, values, g, **kw):
        self.pad |= expected(self.want, self.buf.lead + off, values, g, **kw)

    def bitwise(self, what):
        got = self.buf.now()
        assert same_bits(got, self.want), "%s: %d floats differ" % (what, int((T.bits(got) != T.bits(self.want)).sum()))

    def within(self, limit, what):
        """guards and untouched tiles keep their NaN bits, padding is +0.0, the rest lies within limit of want"""
        got = self.buf.now()
        written = ~torch.isnan(self.want)
        assert same_bits(got[~written], self.want[~written]), what + ": wrote outside its tiles"
        assert int(T.bits(got[self.pad]).count_nonzero()) == 0, what + ": padding is not +0.0"
        err = (got[written].double() - self.want[written].double()).abs().max().item()
        assert err <= limit, "%s: off by %g, limit %g" % (what, err, limit)


def source(w, som, lead=4):
    return dense(w if som else w.permute(1, 0, 2, 3).contiguous(), lead)


@pytest.mark.parametrize("som", (1, 0), ids=("out-major", "in-major"))
@pytest.mark.parametrize("order", ORDERS, ids=lambda o: "k%ds%dp%d%s" % (o[0], o[1], o[2], "T" if o[3] else ""))
def test_every_channel_tail_and_tap_order_is_a_copy(order, som):
    """25 jobs (two launches) of every Cout x Cin tail for one tap order and source layout, bit for bit, guards included"""
    k, stride, pad, tr = order
    jobs, dests, srcs = [], [], []
    for Cout in COUTS:
        for Cin in CINS:
            g = G(Cout, Cin, k, stride, pad, tr)
            assert packed_floats(g) == sum(T.packed_floats(g._replace(KH=len(t), KW=1)) for t in class_taps(g, 0))
            w = weights(g)
            d, s = Dest(packed_floats(g)), source(w, som)
            d.expect(0, w.reshape(Cout, Cin, -1), g)
            jobs.append(pack_job(s, d.buf.ptr, g, som))
            dests.append((d, "%dx%d" % (Cout, Cin)))
            srcs.append(s)
    assert run_pack(jobs) == R.OK
    for d, what in dests:
        d.bitwise(what)
    assert all(s.unchanged() for s in srcs)


@pytest.mark.parametrize("wino", (1, 2))
@pytest.mark.parametrize("which", ("grid", "real"))
def test_winograd_points(which, wino):
    jobs, dests = [], []
    for Cout in COUTS:
        for Cin in CINS:
            for som in (1, 0):
                g = G(Cout, Cin, 3, 1, 1, 1 if wino == 2 else 0)
                w = weights(g, which, member=som)
                u64, u32 = wino_points(w, wino, R.F64), wino_points(w, wino, torch.float32)
                d, s = Dest(packed_floats(g, wino)), source(w, som)
                assert d.buf.n == T.packed_floats(g, True)
                d.expect(0, u64.float(), g, wino=wino)
                limit = R.FACTOR * (u32.double() - u64).abs().max().item() + R.FACTOR * R.U * u64.abs().max().item()
                jobs.append(pack_job(s, d.buf.ptr, g, som, wino))
                dests.append((d, limit, "%dx%d som %d" % (Cout, Cin, som), s))
    assert run_pack(jobs) == R.OK
    for d, limit, what, s in dests:
        if which == "grid":
            d.bitwise(what)
        d.within(limit, what)
        assert s.unchanged()


@pytest.mark.parametrize("order", [(1, 1, 0, 0), (3, 1, 1, 0), (5, 2, 2, 1)], ids=("1x1", "3x3", "5x5T"))
def test_nonneg(order):
    k, stride, pad, tr = order
    jobs, dests = [], []
    for Cout in COUTS:
        for Cin in CINS:
            for som in (1, 0):
                g = G(Cout, Cin, k, stride, pad, tr)
                t = R.make_inputs(R.case("pack", g, inputs="real", nonneg=True, member=som))
                d, s = Dest(packed_floats(g)), source(t["w_raw"], som)
                d.expect(0, t["w64"].float().reshape(Cout, Cin, -1), g)
                limit = R.FACTOR * (t["w"].double() - t["w64"]).abs().max().item() + R.FACTOR * R.U * t["w64"].abs().max().item()
                jobs.append(pack_job(s, d.buf.ptr, g, som, 0, 1))
                dests.append((d, limit, "%dx%d som %d" % (Cout, Cin, som), s))
    assert run_pack(jobs) == R.OK
    for d, limit, what, s in dests:
        d.within(limit, what)
        assert s.unchanged()


@pytest.mark.parametrize("som", (1, 0), ids=("out-major", "in-major"))
@pytest.mark.parametrize("k", (1, 3))
def test_sub_matrix_rows(k, som):
    """src_ld > count with src_off odd (rows off 16-byte alignment: dword reads), src_off = 8 in rows of a multiple of four
    floats (16-byte reads of a sub-matrix) and a source pointer off 16-byte alignment; NaN around the sub-matrix"""
    for Cout, Cin in ((33, 40), (80, 9), (31, 7)):
        g = G(Cout, Cin, k)
        w = weights(g)
        own = w if som else w.permute(1, 0, 2, 3)
        for src_off, extra, lead in ((3, 2, 4), (5, 6, 4), (8, 8, 4), (8, 8, 5), (0, 0, 7)):
            ld = src_off + own.shape[1] + extra
            wide = torch.full((own.shape[0], ld, k, k), NAN)
            wide[:, src_off:src_off + own.shape[1]] = own
            s, d = dense(wide, lead), Dest(packed_floats(g))
            assert (s.ptr % 16 == 0) == (lead == 4)
            d.expect(0, w.reshape(Cout, Cin, -1), g)
            assert run_pack([pack_job(s, d.buf.ptr, g, som, src_ld=ld, src_off=src_off)]) == R.OK
            d.bitwise("%dx%d src_off %d src_ld %d lead %d" % (Cout, Cin, src_off, ld, lead))
            assert s.unchanged()


@pytest.mark.parametrize("k,wino", ((1, 0), (3, 0), (3, 1)), ids=("1x1", "3x3", "3x3-wino"))
def test_concatenation_of_three_members(k, wino):
    """dst_ncot / dst_cot_off: three members of 2, 1 and 1 tiles (the last one ragged) side by side in one buffer, in
    both source layouts; then K-concatenation of three jobs by pointer offset"""
    Cin = 40
    d = Dest(packed_floats(G(128, Cin, k), wino))
    jobs, off = [], 0
    for i, Cout in enumerate((64, 32, 24)):
        g = G(Cout, Cin, k)
        w = weights(g, member=i)
        s = source(w, i & 1)
        d.expect(0, wino_points(w, 1, R.F64).float() if wino else w.reshape(Cout, Cin, -1), g, wino=wino, dst_ncot=4, dst_cot_off=off)
        jobs.append((pack_job(s, d.buf.ptr, g, i & 1, wino, dst_ncot=4, dst_cot_off=off), s))
        off += R.cdiv(Cout, 32)
    assert run_pack([j for j, _ in jobs]) == R.OK
    d.bitwise("M-concatenation")
    # K: channels [0, 16), [16, 40) and [40, 49) of one 33-row weight, each job at the end of the one before
    g = G(33, 49, k)
    w = weights(g)
    d = Dest(packed_floats(g, wino))
    s = source(w, 1)
    jobs, off = [], 0
    for c0, cn in ((0, 16), (16, 24), (40, 9)):
        gk = g._replace(Cin=cn)
        part = w[:, c0:c0 + cn]
        d.expect(off, wino_points(part, 1, R.F64).float() if wino else part.reshape(33, cn, -1), gk, wino=wino)
        jobs.append(pack_job(s, d.buf.ptr + 4 * off, gk, 1, wino, src_ld=49, src_off=c0))
        off += packed_floats(gk, wino)
    assert off == d.buf.n and run_pack(jobs) == R.OK
    d.bitwise("K-concatenation")
    assert s.unchanged()


def _unequal_jobs(n):
    """n jobs from one 1 x 1 weight pair up to 25-tap and Winograd weights of several tiles and chunks"""
    shapes = [(1, 1, 1, 0), (160, 72, 5, 0), (1, 7, 3, 0), (80, 40, 3, 1), (33, 9, 1, 0), (96, 136, 3, 2), (31, 8, 5, 0),
              (128, 64, 1, 0)]
    out = []
    for i in range(n):
        Cout, Cin, k, wino = shapes[i % len(shapes)]
        g = G(Cout + (i // len(shapes)), Cin, k, 1, k // 2, 1 if wino == 2 else 0)
        w = weights(g, member=i & 1)
        out.append((g, w, wino, i & 1))
    return out


@pytest.mark.parametrize("n", (24, 25), ids=("one-launch", "two-launches"))
def test_unequal_jobs_in_one_batch(n):
    """24 tap classes fill one launch, the 25th opens a second; two identical batches agree bit for bit"""
    runs = []
    for _ in range(2):
        jobs, dests = [], []
        for g, w, wino, som in _unequal_jobs(n):
            d, s = Dest(packed_floats(g, wino)), source(w, som)
            d.expect(0, wino_points(w, wino, R.F64).float() if wino else w.reshape(g.Cout, g.Cin, -1), g, wino=wino)
            jobs.append(pack_job(s, d.buf.ptr, g, som, wino))
            dests.append((d, s))
        assert run_pack(jobs) == R.OK
        for i, (d, s) in enumerate(dests):
            d.bitwise("job %d" % i)
            assert s.unchanged()
        runs.append([d.buf.now() for d, _ in dests])
    assert all(same_bits(a, b) for a, b in zip(*runs))


def test_single_job_entry_point():
    """icm_pack_weights: every tap class of a stride-2 scatter, nonneg off and on"""
    L = T.lib()
    for Cout, Cin in ((33, 9), (80, 40)):
        g = G(Cout, Cin, 5, 2, 2, 1)
        t = R.make_inputs(R.case("pack", g, inputs="real", nonneg=True))
        for nonneg in (0, 1):
            d, s = Dest(packed_floats(g)), source(t["w_raw"], 1)
            d.expect(0, (t["w64"].float() if nonneg else t["w_raw"]).reshape(Cout, Cin, -1), g)
            rc = L.lib().icm_pack_weights(s.ptr, d.buf.ptr, Cout, Cin, 5, 5, 1, 1, 2, 2, nonneg, R.NONNEG_BOUND, R.NONNEG_PED,
                                          L.stream())
            torch.cuda.synchronize()
            assert rc == R.OK
            if nonneg:
                d.within(R.FACTOR * (t["w"].double() - t["w64"]).abs().max().item() + R.FACTOR * R.U * t["w64"].abs().max().item(),
                         "nonneg")
            else:
                d.bitwise("copy")
            assert s.unchanged()
