"""The forward / input-gradient convolution kernels (csrc/conv_igemm.hip, conv_ks8.hip, conv_1x1.hip, conv_wino.hip) and
the weight-packing kernels that feed them, through the C ABI against float64: every staged row and both K-split blocks
forced on the geometries that admit them, every pointwise row a geometry reaches (and, in a child process, the one only
ICM_1X1_CFG reaches), the Winograd kernels with the raw and the pre-transformed operand, every argument of
icm_conv_args (operand activation, every epilogue kind, bias null / set, accum against a non-zero prefill, y2 null /
separate / == y, pixel_shuffle, the blocked channel map, every batch stride, x 4 bytes off 16-byte alignment), grouped
launches of 1 - 12 members, icm_pack_weights_batch (sub-matrix, M- and K-concatenation, nonneg, both source layouts, both
Winograd orientations), the int32 guard and every refusal.

Every operand lies in its own allocation between NaN guards; strided operands are slices of wider NaN-filled buffers; y
and y2 start as NaN unless the call accumulates; the packed weights are exactly icm_packed_weight_floats floats,
NaN-prefilled, and finite everywhere after packing.  After every call the inputs, every guard and every float of y / y2
outside the written set must be bit-identical, and after a refused call the outputs too.  `grid` inputs must give
conv64(...).float() bit for bit where the epilogue is exact arithmetic; everything else is held to tests/_conv_ref.py's
limit (its docstring states the rule; none of it is taken from a kernel's output), and tests/test_conv_ref.py asserts
without a GPU that each case reaches the branch it is named for.  Each `real` check prints its error / limit
(pytest -s); DESIGN.md "Convolution numerics" holds one such run."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import _conv_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
TAIL = 4                        # guard floats behind every operand


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def lib():
    from icm_amd import _lib
    return _lib


def bits(t):
    return t.contiguous().reshape(-1).view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


class Buf:
    """`n` floats behind `lead` guard floats and in front of TAIL more, NaN wherever `fill` puts nothing"""

    def __init__(self, n, lead=4, fill=None):
        self.n, self.lead = int(n), lead
        self.cpu0 = torch.full((lead + self.n + TAIL,), NAN, dtype=torch.float32)
        if fill is not None:
            fill(self.cpu0[lead:lead + self.n])
        self.dev = self.cpu0.to(dev())
        assert self.dev.data_ptr() % 16 == 0
        self.ptr = self.dev.data_ptr() + 4 * lead

    def now(self):
        return self.dev.cpu()

    def body(self):
        return self.now()[self.lead:self.lead + self.n]

    def unchanged(self):
        return same_bits(self.now(), self.cpu0)

    def snapshot(self):
        """from here on `unchanged` compares with the present contents (an input that a kernel of the test itself wrote)"""
        self.cpu0 = self.now()


def dense(v, lead=4):
    return Buf(v.numel(), lead, lambda d: d.copy_(v.reshape(-1)))


def operand(x, bs, lead=4):
    """[N, C, h, w] as N slices bs floats apart in a NaN-filled buffer"""
    N, per = x.shape[0], x[0].numel()

    def fill(v):
        for n in range(N):
            v[n * bs:n * bs + per] = x[n].reshape(-1)
    return Buf((N - 1) * bs + per, lead, fill)


def pack_job(w_buf, wp_ptr, g, src_out_major=1, wino=0, nonneg=0, **kw):
    J = lib().PackJob()
    J.w, J.wp, J.Cout, J.Cin, J.KH, J.KW = w_buf.ptr, wp_ptr, g.Cout, g.Cin, g.KH, g.KW
    J.src_out_major, J.transposed, J.stride, J.pad, J.nonneg = src_out_major, g.transposed, g.stride, g.pad, nonneg
    J.bound, J.pedestal, J.wino = R.NONNEG_BOUND, R.NONNEG_PED, wino
    for k, v in kw.items():
        setattr(J, k, v)
    return J


def run_pack(jobs):
    arr = (lib().PackJob * len(jobs))(*jobs)
    rc = lib().lib().icm_pack_weights_batch(arr, len(jobs), lib().stream())
    torch.cuda.synchronize()
    return rc


def packed_floats(g, wino=False):
    return int(lib().lib().icm_packed_weight_floats(g.Cout, g.Cin, 4 if wino else g.KH, 4 if wino else g.KW))


class Member:
    """one problem: operands, packed weights and outputs of a case of _conv_ref, each in its own guarded allocation.
    Members with an odd index hand the canonical weights over in the [Cin][Cout] layout (src_out_major = 0)."""

    def __init__(self, c, share_x=None, pack=True):
        self.c = c
        g = self.g = c["g"]
        t = self.t = R.make_inputs(c)
        s = self.s = R.strides_of(c)
        wino = c["algo"] == R.WINOGRAD
        self.x = share_x or operand(t["x"], s["x"], 4 + c["x_off"])
        assert (self.x.ptr % 16 == 0) == (c["x_off"] % 4 == 0)
        som = 1 - (c["member"] & 1)
        wsrc = t.get("w_raw", t["w"])
        self.w = dense(wsrc if som else wsrc.permute(1, 0, 2, 3).contiguous())
        self.wp = Buf(packed_floats(g, wino))
        if pack:            # (a kernel the packing itself refuses keeps its NaN buffer: the launch must be refused too)
            rc = run_pack([pack_job(self.w, self.wp.ptr, g, som, (2 if g.transposed else 1) if wino else 0, int(c["nonneg"]))])
            assert rc == R.OK, "packing refused"
            assert self.wp.now()[:4].isnan().all() and self.wp.now()[-TAIL:].isnan().all(), "packing wrote outside the buffer"
            assert torch.isfinite(self.wp.body()).all(), "packing left a float of the packed buffer unwritten"
            assert self.w.unchanged()
            self.wp.snapshot()
        self.bias = dense(t["bias"]) if c["bias"] else None
        rd = R.reads(c["epi"])
        self.res = operand(t["res"], s["res"]) if rd["res"] else None
        self.aux = operand(t["aux"], s["aux"]) if rd["aux"] else None
        self.aux2 = operand(t["aux2"], s["aux2"]) if rd["aux2"] else None
        osh = R.out_shape(c)
        per = osh[1] * osh[2] * osh[3]
        self.per = per
        pre = t["prefill"] if c["accum"] else None

        def out_buf(bs, prefill):
            def fill(v):
                if prefill is not None:
                    for n in range(g.N):
                        v[n * bs:n * bs + per] = prefill[n].reshape(-1)
            return Buf((g.N - 1) * bs + per, 4, fill)
        self.y = out_buf(s["y"], pre)
        # a separate y2 is never read: it starts as NaN even when the call accumulates
        self.y2 = out_buf(s["y2"], None) if c["y2"] == "sep" else None
        self.xv = None
        self.args = None
        self.build_args()
        if c["xv"]:
            n = int(lib().lib().icm_wino_transform_floats(C.byref(self.args)))
            assert n > 0
            self.xv = Buf(n)
            self.build_args()

    def build_args(self):
        p = {"x": self.x.ptr, "wp": self.wp.ptr, "y": self.y.ptr}
        for name in ("bias", "res", "aux", "aux2", "xv"):
            b = getattr(self, name)
            p[name] = b.ptr if b is not None else 0
        p["y2"] = self.y.ptr if self.c["y2"] == "same" else (self.y2.ptr if self.y2 is not None else 0)
        self.args = R.conv_args(self.c, p)

    def inputs(self):
        return [b for b in (self.x, self.w, self.wp, self.bias, self.res, self.aux, self.aux2, self.xv) if b is not None]

    def untouched(self, what):
        """after a refused call: inputs, outputs and every guard bit-identical"""
        for i, b in enumerate(self.inputs() + [b for b in (self.y, self.y2) if b is not None]):
            assert b.unchanged(), f"{what}: a refused call changed buffer {i} of member {self.c['member']}"

    def _output(self, buf, bs, what, name):
        now = buf.now()
        N, per = self.g.N, self.per
        idx = (torch.arange(N).view(-1, 1) * bs + torch.arange(per).view(1, -1)).reshape(-1) + buf.lead
        got = now[idx].reshape(R.out_shape(self.c)).clone()
        ref = buf.cpu0.clone()
        now[idx] = 0.0
        ref[idx] = 0.0
        assert same_bits(now, ref), f"{what}: {name} was written outside its planes (guards / gaps between batch slices)"
        assert torch.isfinite(got).all(), f"{what}: {name} kept (or read) its NaN prefill in {int((~torch.isfinite(got)).sum())} elements"
        return got

    def results(self, what):
        """(y, y2 or None) after checking inputs, guards and every float outside the written planes"""
        for i, b in enumerate(self.inputs()):
            assert b.unchanged(), f"{what}: input buffer {i} (or its guards) changed"
        y = self._output(self.y, self.s["y"], what, "y")
        y2 = self._output(self.y2, self.s["y2"], what, "y2") if self.y2 is not None else None
        return y, y2


def transform(members):
    L = lib()
    arr = (L.ConvArgs * len(members))(*[m.args for m in members])
    rc = L.lib().icm_wino_transform(arr, len(members), L.stream())
    torch.cuda.synchronize()
    if rc == R.OK:
        for m in members:
            assert torch.isfinite(m.xv.body()).all() and m.xv.now()[:4].isnan().all() and m.xv.now()[-TAIL:].isnan().all()
            m.xv.snapshot()
    return rc


def launch(members, cfg=R.CFG_AUTO, f1x1=-1, grouped=None, n=None, view=None):
    L = lib()
    arr = (L.ConvArgs * len(members))(*[m.args for m in members])
    n = len(members) if n is None else n
    if grouped is None:
        grouped = n != 1
    with R.forced(cfg, f1x1):
        if view:
            rc = getattr(L.lib(), view)(C.byref(arr[0]), L.stream())
        elif grouped:
            rc = L.lib().icm_conv_run_grouped(arr, n, L.stream())
        else:
            rc = L.lib().icm_conv_run(C.byref(arr[0]), L.stream())
    torch.cuda.synchronize()
    return rc


def check(m, what, n=1):
    """member m's outputs against its own reference: bit equality where `grid` makes the arithmetic exact, the limit
    rule everywhere else"""
    c = m.c
    y, y2 = m.results(what)
    o64, acc64, _ = R.conv64(c)
    ex_y, ex_y2 = R.exact_on_grid(c)
    plans = R.class_plans(c, n)
    fam = R.FAMILY_NAMES[plans[0].family]
    lim = None
    for name, got, want, exact in (("y", y, o64.y, ex_y), ("y2", y2, o64.y2, ex_y2)):
        assert (got is None) == (want is None), f"{what}: {name}"
        if got is None:
            continue
        if exact:
            w32 = want.float()
            assert same_bits(got + 0.0, w32 + 0.0), f"{what}: {name} differs from the exact result in " \
                f"{int((got != w32).sum())} elements, by up to {(got.double() - want).abs().max().item():g}, first at " \
                f"{(got != w32).nonzero()[:1].tolist()}"
            continue
        if lim is None:
            a32 = acc64.float() if (c["inputs"] == "grid") else R.acc32(c, plans)
            lim = R.limits(c, a32)
        l, e32 = (lim.y, lim.e32_y) if name == "y" else (lim.y2, lim.e32_y2)
        err = (got.double() - want).abs().max().item()
        print(f"\nCVNUM {fam} {name} {what}: gpu {err:.3e} limit {l:.3e} ratio {err / l if l else 0:.3f} ref32 {e32:.3e}")
        assert err <= l, f"{what} {name}: {err:.3e} > limit {l:.3e} (float32 restatement errs {e32:.3e})"
    return y, y2


def run_single(c, what=None):
    what = what or c["id"]
    m = Member(c)
    if c["xv"]:
        assert transform([m]) == R.OK, what
    assert launch([m], c["cfg"], c["f1x1"]) == R.OK, what
    return check(m, what)


def run_group(cs, what, shared_x=False):
    ms = []
    for c in cs:
        ms.append(Member(c, share_x=ms[0].x if (shared_x and ms) else None))
    if cs[0]["xv"]:
        assert transform(ms) == R.OK, what
    assert launch(ms, cs[0]["cfg"], cs[0]["f1x1"], grouped=True) == R.OK, what
    return [check(m, f"{what}, member {i}", len(cs)) for i, m in enumerate(ms)]


def ids(cases):
    return [c["id"] for c in cases]


def both(cid, g, **kw):
    return [R.case(cid + "-grid", g, **kw), R.case(cid + "-real", g, inputs="real", **kw)]


# ================================================================================================ geometries, automatic choice
GEOMETRY_CASES = [c for g in R.ONE_TRIP + R.TRANSPOSED_S2 + R.TINY + R.BLOCKS + [R.multi_trip_geom(k) for k in (1, 3, 5)]
                  for c in both("auto-" + R.gname(g), g)]


@pytest.mark.parametrize("c", GEOMETRY_CASES, ids=ids(GEOMETRY_CASES))
def test_every_geometry(c):
    run_single(c)


FORCED = R.forced_row_table()


@pytest.mark.parametrize("g,cfg,rc", FORCED, ids=["%s-%s%s" % (R.gname(g), R.cfg_name(cfg), "-refused" if rc else "") for g, cfg, rc in FORCED])
def test_every_row_and_k_split_block_forced(g, cfg, rc):
    """every row of the staged table and both K-split blocks on the one-trip 3x3, 3x3 s2, 5x5 s2, transposed 5x5 s2 and a
    multi-trip shape: exact on `grid`, within the limit on `real`; a row the planner refuses returns its code with
    nothing written"""
    if rc:
        m = Member(R.case("refused", g, cfg=cfg))
        assert launch([m], cfg) == rc
        m.untouched(f"{R.cfg_name(cfg)} refused")
        return
    for c in both(R.cfg_name(cfg), g, cfg=cfg):
        run_single(c)


BLOCK_ROWS = [R.case("%s-row%d-%s" % (R.gname(g), r, which), g, cfg=r, inputs=which) for g in R.BLOCKS
              for r in range(R.NROWS) if R.plan(R.case("probe", g, cfg=r)).rc == R.OK for which in ("grid", "real")]


@pytest.mark.parametrize("c", BLOCK_ROWS, ids=ids(BLOCK_ROWS))
def test_ragged_last_co_block_under_every_row(c):
    run_single(c)


def test_automatic_k_split_choice():
    """12 members of 16 workgroups each: one nearly full round of the chip, which the planner gives the K-split kernel"""
    for which in ("grid", "real"):
        run_group([dict(R.KS8_AUTO, member=i, inputs=which) for i in range(R.KS8_AUTO_N)], "ks8 auto " + which)


# ================================================================================================ arguments
CROSS = R.cross_cases()


@pytest.mark.parametrize("c", CROSS, ids=ids(CROSS))
def test_argument_cross(c):
    run_single(c)


STAGING = [c for c, _, _ in R.staging_cases()]


@pytest.mark.parametrize("c", STAGING, ids=ids(STAGING))
def test_staging_forms_and_their_fallbacks(c):
    run_single(c)
    if c["inputs"] == "grid":
        run_single(dict(c, inputs="real"), c["id"] + " real")


# ================================================================================================ the pointwise kernel
POINTWISE = sorted(R.pointwise_row_cases().items())


@pytest.mark.parametrize("row,ng", POINTWISE, ids=["row%d" % r for r, _ in POINTWISE])
def test_pointwise_rows(row, ng):
    """every row of the pointwise table a geometry reaches, at the smallest launch that selects it"""
    n, g = ng
    for which in ("grid", "real"):
        cs = [R.case("p1-row%d-%s" % (row, which), g, inputs=which, f1x1=1, member=i, ngroups=n) for i in range(n)]
        if n > 1:
            run_group(cs, cs[0]["id"])
        else:
            run_single(cs[0])


POINTWISE_CHUNK_CASES = [c for g in R.POINTWISE_CHUNKS for c in both("p1-chunks%d" % (g.Cin // 8), g, f1x1=1)] + \
    [R.case("p1-chunks%d-gelu-lrp" % (g.Cin // 8), g, f1x1=1, pro_act=R.GELU, epi=R.E_LRP, y2="sep", inputs="real") for g in R.POINTWISE_CHUNKS]


@pytest.mark.parametrize("c", POINTWISE_CHUNK_CASES, ids=ids(POINTWISE_CHUNK_CASES))
def test_pointwise_chunk_counts(c):
    """1 / 3 / 40 chunks: below, not a multiple of and ten times the prefetch depth"""
    run_single(c)


def test_pointwise_automatic_threshold():
    n, g = R.pointwise_row_cases()[3]
    run_group([R.case("p1-auto", g, member=i, ngroups=n) for i in range(n)], "pointwise, automatic")


CHILD = r"""
import sys
sys.path[:0] = %r
import test_gpu_conv_numerics as T
import _conv_ref as R
row = int(sys.argv[1])
for g in (R.pointwise_row_cases()[5][1], R.pointwise_row_cases()[6][1]._replace(Cin=24)):
    for which in ("grid", "real"):
        c = R.case("env-row%%d-%%s" %% (row, which), g, inputs=which, f1x1=1)
        p = R.plan(c)
        assert p.family == R.P1 and p.row == row, p
        T.run_single(c)
print("child ok", row)
"""


@pytest.mark.parametrize("row", R.POINTWISE_UNREACHABLE)
def test_rows_only_an_environment_switch_reaches(row):
    """row 7 <2,1> of the pointwise table wins for no geometry (tests/test_conv_ref.py): a fresh child process per row
    runs two pointwise cases under ICM_1X1_CFG against the same reference"""
    env = dict(os.environ, ICM_1X1_CFG=str(row))
    r = subprocess.run([sys.executable, "-c", CHILD % (sys.path,), str(row)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "child ok %d" % row in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


# ================================================================================================ Winograd
WINO = R.wino_cases()


@pytest.mark.parametrize("c", WINO, ids=ids(WINO))
def test_winograd(c):
    run_single(c)


@pytest.mark.parametrize("c", R.W8_CASES, ids=ids(R.W8_CASES))
def test_winograd_eight_wave_kernel(c):
    run_group([dict(c, member=i) for i in range(R.WINO_W8_N)], c["id"])


# ================================================================================================ grouped launches
@pytest.mark.parametrize("n", R.GROUP_NS)
@pytest.mark.parametrize("g", R.GROUP_GEOMS, ids=R.gname)
def test_grouped_launch(g, n):
    """members with their own inputs and outputs, each against its own reference"""
    run_group([R.case("m%d" % i, g, member=i, ngroups=n, epi=R.E_RES, y2="sep") for i in range(n)], f"group of {n}")


def test_grouped_launch_real_and_shared_x():
    cs = [R.case("m%d" % i, R.G3, member=i, ngroups=3, inputs="real") for i in range(3)]
    run_group(cs, "real group of 3")
    # one launch with a shared x: the members' inputs differ in the weights only
    cs = [R.case("m%d" % i, R.G3, member=i, ngroups=3) for i in range(3)]
    ms = [Member(cs[0])]
    for c in cs[1:]:
        ms.append(Member(c, share_x=ms[0].x))
    assert launch(ms, grouped=True) == R.OK
    for i, m in enumerate(ms):
        y, _ = m.results(f"shared x, member {i}")
        t = dict(R.make_inputs(cs[i]), x=R.make_inputs(cs[0])["x"])
        want = R.conv64(cs[i], t)[0].y
        assert same_bits(y + 0.0, want.float() + 0.0), f"shared x, member {i}"


def test_thirteen_members_are_refused():
    ms = [Member(R.case("m%d" % i, R.G3, member=i)) for i in range(2)]
    assert launch(ms + [ms[0]] * 11, grouped=True, n=13) == R.ERR_ARG
    assert launch(ms, grouped=True, n=0) == R.ERR_ARG
    for m in ms:
        m.untouched("13 members")


# ================================================================================================ packing
def test_pack_sub_matrix_equals_the_pack_of_the_slice():
    """src_ld / src_off: a job on a sub-matrix of a wider canonical weight gives the buffer of the sliced matrix bit for
    bit, in both source layouts and for a transposed stride-2 tap order"""
    for g in (R.G3, R.G5T, R.G1):
        w = R.make_inputs(R.case("t", g, inputs="real"))["w"]                    # [Cout, Cin, KH, KW]
        for som in (1, 0):
            wide_i = 8 + (g.Cin if som else g.Cout) + 5
            src = torch.full((g.Cout, wide_i, g.KH, g.KW) if som else (g.Cin, wide_i, g.KH, g.KW), NAN)
            own = w if som else w.permute(1, 0, 2, 3)
            src[:, 8:8 + own.shape[1]] = own
            wide, narrow = dense(src), dense(own.contiguous())
            a, b = Buf(packed_floats(g)), Buf(packed_floats(g))
            assert run_pack([pack_job(wide, a.ptr, g, som, src_ld=wide_i, src_off=8), pack_job(narrow, b.ptr, g, som)]) == R.OK
            assert torch.isfinite(a.body()).all() and same_bits(a.now(), b.now()), (R.gname(g), som)
            assert wide.unchanged() and narrow.unchanged()


def _conv_with_packed(c, wp, what):
    m = Member(c)
    m.wp = wp
    m.build_args()
    assert launch([m], c["cfg"]) == R.OK
    y, _ = m.results(what)
    want = R.conv64(c)[0].y
    assert same_bits(y + 0.0, want.float() + 0.0), f"{what}: differs by up to {(y.double() - want).abs().max().item():g}"


@pytest.mark.parametrize("k", [3, 1, 5], ids=["3x3", "1x1", "5x5"])
def test_pack_concatenation_feeds_the_convolution(k):
    """dst_ncot / dst_cot_off (M-concatenation) and consecutive jobs (K-concatenation): the convolution of the
    concatenated weights, on `grid`, bit for bit; the channel tails of the packed buffer are zeros, not NaN"""
    g = R.geom(3, 11, 13, k, 1, k // 2, ch=(40, 88))
    c = R.case("concat", g)
    w = R.make_inputs(c)["w"]
    # M: rows [0, 64) and [64, 88) from two jobs into one buffer of 3 tiles per step
    gm0, gm1 = g._replace(Cout=64), g._replace(Cout=24)
    wp = Buf(packed_floats(g))
    w0, w1 = dense(w[:64].contiguous()), dense(w[64:].permute(1, 0, 2, 3).contiguous())
    j0 = pack_job(w0, wp.ptr, gm0, 1, dst_ncot=3, dst_cot_off=0)
    j1 = pack_job(w1, wp.ptr, gm1, 0, dst_ncot=3, dst_cot_off=2)
    assert run_pack([j0, j1]) == R.OK and torch.isfinite(wp.body()).all()
    wp.snapshot()
    _conv_with_packed(c, wp, "M-concatenation")
    # K: channels [0, 24) and [24, 40) from consecutive jobs, the second buffer packed_floats of the first further on
    gk0, gk1 = g._replace(Cin=24), g._replace(Cin=16)
    wp = Buf(packed_floats(g))
    assert packed_floats(gk0) + packed_floats(gk1) == packed_floats(g)
    w0, w1 = dense(w[:, :24].contiguous()), dense(w)
    j0 = pack_job(w0, wp.ptr, gk0, 1)
    j1 = pack_job(w1, wp.ptr + 4 * packed_floats(gk0), gk1, 1, src_ld=40, src_off=24)
    assert run_pack([j0, j1]) == R.OK and torch.isfinite(wp.body()).all()
    assert w0.unchanged() and w1.unchanged()
    wp.snapshot()
    _conv_with_packed(c, wp, "K-concatenation")


NONNEG = [R.case("nonneg-%s-%s" % (R.gname(g), which), g, inputs=which, nonneg=True, member=m)
          for g in (R.G1, R.G3, R.G5T) for which in ("real",) for m in (0, 1)]


@pytest.mark.parametrize("c", NONNEG, ids=ids(NONNEG))
def test_pack_nonneg(c):
    """max(w, bound)^2 - pedestal while packing, against float64 under the `real` limit, both source layouts"""
    run_single(c)


def test_pack_zero_fills_the_channel_tails():
    """packed into a NaN-filled destination from weights without a zero among them: every float is finite and the
    zeros of the buffer are exactly the co tail rows and ci tail columns of every tap class, counted"""
    for g in (R.G3, R.G5T, R.geom(3, 11, 13, 3, 1, 1, ch=(4, 40))):
        wp = Buf(packed_floats(g))
        w = dense(R.make_inputs(R.case("t", g))["w"] + 3.0)                        # no zero among the real entries
        assert run_pack([pack_job(w, wp.ptr, g, 1)]) == R.OK
        body = wp.body()
        ncot, n8 = R.cdiv(g.Cout, 32), R.cdiv(g.Cin, 8)
        assert torch.isfinite(body).all()
        assert int((body == 0).sum()) == body.numel() - g.Cout * g.Cin * g.KH * g.KW == (ncot * 32 * n8 * 8 - g.Cout * g.Cin) * g.KH * g.KW


def _j(**kw):
    return lambda J: [setattr(J, k, v) for k, v in kw.items()]


PACK_REFUSALS = [("w-null", _j(w=0)), ("wp-null", _j(wp=0)), ("Cout-zero", _j(Cout=0)), ("Cin-negative", _j(Cin=-1)),
                 ("33-taps", _j(KH=3, KW=11)), ("stride-3", _j(stride=3)), ("stride-0", _j(stride=0)),
                 ("wino-3", _j(wino=3)), ("wino-negative", _j(wino=-1)), ("wino-5x5", _j(wino=1, KH=5, KW=5, pad=2)),
                 ("wino-3x1", _j(wino=1, KW=1)), ("wino-stride-2", _j(wino=2, stride=2)), ("wino-pad-0", _j(wino=1, pad=0)),
                 ("wino-nonneg", _j(wino=1, nonneg=1)), ("src_off-negative", _j(src_off=-1)),
                 ("src-window-past-the-row", _j(src_ld=44, src_off=5)), ("src_ld-below-Cin", _j(src_ld=39)),
                 ("dst_cot_off-negative", _j(dst_cot_off=-1)), ("dst-window-past-the-step", _j(dst_ncot=2, dst_cot_off=2)),
                 ("dst_ncot-below-the-tiles", _j(dst_ncot=1, dst_cot_off=0))]


@pytest.mark.parametrize("rid,tweak", PACK_REFUSALS, ids=[r[0] for r in PACK_REFUSALS])
def test_pack_refusals_write_nothing(rid, tweak):
    g = R.geom(3, 11, 13, 3, 1, 1, ch=(40, 40))
    w = dense(torch.full((g.Cout, 48, 3, 3), 1.0))
    wp, wp_ok = Buf(4 * packed_floats(g)), Buf(packed_floats(g))
    good, bad = pack_job(w, wp_ok.ptr, g), pack_job(w, wp.ptr, g)
    tweak(bad)
    # a refused job stops this two-job batch before anything is launched, the valid job in front of it included (a batch
    # launches every ICM_PACK_NB = 24 tap classes: jobs that many classes in front of a bad one are packed all the same)
    assert run_pack([good, bad]) == R.ERR_ARG
    assert wp.unchanged() and wp_ok.unchanged() and w.unchanged()


def test_pack_refuses_an_empty_batch():
    L = lib()
    assert L.lib().icm_pack_weights_batch(None, 1, L.stream()) == R.ERR_ARG
    g = R.G3
    wp = Buf(packed_floats(g))
    w = dense(R.make_inputs(R.case("t", g))["w"])
    arr = (L.PackJob * 1)(pack_job(w, wp.ptr, g))
    assert L.lib().icm_pack_weights_batch(arr, 0, L.stream()) == R.ERR_ARG
    torch.cuda.synchronize()
    assert wp.unchanged()


# ================================================================================================ near the int32 limit
def test_operand_offsets_past_int32_are_refused():
    """validate()'s guard of the int32 operand byte offsets: N * x_bs past 2^31 bytes is refused before anything is
    launched, so the small real allocations of the natural layout suffice: nothing may be read"""
    g = R.INT32_G
    assert R.int32_guard_refuses(g, R.INT32_REFUSED_BS) and not R.int32_guard_refuses(g, R.INT32_LARGEST_BS)
    m = Member(R.case("int32", g))
    m.args.x_bs = R.INT32_REFUSED_BS
    assert launch([m]) == R.ERR_UNSUPPORTED
    m.untouched("int32 guard")
    m.args.x_bs = R.INT32_LARGEST_BS + 1
    assert launch([m]) == R.ERR_UNSUPPORTED
    m.untouched("int32 guard, first refused value")


def test_largest_accepted_operand_stride():
    """the other side of the guard: the largest accepted x_bs (2^28 - 257 floats) runs and is exact.  The second image
    then lies 1 GiB into x, so this one case needs a real allocation of N * x_bs floats (2 GiB, freed at once)"""
    g, x_bs = R.INT32_G, R.INT32_LARGEST_BS
    c = R.case("int32", g)
    m = Member(c)
    x = R.make_inputs(c)["x"]
    big = torch.empty(g.N * x_bs, dtype=torch.float32, device=dev())
    for i in range(g.N):
        big[i * x_bs:i * x_bs + x[i].numel()] = x[i].reshape(-1).to(dev())
    m.args.x, m.args.x_bs = big.data_ptr(), x_bs
    assert launch([m]) == R.OK
    y, _ = m.results("largest accepted x_bs")
    assert same_bits(y + 0.0, R.conv64(c)[0].y.float() + 0.0)
    for i in range(g.N):
        assert same_bits(big[i * x_bs:i * x_bs + x[i].numel()].cpu(), x[i].reshape(-1)), "x changed"
    del big


# ================================================================================================ refusals
def _set(i=0, **kw):
    def f(ms):
        for k, v in kw.items():
            setattr(ms[i].args, k, v)
    return f


def _bs(i, name, d):
    return lambda ms: setattr(ms[i].args, name, getattr(ms[i].args, name) + d)


G3, G1, G5T = R.G3, R.G1, R.G5T
AX = dict(epi=R.E_AXPY2)
RS = dict(epi=R.E_RES, y2="sep")
WN = dict(algo=R.WINOGRAD)
A, UNS = R.ERR_ARG, R.ERR_UNSUPPORTED
# id, geometry, case kwargs, members, tweak, view, expected code
REFUSALS = [
    ("x-null", G3, {}, 1, _set(x=0), None, A), ("wp-null", G3, {}, 1, _set(wp=0), None, A), ("y-null", G3, {}, 1, _set(y=0), None, A),
    ("N-zero", G3, {}, 1, _set(N=0), None, A), ("Cin-zero", G3, {}, 1, _set(Cin=0), None, A), ("Cout-negative", G3, {}, 1, _set(Cout=-8), None, A),
    ("H-zero", G5T, {}, 1, _set(H=0), None, A), ("W-zero", G5T, {}, 1, _set(W=0), None, A), ("OH-zero", G5T, {}, 1, _set(OH=0), None, A),
    ("OW-negative", G5T, {}, 1, _set(OW=-1), None, A),
    ("KH-zero", G3, {}, 1, _set(KH=0), None, UNS), ("KW-negative", G3, {}, 1, _set(KW=-3), None, UNS),
    ("6x6", R.REFUSED_KERNEL, {}, 1, None, None, UNS), ("1x1-map-5x5-N33", R.TINY_REFUSED, {}, 1, None, None, UNS), ("stride-3", G3, {}, 1, _set(stride=3), None, UNS),
    ("stride-0", G5T, {}, 1, _set(stride=0), None, UNS),
    ("OH-inconsistent", G3, {}, 1, _set(OH=G3.OH - 1), None, A), ("OW-inconsistent", G3, {}, 1, _set(OW=G3.OW - 1), None, A),
    ("pad-inconsistent", G3, {}, 1, _set(pad=0), None, A),
    ("res-null", G3, dict(epi=R.E_RES), 1, _set(res=0), None, A), ("res-null-res_gelu", G3, dict(epi=R.E_RES_GELU), 1, _set(res=0), None, A),
    ("res-null-res_mul_dgelu", G3, dict(epi=R.E_RES_MUL_DGELU), 1, _set(res=0), None, A),
    ("aux-null-gdn", G1, dict(epi=R.E_GDN, pro_act=R.SQUARE), 1, _set(aux=0), None, A), ("aux-null-lrp", G3, dict(epi=R.E_LRP), 1, _set(aux=0), None, A),
    ("aux-null-axpy2", G1, AX, 1, _set(aux=0), None, A), ("aux2-null", G1, AX, 1, _set(aux2=0), None, A),
    ("pixel_shuffle-1", R.PS_G, {}, 1, _set(pixel_shuffle=1), None, UNS), ("pixel_shuffle-3", R.PS_G, {}, 1, _set(pixel_shuffle=3), None, UNS),
    ("pixel_shuffle-Cout%4", R.PS_G, dict(ps=2), 1, _set(Cout=38), None, A),
    ("pixel_shuffle-transposed", R.PS_G, dict(ps=2), 1, _set(transposed=1), None, A),
    ("x_seg_len-negative", G3, {}, 1, _set(x_seg_len=-1), None, A), ("x_seg_gap-negative", G3, dict(seg=(20, 4)), 1, _set(x_seg_gap=-1), None, A),
    ("x_seg_len-65536", G3, {}, 1, _set(x_seg_len=65536), None, A),
    ("algo-2", G3, {}, 1, _set(algo=2), None, A), ("algo-negative", G3, {}, 2, lambda ms: [_set(i, algo=-1)(ms) for i in (0, 1)], None, A),
    ("conv2d_fwd-transposed", G5T, {}, 1, None, "icm_conv2d_fwd", A), ("convT2d_dgrad-transposed", G5T, {}, 1, None, "icm_convT2d_dgrad", A),
    ("conv2d_dgrad-gather", G3, {}, 1, None, "icm_conv2d_dgrad", A), ("convT2d_fwd-gather", G3, {}, 1, None, "icm_convT2d_fwd", A),
    ("winograd-stride-2", R.G3S2, WN, 1, None, None, UNS), ("winograd-5x5", R.geom(3, 11, 13, 5, 1, 2), WN, 1, None, None, UNS),
    ("winograd-pad-0", R.geom(3, 11, 13, 3, 1, 0), WN, 1, None, None, UNS), ("winograd-1x1", G1, WN, 1, None, None, UNS),
    ("winograd-pixel-shuffle", R.PS_G, dict(ps=2, **WN), 1, None, None, UNS),
    ("winograd-axpy2", G3, dict(algo=R.WINOGRAD, **AX), 1, None, None, UNS),
    ("winograd-gdn", G3, dict(algo=R.WINOGRAD, epi=R.E_GDN, pro_act=R.SQUARE), 1, None, None, UNS),
    ("winograd-pro_act-3", G3, WN, 1, _set(pro_act=3), None, UNS),
    ("winograd-xv-of-one-member-only", G3, WN, 2, _set(1, xv=64), None, A),
] + [("member-differs-in-" + f, R.G3T, RS, 2, _set(1, **{f: v}), None, A) for f, v in (
    # member 1 stays valid on its own in every row (tests/test_conv_ref.py asserts it): the refusal is check_group's
    ("N", 2), ("Cin", 32), ("H", 10), ("W", 12), ("Cout", 16), ("OH", 10), ("OW", 12), ("KH", 1), ("KW", 1), ("stride", 2),
    ("pad", 0), ("transposed", 0), ("pro_act", R.SQUARE), ("epi", R.E_RES_GELU), ("accum", 1),
    ("x_seg_len", 20), ("algo", R.WINOGRAD), ("y2", 0), ("bias", 0), ("xv", 64))
] + [("member-differs-in-" + f, R.G3T, RS, 2, _bs(1, f, 4), None, A) for f in ("x_bs", "y_bs", "res_bs", "y2_bs")
] + [("member-differs-in-pixel_shuffle", G3, {}, 2, _set(1, pixel_shuffle=2), None, A),
     ("member-differs-in-x_seg_gap", R.G3T, dict(seg=(20, 4)), 2, _set(1, x_seg_gap=5), None, A),
     ("member-differs-in-aux_bs", G1, AX, 2, _bs(1, "aux_bs", 4), None, A),
     ("member-differs-in-aux2_bs", G1, AX, 2, _bs(1, "aux2_bs", 4), None, A),
     # operand presence under epi NONE, which reads none of them: a pointer more on member 1 (never dereferenced)
     ("member-differs-in-res", R.G3T, {}, 2, _set(1, res=64), None, A),
     ("member-differs-in-aux", R.G3T, {}, 2, _set(1, aux=64), None, A),
     ("member-differs-in-aux2", R.G3T, {}, 2, _set(1, aux2=64), None, A),
     ("second-member-invalid", G3, {}, 2, _set(1, y=0), None, A)]


@pytest.mark.parametrize("rid,g,kw,nm,tweak,view,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_launch_nothing(rid, g, kw, nm, tweak, view, code):
    """the expected code, and outputs, inputs and guards bit-identical: nothing was launched.  Every refused call has
    real allocations for the geometry it names; a tweak only ever shrinks what a launch would touch or is refused
    before any pointer is used"""
    packable = g.KH * g.KW <= R.MAX_TAPS and (kw.get("algo") != R.WINOGRAD or (g.KH, g.KW, g.stride, g.pad) == (3, 3, 1, 1))
    ms = [Member(R.case(rid, g, member=i, **kw), pack=packable) for i in range(nm)]
    if tweak:
        tweak(ms)
    rc = launch(ms, grouped=(nm != 1), view=view)
    assert rc == code, f"{rid}: returned {rc}, expected {code}"
    for m in ms:
        m.untouched(rid)


def test_wino_transform_refusals():
    ms = [Member(R.case("m%d" % i, G3, algo=R.WINOGRAD, xv=True, member=i)) for i in range(2)]
    L = lib()

    def call(n, tweak=None):
        arr = (L.ConvArgs * 13)(*([m.args for m in ms] + [ms[0].args] * 11))
        if tweak:
            tweak(arr)
        rc = L.lib().icm_wino_transform(arr, n, L.stream())
        torch.cuda.synchronize()
        for m in ms:
            assert m.xv.unchanged() and m.x.unchanged()
        return rc
    assert L.lib().icm_wino_transform(None, 1, L.stream()) == A
    assert call(0) == A and call(13) == A
    for f, v in (("N", 2), ("Cin", 32), ("H", 10), ("W", 12), ("x_bs", ms[0].args.x_bs + 4), ("pro_act", R.SQUARE),
                 ("x_seg_len", 20), ("x_seg_gap", 1)):
        assert call(2, lambda arr: setattr(arr[1], f, v)) == A, f
    assert call(2, lambda arr: setattr(arr[1], "xv", 0)) == A and call(1, lambda arr: setattr(arr[0], "x", 0)) == A
    assert call(1, lambda arr: setattr(arr[0], "stride", 2)) == UNS
    a = ms[0].args
    assert L.lib().icm_wino_transform_floats(C.byref(a)) == ms[0].xv.n
    a.pad = 0
    assert L.lib().icm_wino_transform_floats(C.byref(a)) == -1 and L.lib().icm_conv_winograd_ok(C.byref(a)) == 0
    a.pad = 1
    assert L.lib().icm_conv_winograd_ok(C.byref(a)) == 1


# ================================================================================================ reproducibility
REPRO = [R.case("staged", R.G3, cfg=4, inputs="real"), R.case("ks-row", R.G3, cfg=12, inputs="real"),
         R.case("ks8", R.G3, cfg=R.CFG_KS8_64, inputs="real"), R.case("pointwise", R.G1, f1x1=1, inputs="real"),
         R.case("wino44", R.G3, algo=R.WINOGRAD, inputs="real"), R.case("transposed", R.G5T, inputs="real", accum=1)]


@pytest.mark.parametrize("c", REPRO, ids=ids(REPRO))
def test_two_identical_calls_agree_bit_for_bit(c):
    a, b = run_single(c), run_single(c, c["id"] + " (second call)")
    assert same_bits(a[0], b[0])


def test_two_identical_calls_agree_bit_for_bit_eight_wave_winograd():
    """the eight-wave kernel reduces its K split through LDS: 12 members, 25 images, accumulating, twice"""
    c = next(c for c in R.W8_CASES if c["id"] == "wino8-tco4-N25-res_gelu-y2same-accum-real")
    cs = [dict(c, member=i) for i in range(R.WINO_W8_N)]
    assert R.plan(c).family == R.WINO8
    a, b = run_group(cs, "first call"), run_group(cs, "second call")
    for i in range(len(cs)):
        assert same_bits(a[i][0], b[i][0]), f"member {i}"


def all_cases():
    """every launch case of this file (tests/test_conv_ref.py: headroom of the grid cases, validity for the planner)"""
    out = GEOMETRY_CASES + [c for g, cfg, rc in FORCED if not rc for c in both("forced", g, cfg=cfg)] + BLOCK_ROWS + CROSS + \
        STAGING + POINTWISE_CHUNK_CASES + WINO + list(R.W8_CASES) + NONNEG + REPRO + \
        [dict(R.KS8_AUTO, inputs=w) for w in ("grid", "real")]
    for row, (n, g) in POINTWISE:
        out += [R.case("p1-row%d" % row, g, f1x1=1, member=i, ngroups=n) for i in range(n)]
    for g in R.GROUP_GEOMS:
        out += [R.case("group", g, member=i, ngroups=12, epi=R.E_RES, y2="sep") for i in range(12)]
    return out
