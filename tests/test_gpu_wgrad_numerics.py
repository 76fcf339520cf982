"""The weight-gradient kernels (csrc/conv_wgrad.hip, csrc/wgrad_wino.hip) through the C ABI against float64: every row
of the variant table forced on the geometries that admit it, both workgroup orders, every argument of icm_wgrad_args
(activations, accum, dbias / accum_bias against non-zero prefills, dw_ld, batch strides, pointers 4 bytes off 16-byte
alignment, ws_floats unchecked / exact / larger), grouped launches of 1 - 32 members, the Winograd form, the int32
guard of the big-grid offsets, and every refusal.

Every operand lies in its own allocation between NaN guards; strided operands are slices of wider NaN-filled buffers;
dw and dbias start as NaN unless the call accumulates; the workspace is exactly the queried size and starts as NaN.
Inputs, guards and the columns of a wider dw outside the block must be bit-identical afterwards, and after a refused
call so must outputs and workspace.  `grid` inputs must give wgrad64(...).float() bit for bit; `real` inputs are held to
tests/_wgrad_ref.py's limit (its docstring states the rule; none of it is taken from a kernel's output), and
tests/test_wgrad_ref.py asserts without a GPU that each case reaches the branch it is named for.  Each `real` check
prints its error / limit (pytest -s); DESIGN.md "Weight-gradient numerics" holds one such run."""
import ctypes as C

import pytest
import torch

import _wgrad_ref as R

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

    def __init__(self, n, lead, fill=None):
        self.n, self.lead = int(n), lead
        self.cpu0 = torch.full((lead + self.n + TAIL,), NAN, dtype=torch.float32)
        if fill is not None:
            fill(self.cpu0[lead:lead + self.n])
        self.dev = self.cpu0.to(dev())
        assert self.dev.data_ptr() % 16 == 0
        self.ptr = self.dev.data_ptr() + 4 * lead

    def now(self):
        return self.dev.cpu()

    def unchanged(self):
        return same_bits(self.now(), self.cpu0)


def operand(x, bs, lead):
    N, Cc = x.shape[:2]
    plane = x[0, 0].numel()

    def fill(v):
        for n in range(N):
            v[n * bs:n * bs + Cc * plane] = x[n].reshape(-1)
    return Buf(N * bs, lead, fill)


class Member:
    """one problem: operands, outputs and workspace of a case of _wgrad_ref, each in its own guarded allocation"""

    def __init__(self, c, need_ws, member=0):
        self.c, self.member = c, member
        g = self.g = c["g"]
        self.taps = taps = g.KH * g.KW
        if need_ws <= 0:                # a launch the planner refuses: still a real workspace of a plausible size
            need_ws = 4 * (max(taps, 16) * g.Ca * g.Cb + g.Ca)
        self.need_ws = need_ws
        lay = self.lay = R.layout(g, need_ws, c["gs_stride"], c["gb_stride"], c["dw_ld"], c["misalign"], c["ws_mode"])
        which = c["inputs"]
        self.gs = operand(R.make_input(g, which, "gs", member), lay.gs_bs, lay.gs_lead)
        self.gb = operand(R.make_input(g, which, "gb", member), lay.gb_bs, lay.gb_lead)
        ld = lay.dw_ld
        a = torch.arange(g.Ca).view(-1, 1, 1)
        b = torch.arange(g.Cb).view(1, -1, 1)
        t = torch.arange(taps).view(1, 1, -1)
        self.block = ((a * ld + b) * taps + t).reshape(-1)          # offsets of the block from the dw pointer
        self.pre_w = R.make_input(g, which, "dw", member) if c["accum"] else None
        self.pre_b = R.make_input(g, which, "dbias", member) if c["accum_bias"] else None
        col0 = lay.dw_col0 * taps

        def fill_dw(v):
            if self.pre_w is not None:
                v[col0 + self.block] = self.pre_w.reshape(-1)
        self.dw = Buf(g.Ca * ld * taps, lay.dw_lead, fill_dw)
        self.dw_ptr = self.dw.ptr + 4 * col0
        self.col0 = col0
        self.db = Buf(g.Ca, 4, (lambda v: v.copy_(self.pre_b)) if self.pre_b is not None else None) if c["dbias"] else None
        self.ws = Buf(need_ws + lay.ws_extra, lay.ws_lead)
        for name, buf_ptr, lead in (("gs", self.gs.ptr, lay.gs_lead), ("gb", self.gb.ptr, lay.gb_lead),
                                    ("ws", self.ws.ptr, lay.ws_lead)):
            assert (buf_ptr % 16 == 0) == (lead % 4 == 0), name
        A = self.args = lib().WgradArgs()
        A.gs, A.gs_bs, A.Ca, A.OH, A.OW, A.act_s = self.gs.ptr, lay.gs_bs, g.Ca, g.OH, g.OW, c["act_s"]
        A.gb, A.gb_bs, A.Cb, A.H, A.W, A.act_b = self.gb.ptr, lay.gb_bs, g.Cb, g.H, g.W, c["act_b"]
        A.N, A.KH, A.KW, A.stride, A.pad = g.N, g.KH, g.KW, g.stride, g.pad
        A.dw, A.ws, A.accum = self.dw_ptr, self.ws.ptr, c["accum"]
        A.dbias, A.accum_bias = (self.db.ptr if self.db else 0), c["accum_bias"]
        A.ws_floats, A.dw_ld, A.algo = lay.ws_floats_arg, c["dw_ld"], c["algo"]

    def buffers(self):
        return [b for b in (self.gs, self.gb, self.dw, self.db, self.ws) if b is not None]

    def untouched(self, what):
        """after a refused call: inputs, outputs, workspace and every guard bit-identical"""
        for i, b in enumerate(self.buffers()):
            assert b.unchanged(), f"{what}: a refused call changed buffer {i} of member {self.member}"

    def results(self, what):
        """(dw block [Ca, Cb, taps], dbias or None) after checking inputs, guards and everything outside the block"""
        g = self.g
        assert self.gs.unchanged() and self.gb.unchanged(), f"{what}: an input operand (or its guards) changed"
        dw = self.dw.now()
        inner = self.dw.lead + self.col0 + self.block
        blk = dw[inner].reshape(g.Ca, g.Cb, self.taps).clone()
        dw[inner] = 0.0
        ref = self.dw.cpu0.clone()
        ref[inner] = 0.0
        assert same_bits(dw, ref), f"{what}: dw was written outside its block"
        assert torch.isfinite(blk).all(), f"{what}: dw kept (or read) its NaN prefill"
        db = None
        if self.db is not None:
            d = self.db.now()
            assert torch.isnan(d[:4]).all() and torch.isnan(d[4 + g.Ca:]).all(), f"{what}: dbias guards"
            db = d[4:4 + g.Ca].clone()
            assert torch.isfinite(db).all(), f"{what}: dbias kept (or read) its NaN prefill"
        ws = self.ws.now()
        lead = self.ws.lead
        assert torch.isnan(ws[:lead]).all() and torch.isnan(ws[lead + self.need_ws:]).all(), f"{what}: workspace guards"
        return blk, db


def launch(members, variant=-1, xcd=-1, grouped=None, n=None):
    L = lib()
    arr = (L.WgradArgs * len(members))(*[m.args for m in members])
    n = len(members) if n is None else n
    if grouped is None:
        grouped = n != 1
    try:
        L.lib().icm_debug_force_wgrad_cfg(variant, xcd)
        if grouped:
            rc = L.lib().icm_conv_wgrad_grouped(arr, n, L.stream())
        else:
            rc = L.lib().icm_conv_wgrad(C.byref(arr[0]), L.stream())
    finally:
        L.lib().icm_debug_force_wgrad_cfg(-1, -1)
    torch.cuda.synchronize()
    return rc


def need_ws(c, n=1):
    return R.workspace_floats(c["g"], c["act_s"], c["act_b"], n, c["variant"], c["algo"])


def order_of(c, n=1):
    """(ntiles, nsplit, family) of the launch: the summation order of the float32 restatement"""
    g = c["g"]
    if c["algo"] == R.WINOGRAD:
        nsplit, _ = R.wino_splits(g, n)
        return -(-g.N * g.OH * g.OW // 32), nsplit, "wino"
    p = R.plan(g, c["act_s"], c["act_b"], n, c["variant"])
    assert p.rc == 0
    return p.ntiles, p.nsplit, p.family


def check(m, what, n=1):
    """member m's results against its own reference: bit equality on `grid`, the limit rule on `real`"""
    c, g = m.c, m.g
    blk, db = m.results(what)
    r = R.reference(g, c["inputs"], c["act_s"], c["act_b"], m.member)
    ref_w = r.dw + (m.pre_w.double() if m.pre_w is not None else 0)
    ref_b = r.db + (m.pre_b.double() if m.pre_b is not None else 0)
    if c["inputs"] == "grid":
        assert same_bits(blk, ref_w.float()), f"{what}: dw differs from the exact result in " \
            f"{int((blk != ref_w.float()).sum())} elements, by up to {(blk.double() - ref_w).abs().max().item():g}"
        if db is not None:
            assert same_bits(db, ref_b.float()), f"{what}: dbias differs from the exact result by up to " \
                f"{(db.double() - ref_b).abs().max().item():g}"
        return blk, db
    ntiles, nsplit, fam = order_of(c, n)
    w32, b32 = R.reference32(g, c["act_s"], c["act_b"], ntiles, nsplit, m.member)
    if m.pre_w is not None:
        w32 = w32 + m.pre_w
    if m.pre_b is not None:
        b32 = b32 + m.pre_b
    for name, got, r32, r64, floor in (("dw", blk, w32, ref_w, r.floor_w), ("dbias", db, b32, ref_b, r.floor_b)):
        if got is None:
            continue
        lim, e32 = R.limit(r32, r64, floor if R.GELU in (c["act_s"], c["act_b"]) else None)
        err = (got.double() - r64).abs().max().item()
        print(f"\nWGNUM {fam} {name} {what}: gpu {err:.3e} limit {lim:.3e} ratio {err / lim:.3f} ref32 {e32:.3e}")
        assert err <= lim, f"{what} {name}: {err:.3e} > limit {lim:.3e} (float32 restatement errs {e32:.3e})"
    return blk, db


def run_single(c, what=None, xcd=-1):
    what = what or c["id"]
    m = Member(c, need_ws(c))
    assert launch([m], c["variant"], xcd) == R.OK, what
    return check(m, what)


def ids(cases):
    return [c["id"] for c in cases]


# ================================================================================================ geometries, automatic choice
@pytest.mark.parametrize("c", R.geometry_cases(), ids=ids(R.geometry_cases()))
def test_every_geometry_exact_on_grid(c):
    run_single(c)


@pytest.mark.parametrize("c", R.real_cases(), ids=ids(R.real_cases()))
def test_every_geometry_within_the_limit_and_reproducible(c):
    """the limit rule on `real` inputs, and two identical calls on fresh NaN workspaces give the same bits"""
    a = run_single(c)
    b = run_single(c, c["id"] + " (second call)")
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]), c["id"] + ": two identical calls differ"


# ================================================================================================ every variant
VARIANT_ROWS = R.variant_table(R.ONE_TRIP + R.MULTI_TRIP)


@pytest.mark.parametrize("g,v,rc", VARIANT_ROWS, ids=["%s-v%d%s" % (R.gname(g), v, "-refused" if rc else "") for g, v, rc in VARIANT_ROWS])
def test_every_variant_both_orders(g, v, rc):
    """every row of the variant table forced on the one-trip and multi-trip geometries: exact on `grid` in both
    workgroup orders; a row the planner does not admit is refused with the planner's code and nothing is written.  On
    the one-trip geometries, and for one row of every family on the multi-trip ones, also the limit on `real` inputs,
    the two orders bit-identical"""
    if rc:
        m = Member(R.case("refused", g, variant=v), -1)
        assert launch([m], v, 0) == rc == R.ERR_UNSUPPORTED
        m.untouched(f"variant {v} refused")
        return
    sets = ("grid", "real") if v in R.real_variant_rows(g) else ("grid",)
    for which in sets:
        c = R.case("v%d" % v, g, variant=v, inputs=which)
        outs = [run_single(c, f"{R.gname(g)} v{v} {which} xcd{x}", xcd=x) for x in (0, 1)]
        assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1]), \
            f"variant {v} on {which}: the two workgroup orders differ"


@pytest.mark.parametrize("g", R.MULTI_TRIP[:4], ids=R.gname)
def test_workgroup_order_is_a_permutation_on_real_inputs(g):
    """multi-trip launches on `real` inputs: both orders of every admitted variant give the same bits"""
    for v in range(R.NVARIANTS):
        if R.plan(g, variant=v).rc:
            continue
        c = R.case("v%d" % v, g, variant=v, inputs="real")
        outs = []
        for x in (0, 1):
            m = Member(c, need_ws(c))
            assert launch([m], v, x) == R.OK
            outs.append(m.results(f"v{v} xcd{x}"))
        assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1]), f"variant {v}: orders differ"


# ================================================================================================ argument cross
@pytest.mark.parametrize("c", R.cross_cases(), ids=ids(R.cross_cases()))
def test_argument_cross(c):
    run_single(c)


VEC = R.vec_cases()


@pytest.mark.parametrize("c", [c for c, _ in VEC], ids=[c["id"] for c, _ in VEC])
def test_16_byte_forms_and_their_fallbacks(c):
    run_single(c)
    if c["inputs"] == "grid":
        run_single(dict(c, inputs="real"), c["id"] + " real")


# ================================================================================================ grouped launches
@pytest.mark.parametrize("n", R.GROUP_NS)
@pytest.mark.parametrize("g", R.GROUP_GEOMS, ids=R.gname)
def test_grouped_launch(g, n):
    """members differing in data, accum, dw_ld and dbias null / set: each against its own reference, and bit-identical
    to the n single launches although the planner gives those other split counts"""
    cs = R.group_members(g, n, "grid")
    ws = need_ws(cs[0], n)
    ms = [Member(c, ws, i) for i, c in enumerate(cs)]
    assert launch(ms, grouped=True) == R.OK
    for i, m in enumerate(ms):
        blk, db = check(m, f"group of {n}, member {i}", n)
        s = Member(cs[i], need_ws(cs[i]), i)
        assert launch([s]) == R.OK
        sb, sd = s.results(f"single launch of member {i}")
        assert same_bits(blk, sb) and (db is None or same_bits(db, sd)), f"member {i}: grouped and single launch differ"


@pytest.mark.parametrize("g", R.GROUP_GEOMS[:2], ids=R.gname)
def test_grouped_launch_real(g):
    n = 3
    cs = R.group_members(g, n, "real")
    ws = need_ws(cs[0], n)
    ms = [Member(c, ws, i) for i, c in enumerate(cs)]
    assert launch(ms, grouped=True) == R.OK
    for i, m in enumerate(ms):
        check(m, f"real group of {n}, member {i}", n)


# ================================================================================================ Winograd
@pytest.mark.parametrize("c", R.wino_cases(), ids=ids(R.wino_cases()))
def test_winograd(c):
    run_single(c)


@pytest.mark.parametrize("n", [2, 32])
def test_winograd_grouped(n):
    g = R.WINO_GEOMS[4]
    cs = R.group_members(g, n, "grid", algo=R.WINOGRAD)
    ws = need_ws(cs[0], n)
    ms = [Member(c, ws, i) for i, c in enumerate(cs)]
    assert launch(ms, grouped=True) == R.OK
    for i, m in enumerate(ms):
        check(m, f"winograd group of {n}, member {i}", n)


# ================================================================================================ near the int32 limit
@pytest.mark.parametrize("gb_bs", [R.INT32_REFUSED_BS, R.INT32_LARGEST_BS], ids=["refused", "largest-accepted"])
def test_big_grid_offsets_near_int32(gb_bs):
    """the guard of the int32 big-grid byte offsets: a real allocation of N * gb_bs floats backs both sides of it, so
    nothing can be read out of bounds whichever way the guard decides; only the two images' planes are written"""
    g = R.INT32_G
    refused = R.int32_guard_refuses(g, gb_bs)
    assert refused == (gb_bs == R.INT32_REFUSED_BS) and R.int32_guard_refuses(g, R.INT32_LARGEST_BS + 1)
    c = R.case("int32", g)
    m = Member(c, need_ws(c))
    x = R.make_input(g, "grid", "gb")
    big = torch.empty(g.N * gb_bs, dtype=torch.float32, device=dev())
    for i in range(g.N):
        big[i * gb_bs:i * gb_bs + g.Cb * g.H * g.W] = x[i].reshape(-1).to(dev())
    m.args.gb, m.args.gb_bs = big.data_ptr(), gb_bs
    rc = launch([m])
    if refused:
        assert rc == R.ERR_UNSUPPORTED
        m.untouched("int32 guard")
    else:
        assert rc == R.OK
        check(m, "largest accepted gb_bs")
    for i in range(g.N):
        assert same_bits(big[i * gb_bs:i * gb_bs + g.Cb * g.H * g.W].cpu(), x[i].reshape(-1)), "gb changed"
    del big


# ================================================================================================ refusals
def _set(**kw):
    def f(ms):
        for k, v in kw.items():
            setattr(ms[0].args, k, v)
    return f


def _set1(**kw):
    def f(ms):
        for k, v in kw.items():
            setattr(ms[1].args, k, v)
    return f


G3 = R.ONE_TRIP[1]
G1 = R.ONE_TRIP[0]
G5 = R.ONE_TRIP[4]
W = R.WINOGRAD
# id, case kwargs + geometry, members, call count n (None = members), tweak, forced variant, expected code
REFUSALS = [
    ("gs-null", G3, {}, 1, None, _set(gs=0), -1, R.ERR_ARG),
    ("gb-null", G3, {}, 1, None, _set(gb=0), -1, R.ERR_ARG),
    ("dw-null", G3, {}, 1, None, _set(dw=0), -1, R.ERR_ARG),
    ("ws-null", G3, {}, 1, None, _set(ws=0), -1, R.ERR_ARG),
    ("N-zero", G3, {}, 1, None, _set(N=0), -1, R.ERR_ARG),
    ("N-negative", G3, {}, 1, None, _set(N=-1), -1, R.ERR_ARG),
    ("Ca-zero", G3, {}, 1, None, _set(Ca=0), -1, R.ERR_ARG),
    ("Cb-negative", G3, {}, 1, None, _set(Cb=-3), -1, R.ERR_ARG),
    ("OH-inconsistent", G3, {}, 1, None, _set(OH=G3.OH - 1), -1, R.ERR_ARG),
    ("ws-floats-one-short", G3, {}, 1, None, lambda ms: setattr(ms[0].args, "ws_floats", ms[0].need_ws - 1), -1, R.ERR_ARG),
    ("ws-floats-one-short-grouped", G3, {}, 3, None, lambda ms: setattr(ms[2].args, "ws_floats", ms[2].need_ws - 1), -1, R.ERR_ARG),
    ("dw_ld-below-Cb", G3, {}, 1, None, _set(dw_ld=G3.Cb - 1), -1, R.ERR_ARG),
    ("dw_ld-below-Cb-1x1", G1, {}, 1, None, _set(dw_ld=1), -1, R.ERR_ARG),
    ("dw_ld-below-Cb-grouped-member", G3, {}, 3, None, _set1(dw_ld=G3.Cb - 4), -1, R.ERR_ARG),
    ("n-zero", G3, {}, 1, 0, None, -1, R.ERR_ARG),
    ("n-33", G3, {}, 33, None, None, -1, R.ERR_ARG),
    ("algo-2", G3, {}, 1, None, _set(algo=2), -1, R.ERR_ARG),
    ("member-differs-in-Ca", G3, {}, 2, None, _set1(Ca=G3.Ca - 8), -1, R.ERR_ARG),
    ("member-differs-in-gs_bs", G3, {}, 2, None, lambda ms: setattr(ms[0].args, "gs_bs", ms[0].args.gs_bs - 1), -1, R.ERR_ARG),
    ("member-differs-in-act_b", G3, {}, 2, None, _set1(act_b=R.SQUARE), -1, R.ERR_ARG),
    ("member-differs-in-algo", G3, {}, 2, None, _set1(algo=W), -1, R.ERR_ARG),
    ("stride-3", R.geom(2, 4, 5, 3, 3, 1), {}, 1, None, None, -1, R.ERR_UNSUPPORTED),
    ("taps-30", R.REFUSED_KERNELS[0][0], {}, 1, None, None, -1, R.REFUSED_KERNELS[0][1]),
    ("taps-32", R.REFUSED_KERNELS[1][0], {}, 1, None, None, -1, R.REFUSED_KERNELS[1][1]),
    ("7x7", R.REFUSED_KERNELS[2][0], {}, 1, None, None, -1, R.REFUSED_KERNELS[2][1]),
    ("v14-forced-with-gelu", G1, dict(act_s=R.GELU, inputs="real"), 1, None, None, 14, R.ERR_UNSUPPORTED),
    ("v11-forced-with-square-b", G1, dict(act_b=R.SQUARE), 1, None, None, 11, R.ERR_UNSUPPORTED),
    ("v8-forced-with-square", G3, dict(act_b=R.SQUARE), 1, None, None, 8, R.ERR_UNSUPPORTED),
    ("v9-forced-with-gelu", G3, dict(act_s=R.GELU, inputs="real"), 1, None, None, 9, R.ERR_UNSUPPORTED),
    ("v10-forced-with-square", G5, dict(act_s=R.SQUARE), 1, None, None, 10, R.ERR_UNSUPPORTED),
    ("winograd-stride-2", R.ONE_TRIP[3], dict(algo=W), 1, None, None, -1, R.ERR_UNSUPPORTED),
    ("winograd-5x5", R.ONE_TRIP[5], dict(algo=W), 1, None, None, -1, R.ERR_UNSUPPORTED),
    ("winograd-pad-0", R.ONE_TRIP[2], dict(algo=W), 1, None, None, -1, R.ERR_UNSUPPORTED),
    ("winograd-gelu", G3, dict(algo=W, act_s=R.GELU, inputs="real"), 1, None, None, -1, R.ERR_UNSUPPORTED),
    ("winograd-square-b", G3, dict(algo=W, act_b=R.SQUARE), 1, None, None, -1, R.ERR_UNSUPPORTED),
    ("winograd-dw_ld-below-Cb", G3, dict(algo=W), 1, None, _set(dw_ld=G3.Cb - 1), -1, R.ERR_ARG),
    ("winograd-dw_ld-below-Cb-grouped-member", G3, dict(algo=W), 2, None, _set1(dw_ld=3), -1, R.ERR_ARG),
    ("winograd-ws-floats-one-short", G3, dict(algo=W), 1, None, lambda ms: setattr(ms[0].args, "ws_floats", ms[0].need_ws - 1), -1, R.ERR_ARG),
    ("winograd-dw-null", G3, dict(algo=W), 1, None, _set(dw=0), -1, R.ERR_ARG),
    ("winograd-member-differs-in-Cb", G3, dict(algo=W), 2, None, _set1(Cb=G3.Cb - 1), -1, R.ERR_ARG),
]


@pytest.mark.parametrize("rid,g,kw,nm,ncall,tweak,variant,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_launch_nothing(rid, g, kw, nm, ncall, tweak, variant, code):
    """the expected code, and outputs, workspace, inputs and guards bit-identical: nothing was launched.  Every
    refused call has real allocations large enough for the geometry it names"""
    c = R.case(rid, g, **kw)
    ws = R.workspace_floats(g, c["act_s"], c["act_b"], min(nm, 32), -1, c["algo"])
    if rid.startswith("v") and "forced" in rid:
        assert R.plan(g, c["act_s"], c["act_b"], 1, variant).rc == code      # the planner itself refuses
    ms = [Member(c, ws, i) for i in range(min(nm, 3))]
    ms = ms + [ms[0]] * (nm - len(ms))            # n = 33: the surplus descriptors repeat member 0
    if tweak:
        tweak(ms)
    rc = launch(ms, variant, grouped=(nm != 1 or ncall is not None), n=ncall)
    assert rc == code, f"{rid}: returned {rc}, expected {code}"
    for m in ms[:3]:
        m.untouched(rid)
