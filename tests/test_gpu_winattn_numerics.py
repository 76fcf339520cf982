"""The window-attention kernels (csrc/winattn.hip, csrc/winattn_mfma.hip) through the C ABI against float64: every
kernel family (matrix cores for 8x8 and for 4x4 windows, the generic VALU kernels at every window size up to 8x8) at
every head dim of its table, asserted with icm_debug_winattn_route before the call.

Three input sets per row (tests/_winattn_ref.py; their regimes are asserted without a GPU in tests/test_winattn_ref.py):
``mild`` (flat softmax rows, today's regime), ``hot`` (peaked rows: the max subtraction and the normalisation matter)
and, where the windows are shifted, ``leak<L>`` (the -100 of the shift mask competes with the un-masked logits, so a
mask of -inf, another constant or wrongly masked pairs change the result).  out, dq, dk, dv and dtable are compared
each against its own limit, FACTOR (4) times the error of the float32 evaluation of the same formula plus 4 units of
float32 roundoff; no limit is taken from a kernel's output.

Every device operand is the middle of its own allocation between two guard bands; outputs and the workspace start as
NaN.  Each check prints ``err / limit`` (pytest -s); DESIGN.md "Window-attention numerics" holds one such run."""
import contextlib
import math

import pytest
import torch

import _winattn_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 64                      # floats on either side of every operand
PATTERN = 0x5EEDBA5E            # bit pattern of the guard bands (a finite float32, 5.35e18)
ICM_OK, ICM_ERR_ARG, ICM_ERR_UNSUPPORTED = 0, R.ERR_ARG, R.ERR_UNSUPPORTED
CASES = R.MATRIX + R.REDUCTION


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def L():
    from icm_amd import _lib
    return _lib


class Guarded:
    """``n`` floats in the middle of their own allocation: ``value`` or NaN between two bands of PATTERN"""

    def __init__(self, n, value=None):
        self.n = int(n)
        self.buf = torch.full((self.n + 2 * GUARD,), PATTERN, dtype=torch.int32, device=dev())
        self.mid = self.buf[GUARD:GUARD + self.n].view(torch.float32)
        if value is None:
            self.mid.fill_(NAN)
        else:
            self.mid.copy_(value.reshape(-1))
        self.ptr = self.mid.data_ptr()

    def cpu(self, shape=None):
        t = self.mid.cpu()
        return t if shape is None else t.reshape(shape)

    def guards_intact(self):
        b = self.buf.cpu()
        return bool((b[:GUARD] == PATTERN).all() and (b[GUARD + self.n:] == PATTERN).all())

    def all_nan(self):
        return bool(torch.isnan(self.mid).all().item())

    def same_bits(self, value):
        return torch.equal(self.mid.cpu().view(torch.int32), value.reshape(-1).contiguous().view(torch.int32))


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@contextlib.contextmanager
def forced(on):
    lib = L().lib()
    lib.icm_debug_force_winattn_valu(int(on))
    try:
        yield
    finally:
        lib.icm_debug_force_winattn_valu(0)


geometry = R.geometry


def route(case, backward):
    return L().lib().icm_debug_winattn_route(*geometry(case), backward)


def workspace_floats(case):
    N, C, H, W, heads, ws, _ = geometry(case)
    return L().lib().icm_winattn_bwd_workspace_floats(N, C, H, W, heads, ws)


def check(what, got, ref, t, extra=0.0, expected=None):
    """max |got - float64 reference| within the tensor's limit (+ ``extra``); NaN fails"""
    want = ref.x64[t] if expected is None else expected
    err = (got.double() - want).abs().max().item()
    own = (ref.x32[t].double() - ref.x64[t]).abs().max().item()
    lim = ref.lim[t] + extra
    print(f"WINATTN {what} {t}: err {err:.3e} oracle {own:.3e} limit {lim:.3e} err/limit {err / lim:.3f}")
    assert not torch.isnan(got).any(), f"{what} {t}: NaN left in the output"
    assert math.isfinite(err) and err <= lim, f"{what} {t}: {err:.3e} > limit {lim:.3e} (float32 oracle {own:.3e})"


class Operands:
    """device copies of one reference's inputs and fresh NaN outputs, each in its own guarded allocation"""

    def __init__(self, case, ref, ws_floats=None, dtable_prefill=None):
        self.case, self.ref = case, ref
        N, C, H, W, heads, ws, _ = geometry(case)
        self.qkv, self.table, self.dout = Guarded(ref.qkv.numel(), ref.qkv), Guarded(ref.table.numel(), ref.table), \
            Guarded(ref.dout.numel(), ref.dout)
        self.out, self.dqkv = Guarded(N * C * H * W), Guarded(3 * N * C * H * W)
        self.dtable = Guarded(ref.table.numel(), dtable_prefill)
        self.ws_floats = workspace_floats(case) if ws_floats is None else ws_floats
        assert self.ws_floats > 0
        self.wsp = Guarded(self.ws_floats)

    def fwd(self):
        return L().lib().icm_winattn_fwd(self.qkv.ptr, self.table.ptr, self.out.ptr, *geometry(self.case), L().stream())

    def bwd(self, accum=0, ws_floats=None):
        n = self.ws_floats if ws_floats is None else ws_floats
        return L().lib().icm_winattn_bwd(self.qkv.ptr, self.table.ptr, self.dout.ptr, self.dqkv.ptr, self.dtable.ptr, accum,
                                         self.wsp.ptr, n, *geometry(self.case), L().stream())

    def assert_intact(self, what):
        torch.cuda.synchronize()
        for name in ("qkv", "table", "dout", "out", "dqkv", "dtable", "wsp"):
            assert getattr(self, name).guards_intact(), f"{what}: a guard band of {name} changed"
        for name in ("qkv", "table", "dout"):
            assert getattr(self, name).same_bits(getattr(self.ref, name)), f"{what}: input {name} changed"

    def grads(self):
        C = self.case.heads * self.case.hd
        g = self.dqkv.cpu((self.case.N, 3 * C, self.case.H, self.case.W))
        return {"dq": g[:, :C], "dk": g[:, C:2 * C], "dv": g[:, 2 * C:], "dtable": self.dtable.cpu(self.ref.table.shape)}


def run_forward(case, kind, ref):
    with forced(case.force):
        r = route(case, 0)
        assert r == case.route[0], f"{case.name}: forward route {r}, expected {case.route[0]}"
        ops = Operands(case, ref)
        rc = ops.fwd()
        ops.assert_intact(f"{case.name} {kind} fwd")
    assert rc == ICM_OK, rc
    check(f"{case.name} {kind} route{r}", ops.out.cpu(ref.x64["out"].shape), ref, "out")
    assert ops.dqkv.all_nan() and ops.dtable.all_nan() and ops.wsp.all_nan()
    return ops


def run_backward(case, kind, ref):
    with forced(case.force):
        r = route(case, 1)
        assert r == case.route[1], f"{case.name}: backward route {r}, expected {case.route[1]}"
        ops = Operands(case, ref)
        rc = ops.bwd(accum=0)
        ops.assert_intact(f"{case.name} {kind} bwd")
    assert rc == ICM_OK, rc
    for t, g in ops.grads().items():
        check(f"{case.name} {kind} route{r}", g, ref, t)
    assert ops.out.all_nan()
    return ops


@pytest.mark.parametrize("case,kind", [(c, k) for c in CASES for k in R.input_sets(c)],
                         ids=lambda v: v.name if isinstance(v, R.Case) else v)
def test_forward_and_backward(case, kind):
    ref = R.reference(case.name, kind)
    run_forward(case, kind, ref)
    run_backward(case, kind, ref)


def test_reduction_plans_are_the_ones_meant():
    """the shapes of R.REDUCTION reach S = 2 with a ragged last chunk and the capped plan on every route"""
    plans = {}
    for case in R.REDUCTION:
        N, C, H, W, heads, ws, shift = geometry(case)
        nwin = N * (H // ws) * (W // ws)
        slabs = N * (H // 4) * ((W // 4 + 3) // 4) if case.route[1] == R.ROUTE_MFMA16 else nwin
        S, chunk = R.reduction_plan(slabs)
        plans[case.name] = (slabs, S, chunk)
        # the workspace is planned per window on every route
        Sw, _ = R.reduction_plan(nwin)
        assert workspace_floats(case) == (nwin + Sw) * heads * (2 * ws - 1) ** 2
        assert route(case, 1) == case.route[1]
    print(plans)
    assert plans["reduce-valu-33win"] == (33, 2, 17)                 # chunks of 17 and 16
    assert plans["reduce-valu-1056win"] == (1056, 63, 17)            # S capped at 64, last chunk 2
    assert plans["reduce-mfma8-289win"] == (289, 17, 17)
    assert plans["reduce-mfma4-288slabs"] == (288, 18, 16)


@pytest.mark.parametrize("kind", R.input_sets(R.LDS_CASE))
def test_forward_over_the_lds_cap_is_refused_backward_runs(kind):
    """8x8 windows, head dim 48, five heads on the VALU kernels: the forward's four waves need 164 864 bytes of LDS
    and the call refuses, the backward's two waves need 107 008 and it runs"""
    case, ref = R.LDS_CASE, R.reference(R.LDS_CASE.name, kind)
    with forced(1):
        assert route(case, 0) == -ICM_ERR_UNSUPPORTED and route(case, 1) == R.ROUTE_VALU
        ops = Operands(case, ref)
        rc = ops.fwd()
        ops.assert_intact("lds cap fwd")
    assert rc == ICM_ERR_UNSUPPORTED
    assert ops.out.all_nan() and ops.dqkv.all_nan() and ops.dtable.all_nan() and ops.wsp.all_nan()
    run_backward(case, kind, ref)
    # without the hook the matrix cores serve the forward, and the backward (210 KB there) stays on the VALU kernels
    assert route(case, 0) == R.ROUTE_MFMA and route(case, 1) == R.ROUTE_VALU


@pytest.mark.parametrize("name", R.PER_ROUTE)
def test_backward_contract(name):
    case, ref = R.BY_NAME[name], R.reference(name, "mild")
    what = f"{name} contract"
    # accum_table = 1 adds to what dtable holds: one more rounding, of the sum
    prefill = R.Wt._u(f"winattn.{name}.prefill", tuple(ref.table.shape), -1.0, 1.0)
    with forced(case.force):
        ops = Operands(case, ref, dtable_prefill=prefill)
        rc = ops.bwd(accum=1)
        ops.assert_intact(what)
    assert rc == ICM_OK
    expected = prefill.double() + ref.x64["dtable"]
    g = ops.grads()
    check(f"{what} accum route{case.route[1]}", g["dtable"], ref, "dtable", extra=2.0 ** -23 * expected.abs().max().item(),
          expected=expected)
    for t in ("dq", "dk", "dv"):
        check(f"{what} accum route{case.route[1]}", g[t], ref, t)
    # a workspace one float short: refused, nothing written
    with forced(case.force):
        ops = Operands(case, ref)
        rc = ops.bwd(accum=0, ws_floats=ops.ws_floats - 1)
        ops.assert_intact(what)
    assert rc == ICM_ERR_ARG
    assert ops.dqkv.all_nan() and ops.dtable.all_nan() and ops.wsp.all_nan() and ops.out.all_nan()


@pytest.mark.parametrize("name", R.PER_ROUTE)
def test_bitwise_repeatable(name):
    case, ref = R.BY_NAME[name], R.reference(name, "hot")
    runs = []
    with forced(case.force):
        for _ in range(2):
            ops = Operands(case, ref)
            assert ops.fwd() == ICM_OK and ops.bwd(accum=0) == ICM_OK
            ops.assert_intact(f"{name} repeat")
            runs.append((ops.out.cpu(), ops.dqkv.cpu(), ops.dtable.cpu()))
    for a, b, t in zip(runs[0], runs[1], ("out", "dqkv", "dtable")):
        assert not torch.isnan(a).any() and same_bits(a, b), f"{name}: {t} differs between two identical calls"


def _refused(what, geo, want, fwd_null=(), bwd_null=()):
    """both entry points return ``want`` for the geometry (N, C, H, W, heads, ws, shift) and write nothing; *_null:
    operands passed as null pointers"""
    N, C, H, W, heads, ws, shift = geo
    n = max(1, N * C * H * W)
    bufs = {"qkv": Guarded(3 * n), "table": Guarded(max(1, (2 * ws - 1) ** 2 * heads)), "dout": Guarded(n),
            "out": Guarded(n), "dqkv": Guarded(3 * n), "dtable": Guarded(max(1, (2 * ws - 1) ** 2 * heads)),
            "wsp": Guarded(4096)}
    for k in ("qkv", "table", "dout"):
        bufs[k].mid.fill_(0.25)
    lib, st = L().lib(), L().stream()

    def p(k, null):
        return 0 if k in null else bufs[k].ptr
    rc_f = lib.icm_winattn_fwd(p("qkv", fwd_null), p("table", fwd_null), p("out", fwd_null), *geo, st)
    rc_b = lib.icm_winattn_bwd(p("qkv", bwd_null), p("table", bwd_null), p("dout", bwd_null), p("dqkv", bwd_null),
                               p("dtable", bwd_null), 0, p("wsp", bwd_null), 1 << 40, *geo, st)
    torch.cuda.synchronize()
    assert (rc_f, rc_b) == (want, want), f"{what}: forward {rc_f}, backward {rc_b}, expected {want}"
    for k, b in bufs.items():
        assert b.guards_intact(), f"{what}: guard of {k}"
    for k in ("out", "dqkv", "dtable", "wsp"):
        assert bufs[k].all_nan(), f"{what}: {k} was written"


def test_refusals():
    ok = (1, 8, 4, 4, 1, 4, 0)
    lib = L().lib()
    for k in ("qkv", "table", "out"):
        _refused(f"null {k} (forward)", ok, ICM_ERR_ARG, fwd_null=(k,), bwd_null=("qkv",))
    for k in ("qkv", "table", "dout", "dqkv", "dtable", "wsp"):
        _refused(f"null {k} (backward)", ok, ICM_ERR_ARG, fwd_null=("out",), bwd_null=(k,))
    bad = [("shift == ws", (1, 8, 4, 4, 1, 4, 4), ICM_ERR_ARG),
           ("negative shift", (1, 8, 4, 4, 1, 4, -1), ICM_ERR_ARG),
           ("H % ws", (1, 8, 6, 4, 1, 4, 0), ICM_ERR_ARG),
           ("W % ws", (1, 8, 8, 12, 1, 8, 0), ICM_ERR_ARG),
           ("C % heads", (1, 10, 4, 4, 3, 4, 0), ICM_ERR_ARG),
           ("ws = 9", (1, 8, 9, 9, 1, 9, 0), ICM_ERR_UNSUPPORTED),
           ("head dim 12, 4x4", (1, 12, 4, 4, 1, 4, 0), ICM_ERR_UNSUPPORTED),
           ("head dim 12, 8x8", (1, 24, 8, 8, 2, 8, 0), ICM_ERR_UNSUPPORTED),
           ("head dim 12, 2x2", (1, 12, 4, 4, 1, 2, 1), ICM_ERR_UNSUPPORTED)]
    for what, geo, want in bad:
        for backward in (0, 1):
            assert lib.icm_debug_winattn_route(*geo, backward) == -want, what
        _refused(what, geo, want)
    assert lib.icm_winattn_bwd_workspace_floats(1, 8, 6, 4, 1, 4) == -1
    assert lib.icm_winattn_bwd_workspace_floats(1, 8, 4, 6, 1, 4) == -1
    assert lib.icm_winattn_bwd_workspace_floats(0, 8, 4, 4, 1, 4) == -1
    assert lib.icm_winattn_bwd_workspace_floats(1, 8, 4, 4, 0, 4) == -1
    assert lib.icm_winattn_bwd_workspace_floats(1, 8, 4, 4, 1, 0) == -1
    assert lib.icm_winattn_bwd_workspace_floats(1, 8, 4, 4, 1, 4) == 2 * 49
