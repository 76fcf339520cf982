"""The engine's gradient bookkeeping (icm_amd/engine.py: Tape and the op wrappers) on small graphs against torch autograd
on a float64 mirror (tests/_engine_ref.py): bit for bit on the exact `grid` inputs, within the project's limit on `real`.

Every real check prints ``error / limit`` (pytest -s).  Path witnesses are recording wrappers around the engine's Python
functions (_conv_launch, accumulate, flush_wgrads) and around the icm_conv_wgrad_grouped attribute of the loaded library
object; the library itself is not touched."""
import time
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

import _engine_ref as R
import _pointwise_ref as PR

pytestmark = pytest.mark.gpu
_REPORT = []


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _file_runtime():
    t0 = time.perf_counter()
    yield
    print(f"\ntest_gpu_engine_graphs.py: {time.perf_counter() - t0:.1f} s in all")
    for line in _REPORT:
        print(line)


@pytest.fixture
def E(monkeypatch):
    from icm_amd import engine
    monkeypatch.setattr(engine, "_MAT_MIN_PIXELS", 0)      # materialisation engages at these sizes
    return engine


# ================================================================================================ witnesses
Launch = namedtuple("Launch", "tag epi accum n single algo pro_act xs ys")


class Rec:
    def __init__(self):
        self.launches, self.accs, self.flushes, self.wgroups = [], [], 0, []

    def dgrads(self):
        return [l for l in self.launches if l.tag.startswith("dgrad")]

    def accs_of(self, E, t):
        return [a for k, a in self.accs if k == E._key(t)]


def record(monkeypatch, E):
    """wrap the engine's Python functions and the grouped weight-gradient entry of the library object"""
    from icm_amd import _lib
    rec = Rec()
    conv_launch, accumulate, flush, lib = E._conv_launch, E.accumulate, E.flush_wgrads, _lib.lib()
    grouped = lib.icm_conv_wgrad_grouped

    def w_launch(tape, single, xs, wps, biases, ys, **kw):
        rec.launches.append(Launch(kw.get("tag", "fwd"), kw.get("epi", 0), kw.get("accum", 0), len(xs), single,
                                   kw.get("algo", 0), kw.get("pro_act", 0), [E._key(x) for x in xs], [E._key(y) for y in ys]))
        return conv_launch(tape, single, xs, wps, biases, ys, **kw)

    def w_accumulate(tape, dst_t, src, mul_dgelu_of=None):
        if tape.wants(dst_t):
            rec.accs.append((E._key(dst_t), (1 if E._key(dst_t) in tape.ready else 0, mul_dgelu_of is not None)))
        return accumulate(tape, dst_t, src, mul_dgelu_of)

    def w_flush(tape):
        rec.flushes += 1
        return flush(tape)

    def w_grouped(arr, n, st):
        rec.wgroups.append([(arr[i].dw, arr[i].dbias, arr[i].accum, arr[i].accum_bias) for i in range(n)])
        return grouped(arr, n, st)

    monkeypatch.setattr(E, "_conv_launch", w_launch)
    monkeypatch.setattr(E, "accumulate", w_accumulate)
    monkeypatch.setattr(E, "flush_wgrads", w_flush)
    monkeypatch.setattr(lib, "icm_conv_wgrad_grouped", w_grouped)
    return rec


# ================================================================================================ running a graph
Run = namedtuple("Run", "outs grads tape T")


def run(E, name, which, *, setup=None, mid=None, need_grad=True, act_out=True, backward=True):
    """build the graph on the device, bind the fixed upstream gradients, unwind; everything comes back on the CPU"""
    g = R.GRAPHS[name]
    d = dev()
    T = R.NS((k, v.to(d)) for k, v in R.make_inputs(g, which).items())
    before = {k: v.clone() for k, v in T.items()}
    tape = E.Tape(need_grad=need_grad)
    if setup:
        setup(tape)
    for s in g.stops:
        tape.stop(T[s])
    outs = g.build(tape, T, R.opts(E, which, act_out=act_out))
    leaf = outs.pop("_leaf", {})
    grads = {}
    if need_grad and backward:
        ups = R.upstream(g, which, {k: outs[k].shape for k in g.outs})
        for k in g.outs:
            tape.bind_grad(outs[k], ups[k].to(d), True)
        if mid:
            mid(tape)
        tape.backward()
        grads = {k: tape.grad_of(leaf.get(k, T[k])) for k in R.leaves(g)}
        assert not tape._pending_res and not tape.wjobs and not tape.bw
    torch.cuda.synchronize()
    for k, v in T.items():
        assert torch.equal(v, before[k]), f"{name}: input {k} was written to"
    return Run({k: v.detach().cpu() for k, v in outs.items()},
               {k: (None if v is None else v.detach().cpu()) for k, v in grads.items()}, tape, T)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def compare(name, which, got: Run, values_only=False, tag=""):
    """every forward value and every gradient against the mirror; a gradient the graph must not produce is None"""
    g = R.GRAPHS[name]
    ref = R.reference(name, which)
    pairs = [(k, got.outs[k], v) for k, v in ref.outs.items()]
    if not values_only:
        for k in R.leaves(g):
            r = ref.grads.get(k)
            if k in g.zero:
                assert r is None and got.grads[k] is not None and not got.grads[k].any(), f"{name}: {k} must be zeros"
            elif k in g.stops or r is None:
                assert got.grads[k] is None, f"{name}: {k} must have no gradient"
            else:
                assert got.grads[k] is not None, f"{name}: {k} has no gradient"
                pairs.append(("d." + k, got.grads[k], r))
    if which == "grid":
        for k, a, r in pairs:
            if not bits_equal(a, r.float()):
                bad = (a.double() - r).abs()
                raise AssertionError(f"{name}{tag} grid {k}: {int((bad > 0).sum())} of {bad.numel()} elements differ, "
                                     f"largest difference {bad.max().item():g}")
        return
    lim = R.limits(name)
    worst = (0.0, "")
    for k, a, r in pairs:
        err = (a.double() - r).abs().max().item()
        limit = lim[k][0]
        ratio = err / limit if limit > 0 else (0.0 if err == 0 else float("inf"))      # (a gradient that is exactly zero)
        line = f"{name}{tag} real {k}: error {err:.3e} / limit {limit:.3e} = {ratio:.3f}"
        print(line)
        worst = max(worst, (ratio, k))
        assert err == err and err <= limit, line
    _REPORT.append(f"| {name}{tag} | {worst[1]} | {worst[0]:.3f} |")


# ================================================================================================ every graph, with its witness
def _no_witness(*a):
    pass


def w_ride(E, rec, got, which, name):
    """the identity-path term rode on the first convolution's dgrad: no accumulate for x, EPI_RES(_MUL_DGELU), overwrite"""
    x = got.T.x
    assert rec.accs_of(E, x) == []
    last = rec.dgrads()[-1]
    want = E.EPI_RES_MUL_DGELU if (which == "real" and name == "ride_gelu") else E.EPI_RES
    assert (last.epi, last.accum) == (want, 0), last
    assert [l.epi for l in rec.dgrads()[:-1]] == [E.EPI_MUL_DGELU if which == "real" else E.EPI_NONE] * 2


def w_ride_mismatch(E, rec, got, which, name):
    """real: the term has the other activation, so it is flushed (accumulate, first writer) and the dgrad accumulates
    without a residual epilogue.  grid: both activations are NONE, the term rides"""
    last = rec.dgrads()[-1]
    if which == "grid":
        assert rec.accs_of(E, got.T.x) == [] and (last.epi, last.accum) == (E.EPI_RES, 0)
        return
    gelu_res = name.endswith("gelu_res")
    assert rec.accs_of(E, got.T.x) == [(0, gelu_res)]
    assert (last.epi, last.accum) == (E.EPI_NONE if gelu_res else E.EPI_MUL_DGELU, 1), last


def w_ride_preempted(E, rec, got, which, name):
    """add's backward runs between: its grad_for_write flushes the pending term first (first writer), then adds"""
    assert rec.accs_of(E, got.T.x) == [(0, False), (0, False)]    # add's call (seen before the flush), then the flush inside
    last = rec.dgrads()[-1]
    assert (last.epi, last.accum) == (E.EPI_NONE, 1), last


def w_ride_leftover(E, rec, got, which, name):
    assert rec.accs_of(E, got.T.x) == [(0, which == "real")]
    assert all(E._key(got.T.x) not in l.xs for l in rec.dgrads())


def w_ride_twice(E, rec, got, which, name):
    """the second defer flushes the first (y2's identity term, the first to unwind), the end of backward the second"""
    assert rec.accs_of(E, got.T.x) == [(0, False), (1, which == "real")]


def w_ride_slice(E, rec, got, which, name):
    """members share x: private buffers, no ride; the GELU term goes into the non-contiguous bound slice through a
    contiguous temporary (engine.accumulate), not an assertion"""
    x = got.T.X[:, 4:20]
    (dg,) = [l for l in rec.dgrads() if l.n == 2]
    assert dg.accum == 0 and dg.epi == (E.EPI_MUL_DGELU if which == "real" else E.EPI_NONE)
    assert E._key(got.tape.grads[E._key(x)]) not in dg.ys
    # member 0's add is seen first; its grad_for_write flushes the pending term before it lands; then member 1's
    assert rec.accs_of(E, x) == [(1, False), (1, which == "real"), (1, False)]


def w_fanout(E, rec, got, which, name):
    """first writer overwrites, later writers accumulate, in unwinding order; pre-bound: everybody accumulates"""
    pre = name.endswith("prebound")
    assert rec.accs_of(E, got.T.x) == [(1 if pre else 0, False)]
    assert [l.accum for l in rec.dgrads()] == [1, 1, 1, 1]
    assert [l.epi for l in rec.dgrads()] == [E.EPI_NONE] * 4


def w_group_shared(E, rec, got, which, name):
    """shared inputs: one dgrad launch of 4 members into private buffers, then four adds in member order"""
    (dg,) = rec.dgrads()
    own = {E._key(v) for v in got.tape.grads.values()}
    assert dg.n == 4 and dg.accum == 0 and not dg.single and not (set(dg.ys) & own)
    order = [k for k, _ in rec.accs if k in (E._key(got.T.x0), E._key(got.T.x1))]
    assert order == [E._key(got.T.x0)] * 2 + [E._key(got.T.x1)] * 2
    assert [a for _, a in rec.accs if not a[1]][-4:] == [(0, False), (1, False), (0, False), (1, False)]


def w_group_mixed(E, rec, got, which, name):
    """x1 has a gradient already: the others are zeroed and the one launch accumulates in place"""
    dg = rec.dgrads()[-1]
    want = [E._key(got.tape.grads[E._key(got.T["x%d" % i])]) for i in range(3)]
    assert dg.n == 3 and dg.accum == 1 and dg.ys == want


def w_group_partial(E, rec, got, which, name):
    (dg,) = rec.dgrads()
    if name == "group_all_wanted":
        assert dg.accum == 0 and rec.accs == []
    else:
        assert [k for k, _ in rec.accs] == [E._key(got.T.x0), E._key(got.T.x2)]


def w_bias(E, rec, got, which, name):
    """forward conv with the weight wanted: dbias rides on the wgrad; transposed, weight stopped, no bias: it does not"""
    members = [m for grp in rec.wgroups for m in grp]
    if name == "bias_paths":
        assert len(members) == 4 and sum(1 for m in members if m[1]) == 2
    else:
        assert len(members) == 1 and members[0][1]


def w_shared(E, rec, got, which, name):
    """S1: no grouped weight-gradient launch has two members on one dw or on one dbias; on one buffer the overwrite is
    issued before the add"""
    seen = {}
    for grp in rec.wgroups:
        dws = [m[0] for m in grp]
        dbs = [m[1] for m in grp if m[1]]
        assert len(set(dws)) == len(dws) and len(set(dbs)) == len(dbs), "two members of one launch share a buffer"
        for dw, db, acc, accb in grp:
            assert acc == (1 if dw in seen else 0), "the overwriting problem must be issued first"
            seen[dw] = True


def w_gdn(E, rec, got, which, name):
    """the GDN input has a gradient from the add already: the EPI_AXPY2 dgrad accumulates"""
    (dg,) = [l for l in rec.launches if l.tag == "dgrad(gdn)"]
    assert (dg.epi, dg.accum) == (E.EPI_AXPY2, 1)


def w_swin(E, rec, got, which, name):
    """DropPath: the shortcut terms of both residual_scale calls ride on the LayerNorm backward (no accumulate at all)"""
    if name == "swin_droppath":
        assert rec.accs == []


def w_many(E, rec, got, which, name):
    assert sorted(len(grp) for grp in rec.wgroups) == [1, 32]


WITNESS = {"ride": w_ride, "ride_gelu": w_ride, "ride_mismatch_gelu_first": w_ride_mismatch,
           "ride_mismatch_gelu_res": w_ride_mismatch, "ride_preempted": w_ride_preempted, "ride_leftover": w_ride_leftover,
           "ride_twice": w_ride_twice, "ride_slice": w_ride_slice, "fanout": w_fanout, "fanout_prebound": w_fanout,
           "group_shared": w_group_shared, "group_mixed_accum": w_group_mixed, "group_all_wanted": w_group_partial,
           "group_partial_want": w_group_partial, "bias_paths": w_bias, "bias_lrp": w_bias, "shared_weight_same": w_shared,
           "shared_weight_chain": w_shared, "shared_weight_sizes": w_shared, "shared_weight_thin": w_shared,
           "swin_droppath": w_swin, "many33": w_many}
for _n in R.GRAPHS:
    if _n.startswith("gdn_chain"):
        WITNESS[_n] = w_gdn

CASES = [(n, w) for n, g in R.GRAPHS.items() for w in R.whiches(g) if not n.startswith("group_missing")]


@pytest.mark.parametrize("name,which", CASES, ids=["%s-%s" % c for c in CASES])
def test_graph(E, monkeypatch, name, which):
    """forward values and every gradient against the mirror, inputs untouched, no gradient where none may exist, nothing
    pending afterwards, and the branch the graph is named for was the one taken.
    ride_slice states S4's outcome: the gradient is computed (through a contiguous temporary), nothing is refused."""
    rec = record(monkeypatch, E)
    got = run(E, name, which)
    WITNESS.get(name, _no_witness)(E, rec, got, which, name)      # (first: a wrong path is the clearer message)
    compare(name, which, got)


def test_group_partial_want_leaves_the_others_unchanged(E):
    """one member's input is stopped: every other result is bit for bit that of the all-wanted run (grid)"""
    a, b = run(E, "group_all_wanted", "grid"), run(E, "group_partial_want", "grid")
    assert b.grads["x1"] is None
    for k, v in a.outs.items():
        assert bits_equal(v, b.outs[k]), k
    for k, v in a.grads.items():
        assert k == "x1" or bits_equal(v, b.grads[k]), k


def test_group_missing_gradients(E, monkeypatch):
    """a member without a gradient: RuntimeError.  No member with one: backward returns, no gradient exists and neither
    a dgrad nor a weight-gradient launch was made"""
    got = run(E, "group_missing_one", "grid", backward=False)
    compare("group_missing_one", "grid", got, values_only=True)
    g = R.GRAPHS["group_missing_one"]
    d = dev()
    T = R.NS((k, v.to(d)) for k, v in R.make_inputs(g, "grid").items())
    tape = E.Tape()
    outs = g.build(tape, T, R.opts(E, "grid"))
    for k, u in R.upstream(g, "grid", {k: outs[k].shape for k in g.outs}).items():
        tape.bind_grad(outs[k], u.to(d), True)
    with pytest.raises(RuntimeError, match="every member needs a gradient"):
        tape.backward()
    rec = record(monkeypatch, E)
    got = run(E, "group_missing_all", "grid")
    compare("group_missing_all", "grid", got)
    assert all(v is None for v in got.grads.values())
    assert rec.dgrads() == [] and rec.wgroups == [] and rec.accs == []


# ================================================================================================ chain variants
@pytest.mark.parametrize("which", ["grid", "real"])
@pytest.mark.parametrize("wino,pre", [(False, True), (True, True), (True, False)], ids=["direct", "wino-pre", "wino-nopre"])
@pytest.mark.parametrize("mat", [True, False], ids=["mat", "nomat"])
@pytest.mark.parametrize("act_out", [True, False], ids=["actout", "noactout"])
def test_chain_variants(E, monkeypatch, which, wino, pre, mat, act_out):
    """virtual GELU between the layers read from the materialised tensor (act_out and _MATERIALIZE) or evaluated by the
    consumer, on the direct kernels and on Winograd with the input transform as its own launch or in the kernel"""
    monkeypatch.setattr(E, "_MATERIALIZE", mat)
    monkeypatch.setattr(E, "USE_WINO", wino)
    monkeypatch.setattr(E, "WINO_PRE", pre)
    monkeypatch.setattr(E, "_WINO_MIN_WORK", 0.0)
    monkeypatch.setattr(E, "_WINO_MIN_CIN", 16)
    rec = record(monkeypatch, E)
    got = run(E, "chain", which, act_out=act_out)
    tag = "[%s,%s,%s]" % ("wino" + ("" if pre else "-nopre") if wino else "direct", "mat" if mat else "nomat",
                          "actout" if act_out else "noactout")
    compare("chain", which, got, tag=tag)
    fwd = [l for l in rec.launches if l.tag == "fwd"]
    assert [l.algo for l in fwd] == [0, 1 if wino else 0, 0]              # c1 has 8 input channels, c3 is 1x1
    assert [l.algo for l in rec.dgrads()] == [0, 1 if wino else 0, 1 if wino else 0]
    if which == "real":
        read_mat = mat and act_out
        assert [l.pro_act for l in fwd] == [E.ACT_NONE] + [E.ACT_NONE if read_mat else E.ACT_GELU] * 2
        assert (len(got.tape.mat) == 2) == read_mat
        assert [l.epi for l in rec.dgrads()] == [E.EPI_MUL_DGELU, E.EPI_MUL_DGELU, E.EPI_NONE]


# ================================================================================================ scheduling invariance
def _hold_first_half(tape):
    tape.hold_wgrads = True
    tape.bw.insert(len(tape.bw) // 2, lambda: setattr(tape, "hold_wgrads", False))     # unwinding runs from the end


@pytest.mark.parametrize("name", ["chain", "fanout", "group_shared", "shared_weight_sizes", "many33"])
def test_scheduling_invariance(E, monkeypatch, name):
    """flush timing, held flushes and the side stream change when and where weight gradients are issued, never a bit"""
    plain = run(E, name, "grid")
    compare(name, "grid", plain)

    def eager(tape):
        tape.progress_every, tape.min_jobs = 1, 1

    def side(tape):
        eager(tape)
        tape.side = torch.cuda.Stream()

    rec = record(monkeypatch, E)
    for tag, setup, mid in (("eager", eager, None), ("held", eager, _hold_first_half), ("side", side, None),
                            ("side-held", side, _hold_first_half)):
        n0 = rec.flushes
        got = run(E, name, "grid", setup=setup, mid=mid)
        assert rec.flushes - n0 > 1, tag
        for k, v in plain.outs.items():
            assert bits_equal(v, got.outs[k]), (tag, k)
        for k, v in plain.grads.items():
            assert bits_equal(v, got.grads[k]), (tag, k)


@pytest.mark.parametrize("name", ["ride_gelu", "group_shared", "swin"])
def test_repeatability(E, name):
    a, b = run(E, name, "real"), run(E, name, "real")
    for k, v in a.outs.items():
        assert bits_equal(v, b.outs[k]), k
    for k, v in a.grads.items():
        assert bits_equal(v, b.grads[k]), k


@pytest.mark.parametrize("pair", [True, False], ids=["paired", "unpaired"])
def test_gate_branch_pairing(E, monkeypatch, pair):
    monkeypatch.setattr(E, "PAIR_GATE_BRANCHES", pair)
    rec = record(monkeypatch, E)
    got = run(E, "gate", "real")
    compare("gate", "real", got, tag="[paired]" if pair else "[unpaired]")
    assert any(not l.single for l in rec.launches) == pair


# ================================================================================================ inference
GELU_SLOPE = 1.13      # sup |gelu'| = 1.1289...


@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "separate"])
@pytest.mark.parametrize("name,which", [("chain", "grid"), ("chain", "real"), ("ride", "grid"), ("ride", "real"),
                                        ("ride_gelu", "real")])
def test_inference_values(E, monkeypatch, name, which, inplace):
    """need_grad=False: only values.  A layer called with act_out may hold gelu(y) in place of y (tape.mat[y] is y): the
    residual unit's output does; its limit is the pre-activation's through sup |gelu'| plus gelu's own floor.  (grid
    runs pass act_out=False: act_out promises GELU consumers, which the exact twin does not have.)"""
    monkeypatch.setattr(E, "EVAL_INPLACE_ACT", inplace)
    g = R.GRAPHS[name]
    d = dev()
    T = R.NS((k, v.to(d)) for k, v in R.make_inputs(g, which).items())
    tape = E.Tape(need_grad=False)
    outs = g.build(tape, T, R.opts(E, which, act_out=which == "real"))
    torch.cuda.synchronize()
    assert tape.bw == [] and tape.grads == {}
    ref = R.reference(name, which).outs["y"]
    y = outs["y"]
    activated = tape.mat.get(E._key(y)) is y
    assert activated == (inplace and which == "real" and name != "chain")
    if which == "grid":
        assert bits_equal(y.cpu(), ref.float())
        return
    limit = R.limits(name)["y"][0]
    if activated:
        limit = GELU_SLOPE * limit + PR.gelu_floor(ref).max().item() + R.FACTOR * R.U * ref.abs().max().item()
        ref = PR.gelu(ref)
    err = (y.cpu().double() - ref).abs().max().item()
    print(f"{name} inference {'in place' if inplace else 'separate'}: error {err:.3e} / limit {limit:.3e}")
    assert err <= limit


@pytest.mark.parametrize("need_grad", [False, True], ids=["inference", "training"])
@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "separate"])
def test_stale_materialised_activation(E, monkeypatch, inplace, need_grad):
    """S3: a layer materialises gelu(y); a second layer then overwrites y (out=y, act_out=False).  A VT(y, GELU) consumer
    must read gelu of the NEW y: the producer that does not materialise drops tape.mat's entry for its output.
    (values only; limit: FACTOR * float32's own error + roundoff + gelu_floor of the operand through |w|)"""
    monkeypatch.setattr(E, "EVAL_INPLACE_ACT", inplace)
    d = dev()
    x1, x2 = (R._input("eg.stale.x%d" % i, (2, 8, 8, 8), "x", "real") for i in (1, 2))
    w = [R._input("eg.stale.w%d" % i, (8, 8, 3, 3), "w", "real") for i in range(3)]
    b = [R._input("eg.stale.b%d" % i, (8,), "b", "real") for i in range(3)]
    wd, bd, xd = [t.to(d) for t in w], [t.to(d) for t in b], [x1.to(d), x2.to(d)]   # (kept alive: packed copies go by address)
    tape = E.Tape(need_grad=need_grad)
    y = E.conv2d(tape, E.VT(xd[0]), wd[0], bd[0], pad=1, act_out=True)
    assert E._key(y) in tape.mat
    y_again = E.conv2d(tape, E.VT(xd[1]), wd[1], bd[1], pad=1, out=y, act_out=False)
    assert y_again is y and E._key(y) not in tape.mat
    z = E.conv2d(tape, E.VT(y, E.ACT_GELU), wd[2], bd[2], pad=1)
    torch.cuda.synchronize()

    def ref(dt):
        y2 = F.conv2d(x2.to(dt), w[1].to(dt), b[1].to(dt), padding=1)
        return y2, F.conv2d(PR.gelu(y2) if dt == R.F64 else F.gelu(y2), w[2].to(dt), b[2].to(dt), padding=1)
    y64, z64 = ref(R.F64)
    z32 = ref(R.F32)[1]
    floor = F.conv2d(PR.gelu_floor(y64), w[2].double().abs(), padding=1).max().item()
    limit = R.FACTOR * (z32.double() - z64).abs().max().item() + R.FACTOR * R.U * z64.abs().max().item() + floor
    err = (z.cpu().double() - z64).abs().max().item()
    print(f"stale activation: error {err:.3e} / limit {limit:.3e}")
    assert err <= limit


# ================================================================================================ autograd bridge
def test_autograd_bridge(E):
    """tape_function over `chain` (grid): inputs without requires_grad are stopped and get None, an unused second output
    arrives without a gradient of its own, the upstream gradient is a non-contiguous slice; the returned gradients are
    those of the direct tape with the same tensors stopped, bit for bit"""
    g = R.GRAPHS["chain"]
    d = dev()
    names = R.leaves(g)
    frozen = {"c1.w", "c2.b", "c3.w"}
    base = R.make_inputs(g, "grid")
    o = R.opts(E, "grid")

    # the direct tape
    T = R.NS((k, v.to(d)) for k, v in base.items())
    tape = E.Tape()
    for k in frozen:
        tape.stop(T[k])
    y = g.build(tape, T, o)["y"]
    up = R.upstream(g, "grid", {"y": y.shape})["y"].to(d)
    tape.bind_grad(y, up.clone(), True)
    tape.backward()
    direct = {k: tape.grad_of(T[k]) for k in names}
    assert all((direct[k] is None) == (k in frozen) for k in names)

    # through autograd
    ts = [base[k].to(d).requires_grad_(k not in frozen) for k in names]

    def runner(tp, *tensors):
        Tn = R.NS(zip(names, tensors))
        return g.build(tp, Tn, o)["y"], E.add(tp, Tn.x, Tn.x)
    y2, unused = E.tape_function(runner, ts)
    wide = torch.zeros((2, 40, 8, 8), device=d)
    wide[:, 8:32] = up
    gout = wide[:, 8:32]
    assert not gout.is_contiguous()
    y2.backward(gout)
    torch.cuda.synchronize()
    assert bits_equal(y2.detach(), y)
    for k, t in zip(names, ts):
        if k in frozen:
            assert t.grad is None, k
        else:
            assert bits_equal(t.grad, direct[k]), k
    # and against the mirror: the stopped tensors change nobody else's gradient
    ref = R.reference("chain", "grid")
    for k in names:
        if k not in frozen:
            assert bits_equal(direct[k].cpu(), ref.grads[k].float()), k
