"""GPU: icm_gc_code_rdo (csrc/qstep.hip) through the C ABI against the float32 restatement (tests/_rdoq_ref.py), bit for
bit in symbols, indexes and y_hat: the scalar pair at three steps, a map whose byte changes at every position and a
uniform map (which must also equal the scalar call), on the synthetic four-row tables and on the model's own 64 rows,
at the four weights.  At w = 1e30 the outputs are those of icm_gc_code_q / icm_gc_code_qmap.  Every float operand is a
channel slice of its own wider NaN-filled buffer and every output sits between guard bands; every refusal returns
ICM_ERR_ARG and leaves the outputs alone."""
import numpy as np
import pytest
import torch

import _qstep_ref as Q
import _rdoq_ref as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
SENT_F, SENT_I, GUARD = -777.25, -7, 96
ERR_ARG = 1


def _lib():
    from icm_amd import _lib as L
    return L


class Wide:
    """a [N, C, HW] operand that is a channel slice of a wider buffer (batch stride != C * HW) filled with ``fill``"""

    def __init__(self, shape, before, after, data=None, fill=float("nan")):
        N, C, HW = shape
        self.buf = torch.full((N, before + C + after, HW), fill, dtype=torch.float32, device=DEV)
        self.view = self.buf[:, before:before + C]
        self.before, self.C, self.fill = before, C, fill
        if data is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data)).reshape(shape).to(DEV))
        self.ptr, self.bs = self.view.data_ptr(), self.buf.stride(0)
        assert self.bs != C * HW

    def numpy(self):
        return self.view.cpu().contiguous().numpy()

    def outside_untouched(self):
        b = self.buf.cpu()
        out = torch.cat([b[:, :self.before].reshape(-1), b[:, self.before + self.C:].reshape(-1)])
        return bool(torch.isnan(out).all()) if self.fill != self.fill else bool((out == self.fill).all())


class Guarded:
    """a dense int32 [N, C, HW] output between two guard bands"""

    def __init__(self, shape):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), SENT_I, dtype=torch.int32, device=DEV)
        self.ptr, self.shape = self.buf.data_ptr() + 4 * GUARD, shape

    def numpy(self):
        return self.buf[GUARD:GUARD + self.n].cpu().numpy().reshape(self.shape)

    def guards_untouched(self):
        b = self.buf.cpu()
        return bool((b[:GUARD] == SENT_I).all() and (b[GUARD + self.n:] == SENT_I).all())

    def untouched(self):
        return bool((self.buf == SENT_I).all())


class Tables:
    """coder tables on the device, as ``_device_tables()`` gives them, with the restatement's code lengths"""

    def __init__(self, cdf, sizes, offsets, table, bound):
        self.host = (np.ascontiguousarray(cdf, dtype=np.int32), np.ascontiguousarray(sizes, dtype=np.int32),
                     np.ascontiguousarray(offsets, dtype=np.int32), np.ascontiguousarray(table, dtype=F), float(bound))
        self.bits = D.code_length_table(cdf, sizes)
        self.cdf, self.sizes, self.offsets, self.table, self.bits_d = (
            torch.from_numpy(a).to(DEV) for a in (*self.host[:4], self.bits))
        self.stride, self.rows = int(cdf.shape[1]), int(cdf.shape[0])


@pytest.fixture(scope="module")
def tables():
    from icm_amd.zoo import models
    m = models["cnn"]().to(DEV).eval()
    m.update(force=True)
    gc = m.gaussian_conditional
    cdf, sizes, offsets = (t.cpu().numpy() for t in gc._device_tables())
    out = {"synthetic": Tables(*D.synthetic_tables()),
           "model": Tables(cdf, sizes, offsets, gc.scale_table.detach().cpu().numpy(), gc._scale_bound)}
    assert out["model"].rows == 64 and out["synthetic"].rows == 4
    out["gc"] = gc
    return out


_STEP_TABLE = []


def _step_table_dev():
    from icm_amd import bitstream as B
    if not _STEP_TABLE:
        _STEP_TABLE.append(torch.from_numpy(B.step_table()).to(DEV))
    return _STEP_TABLE[0]


def run_rdo(T, shape, y, mu, scale, step, inv, qmap, w):
    """one launch on fresh wide inputs and guarded outputs -> (rc, sym, idx, yh, inputs)"""
    L = _lib()
    N, C, HW = shape
    ys, ms, ss = Wide(shape, 2, 1, y), Wide(shape, 0, 3, mu), Wide(shape, 1, 1, scale)
    yh = Wide(shape, 3, 2, fill=SENT_F)
    sym, idx = Guarded(shape), Guarded(shape)
    if qmap is None:
        pair, qd, qp, sp = (float(step), float(inv)), None, 0, 0
    else:
        qd = torch.from_numpy(np.ascontiguousarray(qmap, dtype=np.int8)).to(DEV)
        pair, qp, sp = (1.0, 1.0), qd.data_ptr(), _step_table_dev().data_ptr()
    rc = L.lib().icm_gc_code_rdo(ys.ptr, ys.bs, ms.ptr, ms.bs, ss.ptr, ss.bs, T.table.data_ptr(), T.rows, T.host[4],
                                 *pair, qp, sp, T.cdf.data_ptr(), T.stride, T.sizes.data_ptr(), T.offsets.data_ptr(),
                                 T.rows, T.bits_d.data_ptr(), float(w), sym.ptr, idx.ptr, yh.ptr, yh.bs, N, C, HW,
                                 L.stream())
    torch.cuda.synchronize()
    return rc, sym, idx, yh, (ys, ms, ss, qd)


def run_plain(T, shape, ins, step, inv, qmap):
    """icm_gc_code_q / icm_gc_code_qmap on the same device operands"""
    L = _lib()
    N, C, HW = shape
    ys, ms, ss, qd = ins
    yh = Wide(shape, 1, 2, fill=SENT_F)
    sym, idx = Guarded(shape), Guarded(shape)
    if qmap is None:
        rc = L.lib().icm_gc_code_q(ys.ptr, ys.bs, ms.ptr, ms.bs, ss.ptr, ss.bs, T.table.data_ptr(), T.rows, T.host[4],
                                   float(step), float(inv), sym.ptr, idx.ptr, yh.ptr, yh.bs, N, C, HW, L.stream())
    else:
        rc = L.lib().icm_gc_code_qmap(ys.ptr, ys.bs, ms.ptr, ms.bs, ss.ptr, ss.bs, T.table.data_ptr(), T.rows, T.host[4],
                                      qd.data_ptr(), _step_table_dev().data_ptr(), sym.ptr, idx.ptr, yh.ptr, yh.bs, N,
                                      C, HW, L.stream())
    torch.cuda.synchronize()
    assert rc == 0
    return sym, idx, yh


CASES = [(s, f, t, n) for s in D.SHAPES[:3] for f in D.FORMS for t in ("synthetic", "model") for n in ("edges", "mixed")]
CASES += [(D.SHAPES[3], "busy", "model", "mixed"), (D.SHAPES[3], "k0", "synthetic", "edges")]     # the channel loop wraps
assert D.SHAPES[3][1] == 40 and [s[2] for s in D.SHAPES[:3]] == [1, 63, 257]


@pytest.mark.parametrize("shape,form,kind,name", CASES,
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_kernel_equals_the_restatement_bit_for_bit(tables, shape, form, kind, name):
    T = tables[kind]
    cdf, sizes, offsets, table, bound = T.host
    step, inv, qmap = D.form_steps(form, shape[2])
    y, mu, scale = D.inputs(name, shape, step, inv, table, bound, sizes, offsets)
    changed = {}
    for w in D.WEIGHTS:
        d = D.decide(y, mu, scale, table, bound, step, inv, sizes, offsets, T.bits, w)
        rc, sym, idx, yh, ins = run_rdo(T, shape, y, mu, scale, step, inv, qmap, w)
        assert rc == 0
        assert np.array_equal(sym.numpy(), d["sym"]), (w, int((sym.numpy() != d["sym"]).sum()))
        assert np.array_equal(idx.numpy(), d["idx"])
        assert np.array_equal(Q.bits(yh.numpy()), Q.bits(d["yh"]))
        assert sym.guards_untouched() and idx.guards_untouched() and yh.outside_untouched()
        for wide, a in zip(ins[:3], (y, mu, scale)):                               # inputs are read only
            assert wide.outside_untouched() and np.array_equal(Q.bits(wide.numpy()), Q.bits(a))
        changed[w] = int(d["change"].sum())
        if w == 1e30:                                                              # the plain fused kernels' outputs
            psym, pidx, pyh = run_plain(T, shape, ins, step, inv, qmap)
            assert np.array_equal(sym.numpy(), psym.numpy()) and np.array_equal(idx.numpy(), pidx.numpy())
            assert np.array_equal(Q.bits(yh.numpy()), Q.bits(pyh.numpy()))
        if form == "uniform":                                                      # the scalar call at k = 5
            s5, i5 = Q.step_of(5)
            rc2, sym2, idx2, yh2, _ = run_rdo(T, shape, y, mu, scale, s5, i5, None, w)
            assert rc2 == 0 and np.array_equal(sym2.numpy(), sym.numpy()) and np.array_equal(idx2.numpy(), idx.numpy())
            assert np.array_equal(Q.bits(yh2.numpy()), Q.bits(yh.numpy()))
    assert changed[1e30] == 0
    if shape[2] == 257:                                                            # the weights matter
        assert changed[1e-30] >= changed[0.25] >= changed[4.0] > 0
        assert changed[1e-30] > changed[4.0]


def test_the_models_cached_code_lengths_are_the_restatements(tables):
    """GaussianConditional._code_lengths: the host function's table on the device, uploaded once, rebuilt when
    update() replaces the coder tables"""
    gc, T = tables["gc"], tables["model"]
    bits = gc._code_lengths()
    assert bits.dtype == torch.float32 and bits.is_cuda and tuple(bits.shape) == tuple(gc._quantized_cdf.shape)
    assert np.array_equal(Q.bits(bits.cpu().numpy()), Q.bits(T.bits))
    assert gc._code_lengths() is bits
    gen = gc._tab_gen
    gc.update()
    assert gc._tab_gen == gen + 1
    again = gc._code_lengths()
    assert again is not bits and torch.equal(again, bits)


def test_refusals_leave_the_outputs_alone(tables):
    L = _lib()
    T = tables["synthetic"]
    cdf, sizes, offsets, table, bound = T.host
    shape = (2, 3, 63)
    N, C, HW = shape
    step, inv, qmap = D.form_steps("busy", HW)
    y, mu, scale = D.inputs("edges", shape, step, inv, table, bound, sizes, offsets)
    ys, ms, ss = Wide(shape, 2, 1, y), Wide(shape, 0, 3, mu), Wide(shape, 1, 1, scale)
    yh = Wide(shape, 3, 2, fill=SENT_F)
    sym, idx = Guarded(shape), Guarded(shape)
    qd = torch.from_numpy(qmap).to(DEV)
    sd = _step_table_dev()
    good = dict(y=ys.ptr, y_bs=ys.bs, mu=ms.ptr, mu_bs=ms.bs, sc=ss.ptr, sc_bs=ss.bs, table=T.table.data_ptr(), ns=4,
                bound=bound, step=1.0, inv=1.0, qmap=qd.data_ptr(), steps=sd.data_ptr(), cdfs=T.cdf.data_ptr(),
                stride=T.stride, sizes=T.sizes.data_ptr(), offsets=T.offsets.data_ptr(), ncdf=4,
                bits=T.bits_d.data_ptr(), w=0.25, sym=sym.ptr, idx=idx.ptr, yh=yh.ptr, yh_bs=yh.bs, N=N, C=C, HW=HW)

    def call(**kw):
        a = {**good, **kw}
        return L.lib().icm_gc_code_rdo(a["y"], a["y_bs"], a["mu"], a["mu_bs"], a["sc"], a["sc_bs"], a["table"], a["ns"],
                                       a["bound"], a["step"], a["inv"], a["qmap"], a["steps"], a["cdfs"], a["stride"],
                                       a["sizes"], a["offsets"], a["ncdf"], a["bits"], a["w"], a["sym"], a["idx"],
                                       a["yh"], a["yh_bs"], a["N"], a["C"], a["HW"], L.stream())

    cases = [{name: 0} for name in ("y", "mu", "sc", "table", "cdfs", "sizes", "offsets", "bits", "sym", "idx", "yh")]
    cases += [{"qmap": 0}, {"steps": 0}]                                            # one of the two without the other
    for dim in ("N", "C", "HW"):
        cases += [{dim: 0}, {dim: -1}]
    cases += [{"ns": 5}, {"ns": 3}, {"ncdf": 5}, {"ncdf": 3}, {"ns": 0, "ncdf": 0}, {"ns": -4, "ncdf": -4}]
    cases += [{"stride": 2}, {"stride": 0}, {"stride": -13}]
    cases += [{"w": v} for v in (0.0, -1.0, -0.0, float("nan"), float("inf"), -float("inf"))]
    cases += [{"qmap": 0, "steps": 0, "step": v} for v in (0.0, -1.0, float("nan"), float("inf"))]
    cases += [{"qmap": 0, "steps": 0, "inv": v} for v in (0.0, float("nan"))]
    cases += [{"N": 65536}]                                                         # an image is a row of the grid
    for kw in cases:
        assert call(**kw) == ERR_ARG, kw
    torch.cuda.synchronize()
    assert sym.untouched() and idx.untouched() and bool((yh.buf == SENT_F).all())
    # and the good call, with both of the pair null or both set, runs
    assert call() == 0 and call(qmap=0, steps=0) == 0
    torch.cuda.synchronize()
    want = D.code(y, mu, scale, table, bound, F(1), F(1), sizes, offsets, T.bits, 0.25)
    assert np.array_equal(sym.numpy(), want[0]) and np.array_equal(idx.numpy(), want[1])
    assert np.array_equal(Q.bits(yh.numpy()), Q.bits(want[2])) and yh.outside_untouched()
    assert sym.guards_untouched() and idx.guards_untouched()
