"""Rate-distortion optimised quantisation (csrc/qstep.hip: icm_gc_code_rdo) restated in numpy float32, operation by
operation, on top of tests/_qstep_ref.py's symbols / indexes / dequantize.  numpy rounds every float32 operation once
and never contracts two of them, and the decision uses no transcendental function (the code lengths come from a table
built in float64 on the host), so this is what the kernel must give bit for bit.  Also here: the code-length table,
the synthetic coder tables and the input sets that the GPU tests run and the CPU tests check the regimes of.

Per element, with (step, inv) the scalar pair, the pair of the element's map position, or (1, 1):
    u = (y - mu) * inv;  s0 = symbol;  idx = index;  s1 = s0 - sign(s0)
    off = offsets[idx];  ov = sizes[idx] - 2;  v_j = s_j - off
    keep s0 if s0 == 0, or a v_j lies outside 0 .. ov - 1, or not J1 < J0, where
    e_j = u - (float)s_j;  J_j = (w * (e_j * e_j)) + bits[idx][v_j]
    y_hat = dequantize(symbol coded);  idx is unchanged"""
import numpy as np

import _qmap_ref as R
import _qstep_ref as Q

F = np.float32


def code_length_table(cdf, sizes):
    """float32 [rows, stride]: f32(16 - log2(f64(cdf[r][v + 1] - cdf[r][v]))) for v < sizes[r] - 2, 0 elsewhere"""
    cdf = np.asarray(cdf, dtype=np.int64)
    bits = np.zeros(cdf.shape, dtype=F)
    for r, size in enumerate(np.asarray(sizes).reshape(-1).tolist()):
        for v in range(size - 2):
            bits[r, v] = F(16.0 - np.log2(np.float64(cdf[r, v + 1] - cdf[r, v])))
    return bits


def decide(y, mu, scale, table, bound, step, inv, sizes, offsets, bits, w):
    """every intermediate of the decision, as arrays of y's shape [N, C, HW]; ``step`` / ``inv`` are float32 scalars or
    [HW] arrays (a quality map's pairs), ``w`` the float32 weight"""
    y, mu = np.asarray(y), np.asarray(mu)
    assert y.dtype == np.float32 and mu.dtype == np.float32 and np.asarray(bits).dtype == np.float32
    stepb, invb = np.broadcast_to(np.asarray(step, dtype=F), y.shape), np.broadcast_to(np.asarray(inv, dtype=F), y.shape)
    w = F(w)
    with np.errstate(over="ignore", invalid="ignore"):
        u = (y - mu) * invb
        s0 = Q.symbols(y, mu, invb)
        idx = Q.indexes(scale, table, bound, invb)
        s1 = s0 - np.sign(s0)
        off = np.asarray(offsets, dtype=np.int64)[idx]
        ov = np.asarray(sizes, dtype=np.int64)[idx] - 2
        v0, v1 = s0.astype(np.int64) - off, s1.astype(np.int64) - off
        in0, in1 = (v0 >= 0) & (v0 < ov), (v1 >= 0) & (v1 < ov)
        cand = (s0 != 0) & in0 & in1
        e0, e1 = u - s0.astype(F), u - s1.astype(F)
        b0 = np.asarray(bits)[idx, np.where(cand, v0, 0)]
        b1 = np.asarray(bits)[idx, np.where(cand, v1, 0)]
        j0 = w * (e0 * e0) + b0
        j1 = w * (e1 * e1) + b1
        assert u.dtype == e0.dtype == j0.dtype == j1.dtype == np.float32
        change = cand & (j1 < j0)
    sym = np.where(change, s1, s0).astype(np.int32)
    return dict(u=u, s0=s0, s1=s1, idx=idx, v0=v0, v1=v1, ov=ov, cand=cand, j0=j0, j1=j1, change=change, sym=sym,
                yh=Q.dequantize(sym, mu, stepb), in0=in0, in1=in1)


def code(y, mu, scale, table, bound, step, inv, sizes, offsets, bits, w):
    """the kernel's three outputs: (symbols, indexes, y_hat)"""
    d = decide(y, mu, scale, table, bound, step, inv, sizes, offsets, bits, w)
    return d["sym"], d["idx"], d["yh"]


def branches(d):
    """how many elements took each way through the decision"""
    s0, cand = d["s0"], d["cand"]
    return {
        "zero": int((s0 == 0).sum()),
        "below": int(((s0 != 0) & (d["v0"] < 0)).sum()),                 # s0 under the table: escaped, kept
        "above": int(((s0 != 0) & (d["v0"] >= d["ov"])).sum()),          # s0 over the table proper: escaped, kept
        "s1_outside": int(((s0 != 0) & d["in0"] & ~d["in1"]).sum()),     # s0 coded in the table, its neighbour not
        "change": int(d["change"].sum()),
        "change_pos": int((d["change"] & (s0 > 0)).sum()),
        "change_neg": int((d["change"] & (s0 < 0)).sum()),
        "keep": int((cand & (d["j1"] > d["j0"])).sum()),
        "keep_pos": int((cand & (d["j1"] > d["j0"]) & (s0 > 0)).sum()),
        "keep_neg": int((cand & (d["j1"] > d["j0"]) & (s0 < 0)).sum()),
        "tie": int((cand & (d["j1"] == d["j0"])).sum()),
        "v0_first": int((cand & (d["v0"] == 0)).sum()),
        "v0_last": int((cand & (d["v0"] == d["ov"] - 1)).sum()),
        "elements": int(s0.size),
    }


# ------------------------------------------------------------------------------------------------ synthetic tables
# four rows of unequal sizes and offsets, the last offset positive; widths out of 2^16, powers of two in the first
# and last row so that their code lengths are whole bits, two equal tail widths in row 2 (equal code lengths: a tie
# at any weight small enough), and the escape bin takes what is left
SYN_WIDTHS = [[8192, 32768, 8192],
              [1024, 4096, 8192, 32768, 8192, 4096, 1024],
              [64, 64, 1024, 2048, 8192, 32768, 8192, 2048, 1024, 64, 64],
              [32768, 16384, 8192, 4096, 2048]]
SYN_OFFSETS = [-1, -3, -5, 1]
SYN_SCALES = [0.5, 1.0, 2.0, 4.0]
SYN_BOUND = 0.25


def synthetic_tables():
    """(cdf int32 [4, 13], sizes int32 [4], offsets int32 [4], scale table float32 [4], scale bound)"""
    stride = max(len(w) for w in SYN_WIDTHS) + 2
    cdf = np.zeros((len(SYN_WIDTHS), stride), dtype=np.int32)
    sizes = []
    for r, w in enumerate(SYN_WIDTHS):
        assert sum(w) < 65536
        cdf[r, 1:len(w) + 1] = np.cumsum(w)
        cdf[r, len(w) + 1] = 65536
        sizes.append(len(w) + 2)
    return cdf, np.array(sizes, dtype=np.int32), np.array(SYN_OFFSETS, dtype=np.int32), np.array(SYN_SCALES, dtype=F), \
        SYN_BOUND


_ORACLE_TABLES = []


def oracle_model_tables():
    """the 64 rows of the models' GaussianConditional as the CPU oracle builds them (the device builds the models' own
    from f32 pmfs of its own: the same shapes and, to the last unit of a width, the same tables): (cdf, sizes, offsets,
    scale table, scale bound)"""
    if not _ORACLE_TABLES:
        from icm_amd.ans import pmf_to_quantized_cdf          # the host's, which the models' update() calls too
        from oracle import wacnn_oracle as O
        table = O.scale_table()
        offset, pmf, tail, length, max_length = O.gc_update_tables(table)
        cdf = np.zeros((len(table), max_length + 2), dtype=np.int32)
        for r, n in enumerate(length.tolist()):
            q = pmf_to_quantized_cdf(pmf[r, :n].tolist() + tail[r, :1].tolist())
            cdf[r, :len(q)] = q
        _ORACLE_TABLES.append((cdf, (length + 2).numpy().astype(np.int32), offset.numpy().astype(np.int32),
                               table.numpy().astype(F), O.SCALE_BOUND))
    return _ORACLE_TABLES[0]


# ------------------------------------------------------------------------------------------------ the forms
SCALAR_KS = [-16, 0, 12]
MAP_KS = [-16, -3, 0, 5, 8, 12]


def form_steps(form, HW):
    """(step, inv, qmap) of a form: float32 scalars with qmap None for "k<K>", [HW] arrays with the int8 map for
    "busy" (the byte changes at every position) and "uniform" (every byte 5: the scalar call at k = 5)"""
    if form.startswith("k"):
        step, inv = Q.step_of(int(form[1:]))
        return step, inv, None
    i = np.arange(HW)
    qmap = np.array(MAP_KS, dtype=np.int8)[(i + 2 * (i // 6)) % len(MAP_KS)] if form == "busy" else np.full(HW, 5, np.int8)
    if form == "busy" and HW > 1:
        assert bool((qmap[1:] != qmap[:-1]).all())
    step, inv = R.steps_of_map(qmap)
    return step, inv, qmap


FORMS = ["k-16", "k0", "k12", "busy", "uniform"]
WEIGHTS = [1e-30, 0.25, 4.0, 1e30]
SHAPES = [(2, 3, 1), (2, 3, 63), (2, 3, 257), (2, 40, 257)]      # one lane; a ragged wave; a second block; the c loop


# ------------------------------------------------------------------------------------------------ the input sets
def inputs(name, shape, step, inv, table, bound, sizes, offsets, seed=0):
    """(y, mu, scale) float32 [N, C, HW] of an input set, built for the coder tables it is coded with: every element
    draws a table row (its scale sits just under the row's entry times the position's step, or at the bound) and a
    symbol relative to that row's range, then a fraction of a step.

      edges  symbols spread over the row's whole range and up to 3 beyond it at both ends, every 7th element exactly
             on a symbol, every 11th on a half (a tie of the rounding; of the squared errors too when s1 follows), a
             few huge ones; the first 8 elements are fixed cases so that the smallest shapes hold a zero, a change
             candidate of either sign and an escape
      mixed  symbols drawn like a Gaussian of 1.5 x the row's own scale, the rows those of scale 0.2 .. 30: under a
             narrow row the neighbour toward zero is much cheaper and RDOQ moves, under a wide one it is not and RDOQ
             stays.  The regime the tests hold it to (a fifth of the elements changed, a fifth non-zero and unchanged)
             is that of the models' 64-row tables at w = 0.25"""
    N, C, HW = shape
    n = N * C * HW
    rng = np.random.default_rng(97 * seed + 13 * len(name) + n % 1009 + len(sizes))
    stepf = np.broadcast_to(np.asarray(step, dtype=F), shape).reshape(-1).astype(np.float64)
    ns = len(table)
    off = np.asarray(offsets, dtype=np.int64)
    ov = np.asarray(sizes, dtype=np.int64) - 2
    if name == "edges":
        row = rng.integers(0, ns, n)
        sym = off[row] - 3 + rng.integers(0, ov[row] + 6)
        frac = rng.uniform(-0.5, 0.5, n)
        k = np.arange(n)
        frac[k % 7 == 3] = 0.0
        frac[k % 11 == 5] = 0.5
        head = [(0, 0.2), (1, 0.45), (-1, -0.45), (2, -0.4), (-2, 0.4), (10 ** 4, 0.1), (-10 ** 4, 0.1), (1, -0.5)]
        for i, (s, f) in enumerate(head[:n]):
            sym[i], frac[i] = s, f
        if n > 40:
            sym[20:24] = [3 * 10 ** 8, -3 * 10 ** 8, 2 ** 31, -2 ** 31]           # the last two clamp at +-2^30
    elif name == "mixed":
        tab = np.asarray(table, dtype=np.float64)
        rows = np.flatnonzero((tab >= 0.2) & (tab <= 30.0))
        row = rows[rng.integers(0, len(rows), n)]
        sym = np.rint(rng.standard_normal(n) * tab[row] * 1.5).astype(np.int64)
        frac = rng.uniform(-0.5, 0.5, n)
    else:
        raise AssertionError(name)
    mu = (np.rint(rng.uniform(-3, 3, n) * 64) / 64).astype(F)
    t = ((sym + frac) * stepf).astype(F)
    y = (mu + t).astype(F)
    scale = (np.asarray(table, dtype=np.float64)[row] * stepf * 0.97).astype(F)
    scale[np.arange(n) % 13 == 7] = F(bound) / F(2)                               # under the bound: the bound's row
    return y.reshape(shape), mu.reshape(shape), scale.reshape(shape)
