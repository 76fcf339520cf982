"""The arithmetic of the quantiser step (csrc/qstep.hip) in numpy float32, operation by operation.  numpy rounds every
float32 operation once and never contracts two of them, so this is an exact restatement of what the kernels must give,
bit for bit; it also holds the host function that turns the step index k into the two floats."""
import numpy as np

F = np.float32
QSTEP_MIN, QSTEP_MAX = -16, 32
SYMBOL_MAX = F(2.0 ** 30)


def step_of(k):
    """(step, inv) as float32: step = f32(2^(k/8)), inv = f32(1 / f64(step))"""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not QSTEP_MIN <= k <= QSTEP_MAX:
        raise ValueError(f"qstep {k!r} outside [{QSTEP_MIN}, {QSTEP_MAX}]")
    step = F(2.0 ** (int(k) / 8))
    return step, F(1.0 / np.float64(step))


def _f32(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    return a


def symbols(y, mu, inv):
    t = _f32(y) - _f32(mu)
    u = t * F(inv)
    s = np.rint(u)                                   # half to even
    s = np.minimum(np.maximum(s, -SYMBOL_MAX), SYMBOL_MAX)
    assert s.dtype == np.float32
    return s.astype(np.int32)


def dequantize(sym, mu, step):
    """y_hat from the integer symbol, as the decoder must form it: a multiply, then an add, two roundings"""
    p = np.asarray(sym, dtype=np.int32).astype(np.float32) * F(step)
    out = p + _f32(mu)
    assert out.dtype == np.float32
    return out


def indexes(scale, table, bound, inv):
    table = _f32(table)
    ns = table.shape[0]
    se = np.maximum(_f32(scale), F(bound)) * F(inv)
    assert se.dtype == np.float32
    count = np.zeros(se.shape, dtype=np.int32)
    for j in range(ns - 1):
        count += (se <= table[j]).astype(np.int32)
    return (ns - 1) - count


def code(y, mu, scale, table, bound, step, inv):
    """the encoder's fused kernel: (symbols, indexes, y_hat)"""
    sym = symbols(y, mu, inv)
    return sym, indexes(scale, table, bound, inv), dequantize(sym, mu, step)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)
