"""Host restatement, in numpy and Python integers, of the codec's error-bounded residual layer (icm_amd/residual.py,
csrc/residual.hip, include/icm_hip.h): the quantiser, the class rule, the plane and index layout and the tables; and the
cases the GPU kernel test runs, with the path each of them is named for, so that a CPU test can check that it gets
there.  Nothing here imports the package."""
import math

import numpy as np

CELL = 16
MAX_ERROR = 32
THRESHOLDS = [int(math.floor(2.0 ** (1 + j / 2) + 0.5)) for j in range(18)]
NCLASSES = 19


# ------------------------------------------------------------------------------------------------- arithmetic
def quantise(x, xhat, d):
    """8-bit [H, W, 3] original and reconstruction -> q, int32 in plane order [3, H, W]"""
    r = np.asarray(x).astype(np.int64) - np.asarray(xhat).astype(np.int64)
    q = np.sign(r) * ((np.abs(r) + d) // (2 * d + 1))
    return np.ascontiguousarray(q.transpose(2, 0, 1)).astype(np.int32)


def reconstruct(xhat_window, q, d, window=None):
    """8-bit [h, w, 3] reconstruction of the window (y0, x0, h, w) and the image's q [3, H, W] -> 8-bit [h, w, 3]"""
    y0, x0, h, w = (0, 0) + tuple(q.shape[1:]) if window is None else window
    qq = q[:, y0:y0 + h, x0:x0 + w].astype(np.int64).transpose(1, 2, 0)
    return np.clip(np.asarray(xhat_window).astype(np.int64) + qq * (2 * d + 1), 0, 255).astype(np.uint8)


def grid(H, W):
    return -(-H // CELL), -(-W // CELL)


def cell_sums(q):
    """(N, S) per cell, int64 [gh, gw] each: the coded samples and the sum of |q| over the three planes"""
    _, H, W = q.shape
    gh, gw = grid(H, W)
    N, S = np.zeros((gh, gw), np.int64), np.zeros((gh, gw), np.int64)
    for cy in range(gh):
        for cx in range(gw):
            blk = q[:, cy * CELL:(cy + 1) * CELL, cx * CELL:(cx + 1) * CELL]
            N[cy, cx], S[cy, cx] = blk.size, int(np.abs(blk.astype(np.int64)).sum())
    return N, S


def classes(q):
    """int32 [gh, gw]: per cell the number of thresholds T_j with 16 S > N T_j"""
    N, S = cell_sums(q)
    return sum((16 * S > N * t).astype(np.int32) for t in THRESHOLDS)


def indexes(cls, H, W):
    """int32 [3, H, W]: every sample's class, the value as found"""
    cls = np.asarray(cls).reshape(grid(H, W))
    full = np.repeat(np.repeat(cls, CELL, axis=0), CELL, axis=1)[:H, :W]
    return np.ascontiguousarray(np.broadcast_to(full, (3, H, W))).astype(np.int32)


# ------------------------------------------------------------------------------------------------- tables
def class_bounds(k):
    """(lower, upper) bound of class k's mean |q|; class 0: a quarter of its upper bound, class 18: up to 1024 / 16"""
    lo = THRESHOLDS[k - 1] if k > 0 else THRESHOLDS[0] / 4
    hi = THRESHOLDS[k] if k < NCLASSES - 1 else 1024
    return lo / 16, hi / 16


def ratio(k):
    """the Q16 ratio at which E|q| = 2 r / (1 - r^2) of the two-sided geometric law is the geometric mean of the bounds"""
    lo, hi = class_bounds(k)
    e = math.sqrt(lo * hi)
    return int(math.floor((math.sqrt(1 + e * e) - 1) / e * 65536 + 0.5))


def weights(k, r=None):
    """[w(0), ..., w(L)] in Python integers"""
    r = ratio(k) if r is None else r
    w, out = 1 << 24, []
    while w > 0 and len(out) <= 255:
        out.append(w)
        w = (w * r) >> 16
    return out


def quantized_cdf(pmf, precision=16):
    """the algorithm of ``icm_pmf_to_quantized_cdf`` on float32 weights, in Python integers"""
    one = 1 << precision
    c = [0] + [int(np.round(np.float32(p) * np.float32(one))) for p in pmf]      # halves do not occur in these tables
    total, run = sum(c), 0
    for i in range(len(c)):
        run += one * c[i] // total
        c[i] = run
    n = len(pmf)
    c[n] = one
    for i in range(n):
        if c[i] != c[i + 1]:
            continue
        best, donor = None, -1
        for j in range(n):
            f = c[j + 1] - c[j]
            if f > 1 and (best is None or f < best):
                best, donor = f, j
        assert donor >= 0
        if donor < i:
            for j in range(donor + 1, i + 1):
                c[j] -= 1
        else:
            for j in range(i + 1, donor + 1):
                c[j] += 1
    return c


def tables():
    """(cdf int32 [20, stride], sizes, offsets): rows 0..18 the classes' laws with the escape bin's weight 1, row 19
    uniform over the classes"""
    rows, offsets = [], []
    for k in range(NCLASSES):
        w = weights(k)
        pmf = [np.float32(v) * np.float32(2.0 ** -24) for v in w[:0:-1] + w + [1]]
        rows.append(quantized_cdf(pmf))
        offsets.append(-(len(w) - 1))
    rows.append(quantized_cdf([np.float32(1.0)] * NCLASSES + [np.float32(2.0 ** -24)]))
    offsets.append(0)
    sizes = np.asarray([len(r) for r in rows], np.int32)
    cdf = np.zeros((len(rows), int(sizes.max())), np.int32)
    for i, r in enumerate(rows):
        cdf[i, :len(r)] = r
    return cdf, sizes, np.asarray(offsets, np.int32)


def string_layout(q, cls):
    """(symbols, indexes, run lengths) of the one string: the class map under table 19, then the three planes"""
    _, H, W = q.shape
    sym = np.concatenate([np.asarray(cls).reshape(-1), q.reshape(-1)]).astype(np.int32)
    idx = np.concatenate([np.full(cls.size, NCLASSES), indexes(cls, H, W).reshape(-1)]).astype(np.int32)
    return sym, idx, [int(cls.size), H * W, H * W, H * W]


# ------------------------------------------------------------------------------------------------- kernel cases
SHAPES = [(1, 1), (16, 16), (17, 33), (37, 53), (64, 48)]
BOUNDS = [0, 1, 3, 32]


def run_paths(H, W, byte_offset=0, elem_offset=0):
    """what the kernels' runs of four pixels of an H x W image do, given buffers whose first byte lies ``byte_offset``
    (8-bit) / whose first element lies ``elem_offset`` (int32) past a 16-byte boundary: the set of "dword" / "byte" for
    the interleaved side and of "vec" / "scalar" for the planar side, and "full" / "partial" for the cells"""
    seen = set()
    for y in range(H):
        for x0 in range(0, W, 4):
            n = min(4, W - x0)
            seen.add("dword" if n == 4 and (byte_offset + (y * W + x0) * 3) % 4 == 0 else "byte")
            for c in range(3):
                seen.add("vec" if n == 4 and (elem_offset + c * H * W + y * W + x0) % 4 == 0 else "scalar")
    gh, gw = grid(H, W)
    for cy in range(gh):
        for cx in range(gw):
            seen.add("full" if min(CELL, H - cy * CELL) == CELL and min(CELL, W - cx * CELL) == CELL else "partial")
    return seen


def random_pair(H, W, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    # half of the image close to x (small classes), half independent (large ones)
    near = np.clip(x.astype(np.int64) + rng.integers(-6, 7, size=x.shape), 0, 255).astype(np.uint8)
    far = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    return x, np.where((np.arange(W) < (W + 1) // 2)[None, :, None], near, far).astype(np.uint8)


def extreme_pair(H, W, reverse):
    a, b = np.full((H, W, 3), 255, np.uint8), np.zeros((H, W, 3), np.uint8)
    return (b, a) if reverse else (a, b)


def max_symbol(d):
    return (255 + d) // (2 * d + 1)


def _cell_with_sum(n_samples, total, d, amax):
    """x, xhat bytes of n_samples samples whose |q| add up to ``total``: magnitudes as even as integers allow, signs
    alternating (xhat = 0 below a positive difference, 255 above a negative one)"""
    base, rem = divmod(total, n_samples)
    assert base + (1 if rem else 0) <= amax, (n_samples, total, d)
    a = np.full(n_samples, base, np.int64)
    a[:rem] += 1
    r = np.minimum(a * (2 * d + 1), 255)
    neg = np.arange(n_samples) % 2 == 1
    xhat = np.where(neg, 255, 0)
    x = np.where(neg, 255 - r, r)
    return x.astype(np.uint8), xhat.astype(np.uint8)


def threshold_js(d):
    """the thresholds a cell's mean |q| can reach under the bound d"""
    return [j for j, t in enumerate(THRESHOLDS) if t + 1 <= 16 * max_symbol(d)]


def threshold_image(d):
    """An image of full cells, two per reachable threshold j: one with 16 S = N T_j exactly (N = 768, S = 48 T_j: the
    class is j) and one with the next sum, S + 1 (the class is j + 1).  -> (x, xhat, [(cy, cx, j, class expected)])"""
    js = threshold_js(d)
    cols = 6
    rows = -(-2 * len(js) // cols)
    x = np.zeros((rows * CELL, cols * CELL, 3), np.uint8)
    xhat = x.copy()
    want = []
    for i, (j, above) in enumerate((j, a) for j in js for a in (0, 1)):
        cy, cx = divmod(i, cols)
        cx_, ch_ = _cell_with_sum(768, 48 * THRESHOLDS[j] + above, d, max_symbol(d))
        # samples are laid out in the cell as [y][x][c]: which sample holds which magnitude is immaterial to S
        x[cy * CELL:(cy + 1) * CELL, cx * CELL:(cx + 1) * CELL] = cx_.reshape(CELL, CELL, 3)
        xhat[cy * CELL:(cy + 1) * CELL, cx * CELL:(cx + 1) * CELL] = ch_.reshape(CELL, CELL, 3)
        want.append((cy, cx, j, j + above))
    return x, xhat, want


def odd_threshold_strips(d):
    """16 S is a multiple of 16, so 16 S = N T_j + 1 needs N T_j = 15 (mod 16): no N does that for an even T_j, and for an
    odd one the partial cell of a 1 x w image with w T_j = 5 (mod 16) does (N = 3 w).  -> [(j, x, xhat)] with
    16 S = N T_j + 1 exactly: the class is j + 1, by the smallest margin there is"""
    out = []
    for j in threshold_js(d):
        t = THRESHOLDS[j]
        if t % 2 == 0:
            continue
        w = next(w for w in range(1, 17) if (w * t) % 16 == 5)
        n = 3 * w
        assert (n * t + 1) % 16 == 0
        x, xhat = _cell_with_sum(n, (n * t + 1) // 16, d, max_symbol(d))
        out.append((j, x.reshape(1, w, 3), xhat.reshape(1, w, 3)))
    return out


def kernel_cases():
    """every case of the GPU kernel test: dicts with name, x, xhat (8-bit [H, W, 3]), d, byte_offset / elem_offset of the
    buffers, and ``paths``: what of ``run_paths`` the case is there for"""
    cases = []
    for k, (H, W) in enumerate(SHAPES):
        for d in BOUNDS:
            x, xhat = random_pair(H, W, 100 * k + d)
            cases.append(dict(name=f"random-{H}x{W}-D{d}", x=x, xhat=xhat, d=d, byte_offset=0, elem_offset=0,
                              paths={(1, 1): {"byte", "scalar", "partial"}, (16, 16): {"dword", "vec", "full"},
                                     (17, 33): {"dword", "byte", "vec", "scalar", "full", "partial"},
                                     (37, 53): {"dword", "byte", "vec", "scalar", "full", "partial"},
                                     (64, 48): {"dword", "vec", "full"}}[(H, W)]))
        for reverse in (False, True):
            x, xhat = extreme_pair(H, W, reverse)
            for d in BOUNDS:
                cases.append(dict(name=f"extreme{'-rev' if reverse else ''}-{H}x{W}-D{d}", x=x, xhat=xhat, d=d,
                                  byte_offset=0, elem_offset=0, paths=set()))
    # buffers off their natural 16-byte boundary: the full runs of the aligned shapes take the slow paths
    x, xhat = random_pair(64, 48, 7)
    cases.append(dict(name="random-64x48-D1-odd-pointers", x=x, xhat=xhat, d=1, byte_offset=1, elem_offset=1,
                      paths={"byte", "scalar", "full"}))
    x, xhat = random_pair(16, 16, 8)
    cases.append(dict(name="random-16x16-D3-odd-pointers", x=x, xhat=xhat, d=3, byte_offset=3, elem_offset=3,
                      paths={"byte", "scalar", "full"}))
    for d in BOUNDS:
        x, xhat, _ = threshold_image(d)
        cases.append(dict(name=f"thresholds-D{d}", x=x, xhat=xhat, d=d, byte_offset=0, elem_offset=0,
                          paths={"dword", "vec", "full"}))
        for j, x, xhat in odd_threshold_strips(d):
            cases.append(dict(name=f"threshold-{j}-plus-one-D{d}", x=x, xhat=xhat, d=d, byte_offset=0, elem_offset=0,
                              paths={"partial"}))
    return cases
