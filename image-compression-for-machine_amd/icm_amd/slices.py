"""Hyperprior + channel-conditional slice loop of the cnn / stf models (compressai/models/cnn.py:144-183 ==
stf.py:596-637), in its two forms, and what they share with each other and with the zigzag loop of stf6 (models.py):

  chain helpers   ``chain_layers``, ``_chain``, ``_chain_pair``, ``_h_s_pair``, ``_copy_op``
  coding          what compress() / decompress() hand a loop as ``coding``: an ``Encoder`` that records the symbols and
                  CDF indexes of every slice, or a ``Decoder`` that takes each slice's y_hat_pre from the entropy decoder;
                  ``gaussian_step`` is the ONE per-slice Gaussian-conditional step of every loop
  prologue / epilogue   ``hyperprior`` (h_a -> entropy bottleneck -> h_s pair), ``prologue`` (shapes, gradient aliasing,
                  the buffers both forms write) and ``epilogue`` (what ``keep`` holds)
  hyper_slices_unsplit   the per-chain form: support buffers, cat -> chain
  hyper_slices_split     the FIRST layer of every chain split by input-channel block, described below

The reference builds, per slice i, ``mean_support = cat([latent_means] + y_hat_slices[:max_support])`` and runs
cc_mean / cc_scale on it (and lrp on ``cat([mean_support, y_hat_slice])``).  A convolution is linear in its input
channels, so the first layer of each of the 3 * num_slices chains is

    W[:, :M] * latent  +  W[:, M:M+c*k] * y_hat[:c*k]  (+ W[:, M+c*k:] * y_hat_pre_i for lrp)  + bias,  k = min(i, max_support)

  A  the latent block (M of M + c*k channels: 72 % of the first-layer FLOP at M=320) depends on NO slice: it is computed
     for all chains up front as two wide convolutions (latent_means -> all cc_mean and lrp chains, latent_scales -> all
     cc_scale chains: weights concatenated along GEMM-M, 4 480 / 2 240 output channels instead of 30 launches of 224);
  B  the support block reads y_hat[:, :c*k], which IS the support (no torch.cat copies): one grouped launch per serial
     slice (three chains) and one per batch of tail slices, accumulated onto A in place;
  C  the lrp chains' own-slice block (c = 32 channels) after the Gaussian conditional.

Only B (K = 9*c*k) and C (K = 9*c) remain inside the serial dependency chain slice 0 -> 1 -> ... -> max_support-1.
Backward mirrors it: the input gradients of block A are two contractions over K = 20*224 / 10*224 channels of the
pre-activation gradient buffer, those of block B one contraction per slice over its three chains (blocked channel map),
and the weight gradients land in column blocks of the canonical [Cout][Cin_total][3][3] tensors (``dw_ld``).

Buffers (NCHW f32): PRE0 / G0 / DPRE0 [N, 3*S*D0, h, w] = first-layer pre-activations, their materialised GELU and
their gradients, laid out family-major: channel ((f*S + i)*D0 + d) for family f in (cc_mean, lrp, cc_scale), slice i.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace
from typing import Dict, Optional

import torch

from . import _lib as L
from . import engine as E
from ._lib import ACT_GELU, EPI_NONE, check, ptr
from .engine import VT, _key

import os as _os
# K-split factors of the wide input-gradient launches (0 / 1 = one launch): same-box A/B switches
KSPLIT_A = int(_os.environ.get("ICM_KSPLIT_A", "4"))
KSPLIT_B = _os.environ.get("ICM_KSPLIT_B", "1") != "0"

FAM = ("cc_mean_transforms", "lrp_transforms", "cc_scale_transforms")   # PRE0 family order: the two latent_means consumers adjacent


def chain_layers(tape, P, names, xvs, layers=(2, 4, 6, 8), outs=None, lrp_auxs=None):
    """the given layers (default: all but the first) of the five-convolution chains ``names`` on the inputs xvs, one
    grouped launch per layer with virtual GELUs between (cnn.py:89-127); outs / lrp_auxs belong to the last layer (8)"""
    ts = None
    for li in layers:
        last = li == 8
        ts = E.conv2d_group(tape, xvs, [P[f"{p}.{li}.weight"] for p in names], [P[f"{p}.{li}.bias"] for p in names],
                            pad=1, outs=outs if last else None, lrp_auxs=lrp_auxs if last else None, act_out=not last)
        xvs = [VT(t, ACT_GELU) for t in ts]
    return ts


def _chain(tape, P, p, xv: VT, strides=(1, 1, 1, 1, 1), out=None, lrp_aux=None):
    """five conv3x3 with virtual GELUs between (cnn.py:54-64, 89-127)."""
    for j, i in enumerate((0, 2, 4, 6, 8)):
        last = j == 4
        t = E.conv2d(tape, xv, P[f"{p}.{i}.weight"], P[f"{p}.{i}.bias"], stride=strides[j], pad=1,
                     out=out if last else None, lrp_aux=lrp_aux if last else None, act_out=not last)
        xv = VT(t, ACT_GELU)
    return t


def _chain_pair(tape, P, p1, p2, xv1: VT, xv2: VT):
    """cc_mean_transforms[i] and cc_scale_transforms[i] are independent and shape-identical: run each of
    their five convolutions as one grouped launch (forward and dgrad)."""
    return chain_layers(tape, P, [p1, p2], [xv1, xv2], (0, 2, 4, 6, 8))


def _h_s_pair(tape, P, p1, p2, z_hat, out1, out2):
    """h_scale_s and h_mean_s (cnn.py:66-88) are independent and shape-identical: each of their five convolutions
    (two with the PixelShuffle store) runs as one grouped launch"""
    xv = [VT(z_hat), VT(z_hat)]
    for name, ps, last in ((".0", 0, False), (".2.0", 2, False), (".4", 0, False), (".6.0", 2, False), (".8", 0, True)):
        ts = E.conv2d_group(tape, xv, [P[p1 + name + ".weight"], P[p2 + name + ".weight"]],
                            [P[p1 + name + ".bias"], P[p2 + name + ".bias"]], pad=1, pixel_shuffle=ps,
                            outs=[out1, out2] if last else None, act_out=not last)
        xv = [VT(ts[0], ACT_GELU), VT(ts[1], ACT_GELU)]
    return ts


def _copy_op(tape, src, dst):
    """dst = src (cat/chunk plumbing) with gradient routed back"""
    E.copy_into(tape, src, dst)
    if tape.need_grad:
        def bwd():
            g = tape.grad_of(dst)
            if g is not None:
                E.accumulate(tape, src, g)
        tape.bw.append(bwd)


# ------------------------------------------------------------------------------------------------ coding
class Encoder:
    """``coding`` of compress() (cnn.py:246-252): the int32 symbols and CDF indexes of every slice, as the quantiser
    codes them, are recorded as device tensors keyed by slice.  With a fused quantiser that is the encoder's ONE launch per
    slice (it writes y_hat_pre too); otherwise it follows the likelihood launch, which wrote y_hat_pre."""
    decoding = False

    def __init__(self, quantiser: E.Quantiser):
        self.q, self.symbols, self.indexes = quantiser, {}, {}
        self.likelihoods = not quantiser.fused

    def slice(self, tape, i, y, mu, sc, yh_pre):
        self.symbols[i], self.indexes[i] = self.q.code(L.stream(), y, mu, sc, yh_pre)


class Decoder:
    """``coding`` of decompress() (cnn.py:289-326): y is None and the loop starts from ``z_hat`` ([N, *, h/4, w/4], M
    latent channels).  The SAME launch sequence runs (identical kernels on identical inputs give the bit-identical mu /
    scale the encoder saw, which the CDF indexes depend on), but each slice's y_hat_pre comes from the entropy decoder:
    scale -> CDF indexes -> ``decode_run`` of ``dec`` (a coder's decoder, ``icm_amd.ans``) -> symbols -> y_hat_pre."""
    decoding, likelihoods = True, False

    def __init__(self, quantiser: E.Quantiser, dec, z_hat, M: int):
        self.q, self.dec, self.z_hat, self.M, self._next = quantiser, dec, z_hat, M, 0

    def slice(self, tape, i, y, mu, sc, yh_pre):
        if i != self._next:
            raise RuntimeError("slices must be decoded in stream order")
        self._next += 1
        sym = self.dec.decode_run(self.q.indexes(tape.st, sc))
        self.q.dequantize(tape.st, sym, mu, yh_pre)

    def finish(self):
        self.dec.finish()

    def close(self):
        self.dec.close()


def gaussian_step(tape, coding, i, sel, y, noise_y, Y_lik, mu, sc, yh_pre, steps=None, qmap=None):
    """GaussianConditional + ste_round of slice i (cnn.py:170-173), the one such step of every loop: likelihoods ->
    Y_lik[sel] and y_hat_pre -> yh_pre from y[sel] (``sel`` indexes the slice in y, the noise and Y_lik), then whatever
    ``coding`` does with the slice.  A fused encoder and the decoder make no likelihood launch: they write yh_pre.
    ``steps`` (forward and training, not with ``coding``): a quantiser step per image, ``engine.gc_likelihood_ste``;
    ``qmap`` (likewise, instead of ``steps``): a step index per image and latent position."""
    if coding is None or coding.likelihoods:
        E.gc_likelihood_ste(tape, y[sel], mu, sc, None if noise_y is None else noise_y[sel], Y_lik[sel], yh_pre,
                            steps=steps, qmap=qmap)
    if coding is not None:
        coding.slice(tape, i, None if y is None else y[sel], mu, sc, yh_pre)


# ------------------------------------------------------------------------------------------------ prologue / epilogue
def hyperprior(tape, P, y, noise_z, z_hat, shape, dev, support: int = 0):
    """h_a + entropy bottleneck (cnn.py:144-152), then the hyper synthesis pair (cnn.py:154-155) into the first M channels
    of two fresh [N, M + support, h, w] buffers -> (z, z_hat, z_likelihoods, scales buffer, means buffer).  ``z_hat``
    given (the decoder's): nothing runs before the pair, z and z_likelihoods are None."""
    N, M, h, w = shape
    z = z_lik = None
    if z_hat is None:
        z = _chain(tape, P, "h_a", VT(y), strides=(1, 1, 2, 1, 2))
        _, z_lik = E.eb_likelihood(tape, z, P, "entropy_bottleneck", noise_z)
        z_hat = E.ste_round_medians(tape, z, P["entropy_bottleneck.quantiles"])
    if (h % 4) or (w % 4):
        raise ValueError("hyper-synthesis output does not match the latent size (input must be a multiple of 64)")
    SS, MS = E.new((N, M + support, h, w), dev), E.new((N, M + support, h, w), dev)
    _h_s_pair(tape, P, "h_scale_s", "h_mean_s", z_hat, SS[:, :M], MS[:, :M])
    return z, z_hat, z_lik, SS, MS


def prologue(tape, P, y, noise_z, num_slices, coding, bucket_marks, support_slices: int = 0):
    """What both forms do before their slices: shapes from y or from the decoder's z_hat, one aliased gradient buffer each
    for y and y_hat (consumed whole and by slices), the hyperprior (its two buffers with room for ``support_slices``
    slices behind the latent channels), and the y_hat / likelihood buffers.  -> a namespace of N, M, h, w, c (channels
    per slice), dev, z, z_hat, z_lik, SS, MS (``hyperprior``), Y_hat, dYh, Y_lik.  The ``bucket_marks`` [2] and [1] are
    set here, [0] by ``epilogue``: positions in ``tape.bw`` by which the Trainer buckets its gradient all-reduces."""
    z_hat = None
    if coding is not None and coding.decoding:
        z_hat = coding.z_hat.contiguous()
        dev, N, M = z_hat.device, z_hat.shape[0], coding.M
        h, w = z_hat.shape[2] * 4, z_hat.shape[3] * 4
        if tape.need_grad:
            raise ValueError("decode mode is inference only")
    else:
        dev, (N, M, h, w) = y.device, y.shape
    if M % num_slices != 0:
        raise ValueError("latent channels must divide into num_slices")
    c = M // num_slices
    if tape.need_grad:
        dY = E.zeros(y.shape, dev)
        tape.bind_grad(y, dY, True)
        for i in range(num_slices):
            tape.bind_grad(y[:, i * c:(i + 1) * c], dY[:, i * c:(i + 1) * c], True)
    if bucket_marks is not None:
        bucket_marks[2] = len(tape.bw)   # backward reaching here => hyper-path gradients are complete
    z, z_hat, z_lik, SS, MS = hyperprior(tape, P, y, noise_z, z_hat, (N, M, h, w), dev, c * support_slices)
    Y_hat = E.new((N, M, h, w), dev)
    Y_lik = E.new((N, M, h, w), dev) if coding is None or coding.likelihoods else None
    dYh = None
    if tape.need_grad:
        dYh = E.zeros(Y_hat.shape, dev)
        tape.bind_grad(Y_hat, dYh, True)
        for i in range(num_slices):
            tape.bind_grad(Y_hat[:, i * c:(i + 1) * c], dYh[:, i * c:(i + 1) * c], True)
    if bucket_marks is not None:
        bucket_marks[1] = len(tape.bw)   # => slice-chain gradients complete
    return SimpleNamespace(N=N, M=M, h=h, w=w, c=c, dev=dev, z=z, z_hat=z_hat, z_lik=z_lik, SS=SS, MS=MS, Y_hat=Y_hat,
                           dYh=dYh, Y_lik=Y_lik)


def epilogue(tape, p, y, mu, scale, keep, bucket_marks):
    """-> (y_hat, y_likelihoods, z_likelihoods); ``keep`` gets the intermediates the parity tests and compress() read.
    mu / scale: [N, M, h, w], or their slices in order"""
    if bucket_marks is not None:
        bucket_marks[0] = len(tape.bw)   # => synthesis-transform gradients complete
    if keep is not None:
        mu, scale = (v if torch.is_tensor(v) else torch.cat(v, 1) for v in (mu, scale))
        keep.update(y=y, z=p.z, z_hat=p.z_hat, y_hat=p.Y_hat, mu=mu, scale=scale, lat_means=p.MS[:, :p.M],
                    lat_scales=p.SS[:, :p.M])
    return p.Y_hat, p.Y_lik, p.z_lik


# ------------------------------------------------------------------------------------------------ the per-chain form
def hyper_slices_unsplit(tape: E.Tape, P: Dict[str, torch.Tensor], y, noise_z, noise_y, num_slices: int,
                         max_support: int, keep: Optional[dict], bucket_marks: Optional[dict], coding, steps=None,
                         qmap=None):
    """torch.cat / chunk become channel-slice views of persistent support buffers: MS / SS hold the latent means / scales
    followed by the y_hat of the first max_support slices, LS of a slice its mean support followed by its y_hat_pre."""
    S, ms = num_slices, max_support
    p = prologue(tape, P, y, noise_z, S, coding, bucket_marks, support_slices=ms)
    N, M, h, w, c, dev, MS, SS, Y_hat = p.N, p.M, p.h, p.w, p.c, p.dev, p.MS, p.SS, p.Y_hat
    need = tape.need_grad
    if need:
        dMS, dSS = E.zeros(MS.shape, dev), E.zeros(SS.shape, dev)
        for k in range(ms + 1):
            tape.bind_grad(MS[:, :M + c * k], dMS[:, :M + c * k], True)
            tape.bind_grad(SS[:, :M + c * k], dSS[:, :M + c * k], True)
        for j in range(ms):
            sl = slice(M + c * j, M + c * (j + 1))
            tape.bind_grad(MS[:, sl], dMS[:, sl], True)
            tape.bind_grad(SS[:, sl], dSS[:, sl], True)
    mus, scs = [], []

    def chains(idx, k, serial):
        """slices idx, all with the support of k slices: their mean / scale chains as one grouped launch per layer, the
        Gaussian step of each, their lrp chains (LRP tail fused into the last launch).  serial: one slice, whose lrp
        chain is a plain launch per layer and whose y_hat joins the support of the next"""
        nt = len(idx)
        sup_m, sup_s = MS[:, :M + c * k], SS[:, :M + c * k]
        names = [f"cc_mean_transforms.{i}" for i in idx] + [f"cc_scale_transforms.{i}" for i in idx]
        ts = chain_layers(tape, P, names, [VT(sup_m)] * nt + [VT(sup_s)] * nt, (0, 2, 4, 6, 8))
        LSs, pres = [], []
        for j, i in enumerate(idx):
            LS = E.new((N, M + c * (k + 1), h, w), dev)
            yh_pre = LS[:, M + c * k:]
            if need:
                dLS = E.zeros(LS.shape, dev)
                tape.bind_grad(LS, dLS, True)
                tape.bind_grad(LS[:, :M + c * k], dLS[:, :M + c * k], True)
                tape.bind_grad(yh_pre, dLS[:, M + c * k:], True)
            _copy_op(tape, sup_m, LS[:, :M + c * k])
            gaussian_step(tape, coding, i, (slice(None), slice(i * c, (i + 1) * c)), y, noise_y, p.Y_lik, ts[j], ts[nt + j],
                          yh_pre, steps, qmap)
            LSs.append(LS)
            pres.append(yh_pre)
        outs = [Y_hat[:, i * c:(i + 1) * c] for i in idx]
        if serial:
            _chain(tape, P, f"lrp_transforms.{idx[0]}", VT(LSs[0]), out=outs[0], lrp_aux=pres[0])
            sl = slice(M + c * k, M + c * (k + 1))
            _copy_op(tape, outs[0], MS[:, sl])
            _copy_op(tape, outs[0], SS[:, sl])
        else:
            chain_layers(tape, P, [f"lrp_transforms.{i}" for i in idx], [VT(LS) for LS in LSs], (0, 2, 4, 6, 8), outs=outs,
                         lrp_auxs=pres)
        mus.extend(ts[:nt])
        scs.extend(ts[nt:])

    # ---- the support of slice i is y_hat_slices[:max_support] (cnn.py:161): slices 0..max_support-1 form a serial chain,
    # but every slice >= max_support sees the SAME fixed support (latent + the first max_support slices) and is
    # independent of its neighbours -> their chains run as grouped launches, in batches
    n_serial = min(S, ms)
    for i in range(n_serial):
        chains([i], i, True)
    tail = list(range(n_serial, S))
    for t0 in range(0, len(tail), E.MAX_GROUP // 2):
        chains(tail[t0:t0 + E.MAX_GROUP // 2], ms, False)
    return epilogue(tape, p, y, mus, scs, keep, bucket_marks)


# ------------------------------------------------------------------------------------------------ the split form
def _ksplit_dgrad(tape, x, wp, K, Cout, taps, gx, acc, ks, conv_b, tag):
    """Input gradient of a wide first-layer block, x [N, K, h, w] (contiguous channel range) -> gx [N, Cout, h, w], with
    the contraction split into ``ks`` equal channel ranges that run as the members of ONE grouped launch and write
    partial results, which are then added in member order (deterministic).  Such a launch has few output tiles (Cout =
    160 / 320 channels x 4 096 pixels) and a very deep K: on its own it occupies 160 of the 256 CUs; split four ways
    it fills whole rounds of the chip.  wp: the K-concatenated packed weights (chunk-major, so a channel range is a
    pointer offset: taps * cdiv(Cout, 32) * 256 floats per 8 channels)."""
    if ks <= 1 or K % (8 * ks):
        E.conv_launch(tape, x, wp, None, gx, Cin=K, Cout=Cout, transposed=1, accum=acc, tag=tag, **conv_b)
        return
    kp = K // ks
    per8 = taps * ((Cout + 31) // 32) * 256
    N, _, h, w = x.shape
    parts = [E.new((N, Cout, h, w), x.device) for _ in range(ks)]
    E.conv_launch_grouped(tape, [x[:, i * kp:(i + 1) * kp] for i in range(ks)], [wp[(i * kp // 8) * per8:] for i in range(ks)],
                          None, parts, Cin=kp, Cout=Cout, transposed=1, tag=tag, **conv_b)
    for i, part in enumerate(parts):
        if gx.is_contiguous():
            check(L.lib().icm_add_grad(ptr(part), 0, ptr(gx), part.numel(), acc if i == 0 else 1, tape.st), "add_grad")
        else:
            E.copy_into(tape, part, gx, acc if i == 0 else 1)


def _block_grad(tape, w):
    """gradient tensor of a weight that is written in disjoint column blocks: always accumulate into a defined buffer"""
    g, acc = tape.grad_for_write(w)
    if not acc:
        g.zero_()
    return g


def hyper_slices_split(tape: E.Tape, P: Dict[str, torch.Tensor], y, noise_z, noise_y, num_slices: int, max_support: int,
                       keep: Optional[dict], bucket_marks: Optional[dict], coding, steps=None, qmap=None):
    """see module docstring"""
    S, ms = num_slices, max_support
    p = prologue(tape, P, y, noise_z, S, coding, bucket_marks)
    N, M, h, w, c, dev, Y_hat, dYh = p.N, p.M, p.h, p.w, p.c, p.dev, p.Y_hat, p.dYh
    LM, LSC = p.MS, p.SS                            # latent_means, latent_scales (cnn.py:154-155)
    need = tape.need_grad

    W0 = {(i, f): P[f"{FAM[f]}.{i}.0.weight"] for i in range(S) for f in range(3)}
    B0 = {(i, f): P[f"{FAM[f]}.{i}.0.bias"] for i in range(S) for f in range(3)}
    D0 = W0[(0, 0)].shape[0]
    KH = W0[(0, 0)].shape[2]
    pad = KH // 2
    for (i, f), wt in W0.items():
        k = min(i, ms)
        if tuple(wt.shape) != (D0, M + c * k + (c if f == 1 else 0), KH, KH):
            raise ValueError(f"{FAM[f]}.{i}.0.weight: unexpected shape {tuple(wt.shape)}")
    if D0 % 32:
        raise ValueError("first-layer width must be a multiple of 32 (concatenated GEMM-M tiles)")
    CT = 3 * S * D0

    def off(i, f):
        return (f * S + i) * D0

    PRE0 = E.new((N, CT, h, w), dev)
    mat = E._MATERIALIZE and N * h * w >= E._MAT_MIN_PIXELS
    G0 = E.new((N, CT, h, w), dev) if mat else None
    pre = {k_: PRE0[:, off(*k_):off(*k_) + D0] for k_ in W0}
    g0 = {k_: G0[:, off(*k_):off(*k_) + D0] for k_ in W0} if mat else None
    DPRE0 = None
    if need:
        DPRE0 = E.new((N, CT, h, w), dev)
        for k_ in W0:
            tape.bind_grad(pre[k_], DPRE0[:, off(*k_):off(*k_) + D0], False)   # first writer: the second layer's dgrad
    YP = E.new((N, M, h, w), dev)                   # y_hat before the LRP correction, per slice (cnn.py:171-173)
    MU, SC = E.new((N, M, h, w), dev), E.new((N, M, h, w), dev)
    lib = L.lib()
    conv = dict(KH=KH, KW=KH, stride=1, pad=pad, OH=h, OW=w)
    px = float(N) * h * w

    def algo(cin, cout, members=1):
        """(forward pack flag, input-gradient pack flag, launch argument dicts) of a block launch: Winograd when the
        launch is large enough (engine.wino_ok), else the direct implicit GEMM"""
        on = E.wino_ok(KH, KH, 1, pad, min(cin, cout), work=px * cin * cout * members)
        return (1 if on else 0), (2 if on else 0), dict(conv, algo=1 if on else 0)

    def done(i, f):
        """pre(i, f) is complete: its consumers read the materialised GELU"""
        if mat:
            tape.mat[_key(pre[(i, f)])] = g0[(i, f)]

    # ---------------------------------------------------------------------------------------------- A: latent blocks
    order = [(i, f) for f in range(3) for i in range(S)]                # PRE0 channel order
    bias0 = E.new((CT,), dev)
    srcs = (C.c_void_p * len(order))(*[ptr(B0[k_]) for k_ in order])
    check(lib.icm_gather_vectors(srcs, len(order), D0, ptr(bias0), tape.st), "gather_vectors")
    # slice 0's mean / scale chains have no other block: their first layer is complete (and materialised) here
    wf, _, conv_f = algo(M, D0, 2)
    wp0 = [tape.pack_cat([(W0[(0, f)], 0)], D0, M, KH, KH, 1, 0, 1, pad, "M", wino=wf) for f in (0, 2)]
    E.conv_launch_grouped(tape, [LM, LSC], wp0, [B0[(0, 0)], B0[(0, 2)]], [pre[(0, 0)], pre[(0, 2)]], Cin=M, Cout=D0,
                          transposed=0, y2s=[g0[(0, 0)], g0[(0, 2)]] if mat else None, tag="fwd(A0)", **conv_f)
    done(0, 0)
    done(0, 2)
    # everything else: latent_means -> channels [D0, 2*S*D0), latent_scales -> [2*S*D0 + D0, 3*S*D0)
    mem_m = [k_ for k_ in order if k_[1] in (0, 1)][1:]
    mem_s = [k_ for k_ in order if k_[1] == 2][1:]
    for xin, mem in ((LM, mem_m), (LSC, mem_s)):
        c0 = off(*mem[0])
        wf, _, conv_f = algo(M, len(mem) * D0)
        wpA = tape.pack_cat([(W0[k_], 0) for k_ in mem], D0, M, KH, KH, 1, 0, 1, pad, "M", wino=wf)
        E.conv_launch(tape, xin, wpA, bias0[c0:c0 + len(mem) * D0], PRE0[:, c0:c0 + len(mem) * D0], Cin=M,
                      Cout=len(mem) * D0, transposed=0, tag="fwd(A)", **conv_f)
    if need:
        def bwd_A():
            # weight (+ bias) gradients of the latent blocks: 3*S problems of one geometry, columns [0, M) of each weight
            for k_ in order:
                gw = _block_grad(tape, W0[k_])
                gb_, accb = tape.grad_for_write(B0[k_])
                E.wgrad_defer(tape, DPRE0[:, off(*k_):off(*k_) + D0], LM if k_[1] != 2 else LSC, gw[:, :M], Ca=D0, Cb=M,
                              KH=KH, KW=KH, stride=1, pad=pad, accum=1, dbias=gb_, accum_bias=accb, dw_ld=W0[k_].shape[1])
            # input gradients: ONE contraction per latent tensor over all of its consumers' channels
            for xin, mem in ((LM, [k_ for k_ in order if k_[1] in (0, 1)]), (LSC, [k_ for k_ in order if k_[1] == 2])):
                if not tape.wants(xin):
                    continue
                c0 = off(*mem[0])
                _, wbk, conv_b = algo(len(mem) * D0, M)
                wpb = tape.pack_cat([(W0[k_], 0) for k_ in mem], M, D0, KH, KH, 0, 1, 1, pad, "K", wino=wbk)
                gx, acc = tape.grad_for_write(xin)
                _ksplit_dgrad(tape, DPRE0[:, c0:c0 + len(mem) * D0], wpb, len(mem) * D0, M, 16 if wbk else KH * KH, gx, acc,
                              KSPLIT_A, conv_b, "dgrad(A)")
        tape.bw.append(bwd_A)

    # ---------------------------------------------------------------------------------------------- B / C helpers
    def support_block(idx, k):
        """B: y_hat[:, :c*k] (the support of slices idx, contiguous, all with the same k > 0) into the first layers of
        their three chains, accumulated in place; one member per family (weights of the slices concatenated along M)"""
        n = len(idx)
        sup = Y_hat[:, :c * k]
        r0 = [off(idx[0], f) for f in range(3)]
        wf, _, conv_f = algo(c * k, n * D0, 3)
        wps = [tape.pack_cat([(W0[(i, f)], M) for i in idx], D0, c * k, KH, KH, 1, 0, 1, pad, "M", wino=wf) for f in range(3)]
        ys = [PRE0[:, r:r + n * D0] for r in r0]
        y2s = [G0[:, r:r + n * D0] for r in r0] if mat else None
        E.conv_launch_grouped(tape, [sup] * 3, wps, None, ys, Cin=c * k, Cout=n * D0, transposed=0, y2s=y2s, accum=1,
                              tag="fwd(B)", **conv_f)
        for i in idx:
            done(i, 0)
            done(i, 2)
        if need:
            def bwd_B():
                for i in idx:
                    for f in range(3):
                        gw = _block_grad(tape, W0[(i, f)])
                        E.wgrad_defer(tape, DPRE0[:, off(i, f):off(i, f) + D0], sup, gw[:, M:M + c * k], Ca=D0, Cb=c * k,
                                      KH=KH, KW=KH, stride=1, pad=pad, accum=1, dw_ld=W0[(i, f)].shape[1])
                # d y_hat[:, :c*k] += sum over the 3*n chains: one contraction, channels (f, i) picked by the blocked map
                _, wbk, conv_b = algo(3 * n * D0, c * k)
                wpb = tape.pack_cat([(W0[(i, f)], M) for f in range(3) for i in idx], c * k, D0, KH, KH, 0, 1, 1, pad, "K",
                                    wino=wbk)
                gx, acc = tape.grad_for_write(sup)
                if n > 1 and KSPLIT_B:
                    # batch of tail slices: one member per family (each a contiguous channel run: no blocked map needed),
                    # partial sums added in family order
                    per8 = (16 if wbk else KH * KH) * ((c * k + 31) // 32) * 256
                    parts = [E.new((N, c * k, h, w), dev) for _ in range(3)]
                    E.conv_launch_grouped(tape, [DPRE0[:, r:r + n * D0] for r in r0],
                                          [wpb[(f * n * D0 // 8) * per8:] for f in range(3)], None, parts, Cin=n * D0,
                                          Cout=c * k, transposed=1, tag="dgrad(B)", **conv_b)
                    for f, part in enumerate(parts):
                        E.copy_into(tape, part, gx, acc if f == 0 else 1)
                else:
                    E.conv_launch(tape, DPRE0[:, r0[0]:], wpb, None, gx, Cin=3 * n * D0, Cout=c * k, transposed=1,
                                  accum=acc, seg=(n * D0, (S - n) * D0), tag="dgrad(B)", **conv_b)
            tape.bind_grad(sup, dYh[:, :c * k], True)
            tape.bw.append(bwd_B)

    def own_block(idx, k):
        """C: y_hat_pre of slice i (c channels) into the first layer of its lrp chain (cnn.py:174), completing it"""
        xs = [YP[:, i * c:(i + 1) * c] for i in idx]
        wf, _, conv_f = algo(c, D0, len(idx))
        wps = [tape.pack_cat([(W0[(i, 1)], M + c * k)], D0, c, KH, KH, 1, 0, 1, pad, "M", wino=wf) for i in idx]
        E.conv_launch_grouped(tape, xs, wps, None, [pre[(i, 1)] for i in idx], Cin=c, Cout=D0, transposed=0,
                              y2s=[g0[(i, 1)] for i in idx] if mat else None, accum=1, tag="fwd(C)", **conv_f)
        for i in idx:
            done(i, 1)
        if need:
            def bwd_C():
                gxs = []
                for i, x in zip(idx, xs):
                    gw = _block_grad(tape, W0[(i, 1)])
                    E.wgrad_defer(tape, DPRE0[:, off(i, 1):off(i, 1) + D0], x, gw[:, M + c * k:M + c * k + c], Ca=D0, Cb=c,
                                  KH=KH, KW=KH, stride=1, pad=pad, accum=1, dw_ld=W0[(i, 1)].shape[1])
                    gx, acc = tape.grad_for_write(x)
                    if not acc:          # (the LRP tail's identity path wrote it first; a launch has one accumulate flag)
                        gx.zero_()
                    gxs.append(gx)
                _, wbk, conv_b = algo(D0, c, len(idx))
                wpb = [tape.pack_cat([(W0[(i, 1)], M + c * k)], c, D0, KH, KH, 0, 1, 1, pad, "K", wino=wbk) for i in idx]
                E.conv_launch_grouped(tape, [DPRE0[:, off(i, 1):off(i, 1) + D0] for i in idx], wpb, None, gxs, Cin=D0,
                                      Cout=c, transposed=1, accum=1, tag="dgrad(C)", **conv_b)
            tape.bw.append(bwd_C)

    def chains(idx, k):
        if k > 0:
            support_block(idx, k)
        # layers 2..8 of the mean / scale chains of these slices, straight into the mu / scale buffers
        names = [f"cc_mean_transforms.{i}" for i in idx] + [f"cc_scale_transforms.{i}" for i in idx]
        xvs = [VT(pre[(i, 0)], ACT_GELU) for i in idx] + [VT(pre[(i, 2)], ACT_GELU) for i in idx]
        outs = [MU[:, i * c:(i + 1) * c] for i in idx] + [SC[:, i * c:(i + 1) * c] for i in idx]
        chain_layers(tape, P, names, xvs, outs=outs)
        for i in idx:                                # GaussianConditional + ste_round: y_hat_pre -> YP, likelihoods -> Y_lik
            s1 = slice(i * c, (i + 1) * c)
            gaussian_step(tape, coding, i, (slice(None), s1), y, noise_y, p.Y_lik, MU[:, s1], SC[:, s1], YP[:, s1], steps,
                          qmap)
        own_block(idx, k)
        lnames = [f"lrp_transforms.{i}" for i in idx]
        chain_layers(tape, P, lnames, [VT(pre[(i, 1)], ACT_GELU) for i in idx],
                     outs=[Y_hat[:, i * c:(i + 1) * c] for i in idx], lrp_auxs=[YP[:, i * c:(i + 1) * c] for i in idx])

    # ---- serial slices 0 .. max_support-1, then the tail slices (all with the same, complete support) in batches
    n_serial = min(S, ms)
    for i in range(n_serial):
        chains([i], i)
    tail = list(range(n_serial, S))
    step = max(1, E.MAX_GROUP // 2)
    for t0 in range(0, len(tail), step):
        chains(tail[t0:t0 + step], ms)
    return epilogue(tape, p, y, MU, SC, keep, bucket_marks)
