"""compressai/models mirror for the `cnn` model: CompressionModel (models/base.py) and WACNN (models/cnn.py).

``WACNN.forward(x)`` keeps the reference contract ``{"x_hat", "likelihoods": {"y", "z"}}`` and the 585-key
state-dict, but executes as ONE hand-scheduled tape of HIP kernels (``wacnn_forward``): torch.cat / chunk are
replaced by writes into persistent support buffers, GELU / PixelShuffle / residual adds / the LRP tail are
fused into the implicit-GEMM prologues and epilogues, and the backward pass is the tape's closures."""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import engine as E
from .ans import coder_for
from .bitstream import check_qmap, check_qstep, check_rdoq, uniform_qmap
from .engine import VT
from .entropy_models import EntropyBottleneck, GaussianConditional
from .layers import (GDN, Conv2d, Win_noShift_Attention, WindowAttention, conv, conv3x3, deconv, subpel_conv3x3,
                     _named)
from .slices import (Decoder, Encoder, _chain, _chain_pair, _copy_op, gaussian_step, hyper_slices_split,
                     hyper_slices_unsplit, hyperprior)

SCALES_MIN, SCALES_MAX, SCALES_LEVELS = 0.11, 256, 64


def get_scale_table(min=SCALES_MIN, max=SCALES_MAX, levels=SCALES_LEVELS):
    return torch.exp(torch.linspace(math.log(min), math.log(max), levels))


def _map_dims(qmap) -> int:
    return qmap.dim() if torch.is_tensor(qmap) else np.asarray(qmap).ndim


def _cat_outputs(outs):
    return {"x_hat": torch.cat([o["x_hat"] for o in outs]),
            "likelihoods": {name: torch.cat([o["likelihoods"][name] for o in outs]) for name in ("y", "z")}}


class CompressionModel(nn.Module):
    """models/base.py:5-70."""

    def __init__(self, init_weights=True):
        super().__init__()
        # the reference calls _initialize_weights() here, before any sub-module exists: a no-op

    def _pack_cache(self) -> Optional[dict]:
        """eval mode: the MFMA-order weight copies are kept between calls (inference serving: packing 300 MB of weights
        per call costs more than a batch-1 forward).  The cache is dropped whenever a parameter changed -- in place
        through torch (version counters) or through the HIP optimiser (engine weight generation); train mode and
        graph capture (icm_amd/graphs.py: the packing launches belong in the graph) do not use it."""
        if self.training or getattr(self, "_eval_cache_off", False):
            return None
        sig = (E._weight_gen[0], sum(p._version for p in self.parameters()))
        if getattr(self, "_pack_sig", None) != sig:
            self._pack_eval, self._pack_sig = {}, sig
        return self._pack_eval

    def aux_loss(self):
        return sum(m.loss() for m in self.modules() if isinstance(m, EntropyBottleneck))

    def forward(self, *args):
        raise NotImplementedError()

    def _forward_each(self, x, qstep, qmap=None):
        """Eval mode with a step per image (``qstep`` a sequence or a tensor, more than one image): every image runs as
        its own batch of one and the results are concatenated -> the forward's dict, or None where this does not apply.
        The codec codes one image per stream, and the convolution plans are chosen by launch size, batch included, so
        only a batch of one gives image n the bits ``decompress(compress(x[n:n+1], qstep=K_n))`` gives it.  Training
        (and ``Trainer``, which calls the slice loop itself) keeps the batch in one launch sequence.
        The same for a quality map per image, ``qmap`` [B, h, w].  A step and a map together: ValueError."""
        if qmap is not None:
            if E.qstep_indexes(qstep, x.shape[0]) is not None:
                raise ValueError("forward: qstep and qmap are two forms of one thing; give one (a uniform map is its step)")
            if self.training or _map_dims(qmap) != 3 or x.shape[0] < 2:
                return None
            if len(qmap) != x.shape[0]:
                raise ValueError(f"forward: qmap holds {len(qmap)} maps for a batch of {x.shape[0]}")
            return _cat_outputs([self(x[n:n + 1], qmap=qmap[n]) for n in range(x.shape[0])])
        if self.training or not E.qstep_per_image(qstep) or x.shape[0] < 2:
            return None
        ks = E.qstep_indexes(qstep, x.shape[0])
        if ks is None:
            return None
        return _cat_outputs([self(x[n:n + 1], qstep=k) for n, k in enumerate(ks)])

    @staticmethod
    def _forward_quality(x, qstep, qmap):
        """(steps, maps) as the slice loop takes them, from what ``forward(x, qstep=, qmap=)`` was given; a map has
        the size of the latent of ``x`` padded to a multiple of 64 (``_pad_eval_input``).  ``qmap``: one map [h, w] for the
        batch, or (training, or a batch of one: ``_forward_each`` has taken the others) a map per image [B, h, w]; every
        map is checked by ``bitstream.check_qmap``.  One map that is uniform is its scalar step."""
        B, dev = x.shape[0], x.device
        if qmap is None:
            return E.qstep_steps(qstep, B, dev), None
        hw = (-(-x.shape[2] // 64) * 4, -(-x.shape[3] // 64) * 4)
        if _map_dims(qmap) == 3:
            if len(qmap) != B:
                raise ValueError(f"forward: qmap holds {len(qmap)} maps for a batch of {B}")
            if B > 1:
                maps = [check_qmap(m, hw, 0, "forward: ") for m in qmap]
                return None, torch.from_numpy(np.stack(maps)).to(dev)
            qmap = qmap[0]
        qmap = check_qmap(qmap, hw, 0, "forward: ")
        k = uniform_qmap(qmap)
        if k is not None:
            return E.qstep_steps(k, B, dev), None
        return None, torch.from_numpy(qmap).to(dev).unsqueeze(0).expand(B, *hw).contiguous()

    def update(self, force=False):
        """models/base.py:43-60: refresh the CDF tables of every EntropyBottleneck child"""
        updated = False
        for m in self.children():
            if not isinstance(m, EntropyBottleneck):
                continue
            updated |= m.update(force=force)
        return updated

    # ---- shared by the cnn and stf models: entropy coding around the slice loop (cnn.py:133-139,210-332)
    def _update_tables(self, scale_table=None, force=False):
        if scale_table is None:
            scale_table = get_scale_table()
        updated = self.gaussian_conditional.update_scale_table(scale_table, force=force)
        updated |= CompressionModel.update(self, force=force)
        return updated

    def _params(self):
        names, params = _named(self)
        return dict(zip(names, [p.detach() for p in params]))

    def _compress_latent(self, tape, P, y, coder, debug=None, qstep=0, qmap=None, rdoq=None):
        """cnn.py:214-266 from ``y`` on: {"strings": [[y_string], z_strings], "shape": z spatial size, "qstep"}.
        ``coder`` (``icm_amd.ans.coder_for``) codes the recorded device tensors of all slices as one y string, a run
        per slice, and the z strings as single-run strings.  ``qstep``: step index of the quantiser step on y (0: none;
        z and its EntropyBottleneck know no step).  ``qmap``: a non-uniform quality map as ``_quality`` returns it (a
        checked int8 host array; ``qstep`` is then 0), returned under "qmap" with "qstep": None.  ``rdoq``: the checked
        weight of rate-distortion optimised quantisation (``bitstream.check_rdoq``) or None; it changes which symbols
        are coded, not the result's keys, and the decoder is not told."""
        gc = self.gaussian_conditional
        codec = Encoder(E.Quantiser(gc, qstep, _qmap_on(qmap, y.device), rdoq))
        keep = {}
        hyper_slices(tape, P, y, None, None, self.num_slices, self.max_support_slices, keep=keep, coding=codec)
        z = keep["z"]
        z_strings = self.entropy_bottleneck.compress(z, coder=coder)
        sym = torch.cat([codec.symbols[i].reshape(-1) for i in range(self.num_slices)])
        idx = torch.cat([codec.indexes[i].reshape(-1) for i in range(self.num_slices)])
        gc._check_tables()
        y_string = coder.encode(sym, idx, [codec.symbols[i].numel() for i in range(self.num_slices)], gc)
        if debug is not None:      # tests: the coded symbols / CDF indexes (slice-major, cnn.py:254-255), the final y_hat
            debug.update(symbols=sym.cpu().numpy(), indexes=idx.cpu().numpy(), y_hat=keep["y_hat"])
        if qmap is not None:
            return {"strings": [[y_string], z_strings], "shape": z.size()[-2:], "qstep": None, "qmap": qmap}
        return {"strings": [[y_string], z_strings], "shape": z.size()[-2:], "qstep": qstep}

    @torch.no_grad()
    def compress_latent(self, y, _debug=None, coder="host", symbols_per_wave=None, qstep=0, qmap=None, rdoq=None):
        """``compress`` from the latent on: ``y`` is what ``analysis(x)`` returned.  A rate search runs the analysis
        transform once per image and this once per probe."""
        qstep = check_qstep(qstep, "compress: ")
        rdoq = check_rdoq(rdoq, "compress: ")
        coder = coder_for(coder, symbols_per_wave)
        if not isinstance(y, torch.Tensor) or y.dim() != 4 or y.dtype != torch.float32:
            raise ValueError("compress_latent: expected the f32 [B,M,h,w] latent of analysis()")
        qstep, qmap = _quality(qstep, qmap, y.shape[2:], "compress: ")
        tape = E.Tape(need_grad=False, packed_cache=self._pack_cache())
        return self._compress_latent(tape, self._params(), y.contiguous(), coder, _debug, qstep, qmap, rdoq)

    def _decompress_latent(self, tape, P, strings, shape, coder, qstep=0, qmap=None):
        """cnn.py:289-328: y_hat from the two streams"""
        if not isinstance(strings, (list, tuple)) or len(strings) != 2:
            raise ValueError("strings must be [y_strings, z_strings]")
        z_hat = self.entropy_bottleneck.decompress(strings[1], shape, coder=coder)
        return decode_slices(tape, P, z_hat, strings[0][0], self.gaussian_conditional, self.num_slices,
                             self.max_support_slices, self.M, coder, qstep, _qmap_on(qmap, z_hat.device))

    # ---- the codec of a model whose subclass gives the latent width ``M`` and the two transforms as hooks on one tape:
    # ``_g_a(tape, P, x) -> y`` and ``_g_s(tape, P, y_hat) -> x_hat``
    @torch.no_grad()
    def analysis(self, x):
        """the analysis transform g_a alone -> y, what ``compress_latent`` takes"""
        _check_codec_input(x)
        tape = E.Tape(need_grad=False, packed_cache=self._pack_cache())
        return self._g_a(tape, self._params(), x.contiguous())

    @torch.no_grad()
    def compress(self, x, _debug=None, coder="host", symbols_per_wave=None, qstep=0, qmap=None, rdoq=None):
        """cnn.py:210-266 -> {"strings": [[y_string], z_strings], "shape": z.shape[-2:], "qstep"}; ``coder``: "host"
        (the reference's scalar stream) or "lanes" (lane streams coded on the device, ``symbols_per_wave`` symbols of
        a slice per wave body, None: ``icm_amd.ans.SYMBOLS_PER_WAVE``); ``qstep``: step index k of a quantiser step
        2^(k/8) on y (``icm_amd.bitstream.step_of``; 0: none, a larger k a smaller stream; parity unpinned: no
        counterpart in the reference); the decoder must be told the same coder and the same step.
        ``qmap`` (instead of ``qstep``): a quality map, a 2-D integer array or tensor of the latent's spatial size
        (H / 16, W / 16) holding a step index per position, shared by the batch and all channels.  A map whose
        entries are all k is ``qstep=k``, and that is what is returned; any other comes back, as an int8 host array,
        under "qmap" with "qstep": None, and the decoder must be given it.
        ``rdoq``: None, or the weight w > 0 of rate-distortion optimised quantisation: an element of y is coded one
        symbol nearer zero where w x the added squared error (in symbol units) is less than the bits the coder's tables
        say it saves (csrc/qstep.hip: ``icm_gc_code_rdo``; a smaller w trades more error for bits).  Encoder only: the
        strings are ordinary strings, and ``decompress`` takes the same arguments as without.  z knows no such choice."""
        qstep = check_qstep(qstep, "compress: ")
        rdoq = check_rdoq(rdoq, "compress: ")
        coder = coder_for(coder, symbols_per_wave)
        _check_codec_input(x)
        qstep, qmap = _quality(qstep, qmap, (x.shape[2] // 16, x.shape[3] // 16), "compress: ")
        P = self._params()
        tape = E.Tape(need_grad=False, packed_cache=self._pack_cache())
        return self._compress_latent(tape, P, self._g_a(tape, P, x.contiguous()), coder, _debug, qstep, qmap, rdoq)

    @torch.no_grad()
    def decompress(self, strings, shape, coder="host", qstep=0, qmap=None):
        """cnn.py:289-332 -> {"x_hat"} clamped to [0, 1]"""
        qstep = check_qstep(qstep, "decompress: ")
        coder = coder_for(coder)
        qstep, qmap = _quality(qstep, qmap, None if qmap is None else _latent_hw(shape), "decompress: ")
        P = self._params()
        tape = E.Tape(need_grad=False, packed_cache=self._pack_cache())
        x_hat = self._g_s(tape, P, self._decompress_latent(tape, P, strings, shape, coder, qstep, qmap))
        L.check(L.lib().icm_clamp(L.ptr(x_hat), x_hat.numel(), 0.0, 1.0, tape.st), "clamp")
        return {"x_hat": x_hat}

    def load_state_dict(self, state_dict, strict: bool = False):
        # models/base.py:62-70: resize the CDF buffers to whatever the checkpoint holds, then strict=False
        sd = dict(state_dict)
        for mod_name in ("entropy_bottleneck", "gaussian_conditional"):
            mod = getattr(self, mod_name, None)
            if mod is None:
                continue
            for b in ("_quantized_cdf", "_offset", "_cdf_length", "scale_table"):
                k = f"{mod_name}.{b}"
                if k in sd and hasattr(mod, b):
                    buf = getattr(mod, b)
                    if buf.numel() == 0 and sd[k].numel() != 0:
                        setattr(mod, b, torch.empty(sd[k].shape, dtype=buf.dtype, device=buf.device))
        return super().load_state_dict(sd, strict=False)


# ICM_SLICE_SPLIT=1 (default): the first layer of every slice chain is split by input-channel block (slices.py): the
# latent block of all 3 * num_slices chains runs as two wide convolutions outside the serial slice loop.  0 = the
# per-chain form (slices.hyper_slices_unsplit: support buffers, cat -> chain).  Both are kept and both are parity-tested at the bench geometry.
# Same-box A/B on MI355X (round 3, B=16): with the direct kernels only the split form LOSES (329.7 vs 335.7 img/s: its
# wide launches have few output tiles, and the support / own-slice blocks add ~30 small launches per direction); with
# the eight-wave Winograd kernel, whose wide co blocks are exactly what the 4 256-channel latent launch wants (460 us,
# 218 TF algorithmic), training is a tie (370.9 vs 371.8) and the eval forward gains 3 % (1 216 vs 1 180 img/s).
import os as _os
SLICE_SPLIT = _os.environ.get("ICM_SLICE_SPLIT", "1") != "0"


def hyper_slices(tape: E.Tape, P: Dict[str, torch.Tensor], y: torch.Tensor, noise_z, noise_y, num_slices: int,
                 max_support: int, keep: Optional[dict] = None, bucket_marks: Optional[dict] = None, coding=None,
                 steps=None, qmap=None):
    """Hyperprior + channel-conditional slice loop shared by the cnn and stf models
    (cnn.py:144-183 == stf.py:596-637) -> (y_hat, y_likelihoods, z_likelihoods), in the form SLICE_SPLIT names (read at
    call time).  coding: None (forward, training), or what compress() / decompress() code the slices with -- a
    ``slices.Encoder`` (y_likelihoods is None if its quantiser is fused) or a ``slices.Decoder`` (y is None, inference
    only, both likelihoods are None).  keep: a dict that receives the intermediates (``slices.epilogue``).
    steps (with coding None): the quantiser step of each image as ``engine.qstep_steps`` gives it -- likelihoods and
    y_hat are then those of the codec at that step (``engine.gc_likelihood_ste``); z knows no step.
    qmap (likewise, instead of steps): a device int8 [N, h, w] tensor, a step index per image and latent position."""
    if (steps is not None or qmap is not None) and coding is not None:
        raise ValueError("hyper_slices: a coding object carries its own quantiser; steps are for the forward pass")
    form = hyper_slices_split if SLICE_SPLIT else hyper_slices_unsplit
    return form(tape, P, y, noise_z, noise_y, num_slices, max_support, keep, bucket_marks, coding, steps, qmap)


def _quality(qstep, qmap, hw, who):
    """(qstep, qmap) as the latent coder takes them, from the public pair: ``qmap`` checked against the latent's
    spatial size ``hw`` (``bitstream.check_qmap``: ValueError before any GPU work, also for a map given together with
    a step).  A uniform map *is* its scalar step: (k, None).  A non-uniform one: (0, int8 host array)."""
    if qmap is None:
        return qstep, None
    qmap = check_qmap(qmap, hw, qstep, who)
    k = uniform_qmap(qmap)
    return (k, None) if k is not None else (0, qmap)


def _qmap_on(qmap, dev):
    """the host quality map of ``_quality`` as the device tensor the quantiser takes"""
    return None if qmap is None else torch.from_numpy(qmap).to(dev)


def decode_slices(tape: E.Tape, P, z_hat, y_string: bytes, gc, num_slices: int, max_support: int, M: int, coder,
                  qstep: int = 0, qmap: Optional[torch.Tensor] = None):
    """Decoder side of the slice loop (cnn.py:296-326): hyper_slices with a ``slices.Decoder`` -- per slice the chains
    give mu / scale -> CDF indexes -> ``decode_run`` of the coder's decoder yields the symbols -> y_hat_pre = symbols + mu;
    the LRP correction and the support bookkeeping are the forward's own.  Returns y_hat [N,M,h,w].  ``coder``: of
    ``icm_amd.ans.coder_for``; what a ``decode_run`` costs (host: a copy down and one up; lanes: one launch, no wait,
    the status read by ``finish`` after the loop) is the coder's business.  With a quantiser step ``qstep`` or a quality
    map ``qmap`` (a device int8 [h, w] tensor) the two launches around ``decode_run`` are the quantiser's
    (``engine.Quantiser``), which share their arithmetic with the encoder's kernel."""
    gc._check_tables()
    coding = Decoder(E.Quantiser(gc, qstep, qmap), coder.decoder(y_string, gc), z_hat, M)
    try:
        Y_hat, _, _ = hyper_slices(tape, P, None, None, None, num_slices, max_support, coding=coding)
        coding.finish()
    finally:
        coding.close()
    return Y_hat


def _split_lik(tape, Y_lik, num_slices):
    """runs FIRST in backward (registered last): hand the seeded d(y_likelihoods) to the per-slice consumers"""
    sc_ = Y_lik.shape[1] // num_slices

    def split():
        g = tape.grad_of(Y_lik)
        if g is not None:
            for i in range(num_slices):
                tape.bind_grad(Y_lik[:, i * sc_:(i + 1) * sc_], g[:, i * sc_:(i + 1) * sc_], True)
    tape.bw.append(split)


def wacnn_forward(tape: E.Tape, P: Dict[str, torch.Tensor], x: torch.Tensor, noise_z=None, noise_y=None,
                  num_slices: int = 10, max_support: int = 5, keep: Optional[dict] = None,
                  bucket_marks: Optional[dict] = None, steps=None, qmap=None):
    """WACNN.forward (models/cnn.py:141-189) on the HIP engine -> (x_hat, y_likelihoods, z_likelihoods).
    steps: a quantiser step per image, or qmap: one per image and latent position (``hyper_slices``)."""
    y = wacnn_g_a(tape, P, x)
    Y_hat, Y_lik, z_lik = hyper_slices(tape, P, y, noise_z, noise_y, num_slices, max_support, keep, bucket_marks,
                                       steps=steps, qmap=qmap)
    x_hat = wacnn_g_s(tape, P, Y_hat)
    if tape.need_grad:
        _split_lik(tape, Y_lik, num_slices)
    return x_hat, Y_lik, z_lik


def wacnn_g_a(tape: E.Tape, P, x):
    """analysis transform g_a (cnn.py:31-41)"""
    t = E.conv2d_thin_in(tape, x, P["g_a.0.weight"], P["g_a.0.bias"], stride=2, pad=2)
    t = E.gdn(tape, t, P["g_a.1.beta"], P["g_a.1.gamma"], False)
    t = E.conv2d(tape, VT(t), P["g_a.2.weight"], P["g_a.2.bias"], stride=2, pad=2)
    t = E.gdn(tape, t, P["g_a.3.beta"], P["g_a.3.gamma"], False)
    t = E.attention_gate(tape, t, P, "g_a.4", 8, 8, 4)
    t = E.conv2d(tape, VT(t), P["g_a.5.weight"], P["g_a.5.bias"], stride=2, pad=2)
    t = E.gdn(tape, t, P["g_a.6.beta"], P["g_a.6.gamma"], False)
    t = E.conv2d(tape, VT(t), P["g_a.7.weight"], P["g_a.7.bias"], stride=2, pad=2)
    return E.attention_gate(tape, t, P, "g_a.8", 8, 4, 2)


def wacnn_g_s(tape: E.Tape, P, Y_hat):
    """synthesis transform g_s (cnn.py:42-52)"""
    t = E.attention_gate(tape, Y_hat, P, "g_s.0", 8, 4, 2)
    t = E.conv2d(tape, VT(t), P["g_s.1.weight"], P["g_s.1.bias"], stride=2, pad=2, transposed=True, output_padding=1)
    t = E.gdn(tape, t, P["g_s.2.beta"], P["g_s.2.gamma"], True)
    t = E.conv2d(tape, VT(t), P["g_s.3.weight"], P["g_s.3.bias"], stride=2, pad=2, transposed=True, output_padding=1)
    t = E.gdn(tape, t, P["g_s.4.beta"], P["g_s.4.gamma"], True)
    t = E.attention_gate(tape, t, P, "g_s.5", 8, 8, 4)
    t = E.conv2d(tape, VT(t), P["g_s.6.weight"], P["g_s.6.bias"], stride=2, pad=2, transposed=True, output_padding=1)
    t = E.gdn(tape, t, P["g_s.7.beta"], P["g_s.7.gamma"], True)
    return E.convT2d_thin_out(tape, VT(t), P["g_s.8.weight"], P["g_s.8.bias"], stride=2, pad=2, output_padding=1)


# ------------------------------------------------------------------------------------------------ stf
STF_DEPTHS = (2, 2, 6, 2)
STF_HEADS = (3, 6, 12, 24)


def stf_drop_path_rates(drop_path_rate: float = 0.2, depths=STF_DEPTHS) -> Dict[str, float]:
    """stf.py:357 + 361-398: linspace(0, rate, sum(depths)); the synthesis layers index the same list with the
    reversed depths."""
    dpr = [v.item() for v in torch.linspace(0, drop_path_rate, sum(depths))]
    out, o = {}, 0
    for i, d in enumerate(depths):
        for j in range(d):
            out[f"layers.{i}.blocks.{j}"] = dpr[o + j]
        o += d
    o = 0
    for i, d in enumerate(depths[::-1]):
        for j in range(d):
            out[f"syn_layers.{i}.blocks.{j}"] = dpr[o + j]
        o += d
    return out


def _basic_layer(tape, P, p, t, depth, heads, ws, down, drops):
    """BasicLayer.forward (stf.py:271-313): the SW-MSA mask is address arithmetic inside the attention kernel."""
    for j in range(depth):
        key = f"{p}.blocks.{j}"
        t = E.swin_block(tape, t, P, key, heads, ws, 0 if j % 2 == 0 else ws // 2,
                         None if drops is None else drops.get(key))
    if down == "merge":
        return E.patch_merging(tape, t, P, p + ".downsample")
    if down == "split":
        return E.patch_split(tape, t, P, p + ".downsample")
    return t


def stf_forward(tape: E.Tape, P: Dict[str, torch.Tensor], x: torch.Tensor, noise_z=None, noise_y=None,
                drops: Optional[Dict[str, torch.Tensor]] = None, num_slices: int = 12, max_support: int = 6,
                window: int = 4, keep: Optional[dict] = None, bucket_marks: Optional[dict] = None, steps=None,
                qmap=None):
    """SymmetricalTransFormer.forward (models/stf.py:582-645) on the HIP engine.  Tokens stay NCHW end to end:
    [B, L, C] <-> [B, C, H, W] transposes of the reference vanish, Linear layers are 1x1 implicit GEMMs,
    LayerNorm normalises the channel axis per pixel.  drops: {"<layer>.blocks.<j>": [2,B] DropPath scales};
    steps: a quantiser step per image, or qmap: one per image and latent position (``hyper_slices``)."""
    y = stf_analysis(tape, P, x, drops, window)
    Y_hat, Y_lik, z_lik = hyper_slices(tape, P, y, noise_z, noise_y, num_slices, max_support, keep, bucket_marks,
                                       steps=steps, qmap=qmap)
    x_hat = stf_synthesis(tape, P, Y_hat, drops, window)
    if tape.need_grad:
        _split_lik(tape, Y_lik, num_slices)
    return x_hat, Y_lik, z_lik


def stf_analysis(tape: E.Tape, P, x, drops=None, window: int = 4):
    """patch_embed + layers (stf.py:582-595)"""
    if x.shape[2] % 2 or x.shape[3] % 2:
        raise ValueError("stf: odd image sizes need PatchEmbed padding (pad the input to a multiple of 64)")
    # ---- patch_embed (stf.py:331-351): conv 2x2 s2 + LayerNorm
    t = E.conv2d_thin_in(tape, x, P["patch_embed.proj.weight"], P["patch_embed.proj.bias"], stride=2, pad=0)
    t = E.layernorm(tape, t, P["patch_embed.norm.weight"], P["patch_embed.norm.bias"])
    for i in range(4):
        t = _basic_layer(tape, P, f"layers.{i}", t, STF_DEPTHS[i], STF_HEADS[i], window, "merge" if i < 3 else None,
                         drops)
    return t


def stf_synthesis(tape: E.Tape, P, Y_hat, drops=None, window: int = 4):
    """syn_layers + end_conv (stf.py:638-645)"""
    t = Y_hat
    for i in range(4):
        t = _basic_layer(tape, P, f"syn_layers.{i}", t, STF_DEPTHS[3 - i], STF_HEADS[3 - i], window,
                         "split" if i < 3 else None, drops)
    # ---- end_conv (stf.py:401-404): conv5x5 -> PixelShuffle(2) (fused store) -> conv3x3
    t = E.conv2d(tape, VT(t), P["end_conv.0.weight"], P["end_conv.0.bias"], pad=2, pixel_shuffle=2)
    if E.THIN_OUT:   # 48 -> 3 output channels: dense 27-row GEMM + col2im instead of a 32-row tile per tap
        return E.conv2d_thin_out(tape, VT(t), P["end_conv.2.weight"], P["end_conv.2.bias"], pad=1)
    return E.conv2d(tape, VT(t), P["end_conv.2.weight"], P["end_conv.2.bias"], pad=1)



# ------------------------------------------------------------------------------------------------ stf6 (zigzag + Swin-refined means)
STF6_SLICES, STF6_NUMBER, STF6_SUPPORT, STF6_MU_HEADS = 6, 2, 16, 4


def stf6_drop_path_rates(drop_path_rate: float = 0.2, depths=STF_DEPTHS, nblocks: int = STF6_SLICES * 4) -> Dict[str, float]:
    """stf's rates plus the refinement stacks (stf6.py:469-484: built after ``depths = depths[::-1]``)"""
    out = stf_drop_path_rates(drop_path_rate, depths)
    dpr = [v.item() for v in torch.linspace(0, drop_path_rate, sum(depths))]
    for b in range(nblocks):
        o = 0
        for i, d in enumerate(depths[::-1]):
            for j in range(d):
                out[f"mu_Swin.{b}.{i}.blocks.{j}"] = dpr[o + j]
            o += d
    return out


def hyper_slices_zigzag(tape: E.Tape, P: Dict[str, torch.Tensor], y: torch.Tensor, noise_z, noise_y, drops,
                        num_slices: int = STF6_SLICES, max_support: int = STF6_SUPPORT, window: int = 4,
                        keep: Optional[dict] = None, bucket_marks: Optional[dict] = None):
    """Hyperprior + zigzag slice loop of SymmetricalTransFormer3.forward (stf6.py:778-858) ->
    (y_hat [B,M,h,w], y_likelihoods [B, nb*M/ns, h/2, w/2] in zigzag block order, z_likelihoods).
    The latent, its means and scales are cut into nb = ns*2*2 blocks by one permutation launch each; block i is coded
    from cat[means_i, y_hat of the previous min(i, max_support) blocks]: the y_hat blocks live in ONE buffer in coding
    order, so that support is a contiguous channel range copied behind the block's own means; the mean is refined by
    four Swin BasicLayers on the block map (mu_Swin[i]) before the likelihood; ZigzagReverse assembles y_hat.
    noise_y: None or [B, nb, M/ns, h/2, w/2] (zigzag order)."""
    dev, N, M, h, w = y.device, y.shape[0], y.shape[1], y.shape[2], y.shape[3]
    need = tape.need_grad
    nH = nW = STF6_NUMBER
    nb, cs, hb, wb = num_slices * nH * nW, M // num_slices, h // nH, w // nW
    if M % num_slices or h % nH or w % nW or hb % window or wb % window:
        raise ValueError("stf6: the latent must split into 2 x 2 blocks that are multiples of the window (input % 128 == 0)")
    if bucket_marks is not None:
        bucket_marks[2] = len(tape.bw)
    z, z_hat, z_lik, lat_scales, lat_means = hyperprior(tape, P, y, noise_z, None, (N, M, h, w), dev)
    y_zz = E.zigzag_splits(tape, y, num_slices, nH, nW)
    sc_zz = E.zigzag_splits(tape, lat_scales, num_slices, nH, nW)
    mu_zz = E.zigzag_splits(tape, lat_means, num_slices, nH, nW)
    YH = E.new((N, nb, cs, hb, wb), dev)          # y_hat blocks in coding order
    YHc = YH.view(N, nb * cs, hb, wb)
    Y_lik = E.new((N, nb, cs, hb, wb), dev)
    if need:
        dYH = E.zeros(YH.shape, dev)
        dYHc = dYH.view(N, nb * cs, hb, wb)
        tape.bind_grad(YH, dYH, True)
        for i in range(nb):
            tape.bind_grad(YH[:, i], dYH[:, i], True)
            k = min(i, max_support)
            if k > 1:
                tape.bind_grad(YHc[:, cs * (i - k):cs * i], dYHc[:, cs * (i - k):cs * i], True)
    if bucket_marks is not None:
        bucket_marks[1] = len(tape.bw)
    mus, scs = [], []
    rdepths = STF_DEPTHS[::-1]
    for i in range(nb):
        k = min(i, max_support)
        MSi, SSi = E.new((N, cs * (1 + k), hb, wb), dev), E.new((N, cs * (1 + k), hb, wb), dev)
        LSi = E.new((N, cs * (2 + k), hb, wb), dev)
        yh_pre = LSi[:, cs * (1 + k):]
        if need:
            for buf in (MSi, SSi, LSi):
                d = E.zeros(buf.shape, dev)
                tape.bind_grad(buf, d, True)
                tape.bind_grad(buf[:, :cs], d[:, :cs], True)
                if k > 0:
                    tape.bind_grad(buf[:, cs:cs * (1 + k)], d[:, cs:cs * (1 + k)], True)
                if buf is LSi:
                    tape.bind_grad(buf[:, :cs * (1 + k)], d[:, :cs * (1 + k)], True)
                    tape.bind_grad(yh_pre, d[:, cs * (1 + k):], True)
        _copy_op(tape, mu_zz[:, i], MSi[:, :cs])
        _copy_op(tape, sc_zz[:, i], SSi[:, :cs])
        if k > 0:
            sup = YHc[:, cs * (i - k):cs * i]
            _copy_op(tape, sup, MSi[:, cs:])
            _copy_op(tape, sup, SSi[:, cs:])
        mu, sc = _chain_pair(tape, P, f"cc_mean_transforms2.{i}", f"cc_scale_transforms2.{i}", VT(MSi), VT(SSi))
        t = mu
        for l in range(4):
            t = _basic_layer(tape, P, f"mu_Swin.{i}.{l}", t, rdepths[l], STF6_MU_HEADS, window, None, drops)
        mu = E.add(tape, mu, t)
        gaussian_step(tape, None, i, (slice(None), i), y_zz, noise_y, Y_lik, mu, sc, yh_pre)
        _copy_op(tape, MSi, LSi[:, :cs * (1 + k)])
        _chain(tape, P, f"lrp_transforms2.{i}", VT(LSi), out=YH[:, i], lrp_aux=yh_pre)
        if keep is not None:
            mus.append(mu)
            scs.append(sc)
    if bucket_marks is not None:
        bucket_marks[0] = len(tape.bw)
    Y_hat = E.zigzag_reverse(tape, YH, num_slices, nH, nW)
    Y_lik4 = Y_lik.view(N, nb * cs, hb, wb)
    if keep is not None:
        keep.update(y=y, z=z, z_hat=z_hat, y_hat=Y_hat, y_zz=y_zz, mu=torch.stack(mus, 1), scale=torch.stack(scs, 1))
    return Y_hat, Y_lik4, z_lik


def stf6_forward(tape: E.Tape, P: Dict[str, torch.Tensor], x: torch.Tensor, noise_z=None, noise_y=None,
                 drops: Optional[Dict[str, torch.Tensor]] = None, window: int = 4, keep: Optional[dict] = None,
                 bucket_marks: Optional[dict] = None):
    """SymmetricalTransFormer3.forward (models/stf6.py:764-872) on the HIP engine: stf's analysis / synthesis stacks
    around the zigzag slice loop."""
    y = stf_analysis(tape, P, x, drops, window)
    Y_hat, Y_lik, z_lik = hyper_slices_zigzag(tape, P, y, noise_z, noise_y, drops, window=window, keep=keep,
                                              bucket_marks=bucket_marks)
    x_hat = stf_synthesis(tape, P, Y_hat, drops, window)
    if tape.need_grad:
        _split_lik(tape, Y_lik, STF6_SLICES * 4)
    return x_hat, Y_lik, z_lik


def _pad_eval_input(x, training: bool):
    """Inputs whose sides are not multiples of 64 (six stride-2 stages).  The reference pads feature maps inside its
    Swin blocks (stf.py:158-163) and crops the slice-chain outputs (cnn.py:165,169), but its own evaluation entry
    point zero-pads the IMAGE to a multiple of 64 first (utils/eval_model/__main__.py:162-175), after which none of
    those branches is taken; this mirror does exactly that outer padding in eval mode and crops x_hat back
    (likelihoods cover the padded image, as they do in the reference's eval loop).  Training crops are 256x256."""
    if x.shape[2] % 64 == 0 and x.shape[3] % 64 == 0:
        return x, None
    if training or torch.is_grad_enabled() and x.requires_grad:
        raise ValueError("training inputs must be multiples of 64 (the reference trains on 256x256 crops)")
    from .utils import pad_to_multiple
    return pad_to_multiple(x, 64)


def _crop_eval_output(x_hat, pads):
    if pads is None:
        return x_hat
    from .utils import crop
    return crop(x_hat, pads)


def _latent_hw(shape):
    """spatial size of the latent y for the ``shape`` entry (z's) of a compress() result"""
    try:
        zh, zw = (int(s) for s in shape)
    except (TypeError, ValueError):
        raise ValueError(f"decompress: shape must be the two spatial sizes of z, got {shape!r}")
    return 4 * zh, 4 * zw


def _check_codec_input(x):
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError("expected [B,3,H,W]")
    if x.shape[2] % 64 or x.shape[3] % 64:
        raise ValueError("compress(): pad the image to a multiple of 64 first (icm_amd.utils.pad_to_multiple; the "
                         "reference's eval loop does the same, utils/eval_model/__main__.py:102-117)")


def _train_noise(injected, x, cz, cy):
    """U(-1/2,1/2) samples the entropy models add in train mode (entropy_models.py:131-135)"""
    B, _, H, W = x.shape
    dev = x.device
    if injected is not None:
        return (injected["z"].to(dev, torch.float32).contiguous(), injected["y"].to(dev, torch.float32).contiguous())
    return (torch.rand((B, cz, H // 64, W // 64), dtype=torch.float32, device=dev) - 0.5,
            torch.rand((B, cy, H // 16, W // 16), dtype=torch.float32, device=dev) - 0.5)


class WACNN(CompressionModel):
    """CNN based model (models/cnn.py:23-189): same modules, names and defaults as the reference."""
    M = 320

    def __init__(self, N=192, M=320, **kwargs):
        super().__init__(**kwargs)
        self.num_slices = 10
        self.max_support_slices = 5
        self.g_a = nn.Sequential(
            conv(3, N, kernel_size=5, stride=2), GDN(N),
            conv(N, N, kernel_size=5, stride=2), GDN(N),
            Win_noShift_Attention(dim=N, num_heads=8, window_size=8, shift_size=4),
            conv(N, N, kernel_size=5, stride=2), GDN(N),
            conv(N, M, kernel_size=5, stride=2),
            Win_noShift_Attention(dim=M, num_heads=8, window_size=4, shift_size=2))
        self.g_s = nn.Sequential(
            Win_noShift_Attention(dim=M, num_heads=8, window_size=4, shift_size=2),
            deconv(M, N, kernel_size=5, stride=2), GDN(N, inverse=True),
            deconv(N, N, kernel_size=5, stride=2), GDN(N, inverse=True),
            Win_noShift_Attention(dim=N, num_heads=8, window_size=8, shift_size=4),
            deconv(N, N, kernel_size=5, stride=2), GDN(N, inverse=True),
            deconv(N, 3, kernel_size=5, stride=2))
        self.h_a = nn.Sequential(conv3x3(320, 320), nn.GELU(), conv3x3(320, 288), nn.GELU(),
                                 conv3x3(288, 256, stride=2), nn.GELU(), conv3x3(256, 224), nn.GELU(),
                                 conv3x3(224, 192, stride=2))

        def hs():
            return nn.Sequential(conv3x3(192, 192), nn.GELU(), subpel_conv3x3(192, 224, 2), nn.GELU(),
                                 conv3x3(224, 256), nn.GELU(), subpel_conv3x3(256, 288, 2), nn.GELU(),
                                 conv3x3(288, 320))
        self.h_mean_s = hs()
        self.h_scale_s = hs()

        def cc(extra):
            return nn.ModuleList(nn.Sequential(
                conv(320 + 32 * min(i + extra, 5 + extra), 224, stride=1, kernel_size=3), nn.GELU(),
                conv(224, 176, stride=1, kernel_size=3), nn.GELU(),
                conv(176, 128, stride=1, kernel_size=3), nn.GELU(),
                conv(128, 64, stride=1, kernel_size=3), nn.GELU(),
                conv(64, 32, stride=1, kernel_size=3)) for i in range(10))
        self.cc_mean_transforms = cc(0)
        self.cc_scale_transforms = cc(0)
        self.lrp_transforms = cc(1)
        self.entropy_bottleneck = EntropyBottleneck(N)
        self.gaussian_conditional = GaussianConditional(None)
        self._noise = None

    def inject_noise(self, noise: Optional[dict]):
        """testing hook: {"z": [B,192,h/4,w/4], "y": [B,320,h,w]} U(-1/2,1/2) samples used in train mode"""
        self._noise = noise

    def forward(self, x, qstep=None, qmap=None):
        """``qstep``: None, or the step index k of a quantiser step 2^(k/8) on y -- an int, or a sequence / integer
        tensor of B of them, one per image (``engine.qstep_steps``).  The likelihoods of y are then the codec's at that
        step and, in eval mode on a 64-multiple input, x_hat.clamp(0, 1) is what ``decompress(compress(x, qstep=k))``
        returns, bit for bit -- of the whole batch for one k, of each image alone for a k per image (``_forward_each``);
        in train mode the noise is added in symbol units (parity unpinned, like ``compress``).
        ``qmap`` (instead of ``qstep``): a quality map, a 2-D integer array or tensor [h, w] of step indexes of the padded
        latent's size, one map for the batch as in the codec (``bitstream.check_qmap``); in eval mode on a 64-multiple
        input x_hat.clamp(0, 1) is ``decompress(compress(x, qmap=M), qmap=M)`` bit for bit, and a uniform map is its
        scalar step.  [B, h, w]: a map per image, each image its own batch of one in eval mode."""
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("WACNN.forward expects [B,3,H,W]")
        each = self._forward_each(x, qstep, qmap)
        if each is not None:
            return each
        names, params = _named(self)
        training = self.training
        dev = x.device
        steps, maps = self._forward_quality(x, qstep, qmap)
        x, pads = _pad_eval_input(x, training)
        nz = ny = None
        if training:
            nz, ny = _train_noise(self._noise, x, 192, 320)
        ns, ms = self.num_slices, self.max_support_slices

        def runner(tape, xin, *ps):
            return wacnn_forward(tape, dict(zip(names, ps)), xin, nz, ny, ns, ms, steps=steps, qmap=maps)

        x_hat, y_lik, z_lik = E.tape_function(runner, [x.contiguous(), *params], self._pack_cache())
        return {"x_hat": _crop_eval_output(x_hat, pads), "likelihoods": {"y": y_lik, "z": z_lik}}

    @classmethod
    def from_state_dict(cls, state_dict):
        net = cls(192, 320)
        net.load_state_dict(state_dict)
        return net

    def update(self, scale_table=None, force=False):
        """cnn.py:133-138"""
        return self._update_tables(scale_table, force)

    def _g_a(self, tape, P, x):
        return wacnn_g_a(tape, P, x)

    def _g_s(self, tape, P, y_hat):
        return wacnn_g_s(tape, P, y_hat)


# ------------------------------------------------------------------------------------------------ stf modules
class Mlp(nn.Module):
    """stf.py:24-40 (parameter holder; runs inside the model tape)."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        if drop != 0.0:
            raise NotImplementedError("icm Mlp: dropout is unused by the reference")
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)


class SwinTransformerBlock(nn.Module):
    """stf.py:124-193.  forward(x, mask_matrix=None) takes an NCHW map [B, C, H, W] (the reference's token layout
    [B, H*W, C] is its transpose; the mask is derived inside the kernel, the argument is ignored)."""

    def __init__(self, dim, num_heads, window_size=7, shift_size=0, mlp_ratio=4., qkv_bias=True, qk_scale=None,
                 drop=0., attn_drop=0., drop_path=0., act_layer=nn.GELU, norm_layer=nn.LayerNorm, inverse=False):
        super().__init__()
        self.dim, self.num_heads, self.window_size, self.shift_size = dim, num_heads, window_size, shift_size
        self.mlp_ratio = mlp_ratio
        assert 0 <= self.shift_size < self.window_size, "shift_size must in 0-window_size"
        self.norm1 = norm_layer(dim)
        self.attn = WindowAttention(dim, window_size=(window_size, window_size), num_heads=num_heads,
                                    qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=drop)
        self.drop_path_rate = float(drop_path)
        self.drop_path = nn.Identity()   # stochastic depth is drawn by the model forward (per-sample scales)
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.H = self.W = None

    def forward(self, x, mask_matrix=None):
        from .layers import run_module
        h, ws, sh = self.num_heads, self.window_size, self.shift_size
        dp = _draw_drop(self.drop_path_rate, x.shape[0], x.device) if self.training else None
        return run_module(self, lambda tape, P, t: (E.swin_block(tape, t, {"b." + k: v for k, v in P.items()}, "b", h,
                                                                 ws, sh, dp),), x.contiguous())[0]


class PatchMerging(nn.Module):
    """stf.py:196-233 on NCHW maps: [B, C, H, W] -> [B, 2C, H/2, W/2]."""

    def __init__(self, dim, norm_layer=nn.LayerNorm):
        super().__init__()
        self.dim = dim
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = norm_layer(4 * dim)

    def forward(self, x, H=None, W=None):
        from .layers import run_module
        return run_module(self, lambda tape, P, t: (E.patch_merging(tape, t, {"d." + k: v for k, v in P.items()}, "d"),),
                          x.contiguous())[0]


class PatchSplit(nn.Module):
    """stf.py:236-259 on NCHW maps: [B, C, H, W] -> [B, C/2, 2H, 2W]."""

    def __init__(self, dim, norm_layer=nn.LayerNorm):
        super().__init__()
        self.dim = dim
        self.reduction = nn.Linear(dim, dim * 2, bias=False)
        self.norm = norm_layer(dim)
        self.shuffle = nn.PixelShuffle(2)

    def forward(self, x, H=None, W=None):
        from .layers import run_module
        return run_module(self, lambda tape, P, t: (E.patch_split(tape, t, {"d." + k: v for k, v in P.items()}, "d"),),
                          x.contiguous())[0]


class BasicLayer(nn.Module):
    """stf.py:261-313 (parameter holder; stf_forward walks the blocks)."""

    def __init__(self, dim, depth, num_heads, window_size=7, mlp_ratio=4., qkv_bias=True, qk_scale=None, drop=0.,
                 attn_drop=0., drop_path=0., norm_layer=nn.LayerNorm, downsample=None, use_checkpoint=False,
                 inverse=False):
        super().__init__()
        self.window_size, self.shift_size, self.depth = window_size, window_size // 2, depth
        self.blocks = nn.ModuleList([
            SwinTransformerBlock(dim=dim, num_heads=num_heads, window_size=window_size,
                                 shift_size=0 if (i % 2 == 0) else window_size // 2, mlp_ratio=mlp_ratio,
                                 qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop, attn_drop=attn_drop,
                                 drop_path=drop_path[i] if isinstance(drop_path, list) else drop_path,
                                 norm_layer=norm_layer, inverse=inverse) for i in range(depth)])
        self.downsample = downsample(dim=dim, norm_layer=norm_layer) if downsample is not None else None


class PatchEmbed(nn.Module):
    """stf.py:316-351."""

    def __init__(self, patch_size=4, in_chans=3, embed_dim=96, norm_layer=None):
        super().__init__()
        self.patch_size = (patch_size, patch_size)
        self.in_chans, self.embed_dim = in_chans, embed_dim
        self.proj = Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)
        self.norm = norm_layer(embed_dim) if norm_layer is not None else None


def _draw_drop(rate: float, B: int, device, generator=None):
    """timm DropPath in train mode: per-sample Bernoulli(keep)/keep, one draw per residual branch -> [2, B]"""
    if rate <= 0.0:
        return None
    keep = 1.0 - rate
    return (torch.rand((2, B), device=device, generator=generator) < keep).to(torch.float32) / keep


class SymmetricalTransFormer(CompressionModel):
    """Swin-transformer codec (models/stf.py:318-645): same modules, names, defaults and state-dict as the
    reference; ``forward`` runs as one tape of HIP kernels (``stf_forward``)."""
    M = 384

    def __init__(self, pretrain_img_size=256, patch_size=2, in_chans=3, embed_dim=48, depths=[2, 2, 6, 2],
                 num_heads=[3, 6, 12, 24], window_size=4, num_slices=12, mlp_ratio=4., qkv_bias=True, qk_scale=None,
                 drop_rate=0., attn_drop_rate=0., drop_path_rate=0.2, norm_layer=nn.LayerNorm, patch_norm=True,
                 frozen_stages=-1, use_checkpoint=False):
        super().__init__()
        if (patch_size, in_chans, embed_dim, list(depths), list(num_heads), mlp_ratio, patch_norm) != \
                (2, 3, 48, [2, 2, 6, 2], [3, 6, 12, 24], 4., True) or drop_rate or attn_drop_rate or frozen_stages >= 0:
            raise NotImplementedError("icm SymmetricalTransFormer: only the reference's default architecture")
        self.pretrain_img_size = pretrain_img_size
        self.num_layers = len(depths)
        self.embed_dim = embed_dim
        self.patch_norm = patch_norm
        self.frozen_stages = frozen_stages
        self.num_slices = num_slices
        self.max_support_slices = num_slices // 2
        self.window_size = window_size
        self.drop_path_rate = drop_path_rate
        self.patch_embed = PatchEmbed(patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim,
                                      norm_layer=norm_layer if patch_norm else None)
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = [v.item() for v in torch.linspace(0, drop_path_rate, sum(depths))]
        self.layers = nn.ModuleList()
        for i in range(self.num_layers):
            self.layers.append(BasicLayer(
                dim=int(embed_dim * 2 ** i), depth=depths[i], num_heads=num_heads[i], window_size=window_size,
                mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop_rate, attn_drop=attn_drop_rate,
                drop_path=dpr[sum(depths[:i]):sum(depths[:i + 1])], norm_layer=norm_layer,
                downsample=PatchMerging if (i < self.num_layers - 1) else None, inverse=False))
        depths, num_heads = depths[::-1], num_heads[::-1]
        self.syn_layers = nn.ModuleList()
        for i in range(self.num_layers):
            self.syn_layers.append(BasicLayer(
                dim=int(embed_dim * 2 ** (3 - i)), depth=depths[i], num_heads=num_heads[i], window_size=window_size,
                mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop_rate, attn_drop=attn_drop_rate,
                drop_path=dpr[sum(depths[:i]):sum(depths[:i + 1])], norm_layer=norm_layer,
                downsample=PatchSplit if (i < self.num_layers - 1) else None, inverse=True))
        self.end_conv = nn.Sequential(Conv2d(embed_dim, embed_dim * patch_size ** 2, kernel_size=5, stride=1, padding=2),
                                      nn.PixelShuffle(patch_size),
                                      Conv2d(embed_dim, 3, kernel_size=3, stride=1, padding=1))
        self.num_features = [int(embed_dim * 2 ** i) for i in range(self.num_layers)]
        self.g_a = None
        self.g_s = None
        self.h_a = nn.Sequential(conv3x3(384, 384), nn.GELU(), conv3x3(384, 336), nn.GELU(),
                                 conv3x3(336, 288, stride=2), nn.GELU(), conv3x3(288, 240), nn.GELU(),
                                 conv3x3(240, 192, stride=2))

        def hs():
            return nn.Sequential(conv3x3(192, 240), nn.GELU(), subpel_conv3x3(240, 288, 2), nn.GELU(),
                                 conv3x3(288, 336), nn.GELU(), subpel_conv3x3(336, 384, 2), nn.GELU(),
                                 conv3x3(384, 384))
        self.h_mean_s = hs()
        self.h_scale_s = hs()

        def cc(extra):
            return nn.ModuleList(nn.Sequential(
                conv(384 + 32 * min(i + extra, 6 + extra), 224, stride=1, kernel_size=3), nn.GELU(),
                conv(224, 176, stride=1, kernel_size=3), nn.GELU(),
                conv(176, 128, stride=1, kernel_size=3), nn.GELU(),
                conv(128, 64, stride=1, kernel_size=3), nn.GELU(),
                conv(64, 32, stride=1, kernel_size=3)) for i in range(num_slices))
        self.cc_mean_transforms = cc(0)
        self.cc_scale_transforms = cc(0)
        self.lrp_transforms = cc(1)
        self.entropy_bottleneck = EntropyBottleneck(embed_dim * 4)
        self.gaussian_conditional = GaussianConditional(None)
        self._noise = None
        self._drops = None

    def inject_noise(self, noise: Optional[dict], drops: Optional[dict] = None):
        """testing hook: {"z","y"} U(-1/2,1/2) samples and {"<layer>.blocks.<j>": [2,B]} DropPath scales (train mode)"""
        self._noise, self._drops = noise, drops

    def init_weights(self):
        """stf.py:567-579"""
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=.02, a=-2.0, b=2.0)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.LayerNorm):
                nn.init.constant_(m.bias, 0)
                nn.init.constant_(m.weight, 1.0)

    def draw_drops(self, B: int, device, generator=None) -> Dict[str, torch.Tensor]:
        out = {}
        for k, r in stf_drop_path_rates(self.drop_path_rate).items():
            d = _draw_drop(r, B, device, generator)
            if d is not None:
                out[k] = d
        return out

    def forward(self, x, qstep=None, qmap=None):
        """``qstep``, ``qmap``: as for ``WACNN.forward``"""
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("SymmetricalTransFormer.forward expects [B,3,H,W]")
        each = self._forward_each(x, qstep, qmap)
        if each is not None:
            return each
        names, params = _named(self)
        dev = x.device
        steps, maps = self._forward_quality(x, qstep, qmap)
        x, pads = _pad_eval_input(x, self.training)
        nz = ny = drops = None
        if self.training:
            nz, ny = _train_noise(self._noise, x, 192, 384)
            drops = self._drops if self._drops is not None else self.draw_drops(x.shape[0], dev)
            drops = {k: v.to(dev, torch.float32).contiguous() for k, v in drops.items()}
        ns, ms, ws = self.num_slices, self.max_support_slices, self.window_size

        def runner(tape, xin, *ps):
            return stf_forward(tape, dict(zip(names, ps)), xin, nz, ny, drops, ns, ms, ws, steps=steps, qmap=maps)

        x_hat, y_lik, z_lik = E.tape_function(runner, [x.contiguous(), *params], self._pack_cache())
        return {"x_hat": _crop_eval_output(x_hat, pads), "likelihoods": {"y": y_lik, "z": z_lik}}

    @classmethod
    def from_state_dict(cls, state_dict):
        net = cls()
        net.load_state_dict(state_dict)
        return net

    def update(self, scale_table=None, force=False):
        """stf.py: same table refresh as the cnn model (cnn.py:133-138)"""
        return self._update_tables(scale_table, force)

    def _g_a(self, tape, P, x):
        return stf_analysis(tape, P, x, None, self.window_size)

    def _g_s(self, tape, P, y_hat):
        return stf_synthesis(tape, P, y_hat, None, self.window_size)


class SymmetricalTransFormer3(SymmetricalTransFormer):
    """``stf6`` of the reference's zoo (models/stf6.py:384-872): the stf analysis / synthesis transforms around a
    zigzag-ordered entropy model -- the latent is coded as 24 blocks (6 channel groups x 2 x 2 spatial halves,
    ``ZigzagSplits``), every block's mean is refined by a four-layer Swin stack (``mu_Swin``), up to 16 previous
    blocks condition the next.  Same module names and state-dict as the reference (``sigma_Swin`` / ``LRP_Swin`` are
    registered but unused by ``forward``, as there); inputs must be multiples of 128 (block maps are multiples of the
    4 x 4 window).  ``compress`` / ``decompress`` are not mirrored for this variant."""

    def __init__(self, pretrain_img_size=256, patch_size=2, in_chans=3, embed_dim=48, depths=[2, 2, 6, 2],
                 num_heads=[3, 6, 12, 24], window_size=4, num_slices=6, Mask_win_size=8, num_sliding=4, mlp_ratio=4.,
                 qkv_bias=True, qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.2,
                 norm_layer=nn.LayerNorm, patch_norm=True, frozen_stages=-1, use_checkpoint=False):
        if num_slices != 6:
            raise NotImplementedError("icm SymmetricalTransFormer3: only the reference's default architecture")
        super().__init__(pretrain_img_size, patch_size, in_chans, embed_dim, depths, num_heads, window_size, 12,
                         mlp_ratio, qkv_bias, qk_scale, drop_rate, attn_drop_rate, drop_path_rate, norm_layer, patch_norm,
                         frozen_stages, use_checkpoint)
        # re-register everything after syn_layers in the reference's order (stf6.py:465-621)
        tail = {}
        for name in ("end_conv", "h_a", "h_mean_s", "h_scale_s", "entropy_bottleneck", "gaussian_conditional"):
            tail[name] = getattr(self, name)
            delattr(self, name)
        for name in ("cc_mean_transforms", "cc_scale_transforms", "lrp_transforms"):
            delattr(self, name)
        self.num_slices = num_slices
        self.max_support_slices = STF6_SUPPORT
        self.Mask_win_size = Mask_win_size
        cs = 384 // num_slices
        rdepths = list(depths)[::-1]
        dpr = [v.item() for v in torch.linspace(0, drop_path_rate, sum(depths))]

        def refine_stacks(n):
            return nn.ModuleList(nn.ModuleList(BasicLayer(
                dim=cs, depth=rdepths[i], num_heads=STF6_MU_HEADS, window_size=window_size, mlp_ratio=mlp_ratio,
                qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop_rate, attn_drop=attn_drop_rate,
                drop_path=dpr[sum(rdepths[:i]):sum(rdepths[:i + 1])], norm_layer=norm_layer, downsample=None,
                inverse=True) for i in range(self.num_layers)) for _ in range(n))
        self.mu_Swin = refine_stacks(num_slices * 4)
        self.sigma_Swin = refine_stacks(num_slices)
        self.LRP_Swin = refine_stacks(num_slices)
        for name in ("end_conv", "h_a", "h_mean_s", "h_scale_s"):
            setattr(self, name, tail[name])

        def cc(extra):
            return nn.ModuleList(nn.Sequential(
                conv(cs + cs * min(i + extra, STF6_SUPPORT + extra), 224, stride=1, kernel_size=3), nn.GELU(),
                conv(224, 176, stride=1, kernel_size=3), nn.GELU(),
                conv(176, 128, stride=1, kernel_size=3), nn.GELU(),
                conv(128, 64, stride=1, kernel_size=3), nn.GELU(),
                conv(64, cs, stride=1, kernel_size=3)) for i in range(num_slices * 4))
        self.cc_mean_transforms2 = cc(0)
        self.cc_scale_transforms2 = cc(0)
        self.lrp_transforms2 = cc(1)
        self.entropy_bottleneck = tail["entropy_bottleneck"]
        self.gaussian_conditional = tail["gaussian_conditional"]

    def draw_drops(self, B: int, device, generator=None) -> Dict[str, torch.Tensor]:
        out = {}
        for k, r in stf6_drop_path_rates(self.drop_path_rate).items():
            d = _draw_drop(r, B, device, generator)
            if d is not None:
                out[k] = d
        return out

    def forward(self, x, qstep=None, qmap=None):
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("SymmetricalTransFormer3.forward expects [B,3,H,W]")
        if qmap is not None:
            raise ValueError("stf6 has no codec and so no quantiser step: it takes no quality map")
        if E.qstep_steps(qstep, x.shape[0], "cpu") is not None:
            raise ValueError("stf6 has no codec and so no quantiser step: qstep must be None or 0")
        if x.shape[2] % 128 or x.shape[3] % 128:
            raise ValueError("SymmetricalTransFormer3: image sides must be multiples of 128 (2 x 2 zigzag blocks of "
                             "4 x 4-window Swin maps at 1/16 resolution)")
        names, params = _named(self)
        dev = x.device
        nz = ny = drops = None
        if self.training:
            nz, ny = _train_noise(self._noise, x, 192, 384)
            B, hb, wb = x.shape[0], x.shape[2] // 32, x.shape[3] // 32
            ny = ny.reshape(B, 24, 64, hb, wb) if ny.dim() == 4 else ny.contiguous()   # iid noise: any layout is the same draw
            drops = self._drops if self._drops is not None else self.draw_drops(B, dev)
            drops = {k: v.to(dev, torch.float32).contiguous() for k, v in drops.items()}
        ws = self.window_size

        def runner(tape, xin, *ps):
            return stf6_forward(tape, dict(zip(names, ps)), xin, nz, ny, drops, ws)

        x_hat, y_lik, z_lik = E.tape_function(runner, [x.contiguous(), *params], self._pack_cache())
        return {"x_hat": x_hat, "likelihoods": {"y": y_lik, "z": z_lik}}

    def update(self, scale_table=None, force=False):
        return self._update_tables(scale_table, force)

    def compress(self, x, _debug=None, coder="host", symbols_per_wave=None, qstep=0, qmap=None, rdoq=None):
        raise NotImplementedError("stf6: the zigzag entropy coder loop (stf6.py:898-1057) is not mirrored")

    def compress_latent(self, y, _debug=None, coder="host", symbols_per_wave=None, qstep=0, qmap=None, rdoq=None):
        raise NotImplementedError("stf6: the zigzag entropy coder loop (stf6.py:898-1057) is not mirrored")

    def decompress(self, strings, shape, coder="host", qstep=0, qmap=None):
        raise NotImplementedError("stf6: the zigzag entropy coder loop (stf6.py:898-1057) is not mirrored")
