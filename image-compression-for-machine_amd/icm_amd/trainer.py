"""Data-parallel training step for the `cnn` codec -- the semantics of the reference loop
(train.py:188-214, configure_optimizers train.py:105-169) on the HIP engine, one process per GPU.

    optimizer.zero_grad(); aux_optimizer.zero_grad()
    out = model(x); loss = lmbda*255^2*mse + bpp; loss.backward()
    clip_grad_norm_(model.parameters(), clip); optimizer.step()          # Adam on non-".quantiles"
    aux = model.aux_loss(); aux.backward(); aux_optimizer.step()         # Adam(1e-4) on ".quantiles"

The reference has no distributed code; data parallelism is added here the MI355X
way: the batch is sharded over ranks, every parameter lives in ONE flat f32 buffer (so gradients are a
single contiguous buffer too), gradient ranges are sum-all-reduced over RCCL/xGMI on a side stream as soon as
the backward tape has passed the ops that produce them (4 large buckets, reverse topological order:
g_s -> slice chains -> hyper path -> g_a), and clip + Adam run as two fused kernels over the flat buffers
with the clip coefficient computed on the device (no host sync anywhere in the step).
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.distributed as dist

from . import _lib as L
from . import engine as E
from ._lib import check, ptr
from .bitstream import check_qstep, step_of
from .codec import AQ_STRENGTH_MAX
from .losses import qmap_lmbda_table
from .models import SymmetricalTransFormer, SymmetricalTransFormer3, stf6_forward, stf_forward, wacnn_forward

# bucket -> parameter-name prefixes, in the order their gradients complete during backward
# (synthesis transform | slice chains | hyper path | analysis transform); names of the cnn and the stf model
BUCKETS = [("g_s", "syn_layers", "end_conv"),
           ("cc_mean_transforms", "cc_scale_transforms", "lrp_transforms", "cc_mean_transforms2", "cc_scale_transforms2",
            "lrp_transforms2", "mu_Swin", "sigma_Swin", "LRP_Swin"),
           ("h_a", "h_mean_s", "h_scale_s", "entropy_bottleneck"), ("g_a", "patch_embed", "layers")]


class FlatParams:
    """All trainable tensors of a module re-homed into one flat buffer (views keep names/shapes)."""

    def __init__(self, model: torch.nn.Module, device):
        items = [(n, p) for n, p in model.named_parameters()]
        self.main = [(n, p) for n, p in items if not n.endswith(".quantiles")]
        self.aux = [(n, p) for n, p in items if n.endswith(".quantiles")]
        # order the main parameters bucket by bucket so every bucket is one contiguous range
        order: List[Tuple[str, torch.nn.Parameter]] = []
        self.bucket_ranges: List[Tuple[int, int]] = []
        off = 0
        used = set()
        for prefixes in BUCKETS:
            start = off
            for n, p in self.main:
                if n.split(".")[0] in prefixes:
                    order.append((n, p))
                    used.add(n)
                    off += (p.numel() + 3) // 4 * 4
            self.bucket_ranges.append((start, off))
        rest = [(n, p) for n, p in self.main if n not in used]
        if rest:
            start = off
            for n, p in rest:
                order.append((n, p))
                off += (p.numel() + 3) // 4 * 4
            self.bucket_ranges.append((start, off))
        self.main = order
        self.n_main = off
        self.p = torch.zeros(off, dtype=torch.float32, device=device)
        self.g = torch.zeros(off, dtype=torch.float32, device=device)
        self.m = torch.zeros(off, dtype=torch.float32, device=device)
        self.v = torch.zeros(off, dtype=torch.float32, device=device)
        self.views: Dict[str, torch.Tensor] = {}
        self.gviews: Dict[str, torch.Tensor] = {}
        o = 0
        for n, prm in self.main:
            k = prm.numel()
            v = self.p[o:o + k].view(prm.shape)
            v.copy_(prm.data.to(device))
            prm.data = v
            self.views[n] = v
            self.gviews[n] = self.g[o:o + k].view(prm.shape)
            o += (k + 3) // 4 * 4
        na = sum(p.numel() for _, p in self.aux)
        self.ap = torch.zeros(na, dtype=torch.float32, device=device)
        self.ag = torch.zeros(na, dtype=torch.float32, device=device)
        self.am = torch.zeros(na, dtype=torch.float32, device=device)
        self.av = torch.zeros(na, dtype=torch.float32, device=device)
        o = 0
        for n, prm in self.aux:
            k = prm.numel()
            v = self.ap[o:o + k].view(prm.shape)
            v.copy_(prm.data.to(device))
            prm.data = v
            self.views[n] = v
            self.gviews[n] = self.ag[o:o + k].view(prm.shape)
            o += k


class GradReducer:
    """Sum-all-reduce contiguous ranges of the flat gradient buffer on a side stream (RCCL over xGMI when
    the process group is NCCL; gloo works for CPU tests)."""

    def __init__(self, flat_g: torch.Tensor, ranges, group=None):
        self.g, self.ranges, self.group = flat_g, list(ranges), group
        inited = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(group) if inited else 1
        # ICM_FORCE_COLLECTIVES=1 (tests): run the collective path even in a 1-rank group, so that the side-stream
        # async all-reduce / event ordering / Work.wait() sequence executes on a single-GPU box under RCCL
        self.active = self.world > 1 or (inited and os.environ.get("ICM_FORCE_COLLECTIVES", "0") == "1")
        self.cuda = flat_g.is_cuda
        self.stream = torch.cuda.Stream() if (self.cuda and self.active) else None
        self.works = []
        self.launched = 0     # collectives issued (tests)

    def launch(self, bucket: int, after=()):
        """all-reduce bucket `bucket`; after: extra events (recorded on other streams, e.g. the weight-gradient side
        stream) the collective must wait for besides everything issued so far on the current stream"""
        if not self.active:
            return
        a, b = self.ranges[bucket]
        if b <= a:
            return
        t = self.g[a:b]
        self.launched += 1
        if self.cuda and dist.get_backend(self.group) == "gloo":
            # rehearsal path (several ranks sharing one GPU): stage through the host
            for e in after:
                e.synchronize()
            torch.cuda.current_stream().synchronize()
            h = t.cpu()
            dist.all_reduce(h, op=dist.ReduceOp.SUM, group=self.group)
            t.copy_(h)
            return
        if self.cuda:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            with torch.cuda.stream(self.stream):
                self.stream.wait_event(ev)
                for e in after:
                    self.stream.wait_event(e)
                self.works.append(dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group, async_op=True))
        else:
            self.works.append(dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group, async_op=True))

    def finish(self):
        for w in self.works:
            w.wait()
        self.works = []
        if self.stream is not None:
            torch.cuda.current_stream().wait_stream(self.stream)


def check_qstep_range(qstep_range) -> Tuple[int, int]:
    """(lo, hi) of a variable-rate training range: two step indexes (``bitstream.check_qstep``) with lo <= hi"""
    try:
        lo, hi = qstep_range
    except (TypeError, ValueError):
        raise ValueError(f"qstep_range: expected (lo, hi), got {qstep_range!r}")
    lo, hi = check_qstep(lo, "qstep_range: "), check_qstep(hi, "qstep_range: ")
    if lo > hi:
        raise ValueError(f"qstep_range: lo = {lo} > hi = {hi}")
    return lo, hi


def qstep_tables(qstep_range, lmbda: float, lmbda_exp: float = 2.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """The two tables a variable-rate step gathers from, entry i for step index k = lo + i (host f32 tensors):
    the (step, inv) pairs of ``bitstream.step_of`` [n, 2], and lmbda_k = lmbda * step_k^(-lmbda_exp) =
    lmbda * 2^(-k * lmbda_exp / 8), formed in double [n].  With the default exponent 2 the distortion term
    lmbda_k * D keeps its weight against the rate as the step grows, under the high-rate approximation D ~ step^2
    (a default, not a measured optimum)."""
    lo, hi = check_qstep_range(qstep_range)
    ks = range(lo, hi + 1)
    steps = torch.tensor([step_of(k) for k in ks], dtype=torch.float32)
    lam = torch.tensor([float(lmbda) * 2.0 ** (-k * float(lmbda_exp) / 8.0) for k in ks], dtype=torch.float64)
    return steps, lam.to(torch.float32)


QMAP_RECTS_MAX = 8


def check_qmap_rects(qmap_rects) -> int:
    """the rectangle count of quality-map training: an integer in 0..QMAP_RECTS_MAX (ValueError otherwise)"""
    if isinstance(qmap_rects, bool) or not isinstance(qmap_rects, int) and not hasattr(qmap_rects, "__index__"):
        raise ValueError(f"qmap_rects must be an integer, got {qmap_rects!r}")
    if not 0 <= int(qmap_rects) <= QMAP_RECTS_MAX:
        raise ValueError(f"qmap_rects = {int(qmap_rects)} outside [0, {QMAP_RECTS_MAX}]")
    return int(qmap_rects)


def check_qmap_aq(qmap_aq) -> Optional[Tuple[float, float]]:
    """(slo, hi) of AQ-map training: the range the per-image strength of variance-adaptive quantisation is drawn from,
    two real numbers, not bools, finite, with -AQ_STRENGTH_MAX <= slo <= shi <= AQ_STRENGTH_MAX (``codec.check_aq``'s
    limit), as Python floats.  None and (0, 0) mean off and come back as None.  ValueError otherwise."""
    if qmap_aq is None:
        return None
    try:
        slo, shi = qmap_aq
    except (TypeError, ValueError):
        raise ValueError(f"qmap_aq: expected (slo, shi), got {qmap_aq!r}")
    for v in (slo, shi):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or \
                not math.isfinite(float(v)):
            raise ValueError(f"qmap_aq: expected two finite numbers, got {qmap_aq!r}")
    slo, shi = float(slo), float(shi)
    if not -AQ_STRENGTH_MAX <= slo <= shi <= AQ_STRENGTH_MAX:
        raise ValueError(f"qmap_aq: need -{AQ_STRENGTH_MAX} <= slo <= shi <= {AQ_STRENGTH_MAX}, got ({slo}, {shi})")
    return (slo, shi) if slo or shi else None


def qmap_rects_of(u: torch.Tensor, h: int, w: int, lo: int, hi: int) -> torch.Tensor:
    """The rectangles of a draw: ``u`` [..., 5] uniform on [0, 1) -> int32 [..., 5] = (y0, x0, y1, x1, k), in cells of an
    h x w map, half open.  A pure function of its arguments that runs on the device of ``u``:
        y0 = min(floor(u0 h), h - 1)        y1 = y0 + 1 + min(floor(u2 (h - y0)), h - y0 - 1)
        x0 = min(floor(u1 w), w - 1)        x1 = x0 + 1 + min(floor(u3 (w - x0)), w - x0 - 1)
        k  = lo + min(floor(u4 (hi - lo + 1)), hi - lo)
    so every rectangle is non-empty and inside the map, the corner is uniform over the cells, the extent uniform over
    what fits from there, and k uniform on lo..hi.  (The minima only matter where a float32 product rounds up to its
    bound.)"""
    u = u.to(torch.float32)

    def cells(v, n):       # floor(v n) held to n - 1, as a float tensor of integers (exact: a map side is far below
        c = torch.floor(v * n)                                                   # 2^24); n an int or such a tensor
        return torch.minimum(c, n - 1) if torch.is_tensor(n) else c.clamp(max=n - 1)   # no constant goes to the device
    y0, x0 = cells(u[..., 0], h), cells(u[..., 1], w)
    y1 = y0 + 1 + cells(u[..., 2], h - y0)
    x1 = x0 + 1 + cells(u[..., 3], w - x0)
    k = lo + cells(u[..., 4], hi - lo + 1)
    return torch.stack([y0, x0, y1, x1, k], dim=-1).to(torch.int32)


class Trainer:
    def __init__(self, model, lr: float = 1e-4, aux_lr: float = 1e-4, lmbda: float = 0.0067,
                 clip_max_norm: float = 1.0, device="cuda:0", group=None, seed: int = 0, metric: str = "mse",
                 qstep_range=None, qstep_lmbda_exp: float = 2.0, qmap_rects: int = 0, qmap_aq=None):
        """``qstep_range`` = (lo, hi): variable-rate training -- every step draws a quantiser step index per image,
        uniform on lo..hi, from this rank's device generator (after the noise and DropPath draws, whose order and
        values it leaves alone), and trains the entropy model and the transforms at that step
        (``engine.gc_likelihood_ste(steps=...)``) with the distortion weight lmbda * step^(-qstep_lmbda_exp) of that
        image (``qstep_tables``).  None (default): today's step, launch for launch and draw for draw.
        ``qmap_rects`` = R in 1..8 (with ``qstep_range``): quality-map training -- every image and step gets its own map
        of step indexes over the latent positions.  The background is the index the step draws anyway (the same draw in
        the same place); ONE further draw from the same generator, uniform [B, R, 5], gives R rectangles per image
        (``qmap_rects_of``), painted in order over the background on the device (``icm_qmap_paint``).  The slice loop
        then trains with a step per position (``engine.gc_likelihood_ste(qmap=...)``) and every 16 x 16 cell of pixels
        weighs its distortion by lmbda * step^(-qstep_lmbda_exp) of its position (``icm_rd_loss_m_fwd/bwd``,
        ``losses.qmap_lmbda_table``).  0 (default): the ``qstep_range`` step, launch for launch.
        ``qmap_aq`` = (SLO, SHI) (``check_qmap_aq``; with ``qstep_range``): AQ-map training -- the map of every image is
        the one ``codec encode --aq S`` would make for that crop at the background index the step draws anyway: each
        cell's offset to it follows the variance of the cell's luma against the crop's mean (``codec.aq_offsets``),
        computed on the device inside the step (``icm_qmap_aq``, which takes the place of the ``icm_qmap_paint`` launch;
        no host sync).  The strength S_n = SLO + (SHI - SLO) u_n comes from ONE further draw, uniform [B], the step's
        last, so every earlier draw keeps its value; with ``qmap_rects`` the rectangles are drawn as they are without
        and win over the offsets, as in the codec.  Downstream is the map path of ``qmap_rects``, untouched (offsets
        may leave lo..hi: the weight table covers every step index).  None or (0, 0) (default): off, launch for launch
        and draw for draw."""
        self.qmap_rects = check_qmap_rects(qmap_rects)
        self.qmap_aq = check_qmap_aq(qmap_aq)
        if self.qmap_aq is not None:
            if qstep_range is None:
                raise ValueError("qmap_aq: quality-map training draws its step indexes from qstep_range; give one")
            if metric == "ms-ssim":
                raise ValueError("qmap_aq: the MS-SSIM loss takes a scalar lmbda; per-cell weights are mse only")
            if isinstance(model, SymmetricalTransFormer3):
                raise ValueError("qmap_aq: stf6 has no codec and so no quantiser step")
        if self.qmap_rects:
            if qstep_range is None:
                raise ValueError("qmap_rects: quality-map training draws its step indexes from qstep_range; give one")
            if metric == "ms-ssim":
                raise ValueError("qmap_rects: the MS-SSIM loss takes a scalar lmbda; per-cell weights are mse only")
            if isinstance(model, SymmetricalTransFormer3):
                raise ValueError("qmap_rects: stf6 has no codec and so no quantiser step")
        if metric not in ("mse", "ms-ssim"):
            raise NotImplementedError(f"{metric} is not implemented!")
        self.qstep_range, self.qstep_lmbda_exp = None, float(qstep_lmbda_exp)
        if qstep_range is not None:
            self.qstep_range = check_qstep_range(qstep_range)
            if metric == "ms-ssim":
                raise ValueError("qstep_range: the MS-SSIM loss takes a scalar lmbda; per-image weights are mse only")
            if isinstance(model, SymmetricalTransFormer3):
                raise ValueError("qstep_range: stf6 has no codec and so no quantiser step")
        self.metric = metric
        self.keep_loss_seed = False   # tests: keep (x_hat, dx_hat) of the last step in self.loss_seed
        self.loss_seed = None
        self._ms_ws = None   # ms-ssim: (input shape, workspace, per-plane values), allocated once per shape
        self.model = model.to(device).train()
        self.device = torch.device(device)
        self.flat = FlatParams(self.model, self.device)
        self.lr, self.aux_lr, self.lmbda, self.clip = lr, aux_lr, lmbda, clip_max_norm
        self.reducer = GradReducer(self.flat.g, self.flat.bucket_ranges, group)
        self.world = self.reducer.world
        self.rank = dist.get_rank(group) if self.reducer.active else 0
        # replicas start from rank 0's parameters (what DistributedDataParallel does at construction) ...
        if self.reducer.active:
            for buf in (self.flat.p, self.flat.ap):
                _broadcast0(buf, group)
        # ... but draw their OWN quantisation noise / DropPath masks: one generator per rank, seeded seed + rank
        # (identical noise on every rank would correlate the shards' gradients)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(int(seed) + self.rank)
        self.step_no = 0
        self.names = [n for n, _ in self.flat.main] + [n for n, _ in self.flat.aux]
        # [0:5] rd loss, [5] sqnorm, [6] aux, [7] 1 - ms_ssim (metric="ms-ssim")
        self.scal = torch.zeros(8, dtype=torch.float32, device=self.device)
        self.red_ws = torch.zeros(L.REDUCE_WS_FLOATS, dtype=torch.float32, device=self.device)  # fixed-order partial sums
        self.side = torch.cuda.Stream(device=self.device) if self.device.type == "cuda" else None
        self._side_ws = None
        import os as _os
        self.wg_every = int(_os.environ.get("ICM_WG_EVERY", "8"))
        self.wg_min = int(_os.environ.get("ICM_WG_MIN", "8"))
        if self.wg_every < 0:
            self.side = None
        self._eb = None
        self.hold_chain_wgrads = _os.environ.get("ICM_HOLD_CHAIN_WGRADS", "0") == "1"
        self._pack_seq = None     # weight-packing miss sequence of the first step (windowed batch packing afterwards)
        self.pack_window = int(_os.environ.get("ICM_PACK_WINDOW", "24"))
        self.is_stf = isinstance(model, SymmetricalTransFormer)
        self.is_stf6 = isinstance(model, SymmetricalTransFormer3)
        self.lat_ch = 384 if self.is_stf else 320
        self._maps = bool(self.qmap_rects) or self.qmap_aq is not None   # a step index per latent position
        self.loss_terms = None   # tests (keep_loss_seed, variable rate): likelihoods, drawn step indexes, weights
        if self.qstep_range is not None:   # built once; a step gathers from them on the device
            steps, lam = qstep_tables(self.qstep_range, lmbda, self.qstep_lmbda_exp)
            self._q_steps, self._q_lmbda = steps.to(self.device), lam.to(self.device)
        if self.qmap_rects or self.qmap_aq is not None:
            self._qm_lmbda = qmap_lmbda_table(lmbda, self.qstep_lmbda_exp).to(self.device)
        self._aq_bufs = None   # AQ-map training: (batch shape, ref f64 [B], workspace), allocated once per shape

    def params(self) -> Dict[str, torch.Tensor]:
        return self.flat.views

    def _draw_qsteps(self, B: int):
        """(table rows [B] int64, steps [B, 2], lmbda_n [B]) of one step: a step index per image, uniform on the range,
        from this rank's generator; gathered on the device, nothing comes back to the host"""
        rows = torch.randint(0, self._q_lmbda.numel(), (B,), device=self.device, generator=self.gen)
        return rows, self._q_steps.index_select(0, rows), self._q_lmbda.index_select(0, rows)

    def _draw_qmaps(self, B: int, h: int, w: int):
        """(table rows [B] int64, base [B] int8, rects [B, R, 5] int32) of one quality-map step: the background index of
        each image from the draw of ``_draw_qsteps``, then one more draw for the rectangles; all on the device.  With
        ``qmap_aq`` a fourth entry, the strengths [B] f32 of the step's last draw (and no rectangle draw where R = 0:
        ``rects`` is then empty)."""
        lo, hi = self.qstep_range
        rows = torch.randint(0, self._q_lmbda.numel(), (B,), device=self.device, generator=self.gen)
        if self.qmap_rects:
            u = torch.rand((B, self.qmap_rects, 5), dtype=torch.float32, device=self.device, generator=self.gen)
            rects = qmap_rects_of(u, h, w, lo, hi)
        else:
            rects = torch.empty((B, 0, 5), dtype=torch.int32, device=self.device)
        if self.qmap_aq is None:
            return rows, (rows + lo).to(torch.int8), rects
        slo, shi = self.qmap_aq
        u = torch.rand((B,), dtype=torch.float32, device=self.device, generator=self.gen)
        return rows, (rows + lo).to(torch.int8), rects, slo + (shi - slo) * u

    def _aq_buffers(self, B: int, H: int, W: int):
        """(ref f64 [B], workspace) of ``engine.qmap_aq`` for this batch shape, kept between steps"""
        if self._aq_bufs is None or self._aq_bufs[0] != (B, H, W):
            self._aq_bufs = ((B, H, W), torch.empty((B,), dtype=torch.float64, device=self.device),
                             E.qmap_aq_workspace(B, H, W, self.device))
        return self._aq_bufs[1], self._aq_bufs[2]

    def step_graphed(self, x: torch.Tensor) -> torch.Tensor:
        """step(x) replayed from a captured hipGraph: one host call per iteration instead of ~1 000 (cnn) to ~8 000
        (stf6) launches issued through Python.  The first two calls per input shape run eagerly (they record the
        weight-packing sequence and set kernel attributes); the third captures.  What changes from step to step lives
        in device memory the graph reads: the input batch, the quantisation noise and DropPath scales (drawn outside the
        graph from this rank's generator, in the same order as step() draws them), with ``qstep_range`` the steps and
        distortion weights of the images (drawn last, as in step(); with ``qmap_rects`` the background indexes and the
        rectangles instead, which the graph paints into its map buffer; with ``qmap_aq`` also the strengths, and the
        graph derives the maps from its input batch) and Adam's step-dependent scalars
        (icm_adam_step_hyper) -- so a replayed step equals the eager step bit for bit.  Single process only (the RCCL
        reductions are not captured); the side stream of the weight gradients is forked and joined inside the capture."""
        if self.world > 1:
            raise RuntimeError("step_graphed: single-process training only")
        key = tuple(x.shape)
        g = getattr(self, "_graph", None)
        if g is None or g["key"] != key:
            if getattr(self, "_graph_warm", None) != key:
                self._graph_warm, self._graph_warm_n = key, 0
            if self._graph_warm_n < 2:
                self._graph_warm_n += 1
                return self.step(x)
            g = self._capture(x)
        B, _, H, W = x.shape
        dev = self.device
        self.step_no += 1
        g["hyper"][0].copy_(torch.tensor(_adam_hyper(self.lr, self.step_no), dtype=torch.float32))
        g["hyper"][1].copy_(torch.tensor(_adam_hyper(self.aux_lr, self.step_no), dtype=torch.float32))
        # the same draws, in the same order, as step() makes (z noise, y noise, then the DropPath scales)
        g["nz"].copy_(torch.rand(g["nz"].shape, dtype=torch.float32, device=dev, generator=self.gen) - 0.5)
        g["ny"].copy_((torch.rand((B, self.lat_ch, H // 16, W // 16), dtype=torch.float32, device=dev,
                                  generator=self.gen) - 0.5).reshape(g["ny"].shape))
        if g["drops"] is not None:
            fresh = self.model.draw_drops(B, dev, generator=self.gen)
            for k, v in g["drops"].items():
                v.copy_(fresh[k])
        if g["qsteps"] is not None:   # variable rate: the step's last draw, gathered into the buffers the graph reads
            fresh = self._draw_qmaps(B, H // 16, W // 16) if self._maps else self._draw_qsteps(B)
            for buf, v in zip(g["qsteps"], fresh):   # (the map buffer, the last entry, is written by the graph)
                buf.copy_(v)
        g["x"].copy_(x)
        g["graph"].replay()
        E.bump_weight_generation()
        return self.scal

    def _capture(self, x: torch.Tensor):
        dev = self.device
        B, _, H, W = x.shape
        side = self.side
        if os.environ.get("ICM_GRAPH_SIDE", "1") == "0":
            self.side = None                       # weight gradients on the capture stream
        ny_shape = (B, 24, 64, H // 32, W // 32) if self.is_stf6 else (B, self.lat_ch, H // 16, W // 16)
        g = {"key": tuple(x.shape), "x": x.detach().clone().contiguous(),
             "nz": torch.zeros((B, 192, H // 64, W // 64), dtype=torch.float32, device=dev),
             "ny": torch.zeros(ny_shape, dtype=torch.float32, device=dev),
             "drops": None, "qsteps": None,
             "hyper": (torch.ones(2, dtype=torch.float32, device=dev), torch.ones(2, dtype=torch.float32, device=dev))}
        if self.qstep_range is not None:   # row 0 of the tables: valid steps for the capture run, replaced per replay
            rows = torch.zeros(B, dtype=torch.int64, device=dev)
            g["qsteps"] = (rows, self._q_steps.index_select(0, rows), self._q_lmbda.index_select(0, rows))
        if self.qmap_rects:   # background and one-cell rectangles at lo for the capture run, replaced per replay
            lo = self.qstep_range[0]
            rects = torch.tensor([0, 0, 1, 1, lo], dtype=torch.int32, device=dev).repeat(B, self.qmap_rects, 1)
            g["qsteps"] = (rows, torch.full((B,), lo, dtype=torch.int8, device=dev), rects.contiguous(),
                           torch.zeros((B, H // 16, W // 16), dtype=torch.int8, device=dev))
        if self.qmap_aq is not None:   # ... and strength 0 (a valid one) for the capture run; the maps stay last
            lo = self.qstep_range[0]
            rects = g["qsteps"][2] if self.qmap_rects else torch.empty((B, 0, 5), dtype=torch.int32, device=dev)
            g["qsteps"] = (rows, torch.full((B,), lo, dtype=torch.int8, device=dev), rects,
                           torch.zeros((B,), dtype=torch.float32, device=dev),
                           torch.zeros((B, H // 16, W // 16), dtype=torch.int8, device=dev))
            self._aq_buffers(B, H, W)   # allocated before the capture, not inside it
        if self.is_stf:
            gen_state = self.gen.get_state()       # shapes / keys only: the capture must not consume random numbers
            g["drops"] = {k: v.clone() for k, v in self.model.draw_drops(B, dev, generator=self.gen).items()}
            self.gen.set_state(gen_state)
        step_no = self.step_no
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self.step(g["x"], noise={"z": g["nz"], "y": g["ny"]}, drops=g["drops"], _hyper=g["hyper"],
                      _qsteps=g["qsteps"])
        self.step_no = step_no                      # nothing ran during capture
        self.side = side
        g["graph"] = graph
        self._graph = g
        return g

    def optimizer_state(self):
        """(optimizer, aux_optimizer) checkpoint entries (train.py:521-523): Adam moments per parameter NAME (independent
        of the flat-buffer layout), the step count and the learning rates"""
        f = self.flat

        def pack(items, m, v, pad):
            out_m, out_v, o = {}, {}, 0
            for n, prm in items:
                k = prm.numel()
                out_m[n] = m[o:o + k].view(prm.shape).detach().cpu().clone()
                out_v[n] = v[o:o + k].view(prm.shape).detach().cpu().clone()
                o += (k + 3) // 4 * 4 if pad else k
            return out_m, out_v
        m, v = pack(f.main, f.m, f.v, True)
        am, av = pack(f.aux, f.am, f.av, False)
        return ({"m": m, "v": v, "step": self.step_no, "lr": self.lr},
                {"m": am, "v": av, "step": self.step_no, "lr": self.aux_lr})

    def load_optimizer_state(self, opt, aux=None) -> None:
        f = self.flat

        def unpack(items, m, v, sd, pad):
            o = 0
            for n, prm in items:
                k = prm.numel()
                if n not in sd["m"] or tuple(sd["m"][n].shape) != tuple(prm.shape):
                    raise ValueError(f"optimizer state: missing or mis-shaped entry for {n}")
                m[o:o + k].view(prm.shape).copy_(sd["m"][n])
                v[o:o + k].view(prm.shape).copy_(sd["v"][n])
                o += (k + 3) // 4 * 4 if pad else k
        unpack(f.main, f.m, f.v, opt, True)
        self.step_no = int(opt["step"])
        self.lr = float(opt.get("lr", self.lr))
        if aux is not None:
            unpack(f.aux, f.am, f.av, aux, False)
            self.aux_lr = float(aux.get("lr", self.aux_lr))

    def step(self, x: torch.Tensor, noise: Optional[dict] = None, drops: Optional[dict] = None,
             _hyper: Optional[tuple] = None, _qsteps: Optional[tuple] = None) -> torch.Tensor:
        """one training iteration on this rank's shard x [B,3,H,W]; returns the device tensor
        [bpp, mse, loss, sumlog_y, sumlog_z, grad_sqnorm, aux_loss, ms_ssim_loss] (no host sync; the last entry is
        1 - ms_ssim with metric="ms-ssim" and 0 otherwise; loss is lmbda*255^2*mse + bpp or lmbda*(1 - ms_ssim) + bpp;
        with ``qstep_range`` it is 255^2 * mean_n(lmbda_n * mse_n) + bpp at the steps drawn, mse stays the plain mean).
        _hyper (step_graphed only): device tensors holding Adam's step-dependent scalars for the two optimisers;
        _qsteps (step_graphed only): the (rows, steps, lmbda_n) buffers of ``_draw_qsteps`` the graph reads, or with
        ``qmap_rects`` or ``qmap_aq`` the buffers of ``_draw_qmaps`` followed by the map buffer the graph writes."""
        f, dev = self.flat, self.device
        st = L.stream()
        lib = L.lib()
        if _hyper is None:
            self.step_no += 1
        B, _, H, W = x.shape
        if noise is None:
            nz = torch.rand((B, 192, H // 64, W // 64), dtype=torch.float32, device=dev, generator=self.gen) - 0.5
            ny = torch.rand((B, self.lat_ch, H // 16, W // 16), dtype=torch.float32, device=dev,
                            generator=self.gen) - 0.5
        else:
            nz, ny = noise["z"].to(dev).contiguous(), noise["y"].to(dev).contiguous()
        P = f.views
        tape = E.Tape(need_grad=True)
        tape.side, tape._side_ws, tape.progress_every = self.side, self._side_ws, self.wg_every
        tape.min_jobs = self.wg_min
        tape.stop(x)
        if self.pack_window > 0:
            if self._pack_seq is None:
                tape.pack_log = []
            else:
                tape.use_pack_sequence(self._pack_seq, self.pack_window)
        # Weights are packed just in time (Tape.pack), right before the GEMM that reads them: measured on MI355X,
        # packing all 600 MB up front (icm_pack_weights_batch) is 8 % slower end to end -- the packed fragments
        # fall out of the 256 MB Infinity Cache before they are used and the MFMA waves then wait on HBM.
        # gradients accumulate into the zeroed flat buffer: one 300 MB memset per step replaces the ~150 small
        # first-writer fills (attention tables, LayerNorm parameter sums, ...) that the stf model otherwise issues
        f.g.zero_()
        for n, _ in f.main:   # (the fused EntropyBottleneck backward overwrites its 13 small parameter gradients)
            tape.bind_grad(P[n], f.gviews[n], not n.startswith("entropy_bottleneck."))
        marks = {}
        if self.is_stf and drops is None:   # stochastic depth, drawn per step like timm's DropPath (stf.py:145)
            drops = self.model.draw_drops(B, dev, generator=self.gen)
        # variable rate: the LAST draw of the step, so that the noise and the DropPath scales are those of a plain step
        qs = maps = None
        aq_ref = None
        if self.qmap_aq is not None:   # ... followed by the rectangles' draw (R > 0), then the strengths'; the maps
            qs = _qsteps if _qsteps is not None else self._draw_qmaps(B, H // 16, W // 16)   # come from x, on the device
            maps = qs[4] if len(qs) > 4 else torch.empty((B, H // 16, W // 16), dtype=torch.int8, device=dev)
            aq_ref, aq_ws = self._aq_buffers(B, H, W)
            E.qmap_aq(x.contiguous(), qs[1], qs[3], qs[2] if self.qmap_rects else None, out=maps, ref=aq_ref, ws=aq_ws)
        elif self.qmap_rects:   # ... followed by the one draw of the rectangles; the maps are painted on the device
            qs = _qsteps if _qsteps is not None else self._draw_qmaps(B, H // 16, W // 16)
            maps = qs[3] if len(qs) > 3 else torch.empty((B, H // 16, W // 16), dtype=torch.int8, device=dev)
            check(lib.icm_qmap_paint(ptr(qs[1]), ptr(qs[2]), self.qmap_rects, ptr(maps), B, H // 16, W // 16, st),
                  "qmap_paint")
        elif self.qstep_range is not None:
            qs = _qsteps if _qsteps is not None else self._draw_qsteps(B)
        steps = None if qs is None or maps is not None else qs[1]
        if self.is_stf:
            drops = {k: v.to(dev, torch.float32).contiguous() for k, v in drops.items()}
            if self.is_stf6:   # zigzag blocks: iid noise, so any layout of the same draw is the same distribution
                ny6 = ny if ny.dim() == 5 else ny.reshape(B, 24, 64, H // 32, W // 32)
                x_hat, y_lik, z_lik = stf6_forward(tape, P, x, nz, ny6, drops, bucket_marks=marks)
            else:
                x_hat, y_lik, z_lik = stf_forward(tape, P, x, nz, ny, drops, bucket_marks=marks, steps=steps,
                                                  qmap=maps)
        else:
            x_hat, y_lik, z_lik = wacnn_forward(tape, P, x, nz, ny, bucket_marks=marks, steps=steps, qmap=maps)
        # ---- R-D loss forward + seeds (train.py:53-76)
        dxh, dly, dlz = E.new(x_hat), E.new(y_lik), E.new(z_lik)
        if maps is not None:   # a distortion weight per 16 x 16 cell: the map pair of reductions
            tab = self._qm_lmbda
            check(lib.icm_rd_loss_m_fwd(ptr(x), ptr(x_hat), B, 3, H, W, 16, ptr(maps), ptr(tab), ptr(y_lik),
                                        y_lik.numel(), ptr(z_lik), z_lik.numel(), B * H * W, ptr(self.scal),
                                        ptr(self.red_ws), st), "rd_loss_m_fwd")
            check(lib.icm_rd_loss_m_bwd(ptr(x), ptr(x_hat), B, 3, H, W, 16, ptr(maps), ptr(tab), ptr(y_lik),
                                        y_lik.numel(), ptr(z_lik), z_lik.numel(), B * H * W, 1.0, ptr(dxh), ptr(dly),
                                        ptr(dlz), st), "rd_loss_m_bwd")
        elif qs is not None:   # a distortion weight per image: the weighted pair of reductions
            lam = qs[2]
            check(lib.icm_rd_loss_w_fwd(ptr(x), ptr(x_hat), B, x[0].numel(), ptr(y_lik), y_lik.numel(), ptr(z_lik),
                                        z_lik.numel(), B * H * W, ptr(lam), ptr(self.scal), ptr(self.red_ws), st),
                  "rd_loss_w_fwd")
            check(lib.icm_rd_loss_w_bwd(ptr(x), ptr(x_hat), B, x[0].numel(), ptr(y_lik), y_lik.numel(), ptr(z_lik),
                                        z_lik.numel(), B * H * W, ptr(lam), 1.0, ptr(dxh), ptr(dly), ptr(dlz), st),
                  "rd_loss_w_bwd")
        else:
            # metric="ms-ssim": the fused reduction runs with lmbda = 0, i.e. loss = bpp and dx_hat = 0, as the rate part
            lm = self.lmbda if self.metric == "mse" else 0.0
            check(lib.icm_rd_loss_fwd(ptr(x), ptr(x_hat), x.numel(), ptr(y_lik), y_lik.numel(), ptr(z_lik),
                                      z_lik.numel(), B * H * W, lm, ptr(self.scal), ptr(self.red_ws), st), "rd_loss_fwd")
            check(lib.icm_rd_loss_bwd(ptr(x), ptr(x_hat), x.numel(), ptr(y_lik), y_lik.numel(), ptr(z_lik),
                                      z_lik.numel(), B * H * W, lm, 1.0, ptr(dxh), ptr(dly), ptr(dlz), st), "rd_loss_bwd")
        if self.metric == "ms-ssim":
            # loss += lmbda * (1 - ms_ssim(x_hat, x)) on the device; dx_hat = -lmbda * d ms_ssim / d x_hat overwrites
            # the zero the rate part left there
            if self._ms_ws is None or self._ms_ws[0] != tuple(x.shape):
                from .ops import msssim_workspace
                self._ms_ws = (tuple(x.shape), msssim_workspace(x),
                               torch.empty(B * x.shape[1], dtype=torch.float32, device=dev))
            _, mws, mpl = self._ms_ws
            xc = x.contiguous()
            # out = scal[6:8]: [7] keeps 1 - ms_ssim; [6] (the mean) is overwritten by the aux loss below
            check(lib.icm_msssim_fwd(ptr(x_hat), ptr(xc), B, x.shape[1], H, W, 1.0, ptr(mpl), ptr(self.scal[6:8]),
                                     self.lmbda, ptr(self.scal[2:3]), ptr(mws), mws.numel(), st), "msssim_fwd")
            check(lib.icm_msssim_bwd(ptr(x_hat), ptr(xc), B, x.shape[1], H, W, 0, -self.lmbda, ptr(dxh), ptr(mws),
                                     mws.numel(), st), "msssim_bwd")
        if self.keep_loss_seed:
            self.loss_seed = (x_hat.detach().clone(), dxh.clone())
            if maps is not None:
                self.loss_terms = {"y_lik": y_lik.detach().clone(), "z_lik": z_lik.detach().clone(),
                                   "qstep": qs[0] + self.qstep_range[0], "qmap": maps.clone(), "rects": qs[2].clone()}
                if aq_ref is not None:
                    self.loss_terms.update(aq=qs[3].clone(), aq_ref=aq_ref.clone())
            elif qs is not None:
                self.loss_terms = {"y_lik": y_lik.detach().clone(), "z_lik": z_lik.detach().clone(),
                                   "qstep": qs[0] + self.qstep_range[0], "lmbda_n": qs[2].clone()}
        tape.bind_grad(x_hat, dxh, True)
        tape.bind_grad(y_lik, dly, True)
        tape.bind_grad(z_lik, dlz, True)
        # ---- backward with bucketed all-reduce overlapped (markers fire as the tape unwinds)
        # bucket markers fire as the tape unwinds: flush the queued weight gradients, all-reduce the finished bucket.
        # ICM_HOLD_CHAIN_WGRADS=1 queues the 150 small slice-chain weight gradients between marker 0 (synthesis done)
        # and marker 1 (slice loop done) and issues them in ~15 launches of up to 32 same-geometry problems instead of
        # ~120 launches of 1-4: measured 0.7 % SLOWER on MI355X (same-box A/B, 258.9 vs 260.7 img/s) -- the early,
        # small launches fill CUs next to the latency-bound dgrad chain -- so the default keeps the periodic flush.
        def mark(b):
            if b == 1:
                tape.hold_wgrads = False
            if self.reducer.active:
                # the bucket is complete once the weight gradients queued so far have run on the side stream: the
                # COLLECTIVE waits for them (event on the side stream); the main stream's input-gradient chain does not
                # (round 2 joined the streams here, stalling backward at every bucket boundary)
                E.flush_wgrads(tape)
                after = ()
                if tape.side is not None:
                    ev = torch.cuda.Event()
                    ev.record(tape.side)
                    after = (ev,)
                self.reducer.launch(b, after)
            if b == 0 and self.hold_chain_wgrads:
                tape.hold_wgrads = True
        for name, idx in sorted(marks.items(), key=lambda kv: -kv[1]):
            tape.bw.insert(idx, (lambda b=name: mark(b)))
        tape.backward()
        self._side_ws = tape._side_ws
        if tape.pack_log is not None and self._pack_seq is None:
            self._pack_seq = tape.pack_log
        self.reducer.launch(len(BUCKETS) - 1)   # g_a: last gradients to complete (tape.backward() joined the side stream)
        if len(f.bucket_ranges) > len(BUCKETS):
            self.reducer.launch(len(BUCKETS))
        self.reducer.finish()
        # ---- clip (global L2 norm of the averaged gradients) + Adam, fused over the flat buffers
        gscale = 1.0 / self.world
        sq = self.scal[5:6]
        check(lib.icm_grad_sqnorm(ptr(f.g), f.n_main, ptr(sq), ptr(self.red_ws), st), "grad_sqnorm")
        if _hyper is None:
            check(lib.icm_adam_step(ptr(f.p), ptr(f.g), ptr(f.m), ptr(f.v), f.n_main, self.lr, 0.9, 0.999, 1e-8,
                                    self.step_no, ptr(sq) if self.clip > 0 else 0, float(self.clip), gscale, st), "adam")
        else:
            check(lib.icm_adam_step_hyper(ptr(f.p), ptr(f.g), ptr(f.m), ptr(f.v), f.n_main, 0.9, 0.999, 1e-8,
                                          ptr(_hyper[0]), ptr(sq) if self.clip > 0 else 0, float(self.clip), gscale, st),
                  "adam")
        # ---- aux loss on the UPDATED bottleneck weights, gradient to quantiles only (train.py:212-214)
        prm = E._eb_params(P, "entropy_bottleneck")
        t = math_target()
        check(lib.icm_eb_aux_loss(C.byref(prm), ptr(self.scal[6:7]), ptr(f.ag), 192, t, st), "eb_aux")
        if _hyper is None:
            check(lib.icm_adam_step(ptr(f.ap), ptr(f.ag), ptr(f.am), ptr(f.av), f.ap.numel(), self.aux_lr, 0.9, 0.999,
                                    1e-8, self.step_no, 0, 0.0, 1.0, st), "adam_aux")
        else:
            check(lib.icm_adam_step_hyper(ptr(f.ap), ptr(f.ag), ptr(f.am), ptr(f.av), f.ap.numel(), 0.9, 0.999, 1e-8,
                                          ptr(_hyper[1]), 0, 0.0, 1.0, st), "adam_aux")
        E.bump_weight_generation()   # packed-weight caches keyed before this step are stale now
        return self.scal


def _adam_hyper(lr: float, step: int):
    """the two step-dependent scalars of icm_adam_step, formed in double like torch.optim.Adam forms them"""
    import math
    return [lr / (1.0 - 0.9 ** step), math.sqrt(1.0 - 0.999 ** step)]


def _broadcast0(t: torch.Tensor, group=None):
    """in-place broadcast from rank 0 (RCCL for device tensors; through the host for the gloo rehearsal path)"""
    if t.is_cuda and dist.get_backend(group) == "gloo":
        h = t.cpu()
        dist.broadcast(h, src=0, group=group)
        t.copy_(h)
    else:
        dist.broadcast(t, src=0, group=group)


def math_target(tail_mass: float = 1e-9) -> float:
    import math
    return math.log(2 / tail_mass - 1)
