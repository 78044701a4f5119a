"""PLeaS: layer-wise least-squares fitting of the partially merged model.

Drop-in for the hot-path part of the reference's ``pleas/methods/pleas_merging.py``
(``get_gradient_mask`` :11-60, ``get_model_orig_activations`` :63-149, ``capture_inputs``
:197-231, ``step`` :234-302, ``train`` :305-405).

Objective (reference :281-284): for every Conv2d/Linear layer L of the merged model,
``mean((L(ip) - op)^2)`` where ``ip`` / ``op`` are the block-merged input / output activations
of the two source layers.  ``solver="adam"`` reproduces the reference's optimiser exactly
(Adam, lr 5e-4, cosine schedule, masked gradients, MAX_STEPS+1 updates); ``solver="normal_eq"``
minimises the same objective in closed form (normal equations + Cholesky), which is what
the Adam loop approximates.

MI355X design of one Adam step (13 ms for a ResNet-101 pair at batch 16)
  * the two frozen source forwards run once each, on two HIP streams side by side, under hooks that keep every
    layer's input AND output (the reference re-runs every source layer a second time, :113-114); between the hooked
    layers BatchNorm + residual add + ReLU are one ``pleas_bn_act`` pass (``source_forward.py``);
  * the merged inputs ``ip`` of ALL layers are assembled by ONE grouped launch (``pleas_merge_batch``; reference: 8
    ``index_select`` + 2 ``cat`` per layer);
  * forward, regression target, residual and loss of ALL merged layers are ONE grouped fp32-MFMA launch
    (``pleas_fwd_batch``): the target ``op`` is gathered / averaged from the source outputs inside its epilogue and
    never materialised, only the scaled residual ``2 (out - op) / numel`` and the loss partials are written;
  * the weight gradients of ALL merged layers are ONE grouped fp32-MFMA launch (``pleas_wgrad_batch``) that reads
    residuals and inputs in place from NCHW (autograd in the reference also back-propagates into both source layers);
  * all parameters, gradients, masks and Adam moments live in flat fp32 arenas (k x k weights kernel-position-major),
    so the masked Adam update of the whole model is ONE ``pleas_masked_adam`` launch and the data-parallel gradient
    exchange is one all-reduce.

Who owns what
  * ``frozen_sources.py``: the two source models, their taps and side streams, the queue of ``Generation``s (batch +
    ``SourceTaps``) whose forwards are in flight; ``data_parallel.py``: rank / world and every collective;
  * ``_LayerFitter``: what both solvers need -- the sources, the parameter arena ``p`` with its ``mask``, the ``plans``, the
    ``merge`` / ``wgrad`` batches, the update stream, the loop (``steps`` / ``step``), the generation being read (``gen``);
  * ``PleasFitter``: what Adam adds -- gradient arenas and per-plan gradient views, moments, schedule, losses, the
    grouped forward, and the ``_UpdateRecord`` a later update of the same shape replays (``_replay``);
  * ``NormalEqFitter`` (``normal_eq.py``): the ``A`` / ``B`` arenas and the solve, none of Adam's state.
"""
from __future__ import annotations

import contextlib
import math
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from .. import hip_ops
from ..core.utils import Axis, get_attr
from .data_parallel import _SPIN, _emulated_collective, _force_collectives, dp_all_gather_, dp_reduce_scatter_, dp_slice, dp_sum_  # noqa: F401
from .frozen_sources import (ActivationTap, FrozenSources, Generation, SourceTaps, TapDict, _TapView,  # noqa: F401
                             prepare_sources, tap_pointers)
from .partial_matching import block_maps, get_blocks, spread_blocks
from .source_forward import own_dwconv_ok


# ------------------------------------------------------------------------------------------ reference-shaped helpers
def get_gradient_mask(perm_blocks, model_weights: Dict[str, nn.Module]) -> List[torch.Tensor]:
    """One 0/1 mask per parameter of every layer in ``model_weights`` (reference :11-60).

    For >=2-D parameters two blocks are frozen.  The reference indexes them as
    ``mask[input_separate_1, output_separate_2] = 0`` and ``mask[input_separate_2,
    output_separate_1] = 0`` -- input slices on axis 0, output slices on axis 1 (:57-58) --
    and parity requires exactly that.  Axes missing from the spec fall back to 3 merged
    inputs / 1000 merged outputs (:31-37), i.e. no frozen block.
    """
    masks = []
    for name, layer in model_weights.items():
        frozen = _frozen_blocks(perm_blocks, name)
        for p in layer.parameters():
            mask = torch.ones_like(p)
            if p.dim() >= 2:
                for rows, cols in frozen:
                    mask[rows, cols] = 0.0
            masks.append(mask)
    return masks


def _frozen_blocks(perm_blocks, name: str):
    """The two (axis-0 slice, axis-1 slice) blocks of ``name.weight`` that stay frozen (reference :31-37, :57-58)."""
    bi = perm_blocks.get(Axis("%s.weight" % name, 1))
    bo = perm_blocks.get(Axis("%s.weight" % name, 0))
    ni, mi = (len(bi[0]), len(bi[2])) if bi is not None else (3, 0)
    no, mo = (len(bo[0]), len(bo[2])) if bo is not None else (1000, 0)
    return ((slice(ni, ni + mi), slice(no + mo, no + 2 * mo)), (slice(ni + mi, ni + 2 * mi), slice(no, no + mo)))


def _square_conv(mod: nn.Conv2d) -> bool:
    """Geometry the grouped HIP kernels take: dense, undilated, square kernel / stride / padding."""
    return (mod.groups == 1 and mod.dilation == (1, 1) and mod.stride[0] == mod.stride[1]
            and mod.padding[0] == mod.padding[1] and mod.kernel_size[0] == mod.kernel_size[1])


def cosine_lrs(base_lr: float, t_max: int, n: int) -> List[float]:
    """Learning rate used by update 0..n-1 under ``CosineAnnealingLR(T_max=t_max)`` stepped once
    per update, evaluated with torch's recursive form so the doubles match the reference
    (:358, :375)."""
    lrs, lr = [], base_lr
    for t in range(n):
        if t > 0:
            if (t - 1 - t_max) % (2 * t_max) == 0:
                lr = lr + base_lr * (1 - math.cos(math.pi / t_max)) / 2
            else:
                lr = (1 + math.cos(math.pi * t / t_max)) / (1 + math.cos(math.pi * (t - 1) / t_max)) * lr
        lrs.append(lr)
    return lrs


# ------------------------------------------------------------------------------------------ per-layer plan
class _LayerPlan:
    __slots__ = ("name", "mod", "is_conv", "w", "b", "gw", "gb", "gw2", "gb2", "halves", "w_shape", "off_w", "kpos", "dw")


def _identity_block(n: int):
    e = torch.empty(0, dtype=torch.long)
    return (torch.arange(n), torch.arange(n), e, e)


def _fallback_out_width(separate_classifier: bool, model_type: str, num_classes: int) -> int:
    if not separate_classifier:
        return num_classes
    widths = {"rn50": 2048, "rn101": 2048, "rn20": 1024, "rn18": 512}
    if model_type not in widths:
        raise ValueError("Unknown model type: %s" % model_type)
    return widths[model_type]


MERGING_MODES = ("perm_gradmask", "reg_mean", "perm_separatels", "perm_mixedls")


def merging_mode(merging: str) -> str:
    """The reference tests ``merging`` with ``==`` for reg_mean and with ``in`` for the two stacked modes
    (pleas_merging.py:125, :132, :139); everything else is the default channel-merged form (:146-147)."""
    if merging == "reg_mean":
        return "reg_mean"
    if "perm_separatels" in merging:
        return "perm_separatels"
    if "perm_mixedls" in merging:
        return "perm_mixedls"
    return "perm_gradmask"


def half_maps(mode: str, bi, bo, cin: int, cout_src: int, device):
    """Per HALF-BATCH ``(input maps, output maps)`` -- each ``(row1, row2, n_merged)`` as ``block_maps`` gives them -- of
    the layer's regression problem (reference :125-147).  ``perm_gradmask`` has one half: the channel-merged input and
    target.  The other modes stack TWO half-batches along the sample axis, which here are two entries of the grouped
    launches that share the layer's weights (their gradients are summed):
      reg_mean         [ip1 ; ip2] -> [o1 ; o2], no permutation (source widths)
      perm_separatels  [i11, i1c, 0 ; i22, 0, i2c]                 -> [o11, o1c, 0 ; o22, 0, o2c]
      perm_mixedls     [(i11+i22)/2, i1c, 0 ; (i11+i22)/2, 0, i2c] -> the same targets
    Absent blocks are -1 rows: the kernels write / gather zeros there."""
    i32 = lambda t: t.to(device=device, dtype=torch.int32)
    neg = lambda n: torch.full((int(n),), -1, dtype=torch.int32, device=device)
    if mode == "perm_gradmask":
        return [(block_maps(bi, device), block_maps(bo, device))]
    if mode == "reg_mean":
        ai, ao = torch.arange(cin, dtype=torch.int32, device=device), torch.arange(cout_src, dtype=torch.int32, device=device)
        return [((ai, neg(cin), 0), (ao, neg(cout_src), 0)), ((neg(cin), ai, 0), (neg(cout_src), ao, 0))]

    def side(b, which, averaged):
        b1, b2, b1c, b2c = (i32(t) for t in b)
        n = b1.numel() + b1c.numel() + b2c.numel()
        if which == 0:      # [x11 (or the average), x1c, 0]
            r1 = torch.cat([b1, b1c, neg(b2c.numel())])
            r2 = torch.cat([b2, neg(b1c.numel() + b2c.numel())]) if averaged else neg(n)
        else:               # [x22 (or the average), 0, x2c]
            r2 = torch.cat([b2, neg(b1c.numel()), b2c])
            r1 = torch.cat([b1, neg(b1c.numel() + b2c.numel())]) if averaged else neg(n)
        return r1.contiguous(), r2.contiguous(), (int(b1.numel()) if averaged else 0)

    mixed = mode == "perm_mixedls"
    return [(side(bi, h, mixed), side(bo, h, False)) for h in (0, 1)]


_pad4 = lambda n: (n + 3) // 4 * 4   # every tensor starts 16-byte aligned inside the arenas (vector loads)


class _LayerFitter:
    """What both solvers of the layer-wise objective share: the frozen sources, the flat parameter arena with its mask,
    the per-layer plans, and the loop that hands one tap generation to ``_step`` per batch."""

    def __init__(self, model1, model2, model3, spec, perm, costs, budget_ratios, max_steps: int, lr: float = 5e-4,
                 separate_classifier=False, num_classes=1000, model_type="rn50", data_parallel: bool = False,
                 fuse_sources: bool = True, overlap_sources: bool = True, fused_sources=None, sources: Optional[FrozenSources] = None,
                 merging: str = "perm_gradmask", shard_optimizer: Optional[bool] = None):
        """``lr`` and ``shard_optimizer`` are Adam's (``PleasFitter``); the closed form accepts and ignores them."""
        self.ops = hip_ops
        # data parallel: every update splits the batch's samples over the ranks, gradients (one flat
        # arena) are summed with ONE all-reduce, so all ranks apply the same full-batch update
        self.sources = sources if sources is not None else FrozenSources(
            model1, model2, data_parallel=data_parallel, fuse=fuse_sources, overlap=overlap_sources, fused=fused_sources)
        self.rank, self.world, self.device = self.sources.rank, self.sources.world, self.sources.device
        self.model1, self.model2, self.model3 = model1, model2, model3
        self.merging = merging_mode(merging)
        self.stacked = self.merging != "perm_gradmask"       # two half-batches per layer (reference :125-144)
        self.perm_blocks = spread_blocks(spec, get_blocks(spec, perm, costs, budget_ratios, False))
        # The update's own launches go to a dedicated stream, not to the caller's: measured on the 401-update job,
        # work on torch's default (null) stream overlaps the side streams markedly worse than work on a created stream
        # (8.24 s vs 7.73 s for the whole job).  step() orders that stream after the caller's and the caller's after it.
        self._upd_stream = hip_ops.role_stream(self.device, "updates") if self.sources._side_streams is not None else None
        self.gen: Optional[Generation] = None      # what the update being applied reads: its batch and source taps
        layers = {n: m for n, m in model3.named_modules() if isinstance(m, (nn.Conv2d, nn.Linear))}
        # The grouped HIP kernels take dense, undilated Conv2d layers with a square kernel / stride / padding (and Linear
        # layers on 2-D inputs) -- every layer of the ResNets the reference loads.  Any other geometry (rectangular, dilated or
        # grouped Conv2d; Linear on inputs with more than two axes) is fitted the way the reference fits EVERY layer
        # (`layer(ip)` under autograd, pleas_merging.py:281-287) on the vendor's operators, layer by layer (_fit_layer_vendor);
        # an update that contains such a layer takes the layer-by-layer path every time ("Layer geometries").
        # A depthwise layer (groups == channels) has kernels of its own (csrc/dwconv.hip) under ``hip_ops.depthwise_form("hip")``,
        # read here, once: it is taken when its planned merged input has as many channels as its weight has rows (``plan.dw``).
        self.layer_modules = layers
        self._lay_out_arenas(sum(_pad4(p.numel()) for m in layers.values() for p in m.parameters()), shard_optimizer)
        self.plans: List[_LayerPlan] = []
        off = 0
        for name, mod in layers.items():
            off = self._plan_layer(name, mod, off, (separate_classifier, model_type, num_classes))
        self.vendor_layers = [p.name for p in self.plans if p.is_conv and not _square_conv(p.mod) and not p.dw]
        self.wgrad = hip_ops.WgradBatch(self.device)
        self.dw_wgrad = hip_ops.DwWgradBatch(self.device)
        self.merge = hip_ops.MergeBatch(self.device)

    def _lay_out_arenas(self, total: int, shard_optimizer: Optional[bool]) -> None:      # the flat arenas all layers' tensors are views of
        self.p = torch.zeros(total, dtype=torch.float32, device=self.device)
        self.mask = torch.ones(total, dtype=torch.float32, device=self.device)   # frozen blocks are zeroed in _plan_layer

    def _plan_layer(self, name: str, mod: nn.Module, off: int, fallback: tuple) -> int:
        """Plan of one layer: its parameters copied into the arena from ``off`` on (returns where the next layer starts),
        its frozen blocks zeroed in the mask, and the block maps of its regression problem."""
        plan, dev = _LayerPlan(), self.device
        plan.name, plan.mod, plan.is_conv = name, mod, isinstance(mod, nn.Conv2d)
        plan.b = plan.gw = plan.gb = plan.gw2 = plan.gb2 = None
        # k x k convolutions with Cin % 32 == 0 keep their weight (gradient, mask, Adam state) KERNEL-POSITION-MAJOR
        # [Cout][KH][KW][Cin] in the arenas: the fused forward then has one tap per K chunk, the weight-gradient
        # kernel writes that layout directly, and the elementwise optimiser does not care (finish() permutes back)
        plan.kpos = bool(plan.is_conv and _square_conv(mod) and mod.kernel_size[0] > 1
                         and mod.weight.shape[1] % 32 == 0)   # the tensor's width: module attributes may be stale
        for pname, prm in mod.named_parameters():
            n = prm.numel()
            kp = plan.kpos and pname == "weight"
            shape = (prm.shape[0], prm.shape[2], prm.shape[3], prm.shape[1]) if kp else tuple(prm.shape)
            # model3 may live on the host: move first, permute on the device (a strided copy of a 3x3 weight on the CPU
            # costs milliseconds), and write the mask's frozen blocks straight into the arena
            src = prm.detach().to(dev, non_blocking=True)
            view = self.p[off:off + n].view(shape)
            view.copy_(src.permute(0, 2, 3, 1) if kp else src)
            if prm.dim() >= 2:
                mview = self.mask[off:off + n].view(shape)
                for rows, cols in _frozen_blocks(self.perm_blocks, name):
                    mview[(rows, slice(None), slice(None), cols) if kp else (rows, cols)] = 0.0
            if pname == "weight":
                plan.w, plan.w_shape, plan.off_w = view, tuple(prm.shape), off
            else:
                plan.b = view
            off += _pad4(n)
        src = get_attr(self.model1, name.split("."))
        cin = src.in_channels if plan.is_conv else src.in_features
        bi = self.perm_blocks.get(Axis("%s.weight" % name, 1)) or _identity_block(cin)
        bo = self.perm_blocks.get(Axis("%s.weight" % name, 0)) or _identity_block(_fallback_out_width(*fallback))
        cout_src = src.out_channels if plan.is_conv else src.out_features
        plan.halves = half_maps(self.merging, bi, bo, cin, cout_src, dev)
        plan.dw = bool(plan.is_conv and own_dwconv_ok(mod) and all(im[0].numel() == plan.w_shape[0] for im, _ in plan.halves))
        self.plans.append(plan)
        return off

    def _begin_update(self, x: torch.Tensor, next_x: Optional[torch.Tensor]) -> None:
        """Taps of ``x`` become current (running its sources now unless they were prefetched); the sources of
        ``next_x`` are enqueued BEFORE this update's own kernels, so that they overlap them on the side streams."""
        sources, queue = self.sources, self.sources.queue
        if queue and queue[0].batch is not x:
            raise RuntimeError("PleasFitter.step: a different batch was prefetched than the one passed now")
        self.gen = queue.popleft() if queue else Generation(x, sources.launch(x))
        if next_x is not None and not queue and sources._side_streams is not None:
            sources.enqueue(next_x)
        main = torch.cuda.current_stream(self.device)
        for ev in self.gen.taps.events or ():
            main.wait_event(ev)

    def _end_update(self) -> None:
        # the device copy of the batch was read on the side streams: it is released only now, after this update's
        # kernels (which waited for those streams) are enqueued on the stream that owns its memory
        self.gen = None

    @contextlib.contextmanager
    def _session(self):
        """Make the fitter's own stream current; order it after the caller's stream on entry and the caller's after it
        on exit (so results are visible to whatever the caller enqueues next)."""
        upd = self._upd_stream
        if upd is None or torch.cuda.current_stream(self.device) == upd:
            yield
            return
        caller = torch.cuda.current_stream(self.device)
        upd.wait_stream(caller)
        try:
            with torch.cuda.stream(upd):
                yield
        finally:
            caller.wait_stream(upd)

    def steps(self, batches, lookahead: Optional[bool] = None, sources_per_forward: Optional[int] = None):
        """Run one update per tensor of ``batches``; yields the index of each finished update.  Between two updates the
        consumer's code runs on ITS OWN current stream, ordered after the update just applied (the fitter's stream is
        entered and left per update).

        Up to ``sources_per_forward`` consecutive batches of equal shape (1: every batch on its own) go through the
        frozen sources as ONE forward of the concatenated batch, and the updates read their slices (views) of its taps --
        the sources are in eval mode, so every sample's activations are what a separate forward gives (up to the vendor
        kernels' rounding at another batch size) and the update order is unchanged.  ResNet-101 pair, 16 samples per
        update: 6.6 ms of source forwards per update one by one, 6.2 ms in pairs, and the host dispatches them once per
        group (whole job 7.22 -> 6.94 s).  Groups of four bring nothing more (7.05 s) and every new batch size costs the
        vendor library its first-use set-up, so the default is two per rank: ``2 * world`` under data parallelism, where an
        update's share is ``batch / world`` samples -- the source forward then has the same size for every ``world``, and its
        ~5 ms of host dispatch (which bounds a rank at 6.8 ms per update when every update forwards its own 2 samples,
        ``tools/probe_dp_rank.py``) is paid once per group.  What is left when ``batches`` runs out forms one smaller group
        (a single left-over batch goes alone), so a job meets at most three forward shapes.

        ``lookahead=True``: the source forwards of the NEXT group (or batch) are enqueued before the current group's updates
        and run beside them on the side streams (two tap generations in flight).  On one GPU the update kernels already
        fill the chip: -3 % wall-clock (7.96 s vs 8.19 s, ungrouped) while every grouped kernel takes longer because it
        shares the CUs (fused forward 2.9 -> 4.3 ms per launch), so it is off there and per-kernel timings stay
        interpretable.  Under data parallelism (the default then) the stream that applies the updates idles during every
        gradient all-reduce, and the prefetched source forwards are what fills those gaps."""
        group = max(1, int(2 * self.world if sources_per_forward is None else sources_per_forward))
        if lookahead is None:
            lookahead = self.world > 1
        keep = group if lookahead else 0      # sources are launched whenever no more than `keep` generations are queued
        sources, queue = self.sources, self.sources.queue
        it = iter(batches)
        for gen in list(queue):               # forwards enqueued beforehand (FrozenSources.prefetch): same batches first
            if next(it, None) is not gen.batch:
                raise RuntimeError("PleasFitter.steps: the prefetched batches must be the first ones, in order")
        ahead: List[torch.Tensor] = []        # fetched from `it`, sources not launched yet
        exhausted = False
        idx = 0
        while True:
            # The fitter's stream is current while an update is put together and ONLY then: the session is entered and left
            # per update, so a consumer that breaks out of (or raises inside) the loop is on its own stream, ordered after
            # the updates it has seen -- nothing is left to a generator's finalisation.
            with self._session():
                while len(queue) <= keep:
                    while len(ahead) < 2 * group and not exhausted:      # one group to launch, one whose copies start now
                        nxt = next(it, None)
                        if nxt is None:
                            exhausted = True
                        else:
                            ahead.append(nxt)
                    if not ahead:
                        break
                    run = [ahead[0]]
                    for cand in ahead[1:group]:
                        if torch.is_tensor(cand) and torch.is_tensor(run[0]) and cand.shape == run[0].shape and cand.shape[0] > 0:
                            run.append(cand)
                        else:
                            break
                    if group > 1 and (len(run) == group or (exhausted and len(run) > 1 and len(run) == len(ahead))):
                        # a full group -- or, when the batches have run out, what is left of one (one more forward size,
                        # instead of one forward per left-over batch)
                        sources.launch_group(run)      # one generation per batch of the run
                        del ahead[:len(run)]
                    else:
                        sources.enqueue(ahead.pop(0))
                    sources.stage(ahead[:group])
                if not queue:
                    break
                self.step(queue[0].batch)
            yield idx
            idx += 1

    @torch.no_grad()
    def step(self, x: torch.Tensor, next_x: Optional[torch.Tensor] = None) -> None:
        """One update: reference ``step`` (:234-302) + ``lr_sched.step()`` (:375).  ``next_x`` (optional): the batch
        of the NEXT call; its source forwards are enqueued now and run beside this update.  On return the work is
        ordered before anything enqueued later on the caller's stream.  ``_step`` is the solver's: it begins with
        ``_begin_update`` and ends with ``_end_update``."""
        with self._session():
            self._step(x, next_x)

    def finish(self) -> nn.Module:
        """Write the fitted weights back into ``model3`` and drop the hooks (reference :392-403)."""
        sd = self.model3.state_dict()
        for plan in self.plans:
            sd["%s.weight" % plan.name] = (plan.w.detach().permute(0, 3, 1, 2) if plan.kpos else plan.w.detach()).clone()
            if plan.b is not None:
                sd["%s.bias" % plan.name] = plan.b.detach().clone()
        self.model3.load_state_dict(sd)
        self.sources.close()
        return self.model3


class _UpdateRecord:
    """What the layer-by-layer path of ONE update set up, and all that a later update of the same input shape needs in order
    to repeat it with other tap addresses.  ``_fit_layer`` / ``_fit_layer_vendor`` write here; ``_replay_update`` reads
    nothing else."""

    __slots__ = ("key", "bufs", "names", "fwd_rows", "fwd_loss", "fwd_index", "bias_grads", "vendor_losses", "merge_tab", "fwd_tab", "complete",
                 "merged", "dw_rows", "dw_loss", "dw_index", "dw_tab", "fwd_pos", "dw_pos")

    def __init__(self, key: tuple, bufs: dict):
        self.key, self.bufs = key, bufs    # input shape (_update_key); (layer, half-batch) -> (merged input, residual) of that shape
        # per entry of the grouped forward its plan's index; (residual, plan, bias gradient); vendor layers' (plan index, loss)
        self.fwd_rows, self.bias_grads, self.vendor_losses = [], [], []
        # depthwise layers: per entry of THEIR grouped forward its plan's index; `merged`: per entry of the grouped merge (dense and
        # depthwise entries in layer order) its plan's index and whether it is a depthwise one
        self.dw_rows, self.merged = [], []
        self.names = self.fwd_loss = self.fwd_index = self.merge_tab = self.fwd_tab = None
        self.dw_loss = self.dw_index = self.dw_tab = self.fwd_pos = self.dw_pos = None
        self.complete = bool(key)          # replayable: every layer went through the grouped launches and their tables agree


class PleasFitter(_LayerFitter):
    """State of one PLeaS run: flat arenas + per-layer plans.  ``train`` drives it; the bench uses it directly to time single steps."""

    def __init__(self, model1, model2, model3, spec, perm, costs, budget_ratios, max_steps: int, lr: float = 5e-4, *args, **kwargs):
        super().__init__(model1, model2, model3, spec, perm, costs, budget_ratios, max_steps, lr, *args, **kwargs)
        # per-plan gradients: the views of the gradient arenas at the place the parameter has in `p`
        like = lambda arena, t: None if arena is None or t is None else \
            arena[t.storage_offset():t.storage_offset() + t.numel()].view(t.shape)
        for plan in self.plans:
            plan.gw, plan.gb, plan.gw2, plan.gb2 = like(self.g, plan.w), like(self.g, plan.b), like(self.g2, plan.w), like(self.g2, plan.b)
        self.lrs = cosine_lrs(lr, max_steps, max_steps + 1)
        self.step_count = 0
        self.loss_now = self._g_ext[self.p.numel():]                                             # this step, per layer
        self.loss_sum = torch.zeros(len(self.plans), dtype=torch.float32, device=self.device)   # since last report
        self.fwd = self.ops.FwdBatch(self.device)
        self.dw_fwd = self.ops.DwFwdBatch(self.device)
        # Per input shape: the merged inputs and residuals of every layer live in buffers that are kept between updates
        # (written and read on the update stream only), so the item tables of the three grouped launches change between
        # two updates of that shape in the tap addresses alone -- see _step.
        self._buffers: Dict[tuple, Dict[tuple, Tuple[torch.Tensor, torch.Tensor]]] = {}
        self._loss_bufs: Dict[tuple, Tuple[torch.Tensor, torch.Tensor]] = {}    # forward rows -> (their losses, their plan indices)
        self._replay: Optional[_UpdateRecord] = None      # the latest update's record, if complete
        self.fast_updates = 0    # updates applied by patching the tables (the rest took the layer-by-layer path)

    def _lay_out_arenas(self, total: int, shard_optimizer: Optional[bool]) -> None:
        # shard_optimizer (data parallel; default ON there since round 4, DESIGN.md section 5: the per-update exchange is as
        # long as a rank's per-update compute, so nothing that does not shrink with the ranks may stay on the update's
        # path): rank r keeps the Adam moments of -- and applies the update to -- the r-th
        # 1/world slice of the flat arena only: reduce-scatter of the gradients, Adam on the slice, all-gather of the
        # parameters.  Same bytes on the links as the all-reduce, 1/world of the optimiser's work and state per rank.
        self.shard_optimizer = (shard_optimizer is None or bool(shard_optimizer)) and (self.world > 1 or _force_collectives())
        if self.shard_optimizer:
            total = (total + 4 * self.world - 1) // (4 * self.world) * (4 * self.world)    # equal, 16-byte aligned slices
        self._shard = total // self.world if self.shard_optimizer else total
        super()._lay_out_arenas(total, shard_optimizer)
        dev = self.device
        # the gradient arena carries this update's per-layer losses in its tail: ONE collective per update sums both
        self._g_ext = torch.zeros(total + len(self.layer_modules), dtype=torch.float32, device=dev)
        self.g = self._g_ext[:total]
        # stacked modes: the second half-batch's weight gradients land in an arena of their own (two entries of one grouped
        # launch must not write the same tensor) and are added before the exchange / the optimiser
        self.g2 = torch.zeros(total, dtype=torch.float32, device=dev) if self.stacked else None
        self.m = torch.zeros(self._shard, dtype=torch.float32, device=dev)     # this rank's slice only when sharded
        self.v = torch.zeros(self._shard, dtype=torch.float32, device=dev)
        self._g_shard = torch.zeros(self._shard, dtype=torch.float32, device=dev) if self.shard_optimizer else None

    # -- one layer: merged input; queue forward(+target+residual+loss) and weight gradient for the grouped launches
    def _fit_layer(self, idx: int, plan: _LayerPlan, rec: _UpdateRecord) -> None:
        ops, name, mod, cout = self.ops, plan.name, plan.mod, plan.w_shape[0]
        ip1, ip2 = (t[name] for t in self.gen.taps.inputs)
        o1, o2 = (t[name] for t in self.gen.taps.outputs)
        if plan.dw:
            self._fit_layer_depthwise(idx, plan, rec)
            return
        if not (_square_conv(mod) if plan.is_conv else ip1.dim() == 2):
            self._fit_layer_vendor(idx, plan, rec)
            return
        geo = (tuple(mod.kernel_size), mod.stride[0], mod.padding[0]) if plan.is_conv else ((1, 1), 1, 0)
        # a 1x1 convolution with a stride reads every s-th pixel of every s-th line: the grouped merge writes exactly those, and
        # the layer is a dense 1x1 stride-1 layer for the forward and the weight gradient (16-byte loads along the pixel axis
        # instead of 4-byte loads at a stride; ResNet-101's three downsample layers: 52 -> ~100 TFLOP/s in the grouped forward)
        sub = geo[1] if (plan.is_conv and geo[0] == (1, 1) and geo[1] > 1 and geo[2] == 0) else 1
        if sub > 1:
            geo = ((1, 1), 1, 0)
        for h, (in_maps, (r1, r2, nm)) in enumerate(plan.halves):
            if cout != r1.numel():
                raise RuntimeError("layer %s: %d merged outputs vs %d target blocks" % (name, cout, r1.numel()))
            if in_maps[0].numel() != plan.w_shape[1]:
                raise RuntimeError("layer %s: %d merged inputs vs %d input blocks" % (name, plan.w_shape[1], in_maps[0].numel()))
            # merged input: queued for the ONE grouped merge launch that precedes the grouped forward (merge.flush)
            kept = rec.bufs.get((idx, h))
            ip = self.merge.add(ip1, ip2, 1, *in_maps, out=kept[0] if kept else None, subsample=sub)
            resid = kept[1] if kept else torch.empty((ip.shape[0], cout) + tuple(o1.shape[2:]), dtype=torch.float32,
                                                     device=ip.device)
            if kept is None:
                rec.bufs[(idx, h)] = (ip, resid)
            n = resid.numel() * len(plan.halves) * self.world    # the mean runs over the full (global, stacked) batch
            self.fwd.add(ip, plan.w, plan.b, o1, o2, r1, r2, nm, resid, 2.0 / n, 1.0 / n, *geo,
                         flags=ops.FwdBatch.KPOS_MAJOR if plan.kpos else 0)
            rec.fwd_rows.append(idx)
            rec.merged.append((idx, False))
            gw, gb = (plan.gw, plan.gb) if h == 0 else (plan.gw2, plan.gb2)   # second half: its own arena, added before the exchange
            # every layer, the 3-channel stem included (its rows are (channel, tap) pairs: "virtual channels", csrc/conv.hip)
            self.wgrad.add(resid, ip, gw, *geo, flags=ops.WgradBatch.KPOS_MAJOR if plan.kpos else 0)
            if gb is not None:
                rec.bias_grads.append((resid, plan, gb))

    def _fit_layer_depthwise(self, idx: int, plan: _LayerPlan, rec: _UpdateRecord) -> None:
        """A depthwise layer under ``depthwise_form("hip")``: its merged input joins the grouped merge like any dense layer's; forward,
        target, residual and loss go to ``DwFwdBatch``, the weight gradient to ``DwWgradBatch`` (csrc/dwconv.hip)."""
        name, mod, cout = plan.name, plan.mod, plan.w_shape[0]
        ip1, ip2 = (t[name] for t in self.gen.taps.inputs)
        o1, o2 = (t[name] for t in self.gen.taps.outputs)
        stride, pad = mod.stride[0], mod.padding[0]
        for h, (in_maps, (r1, r2, nm)) in enumerate(plan.halves):
            if cout != r1.numel():
                raise RuntimeError("layer %s: %d merged outputs vs %d target blocks" % (name, cout, r1.numel()))
            kept = rec.bufs.get((idx, h))
            ip = self.merge.add(ip1, ip2, 1, *in_maps, out=kept[0] if kept else None)
            resid = kept[1] if kept else torch.empty((ip.shape[0], cout) + tuple(o1.shape[2:]), dtype=torch.float32, device=ip.device)
            if kept is None:
                rec.bufs[(idx, h)] = (ip, resid)
            n = resid.numel() * len(plan.halves) * self.world    # the mean runs over the full (global, stacked) batch
            self.dw_fwd.add(ip, plan.w, plan.b, o1, o2, r1, r2, nm, resid, 2.0 / n, 1.0 / n, stride, pad)
            rec.dw_rows.append(idx)
            rec.merged.append((idx, True))
            gw, gb = (plan.gw, plan.gb) if h == 0 else (plan.gw2, plan.gb2)
            self.dw_wgrad.add(resid, ip, gw, stride, pad)
            if gb is not None:
                rec.bias_grads.append((resid, plan, gb))

    def _fit_layer_vendor(self, idx: int, plan: _LayerPlan, rec: _UpdateRecord) -> None:
        """A layer the grouped kernels do not take, fitted as the reference fits every layer (pleas_merging.py:116-147, :281-287):
        merged input and target by ``pleas_merge_blocks``, then ``layer(ip)``, the MSE and its gradients on the vendor's operators
        under autograd.  Gradients land in the same arena (mask and Adam are shared with all other layers); the loss joins
        ``loss_now`` after the grouped forward's."""
        ops, name, mod = self.ops, plan.name, plan.mod
        ip1, ip2 = (t[name] for t in self.gen.taps.inputs)
        o1, o2 = (t[name] for t in self.gen.taps.outputs)
        for h, (in_maps, out_maps) in enumerate(plan.halves):
            axis = 1 if plan.is_conv else ip1.dim() - 1      # channels: axis 1 of a feature map, the last axis of a Linear input
            ip = ops.merge_blocks(ip1, ip2, axis, *in_maps)
            op = ops.merge_blocks(o1, o2, axis, *out_maps)
            with torch.enable_grad():
                w = plan.w.detach().requires_grad_(True)
                b = plan.b.detach().requires_grad_(True) if plan.b is not None else None
                if plan.is_conv:
                    out = F.conv2d(ip, w, b, mod.stride, mod.padding, mod.dilation, mod.groups)
                else:
                    out = F.linear(ip, w, b)
                n = out.numel() * len(plan.halves) * self.world      # the mean runs over the full (global, stacked) batch
                loss = ((out - op) ** 2).sum() / n
                grads = torch.autograd.grad(loss, [w] + ([b] if b is not None else []))
            gw, gb = (plan.gw, plan.gb) if h == 0 else (plan.gw2, plan.gb2)
            gw.copy_(grads[0])
            if b is not None:
                gb.copy_(grads[1])
            rec.vendor_losses.append((idx, loss.detach()))
        rec.complete = False      # no table to replay: the next update goes layer by layer again

    def _bias_gradients(self, rec: _UpdateRecord) -> None:
        for resid, plan, gb in rec.bias_grads:      # HIP: one deterministic row-sum launch per biased layer
            self.ops.channel_sum(resid if resid.dim() > 1 else resid.reshape(1, -1), gb)

    def _update_key(self) -> tuple:
        first, taps = self.plans[0].name, self.gen.taps.taps1[0]
        if first not in taps:
            return ()
        n = (taps.hi - taps.lo) if isinstance(taps, _TapView) else taps[first].shape[0]
        return (n,) + tuple(self.gen.taps.x.shape[1:])

    def _step(self, x: torch.Tensor, next_x: Optional[torch.Tensor]) -> None:
        """One update.  The first update of an input shape goes layer by layer (_record_update: checks, buffers, item tables
        of the three grouped launches).  Every further update of that shape differs from it in the addresses of the source
        taps alone, so it rewrites those four pointer columns (numpy, from one address table per source forward) and
        launches again (_replay_update): ~2.3 ms -> ~0.5 ms of host time per update, which is what bounds a rank once its
        share of an update is a few samples."""
        self._begin_update(x, next_x)
        key = self._update_key()
        rec = self._replay if (self._replay is not None and key and self._replay.key == key) else None
        ptrs = None
        if rec is not None:
            ptrs = [tap_pointers(t, rec.names) for t in self.gen.taps.inputs + self.gen.taps.outputs]
            if any(p is None for p in ptrs):
                rec = None
        if rec is not None:
            self._replay_update(rec, ptrs)
        else:
            self._replay = None
            rec = self._record_update(key)
            if rec.complete:
                self._replay = rec
        self._exchange_and_apply()
        self._end_update()

    def _record_update(self, key: tuple) -> _UpdateRecord:
        """The layer-by-layer path: every layer's entries, the three grouped launches, the record of what was launched."""
        rec = _UpdateRecord(key, self._buffers.setdefault(key, {}) if key else {})
        in1, in2 = self.gen.taps.inputs
        with self.ops.pin_stream():
            for idx, plan in enumerate(self.plans):
                if plan.name not in in1 or plan.name not in in2:
                    print("Key error on %s" % plan.name)
                    rec.complete = False
                    continue
                self._fit_layer(idx, plan, rec)
        self.merge.flush()   # ONE grouped launch: the merged inputs of every layer
        if rec.fwd_rows:     # ONE grouped MFMA launch: forward + target + residual + loss of every merged layer
            rec.fwd_loss, rec.fwd_index = self._loss_buffers(tuple(rec.fwd_rows), rec.fwd_rows)
            self.fwd.flush(rec.fwd_loss)
        if rec.dw_rows:      # after the dense launch: forward + target + residual + loss of every depthwise layer
            rec.dw_loss, rec.dw_index = self._loss_buffers(("dw",) + tuple(rec.dw_rows), rec.dw_rows)
            self.dw_fwd.flush(rec.dw_loss)
        self._scatter_losses(rec)
        self._bias_gradients(rec)
        n_wgrad = self.wgrad.pending() + self.dw_wgrad.pending()
        self.wgrad.flush()   # ONE grouped MFMA launch: weight gradients of every merged layer
        self.dw_wgrad.flush()   # and one for the depthwise layers
        rec.complete = rec.complete and n_wgrad > 0
        if rec.complete:
            rec.names = tuple(self.plans[i].name for i, _ in rec.merged)
            rec.fwd_pos = np.array([k for k, (_, dw) in enumerate(rec.merged) if not dw], dtype=np.intp)
            rec.dw_pos = np.array([k for k, (_, dw) in enumerate(rec.merged) if dw], dtype=np.intp)
            rec.merge_tab = self.merge.table()
            rec.fwd_tab = self.fwd.table() if rec.fwd_rows else None
            rec.dw_tab = self.dw_fwd.table() if rec.dw_rows else None
            rows = lambda tab, want: (tab is not None and len(tab) == len(want)) if want else True
            rec.complete = (rec.merge_tab is not None and len(rec.merge_tab) == len(rec.names)
                            and rows(rec.fwd_tab, rec.fwd_rows) and rows(rec.dw_tab, rec.dw_rows))
        return rec

    def _loss_buffers(self, key: tuple, rows: list) -> Tuple[torch.Tensor, torch.Tensor]:
        if key not in self._loss_bufs:
            self._loss_bufs[key] = (torch.zeros(len(rows), dtype=torch.float32, device=self.device),
                                    torch.tensor(rows, dtype=torch.long, device=self.device))
        return self._loss_bufs[key]

    def _replay_update(self, rec: _UpdateRecord, ptrs: list) -> None:
        """The recorded launches again on this update's taps: ``ptrs`` = addresses of both models' inputs, then of their outputs."""
        rec.merge_tab["w1"][:], rec.merge_tab["w2"][:] = ptrs[0], ptrs[1]
        if rec.fwd_rows:
            rec.fwd_tab["o1"][:], rec.fwd_tab["o2"][:] = ptrs[2][rec.fwd_pos], ptrs[3][rec.fwd_pos]
        if rec.dw_rows:
            rec.dw_tab["o1"][:], rec.dw_tab["o2"][:] = ptrs[2][rec.dw_pos], ptrs[3][rec.dw_pos]
        with self.ops.pin_stream():
            self.merge.relaunch()
            if rec.fwd_rows:
                self.fwd.relaunch(rec.fwd_loss)
            if rec.dw_rows:
                self.dw_fwd.relaunch(rec.dw_loss)
        self.fast_updates += 1
        self._scatter_losses(rec)
        self._bias_gradients(rec)
        with self.ops.pin_stream():
            if rec.fwd_rows:
                self.wgrad.relaunch()
            if rec.dw_rows:
                self.dw_wgrad.relaunch()

    def _scatter_losses(self, rec: _UpdateRecord) -> None:
        """Per-layer losses of this update into ``loss_now`` (the gradient arena's tail)."""
        if rec.fwd_rows:
            if self.stacked:        # two entries (half-batches) per layer: their losses add up
                self.loss_now.zero_()
                self.loss_now.index_add_(0, rec.fwd_index, rec.fwd_loss)
            else:
                self.loss_now.index_copy_(0, rec.fwd_index, rec.fwd_loss)
        if rec.dw_rows:             # the depthwise layers' grouped forward, at their layers' indices
            if self.stacked:
                if not rec.fwd_rows:
                    self.loss_now.zero_()
                self.loss_now.index_add_(0, rec.dw_index, rec.dw_loss)
            else:
                self.loss_now.index_copy_(0, rec.dw_index, rec.dw_loss)
        if rec.vendor_losses:       # layers fitted on the vendor's operators (_fit_layer_vendor)
            if not rec.fwd_rows and not rec.dw_rows:
                self.loss_now.zero_()
            seen = set()
            for idx, loss in rec.vendor_losses:
                if idx in seen:
                    self.loss_now[idx] += loss
                else:
                    self.loss_now[idx] = loss
                    seen.add(idx)

    def _exchange_and_apply(self) -> None:
        """Gradients (and losses) summed over the ranks, then ONE masked Adam launch -- on this rank's slice when sharded."""
        if self.stacked:
            self.g.add_(self.g2)     # second half-batch's gradients (same launch, own arena)
        lr = self.lrs[min(self.step_count, len(self.lrs) - 1)]
        self.step_count += 1
        if self.shard_optimizer:
            lo, hi = self.rank * self._shard, (self.rank + 1) * self._shard
            g_mine = dp_reduce_scatter_(self.g, self._g_shard, self.rank, self.world)
            dp_sum_(self.loss_now, self.world)
            self.loss_sum.add_(self.loss_now)
            self.ops.masked_adam(self.p[lo:hi], g_mine, self.mask[lo:hi], self.m, self.v, lr, self.step_count)
            dp_all_gather_(self.p, self.rank, self.world)
        else:
            dp_sum_(self._g_ext, self.world)     # gradients + losses: ONE collective per update
            self.loss_sum.add_(self.loss_now)
            self.ops.masked_adam(self.p, self.g, self.mask, self.m, self.v, lr, self.step_count)


def train(dataloader, model1, model2, model3, spec, perm, costs, budget_ratios, WANDB, MAX_STEPS, wandb_run,
          separate_classifier=False, merging="perm_gradmask", num_classes=1000, lr=5e-4, verbose=False,
          model_type="rn50", solver="adam"):
    """Fit ``model3``'s Conv2d/Linear weights layer by layer (reference :305-405; same positional
    order and defaults; ``solver`` is the only addition).  Consumes one batch per update from a
    single pass over ``dataloader`` and performs ``MAX_STEPS + 1`` updates if it is long enough.
    Puts ``model1``/``model2`` in eval mode (as the reference), mutates and returns ``model3``.
    """
    if solver == "normal_eq":
        from .normal_eq import train_normal_eq

        return train_normal_eq(dataloader, model1, model2, model3, spec, perm, costs, budget_ratios, MAX_STEPS,
                               separate_classifier, num_classes, model_type, verbose, merging=merging)
    if solver != "adam":
        raise ValueError("solver must be 'adam' or 'normal_eq'")
    fit = PleasFitter(model1, model2, model3, spec, perm, costs, budget_ratios, MAX_STEPS, lr, separate_classifier,
                      num_classes, model_type, merging=merging)

    def inputs():
        for idx, batch in enumerate(dataloader):
            if idx > MAX_STEPS:
                break
            yield batch[0]

    for idx in fit.steps(inputs()):
        if verbose:
            print(float(fit.loss_sum.sum()))
        if idx % 20 == 0 and idx:
            per_layer = (fit.loss_sum / 20).cpu()
            total = float(per_layer.sum())
            print("Loss: %.3f" % total)
            if WANDB:
                metrics = {"loss_%s" % p.name: float(v) for p, v in zip(fit.plans, per_layer)}
                metrics["step"], metrics["loss"] = idx, total
                wandb_run.log(metrics)
            fit.loss_sum.zero_()
    return fit.finish()
