"""The source side of a PLeaS run: the two frozen models, the taps on their layers, and the queue of forwards in flight.

``FrozenSources.launch`` returns a ``SourceTaps``; the queue holds ``Generation``s (a ``SourceTaps`` and the batch it was made
for), which the fitters of ``pleas_merging.py`` and ``normal_eq.py`` consume one per update.
"""
import collections
import contextlib
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch
from torch import nn

from .. import hip_ops
from .data_parallel import _dist_info, dp_slice
from .source_forward import fuse_bn_act


def prepare_sources(model1: nn.Module, model2: nn.Module):
    """The two frozen sources as the fitter runs them (eval mode, BatchNorm / add / ReLU chains folded into one HIP pass
    each; a model that cannot be rewritten is returned as it is).  Needs neither the permutation nor the merged model,
    so it can be built early and handed to ``PleasFitter(fused_sources=...)``."""
    model1.eval()
    model2.eval()
    return fuse_bn_act(model1) or model1, fuse_bn_act(model2) or model2


class TapDict(dict):
    """name -> tensor of one forward.  ``packs`` caches, per list of names, the device addresses and per-sample strides of
    those tensors (``tap_pointers``)."""

    __slots__ = ("packs",)

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.packs = {}


class _TapView:
    """The taps of ONE update inside a grouped source forward: samples ``lo:hi`` of every tensor of ``base``, sliced on
    access (an update touches ~420 of them; slicing all of them ahead of time was 0.6 ms of host time per update)."""

    __slots__ = ("base", "lo", "hi")

    def __init__(self, base: TapDict, lo: int, hi: int):
        self.base, self.lo, self.hi = base, lo, hi

    def __getitem__(self, name):
        return self.base[name][self.lo:self.hi]

    def __contains__(self, name):
        return name in self.base

    def __len__(self):
        return len(self.base)

    def keys(self):
        return self.base.keys()

    def items(self):
        return ((k, v[self.lo:self.hi]) for k, v in self.base.items())


def tap_pointers(taps, names: tuple):
    """Device addresses (numpy uint64) of ``taps[name]`` for ``name`` in ``names`` -- of the update's first sample when
    ``taps`` is a view into a grouped forward.  The per-forward part is computed once per (forward, names)."""
    base, lo = (taps.base, taps.lo) if isinstance(taps, _TapView) else (taps, 0)
    packs = getattr(base, "packs", None)
    hit = packs.get(id(names)) if packs is not None else None
    if hit is None or hit[0] is not names:
        ts = [base[k] for k in names]
        if not all(t.is_contiguous() and t.dtype == torch.float32 for t in ts):
            return None
        hit = (names, np.array([t.data_ptr() for t in ts], dtype=np.uint64),
               np.array([t.stride(0) * 4 if t.dim() > 0 else 0 for t in ts], dtype=np.uint64))
        if packs is not None:
            packs[id(names)] = hit
    return hit[1] + np.uint64(lo) * hit[2] if lo else hit[1]


class ActivationTap:
    """Forward hooks on every Conv2d / Linear / LayerNorm of a model that keep the module's
    input and output of the latest forward (reference keeps inputs only, :197-231)."""

    KINDS = (nn.Conv2d, nn.Linear, nn.LayerNorm)

    def __init__(self, model: nn.Module):
        self.inputs: Dict[str, torch.Tensor] = TapDict()
        self.outputs: Dict[str, torch.Tensor] = TapDict()
        self.handles = []
        for name, mod in model.named_modules():
            if isinstance(mod, self.KINDS):
                self.handles.append(mod.register_forward_hook(self._hook(name)))

    def _hook(self, name):
        def hook(module, inp, out):
            if isinstance(inp, tuple):
                assert len(inp) == 1
                inp = inp[0]
            self.inputs[name] = inp
            self.outputs[name] = out

        return hook

    def clear(self):
        self.inputs.clear()
        self.outputs.clear()

    def take(self):
        """Hand over the tensors of the latest forward and start a new generation (the hooks look the dicts up on
        every call, so the next forward fills the fresh ones)."""
        got = (self.inputs, self.outputs)
        self.inputs, self.outputs = TapDict(), TapDict()
        return got

    def remove(self):
        for h in self.handles:
            h.remove()
        self.handles = []


class SourceTaps(NamedTuple):
    """What one forward of both sources left behind (``FrozenSources.launch``), or one update's share (``_TapView``s) of a
    grouped one: the device batch, per model ``(inputs, outputs)`` by layer name, and one event per side stream (or None)."""

    x: torch.Tensor
    taps1: Tuple
    taps2: Tuple
    events: Optional[list]
    inputs = property(lambda self: (self.taps1[0], self.taps2[0]))      # of model1, of model2
    outputs = property(lambda self: (self.taps1[1], self.taps2[1]))


class Generation(NamedTuple):
    """A queue entry: the batch as the caller passed it (what ``step`` recognises it by) and the taps made for it."""

    batch: torch.Tensor
    taps: SourceTaps


class FrozenSources:
    """The two frozen source models as the PLeaS loop runs them: eval mode, BatchNorm / add / ReLU chains folded into one
    HIP pass each (``source_forward.py``), taps on every Conv2d / Linear, each model on its own side stream.  A forward
    produces a ``SourceTaps``; ``queue`` holds the ``Generation``s whose forwards are enqueued, in update order.

    Nothing here depends on the permutation or on the merged model, so the object can be built -- and the first forwards
    enqueued (``prefetch``) -- while the LAP kernel is still running; ``PleasFitter(sources=...)`` then takes it over."""

    def __init__(self, model1: nn.Module, model2: nn.Module, data_parallel: bool = False, fuse: bool = True,
                 overlap: bool = True, fused=None):
        self.ops = hip_ops
        self.rank, self.world = _dist_info() if data_parallel else (0, 1)
        self.device = next(iter(model1.parameters())).device
        if self.device.type != "cuda":
            raise hip_ops.PleasHipError("pleas_merging.train: source models must be on the GPU (got %s)" % self.device)
        self.tap1, self.tap2 = ActivationTap(model1), ActivationTap(model2)
        model1.eval()
        model2.eval()
        # the hooked Conv2d / Linear modules are shared with the rewritten graphs, so the taps see the same tensors
        self.src1, self.src2 = model1, model2
        if fused is not None:               # built ahead of time (prepare_sources)
            self.src1, self.src2 = fused
        elif fuse:
            self.src1, self.src2 = prepare_sources(model1, model2)
        # The two source forwards are independent chains of small kernels (one conv of a batch-16 ResNet fills a
        # fraction of 256 CUs).  Each source gets its own stream: their chains then also run NEXT TO the big grouped
        # kernels of an update when they are enqueued ahead of it.  Equal priorities: favouring either side was slower
        # (chain first 8.7 s, update first 11.5 s).
        self._side_streams = (hip_ops.role_stream(self.device, "model1"),
                              hip_ops.role_stream(self.device, "model2")) if overlap else None
        self._slice_batch = True   # data parallel: every update splits its batch's samples over the ranks
        self.queue: collections.deque = collections.deque()
        self._staged: dict = {}    # id(pinned host batch) -> (batch, device copy, event): copies started ahead of their forward

    def stage(self, batches) -> None:
        """Start the host -> device copies of PINNED host batches now (copy stream); the forward that takes a batch later
        only waits for its event.  ``steps`` stages the group AFTER the one it launches: enqueued together with a group's
        forwards, a copy would sit behind that group's kernels in a shared hardware queue and surface when it is needed."""
        for b in batches:
            if torch.is_tensor(b) and not b.is_cuda and b.is_pinned() and id(b) not in self._staged:
                self._staged[id(b)] = (b,) + self.ops.h2d_start(b, self.device)

    def _to_device(self, b: torch.Tensor) -> torch.Tensor:
        hit = self._staged.pop(id(b), None) if torch.is_tensor(b) else None
        if hit is not None and hit[0] is b:
            return self.ops.h2d_finish(hit[1], hit[2], self.device)
        return self.ops.to_device_async(b, self.device)

    def launch(self, x: torch.Tensor, parts: int = 1, after_current: bool = True) -> SourceTaps:
        """Enqueue both source forwards for ``x``; returns the taps (device batch, taps, events) the update will
        consume.  ``parts`` > 1: ``x`` is that many batches back to back, each of which is sample-sliced on its own."""
        x = self._to_device(x)
        if self._slice_batch:
            if parts > 1 and self.world > 1:
                h = x.shape[0] // parts
                x = torch.cat([dp_slice(x[i * h:(i + 1) * h], self.rank, self.world) for i in range(parts)], 0)
            else:
                x = dp_slice(x, self.rank, self.world)
        events = self.run_eager(x, after_current)
        return SourceTaps(x, self.tap1.take(), self.tap2.take(), events)

    def enqueue(self, b: torch.Tensor, after_current: bool = True) -> None:
        """One source forward for one batch; its generation joins the queue."""
        self.queue.append(Generation(b, self.launch(b, after_current=after_current)))

    @torch.no_grad()
    def launch_group(self, run: List[torch.Tensor], after_current: bool = True) -> None:
        """One source forward for several batches; their generations (views of its taps) join the queue."""
        first = self._side_streams[0] if (self._side_streams is not None and not after_current) else None
        with (torch.cuda.stream(first) if first is not None else contextlib.nullcontext()):
            # pinned host batches travel on a copy stream while the previous group's updates run (hip_ops.to_device_async)
            both = torch.cat([self._to_device(b) for b in run], 0)
            xdev, (in1, out1), (in2, out2), events = self.launch(both, parts=len(run), after_current=after_current)
        n = xdev.shape[0] // len(run)
        for i, b in enumerate(run):
            lo, hi = i * n, (i + 1) * n
            self.queue.append(Generation(b, SourceTaps(xdev, (_TapView(in1, lo, hi), _TapView(out1, lo, hi)),
                                                       (_TapView(in2, lo, hi), _TapView(out2, lo, hi)), events)))

    @torch.no_grad()
    def prefetch(self, batches, group: Optional[int] = None, max_groups: int = 1, memory_fraction: float = 0.5) -> int:
        """Enqueue the source forwards of the first batches NOW, on the side streams only -- not ordered after the work
        already queued on the current stream, which is the point: called from ``activation_matching(while_solving=...)``
        they run beside the LAP kernel (one workgroup per problem, 71 of 256 CUs, 0.28 s).  ``batches`` must be tensors
        whose values are already in place (resident inputs, or host tensors); ``PleasFitter.steps`` must later be given
        the same tensor objects first, in the same order.  Takes whole groups of ``group`` (default ``2 * world``) equal
        batches, at most ``max_groups`` of them and as long as their taps (sized from the first group) fit into
        ``memory_fraction`` of the HBM that is free or idle in the allocator's pools.  Returns the number of batches taken."""
        if self._side_streams is None:
            return 0
        group = max(1, int(group or 2 * self.world))
        batches = list(batches)
        # The side streams skip the current stream's queue (the LAP kernel), but the memory they are about to take from
        # their allocator pools may have been released by the host while its last readers are still queued: updates of an
        # earlier fitter on the update stream (waited for here), matching kernels on model1's stream (in order with it;
        # model2's stream follows model1's in run_eager).
        self._side_streams[0].wait_stream(self.ops.role_stream(self.device, "updates"))
        # what the taps may take: a share of the HBM that is free or sits unused in the caching allocator's pools
        idle = torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)
        budget = (torch.cuda.mem_get_info(self.device)[0] + idle) * memory_fraction
        per_group, taken = None, 0
        for g in range(max_groups):
            run = batches[g * group:(g + 1) * group]
            if len(run) < group or any(not torch.is_tensor(b) or b.shape != run[0].shape or b.shape[0] == 0 for b in run):
                break
            if per_group is not None and (g + 1) * per_group > budget:
                break
            if group > 1:
                self.launch_group(run, after_current=False)
            else:
                self.enqueue(run[0], after_current=False)
            taken += group
            if per_group is None:      # bytes one group's taps hold (inputs and outputs of every hooked layer, both models)
                last = self.queue[-1].taps
                bases = [taps.base if isinstance(taps, _TapView) else taps for taps in last.inputs + last.outputs]
                per_group = sum(t.numel() * t.element_size() for base in bases for t in base.values())
        return taken

    @torch.no_grad()
    def run_eager(self, x: torch.Tensor, after_current: bool = True) -> Optional[list]:
        """Both source forwards (frozen: never under autograd), dispatched op by op; the hooks fill ``tap1`` / ``tap2`` (callers that read them right
        away must synchronise: the models run on side streams).  ``after_current=False``: the side streams are not
        ordered after the current stream's queue (``prefetch``); model2's stream then follows model1's up to here, which
        is where the batch was put together.  Returns one event per side stream, recorded behind its forward."""
        side = self._side_streams
        if side is None:
            with self.ops.pin_stream():
                self.src1(x)
                self.src2(x)
            return None
        main = torch.cuda.current_stream(self.device)
        # The sources' tensors live in the side streams' allocator pools.  They are consumed on `main` (by the update
        # that owns this generation) and released by the host once that update is enqueued; a side stream re-uses them
        # only after a LATER wait_stream(main), i.e. after every consumer enqueued on `main` up to then -- with one
        # batch of look-ahead that is the update two generations back.  No record_stream bookkeeping needed.
        events = []
        if not after_current:          # model2's stream follows model1's up to HERE (the batch is in place), not its forward
            side[1].wait_event(side[0].record_event())
        for stream, model in zip(side, (self.src1, self.src2)):
            if after_current:
                stream.wait_stream(main)
            with torch.cuda.stream(stream), self.ops.pin_stream():
                model(x)
            events.append(stream.record_event())
        return events

    def close(self) -> None:
        self.tap1.remove()
        self.tap2.remove()
        self.queue.clear()
        self._staged.clear()
