"""Activation matching: per-group similarity of two models' activations + one LAP per group.

Drop-in for the reference's ``pleas/methods/activation_matching.py``
(``cross_features_*`` :14-46, ``build_cross_module`` :49-100,
``compute_matching_costs`` :103-136, ``activation_matching`` :139-177).

MI355X design.  Both models run under PyTorch-ROCm inside ONE fx graph (twin copies of every
node).  Right after each tracked node -- i.e. before a following in-place ReLU can overwrite
it -- the graph calls a *sink*.  With the default HIP cross features the sink is
``pleas_gram_accum``: an fp32-MFMA contraction that reads both NCHW activations in place and
adds ``-cdist`` (or the inner product) straight into the node's *group* matrix inside one
flat fp32 arena (the graph itself is built in ``twin_graph.py``).  No per-node C x C tensors, no Python ``sum`` over nodes, and the arena is
what a multi-GPU run all-reduces (one RCCL call) before the batched LAP kernel solves every
group at once.  Any other ``cross_features`` / ``lsa_solver`` callable is honoured through
the reference's plug points (generic path).
"""
from __future__ import annotations

from typing import Callable, Dict, Iterable, List, Optional, Tuple

import torch
from torch import nn

from ..core.solvers import hip_solve_lsa, hip_solve_minimax_assignment
from ..core.utils import Axis, Permutation, PermutationSpec
from .. import hip_ops
from ..hip_ops import cross_features_cdist, cross_features_inner_product  # noqa: F401  (public plug-ins)
from .data_parallel import _collectives_on, _dist_info, _force_collectives, allreduce_sum_  # noqa: F401  (their home; imported from here too)
from .source_forward import BatchesPerForward, batch_runs, uses_batch_statistics
from .twin_graph import _SideStream, _Trace, _bn_chains, _build_twin, _node  # noqa: F401  (their home; tools and tests reach them here)

_FUSED_EPILOGUE = {cross_features_cdist: hip_ops.EPI_NEG_CDIST, cross_features_inner_product: hip_ops.EPI_INNER}


def build_cross_module(model1: nn.Module, model2: nn.Module, axes: Iterable[Axis], cross_features: Callable):
    """One GraphModule that runs ``model1`` and ``model2`` side by side on the same input and
    calls ``cross_features(act1, act2, axis)`` right after every tracked node.

    Same contract as the reference (:49-100): ``model1`` is traced and its graph reused for
    ``model2`` (isomorphic models), submodule targets are prefixed ``0.`` / ``1.`` under a
    ``ModuleList([model1, model2])`` root, and the module returns
    ``([out1, out2], {(node_name, axis): cross_value})``.
    """
    return _build_twin(model1, model2, axes,
                       lambda g, name, a, n1, n2: g.call_function(cross_features, (n1, n2, a)))


class GroupArena:
    """Flat fp32 buffer holding every group's C x C cost matrix back to back (one all-reduce)."""

    def __init__(self, spec: PermutationSpec, device: torch.device):
        self.keys = list(spec.keys())
        sizes = [spec[k].size for k in self.keys]
        self.flat = torch.zeros(sum(s * s for s in sizes), dtype=torch.float32, device=device)
        self.view: Dict[Axis, torch.Tensor] = {}
        off = 0
        for k, s in zip(self.keys, sizes):
            self.view[k] = self.flat[off:off + s * s].view(s, s)
            off += s * s

    def zero_(self):
        self.flat.zero_()


class _FusedSink:
    """Callables placed in the twin graph.  ``grouped=True`` (default): a sink only hands the node's
    two activations to a :class:`GramBatch`; ONE grouped launch per batch contracts all nodes.
    ``grouped=False``: every sink launches ``pleas_gram_accum`` into its group matrix right away."""

    def __init__(self, arena: GroupArena, node_group: Dict[Axis, Axis], epilogue: int, grouped: bool):
        self._accum = hip_ops.gram_accum
        self.arena, self.node_group, self.epilogue = arena, node_group, epilogue
        self.group_index = {key: i for i, key in enumerate(arena.keys)}
        self.index: Dict[Tuple[str, int], List[int]] = {}   # (node name, axis) -> positions in the current GramBatch
        self.batch = hip_ops.GramBatch([arena.view[k] for k in arena.keys], epilogue) if grouped else None
        # batches in the forward that is running: its input is that many batches back to back along dim 0, and every
        # tracked node is queued once PER BATCH (sample slices: contiguous slabs) -- the distance epilogue is per batch.
        # The twin's train-mode BatchNorm folds read the same object.
        self.state = BatchesPerForward()

    def bind(self, node_name: str):
        if self.batch is not None:
            def sink(x, y, a, _name=node_name):
                group = self.group_index[self.node_group[Axis(_name, a)]]
                parts = self.state.parts
                if parts == 1:
                    self.index[_name, a] = [self.batch.add(x, y, a, group)]
                else:
                    if a % x.dim() == 0 or x.shape[0] % parts:
                        raise RuntimeError("node %s: cannot split %s into %d batches along dim 0" % (_name, tuple(x.shape), parts))
                    n = x.shape[0] // parts
                    self.index[_name, a] = [self.batch.add(x[g * n:(g + 1) * n], y[g * n:(g + 1) * n], a, group)
                                            for g in range(parts)]
                return None
        else:
            def sink(x, y, a, _name=node_name):
                self._accum(x, y, a, self.arena.view[self.node_group[Axis(_name, a)]], self.epilogue, True)
                return None

        sink.__name__ = sink.__qualname__ = "gram_sink_%s" % node_name
        return sink

    def bind_derived(self, node_name: str, source_name: str):
        """Sink of an eval-mode BatchNorm node whose input ``source_name`` is tracked on the same axis: nothing is
        contracted, the group's reduce pass derives the node from the source's products, norms and row sums."""
        def sink(scale1, shift1, scale2, shift2, a, _name=node_name, _src=source_name):
            pick = lambda v, g: v[g] if v.dim() == 2 else v      # train mode: one affine map per batch of the forward
            for g, src in enumerate(self.index[_src, a]):      # one derived node per batch of the forward, like its source
                self.batch.add_derived(src, pick(scale1, g), pick(shift1, g), pick(scale2, g), pick(shift2, g),
                                       self.group_index[self.node_group[Axis(_name, a)]])
            return None

        sink.__name__ = sink.__qualname__ = "gram_derived_sink_%s" % node_name
        return sink


def build_fused_module(spec: PermutationSpec, model1: nn.Module, model2: nn.Module, arena: GroupArena, epilogue: int,
                       grouped: bool = True, overlap: bool = False, fuse_bn: bool = False, derive_bn: bool = False):
    """Twin graph whose sinks feed the group arena (the HIP fast path).  Returns (module, sinks).
    ``overlap`` (grouped only): model2's forward runs on a second HIP stream next to model1's."""
    node_group = {nax: key for key, group in spec.items() for nax in group.node}
    sinks = _FusedSink(arena, node_group, epilogue, grouped)
    sinks.streams = _SideStream(arena.flat.device) if (overlap and grouped) else None
    gm = _build_twin(model1, model2, list(node_group.keys()),
                     lambda g, name, a, n1, n2: _node(g, "call_function", sinks.bind(name), (n1, n2, a), "sink"),
                     keep_inputs=grouped,
                     side_stream=sinks.streams, fuse_bn=fuse_bn and sinks.streams is not None,
                     emit_derived=(lambda g, name, src, a, f1, f2: _node(g, "call_function", sinks.bind_derived(name, src),
                                                                         (f1[0], f1[1], f2[0], f2[1], a), "derived_sink"))
                     if (derive_bn and fuse_bn and sinks.streams is not None) else None,
                     state=sinks.state)
    return gm, sinks


# ------------------------------------------------------------------------------------------ cost accumulation
def _model_device(model: nn.Module) -> torch.device:
    return next(iter(model.parameters())).device


def shard_batches(dataloader, num_batches: int, rank: int, world: int):
    """Batches ``b`` with ``b % world == rank`` among the first ``num_batches`` of ``dataloader``
    (whole batches only: the distance epilogue is per batch).  Consumes the loader
    exactly like the reference's ``zip(dataloader, trange(num_batches))`` (:120)."""
    for b, (batch, _) in enumerate(zip(dataloader, range(num_batches))):
        if b % world == rank:
            yield batch


def compute_matching_costs(spec: PermutationSpec, gm_cross: nn.Module, dataloader, num_batches: int,
                           accumulate=True, device: Optional[torch.device] = None,
                           shard: bool = True) -> Dict[Axis, torch.Tensor]:
    """Generic path over a module built by :func:`build_cross_module` with ANY ``cross_features``
    callable (reference: :103-136).  ``accumulate="reference"`` keeps only the last processed
    batch, which is what the reference computes (its membership test at :123-127 compares a
    tuple with ``Axis`` keys and never succeeds); ``True`` sums over batches (and shards them
    over ranks when ``torch.distributed`` is initialised)."""
    if device is None:
        device = _model_device(gm_cross)
    rank, world = _dist_info() if (shard and accumulate is True) else (0, 1)
    per_node: Dict[Axis, torch.Tensor] = {}
    with torch.inference_mode():
        for x, _ in shard_batches(dataloader, num_batches, rank, world):
            _, cross = gm_cross(x.to(device))
            for (name, a), v in cross.items():
                ax = Axis(name, a)
                if accumulate is True and ax in per_node:
                    per_node[ax].add_(v)
                else:
                    per_node[ax] = v
    costs = {}
    for key, group in spec.items():
        total = 0
        for nax in group.node:
            if nax in per_node:
                total = total + per_node[nax]
        if world > 1:
            if not torch.is_tensor(total):  # this rank saw no batch
                total = torch.zeros(group.size, group.size, device=device)
            allreduce_sum_(total, world)
        costs[key] = total
    return costs


def accumulate_costs_fused(spec: PermutationSpec, model1: nn.Module, model2: nn.Module, dataloader, num_batches: int,
                           epilogue: int, accumulate=True, shard: bool = True,
                           grouped: bool = True, overlap: bool = True, fuse_bn: bool = True, derive_bn: bool = True,
                           presharded: bool = False, batches_per_forward: Optional[int] = None) -> Dict[Axis, torch.Tensor]:
    """HIP fast path: every tracked node adds into its group matrix while the forwards run.

    Data parallel: with ``torch.distributed`` initialised (one process per GPU, RCCL), rank r
    takes batches ``b % world == r`` and the flat arena is all-reduced once at the end.  The
    distance epilogue is applied per batch, so sharding at batch granularity is exact
    (SURVEY.md F3).  ``accumulate="reference"`` (last batch only) does not shard.

    ``fuse_bn=True`` (default, two-stream twin only): every eval-mode ``BatchNorm2d -> [+identity] -> [ReLU]`` chain of
    the twin forward is ONE ``pleas_bn_act_tracked`` launch that keeps all nodes of the chain (680 -> 416 launches per
    batch; same folded BatchNorm as the PLeaS phase uses).  Measured on the ResNet-101 job: 17.9 -> 17.1 ms per batch.
    ``fuse_bn=False`` runs the vendor modules.

    ``derive_bn=True`` (default, needs ``fuse_bn``): a tracked eval-mode BatchNorm whose input (the convolution output) is
    tracked on the same channel axis is NOT contracted.  With ``bn(x)_i = a_i x_i + b_i`` its products and distances
    follow from the convolution node's ``G = sum x_i y_j``, squared norms and row sums
    (``<bn x_i, bn' y_j> = a a' G + a b' Sx_i + b a' Sy_j + K b b'``), which the group's reduce pass evaluates in fp64:
    104 of ResNet-101's 344 tracked nodes, i.e. ~30 % of the contraction's flops, and the BatchNorm tensors are not
    written at all.

    ``batches_per_forward`` (default: forwards of up to 64 samples, at most 4 batches): that many consecutive batches of equal shape go through the twin forward as ONE
    forward of the concatenated batch -- the vendor convolutions run 10-25 % faster per sample at 32-128 samples than at
    16 -- while every tracked node is still contracted PER BATCH (sample slices of its activations; the distance epilogue
    is per batch), all batches of the forward in one grouped launch.  Train-mode models (the reference drivers'
    mode) take part: the fused chains fold a train-mode BatchNorm2d on every batch's own samples, in order, in ONE
    launch (``pleas_bn_train_fold_batches``; statistics, running statistics and counter as after k separate forwards) and
    apply each batch's map to its sample range (``pleas_bn_act_tracked_batches``).  One batch per forward remains when a
    normalisation module with batch statistics is still CALLED by the twin graph (``fuse_bn=False``, or a module the
    chains do not cover), and when costs are not summed over batches.

    ``presharded=True`` (data parallel): ``dataloader`` already yields THIS rank's batches only (a loader over a
    ``DistributedSampler``-style partition) and ``num_batches`` counts them; nothing is skipped here and the arena is still
    all-reduced over the whole group.  The default lets every rank walk the same loader and keep every ``world``-th batch,
    which preserves the reference's consumption order (:120) but makes each rank decode all batches.
    """
    device = _model_device(model1)
    if device.type != "cuda":
        raise RuntimeError("activation_matching: models must be on the GPU for the HIP path (got %s)" % device)
    arena = GroupArena(spec, device)
    gm, sinks = build_fused_module(spec, model1, model2, arena, epilogue, grouped,
                                   overlap=overlap and grouped, fuse_bn=fuse_bn, derive_bn=derive_bn)
    rank, world = _dist_info() if (shard and accumulate is True) else (0, 1)
    take = (0, 1) if presharded else (rank, world)      # which of the loader's batches this rank contracts
    # The batches run on a created stream, not on the caller's: work on torch's default (null) stream overlaps the side
    # stream of the split twin graph markedly worse than work on a created stream (see PleasFitter).
    caller = torch.cuda.current_stream(device)
    work = hip_ops.role_stream(device, "model1") if sinks.streams is not None else caller
    work.wait_stream(caller)
    # Several batches share a forward (``source_forward.batch_runs``: the gain is the vendor convolutions' at small
    # batches; the tracked activations of a forward stay alive until its contraction) unless the twin still CALLS something
    # that uses batch statistics: the fused chains fold a train-mode BatchNorm2d per batch, a module called as it is
    # would normalise the concatenated batch as one.
    single = accumulate is not True or sinks.batch is None or uses_batch_statistics(gm)

    def forward(xs):
        if accumulate is not True:
            arena.zero_()
        x = xs[0] if len(xs) == 1 else torch.cat(xs, 0)
        try:
            with sinks.state.of(len(xs)):
                gm(x)
        except BaseException:
            if sinks.streams is not None:
                sinks.streams.restore()
            raise
        if sinks.batch is not None:
            sinks.batch.flush(accumulate=True)

    # pinned host batches: copied on a copy stream, beside the previous forward (a run is forwarded once the batch after it
    # has been pulled, i.e. enqueued)
    batches = (hip_ops.to_device_async(x, device) for x, _ in shard_batches(dataloader, num_batches, *take))
    with torch.inference_mode(), torch.cuda.stream(work):
        for run in batch_runs(batches, batches_per_forward, single):
            forward(run)
    caller.wait_stream(work)
    allreduce_sum_(arena.flat, world)
    return dict(arena.view)


def solve_all(costs: Dict[Axis, torch.Tensor], lsa_solver: Callable, while_solving: Optional[Callable] = None) -> Permutation:
    """One LAP per group.  The default solver runs all groups in ONE batched kernel launch; ``while_solving()`` (if given)
    is called after that launch is enqueued and before its results are awaited -- the largest group keeps two CUs busy
    for ~0.25 s, time the host can spend on work that does not need the permutation.  ``hip_solve_minimax_assignment``
    takes the same road with one batched bottleneck call."""
    if lsa_solver is hip_solve_lsa or lsa_solver is hip_solve_minimax_assignment:
        pending: list = []
        if lsa_solver is hip_solve_lsa:
            batched = hip_ops.solve_lsa_batched
        else:
            def batched(mats, maximize):
                return hip_ops.solve_bottleneck_batched(mats, maximize, deferred=pending)
        mats = list(costs.values())
        dev = mats[0].device if mats else None
        if dev is None or dev.type != "cuda" or while_solving is None:
            outs = batched(mats, maximize=True)
        else:
            # the kernel gets a stream of its own: what `while_solving` enqueues elsewhere (source forwards on side
            # streams) then runs beside it also when the caller is on torch's default stream
            caller, solver = torch.cuda.current_stream(dev), hip_ops.role_stream(dev, "lap")
            solver.wait_stream(caller)
            with torch.cuda.stream(solver):
                outs = batched(mats, maximize=True)
            while_solving()
            caller.wait_stream(solver)
        perm = {k: o.cpu() for k, o in zip(costs.keys(), outs)}
        for status in pending:
            hip_ops.check_bottleneck_status(status)
        return perm
    if while_solving is not None:
        while_solving()
    return {k: lsa_solver(v) for k, v in costs.items()}


def activation_matching(spec: PermutationSpec, model1: nn.Module, model2: nn.Module, dataloader, num_batches=1000,
                        cross_features=cross_features_cdist, lsa_solver=hip_solve_lsa, output_costs=False,
                        accumulate=True, grouped=True, while_solving: Optional[Callable] = None, presharded: bool = False,
                        batches_per_forward: Optional[int] = None):
    """Permutation of ``model2``'s units that best matches ``model1``'s activations.

    Reference: :139-177 (same positional arguments; additions: ``accumulate`` -- ``"reference"``
    reproduces the shipped last-batch-only costs -- and ``grouped`` -- one contraction launch per
    batch (default) instead of one per tracked node -- ``presharded``: under data parallelism the loader already
    yields this rank's batches only -- and ``batches_per_forward``: batches per twin forward, see
    :func:`accumulate_costs_fused`).  Returns ``perm``
    (CPU int64 per group) or ``(perm, costs)`` with fp32 costs on the compute device.
    Does not change the models' train/eval mode and does not move them.
    """
    epilogue = _FUSED_EPILOGUE.get(cross_features)
    if epilogue is not None:
        costs = accumulate_costs_fused(spec, model1, model2, dataloader, num_batches, epilogue, accumulate,
                                       grouped=grouped, presharded=presharded, batches_per_forward=batches_per_forward)
    else:
        axes = [ax for group in spec.values() for ax in group.node]
        gm = build_cross_module(model1, model2, axes, cross_features)
        costs = compute_matching_costs(spec, gm, dataloader, num_batches, accumulate, _model_device(model1))
    perm = solve_all(costs, lsa_solver, while_solving)
    return (perm, costs) if output_costs else perm
