"""The twin fx graph of activation matching: both models in ONE graph, a call after every tracked node.

``_build_twin`` is the entry point (``activation_matching.build_cross_module`` / ``build_fused_module`` call it).  Two
layouts: *interleaved* (the reference's, :49-100: the two copies of a node side by side, the tracked call right behind
them) and *split* (model2's whole chain on a second HIP stream, then model1's, a join, then every tracked call).  Both
lower a node the same way (``_lower``) and track the same table (``_tracked_axes``); the split layout can also emit a
``BatchNorm2d -> [+ other] -> [ReLU / ReLU6]`` chain as one ``pleas_bn_act_tracked`` launch (``_emit_chain``).
tests/golden/graph_pins.json pins the node lists of every configuration.
"""
from __future__ import annotations

import operator
from typing import Callable, Dict, Iterable, List, Optional, Tuple

import torch
import torch.fx
import torch.nn.functional as F
from torch import nn

from ..core.utils import Axis
from .. import hip_ops
from .source_forward import (BatchesPerForward, HipConv, _foldable, _foldable_train, _train_fold, bn_chain, fold_bn,
                             _act_arg, _is_relu, own_conv_ok, own_dwconv_ok)


def _node(graph: torch.fx.Graph, op: str, target, args=(), name: str = "n") -> torch.fx.Node:
    """``graph.create_node`` with an explicit (already valid) base name: without one fx derives it from the target
    through a per-character Python loop (``_snake_case``), ~35 us per node and 0.1 s per job for our ~2000 nodes."""
    return graph.create_node(op, target, tuple(args), {}, name=name)


class _Trace:
    """fx graph of a model without the GraphModule around it (``symbolic_trace`` also generates and compiles Python code
    for a module nobody calls: a third of the twin graph's build time, spent while the GPU waits for its first batch)."""

    def __init__(self, model: nn.Module):
        self.graph = torch.fx.Tracer().trace(model)
        self._model = model

    def named_modules(self):
        return self._model.named_modules()


class _SideStream:
    """Stream fork/join calls placed in a split twin graph: model2's chain is enqueued on a second HIP
    stream, model1's on the caller's stream, and the caller's stream waits for both before the sinks run.
    Side-stream tensors are consumed on the caller's stream and re-used by the side stream only after the
    next ``fork`` (which waits for everything enqueued on the caller's stream) -- no record_stream needed."""

    def __init__(self, device: torch.device):
        self.side = hip_ops.role_stream(device, "model2")
        self.main = None

        def fork(x):
            self.main = torch.cuda.current_stream(x.device)
            self.side.wait_stream(self.main)
            torch.cuda.set_stream(self.side)
            return x

        def back():
            torch.cuda.set_stream(self.main)

        def join():
            self.main.wait_stream(self.side)

        fork.__name__ = fork.__qualname__ = "pleas_stream_fork"
        back.__name__ = back.__qualname__ = "pleas_stream_back"
        join.__name__ = join.__qualname__ = "pleas_stream_join"
        self.fork, self.back, self.join = fork, back, join

    def restore(self):
        """After an exception inside the graph: make the caller's stream current again."""
        if self.main is not None:
            torch.cuda.set_stream(self.main)


# ------------------------------------------------------------------------------------------ one node of one side
def _relu6_in_place(node: torch.fx.Node) -> bool:
    """Does this functional ReLU6 call overwrite its input?  ``F.hardtanh_(x, 0, 6)`` always; ``F.relu6(x, inplace)`` and
    ``F.hardtanh(x, 0, 6, inplace)`` by their ``inplace`` argument, keyword or positional."""
    if node.target is F.hardtanh_:
        return True
    at = 1 if node.target is F.relu6 else 3      # where ``inplace`` stands among the positional arguments
    return bool(node.kwargs.get("inplace") or (len(node.args) > at and node.args[at]))


def _out_of_place(twin: torch.fx.Graph, node: torch.fx.Node, lookup: Callable, submods) -> Optional[torch.fx.Node]:
    """Out-of-place twin of an in-place op (same values, new tensor), or None when ``node`` is not one.
    Deferred sinks read tracked activations after the forward, so nothing may overwrite them."""
    if node.op == "call_module" and isinstance(submods[node.target], nn.ReLU) and submods[node.target].inplace:
        return twin.call_function(torch.relu, (lookup(node.args[0]),))
    if node.op == "call_module" and getattr(submods[node.target], "inplace", False) and _is_relu(node, submods) == hip_ops.ACT_RELU6:
        return twin.call_function(F.relu6, (lookup(node.args[0]),))      # nn.ReLU6 / nn.Hardtanh(0, 6) with inplace=True
    if node.op == "call_function":
        if node.target is operator.iadd:
            return twin.call_function(operator.add, tuple(torch.fx.node.map_arg(node.args, lookup)))
        if node.target is torch.relu_ or (node.target is F.relu and (node.kwargs.get("inplace") or
                                                                    (len(node.args) > 1 and node.args[1]))):
            return twin.call_function(torch.relu, (lookup(node.args[0]),))
        if _is_relu(node, submods) == hip_ops.ACT_RELU6 and _relu6_in_place(node):
            return twin.call_function(F.relu6, (lookup(node.args[0]),))
    if node.op == "call_method" and node.target in ("relu_", "add_") and not node.kwargs:
        return twin.call_method(node.target[:-1], tuple(torch.fx.node.map_arg(node.args, lookup)))
    return None


def _own_conv(twin: torch.fx.Graph, node: torch.fx.Node, side: int, model: nn.Module, env) -> Optional[torch.fx.Node]:
    """The twin-graph call of a k x k convolution on the library's own kernel (``source_forward.HipConv``: bit-for-bit
    repeatable, which the vendor's 3 x 3 kernels are not), or None when ``node`` is not one / the mode says vendor."""
    if node.op != "call_module" or len(node.args) != 1 or node.kwargs:
        return None
    try:
        mod = model.get_submodule(node.target)
    except AttributeError:
        return None
    if not (own_conv_ok(mod) or own_dwconv_ok(mod)):      # a depthwise layer: ``hip_ops.dwconv2d`` under ``depthwise_form("hip")``
        return None
    return _node(twin, "call_function", HipConv(mod, "%d_%s" % (side, node.name)), (env[node.args[0]],), "hip_conv")


def _lower(twin: torch.fx.Graph, node: torch.fx.Node, side: int, model: nn.Module, env: dict, submods,
           keep_inputs: bool) -> torch.fx.Node:
    """Node ``node`` of side ``side`` in the twin, entered into that side's ``env``: out of place when ``keep_inputs``
    asks for it, else the library's own convolution, else a copy whose target lives under ``<side>.`` of the root."""
    new = _out_of_place(twin, node, env.__getitem__, submods) if keep_inputs else None
    if new is None:
        new = _own_conv(twin, node, side, model, env)
    if new is None:
        new = twin.node_copy(node, env.__getitem__)
        if node.op in ("call_module", "get_attr"):
            new.target = "%d.%s" % (side, node.target)
    env[node] = new
    return new


def _tracked_axes(axes: Iterable[Axis]) -> Dict[str, List[int]]:
    """``{node name: [axes]}`` of the tracked node axes: each once, in the order first seen."""
    want: Dict[str, List[int]] = {}
    for ax in axes:
        if ax.axis not in want.setdefault(ax.key, []):
            want[ax.key].append(ax.axis)
    return want


def _returned(graph: torch.fx.Graph) -> torch.fx.Node:
    (ret,) = next(n for n in reversed(graph.nodes) if n.op == "output").args
    return ret


# ------------------------------------------------------------------------------------------ BatchNorm chains
def _bn_chains(traced: _Trace, model1: nn.Module, model2: nn.Module):
    """``BatchNorm2d -> [+ other] -> [ReLU]`` chains of the traced graph whose links have no other consumer:
    ``{last node of the chain: (bn, add or None, relu or None, residual operand or None)}`` and the set of nodes that are
    produced by the chain's single fused launch instead of their own.  The BatchNorm may be in eval mode (constants
    folded once) or in train mode (batch statistics folded per batch, ``hip_ops.bn_train_fold``), per model."""
    mods1, mods2 = dict(model1.named_modules()), dict(model2.named_modules())      # mods1: the traced model's own
    at, absorbed, claimed = {}, set(), set()
    for node in traced.graph.nodes:
        if (node.op != "call_module" or len(node.args) != 1 or node.kwargs
                or not all(_foldable(m) or _foldable_train(m) for m in (mods1.get(node.target), mods2.get(node.target)))):
            continue
        add, relu, res = bn_chain(node, mods1, bare_add=True, claimed=claimed)
        last = relu or add or node
        at[last] = (node, add, relu, res)
        absorbed |= {n for n in (node, add, relu) if n is not None and n is not last}
    return at, absorbed


def _derivable(chains: dict, absorbed: set, want: Dict[str, List[int]]) -> set:
    """BatchNorm nodes of fused chains that are tracked on the channel axis together with their input (the convolution
    output): their matching cost is derived from the input node's contraction instead of contracting again."""
    out = set()
    for bn, _add, _relu, _res in chains.values():
        src = bn.args[0]
        # `want` lists an axis once however often the caller names it (this rule used to read a table that did not, so
        # a doubled Axis(bn, 1) switched the derivation off; the one caller that derives passes dict keys: unique)
        if isinstance(src, torch.fx.Node) and src.op not in ("placeholder", "output") and src not in absorbed \
                and want.get(bn.name) == [1] and 1 in want.get(src.name, ()):
            out.add(bn)
    return out


def _emit_chain(twin: torch.fx.Graph, root: nn.Module, chain, side: int, mod: nn.BatchNorm2d, env: dict,
                state: Optional[BatchesPerForward], write_bn: bool, submods) -> Tuple[torch.fx.Node, torch.fx.Node]:
    """``BatchNorm -> [+ residual] -> [ReLU / ReLU6]`` whose links feed nothing else: ONE launch produces every node of the chain
    (activation matching measures all of them), reading x and the residual once.  Enters the chain's members into
    ``env`` and returns the ``(scale, shift)`` nodes of the BatchNorm's affine map."""
    bn, add, relu, res = chain
    x = env[bn.args[0]]
    if _foldable(mod):          # eval mode: scale / shift are constants of the run
        names = ["_pleas_%s_%d_%s" % (kind, side, bn.name) for kind in ("scale", "shift")]
        for name, buf in zip(names, fold_bn(mod)):
            root.register_buffer(name, buf, persistent=False)
        attrs = (_node(twin, "get_attr", names[0], (), "bn_scale"), _node(twin, "get_attr", names[1], (), "bn_shift"))
    else:                       # train mode (the reference drivers' mode): this batch's statistics, one pass
        fold = _node(twin, "call_function", _train_fold(mod, "%d_%s" % (side, bn.name), state), (x,), "bn_stats")
        attrs = (_node(twin, "call_function", operator.getitem, (fold, 0), "bn_scale"),
                 _node(twin, "call_function", operator.getitem, (fold, 1), "bn_shift"))
    fused = _node(twin, "call_function", hip_ops.bn_act_tracked,
                  (x, attrs[0], attrs[1], env[res] if res is not None else None, _act_arg(relu, submods), write_bn), "bn_chain")
    for slot, member in enumerate((bn, add, relu)):
        if member is not None:
            env[member] = _node(twin, "call_function", operator.getitem, (fused, slot), "chain_out")
    return attrs


# ------------------------------------------------------------------------------------------ the two layouts
def _build_twin(model1: nn.Module, model2: nn.Module, axes: Iterable[Axis], emit: Callable,
                keep_inputs: bool = False, side_stream: Optional[_SideStream] = None, fuse_bn: bool = False,
                emit_derived: Optional[Callable] = None, state: Optional[BatchesPerForward] = None):
    """Twin graph of ``model1``/``model2``; ``emit(graph, name, axis, node1, node2)`` adds the call
    made right after tracked node ``name`` and returns the fx node that holds its value.
    ``keep_inputs`` runs in-place activations out of place (same values, new tensor), so that tracked
    activations stay intact until the end of the forward pass.
    ``side_stream`` (needs ``keep_inputs``): instead of interleaving the two models node by node, emit model2's
    whole chain on the side stream, then model1's chain, then join and only then the ``emit`` calls.
    ``state``: the caller's count of batches in the forwarded tensor, read by the train-mode BatchNorm folds of
    ``fuse_bn`` (None: always one)."""
    if side_stream is not None:
        if not keep_inputs:
            raise ValueError("a split twin graph defers its sinks: it needs keep_inputs=True")
        return _build_split_twin(model1, model2, axes, emit, side_stream, fuse_bn, emit_derived, state)
    traced = _Trace(model1)
    submods = dict(traced.named_modules())
    want = _tracked_axes(axes)
    twin = torch.fx.Graph()
    env = ({}, {})  # original node -> new node, per model
    cross: Dict[Tuple[str, int], torch.fx.Node] = {}
    for node in traced.graph.nodes:
        if node.op == "placeholder":
            env[0][node] = env[1][node] = twin.placeholder(node.target)
        elif node.op != "output":
            made = [_lower(twin, node, side, (model1, model2)[side], env[side], submods, keep_inputs) for side in (0, 1)]
            for a in want.get(node.name, ()):
                cross[node.name, a] = emit(twin, node.name, a, made[0], made[1])
    return _finish(twin, nn.ModuleList([model1, model2]), env, _returned(traced.graph), cross)


def _finish(twin: torch.fx.Graph, root: nn.Module, env, ret: torch.fx.Node, cross: dict) -> torch.fx.GraphModule:
    twin.output(([env[0][ret], env[1][ret]], cross))
    gm = torch.fx.GraphModule(root, twin)
    gm.graph.lint()
    return gm


def _build_split_twin(model1: nn.Module, model2: nn.Module, axes: Iterable[Axis], emit: Callable, streams: _SideStream,
                      fuse_bn: bool, emit_derived: Optional[Callable], state: Optional[BatchesPerForward]):
    traced = _Trace(model1)
    submods = dict(traced.named_modules())
    root = nn.ModuleList([model1, model2])
    want = _tracked_axes(axes)
    chains, absorbed = _bn_chains(traced, model1, model2) if fuse_bn else ({}, set())
    derivable = _derivable(chains, absorbed, want) if emit_derived is not None else set()
    twin = torch.fx.Graph()
    inputs = {node: twin.placeholder(node.target) for node in traced.graph.nodes if node.op == "placeholder"}
    env = (dict(inputs), dict(inputs))
    folds: Tuple[dict, dict] = ({}, {})     # per side: BatchNorm node of a fused chain -> its (scale, shift) nodes
    for side in (1, 0):           # model2 first: its kernels are already queued on the side stream while model1 is enqueued
        model = (model1, model2)[side]
        if side == 1 and inputs:  # fork on the first input: the side stream waits for it, then becomes current
            first = next(iter(inputs))
            env[1][first] = _node(twin, "call_function", streams.fork, (inputs[first],), "fork")
        for node in traced.graph.nodes:
            if node in chains:
                bn = chains[node][0]
                folds[side][bn] = _emit_chain(twin, root, chains[node], side, model.get_submodule(bn.target), env[side],
                                              state, bn not in derivable, submods)
            elif node.op not in ("placeholder", "output") and node not in absorbed:
                _lower(twin, node, side, model, env[side], submods, True)
        if side == 1:
            _node(twin, "call_function", streams.back, (), "back")
    _node(twin, "call_function", streams.join, (), "join")
    cross: Dict[Tuple[str, int], torch.fx.Node] = {}
    for node in traced.graph.nodes:
        for a in want.get(node.name, ()) if node.op not in ("placeholder", "output") else ():
            if node in derivable:
                cross[node.name, a] = emit_derived(twin, node.name, node.args[0].name, a, folds[0][node], folds[1][node])
            else:
                cross[node.name, a] = emit(twin, node.name, a, env[0][node], env[1][node])
    return _finish(twin, root, env, _returned(traced.graph), cross)
