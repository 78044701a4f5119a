#!/usr/bin/env python3
"""The rewritten graphs of ``source_forward.fuse_bn_act`` and the chain recognition of the matching twin, as data.

For the two tiny fixtures, a small model with the add patterns the fixtures lack (``AddPatterns``) and every setting a caller uses, ``graph_pins.json`` holds the node list of the rewritten graph --
``[op, target's name, argument names]`` in order -- and, for the twin, which nodes end a BatchNorm chain (with which BatchNorm /
add / ReLU / residual) and which nodes a chain absorbs -- and, under ``twin_graphs``, the node list of the twin graph itself for
every way a caller builds one (``TWIN_CONFIGS``), in eval and in train mode, with stand-ins for the streams and the sinks, on
``tiny_bottleneck``, ``AddPatterns`` and ``InPlace``.  tests/test_graph_pins.py compares a fresh build with the file: a
change to the graph passes that is meant to keep the graphs must leave it as it is.  No GPU, no reference needed.

  python tests/golden/make_golden_graphs.py
"""
import copy
import json
import os
import sys

import torch.fx
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
PINS = os.path.join(HERE, "graph_pins.json")

# name -> (train mode?, SOURCE_CONV_BN, fuse_bn_act's keyword arguments)
SETTINGS = {
    "default_eval": (False, "1", {}),
    "conv_vendor": (False, "1", {"conv": "vendor"}),
    "conv_kxk": (False, "1", {"conv": "kxk"}),
    "source_conv_bn_off": (False, "0", {}),
    "inference": (False, "1", {"inference": True}),
    "train_stats": (True, "1", {"train_stats": True}),
    "train_stats_train_convs": (True, "1", {"train_stats": True, "train_convs": True}),
}


class AddPatterns(nn.Module):
    """What no ResNet has: ``bn -> add`` that no ReLU follows, ``x + x``, and one add fed by two BatchNorms."""

    def __init__(self):
        super().__init__()
        self.c1, self.c2, self.c3 = (nn.Conv2d(4, 4, 3, padding=1, bias=False) for _ in range(3))
        self.bn1, self.bn2, self.bn3, self.bn4 = (nn.BatchNorm2d(4) for _ in range(4))
        self.relu = nn.ReLU()

    def forward(self, x):
        s = self.bn1(self.c1(x)) + x                 # an add without a ReLU behind it
        d = self.bn2(self.c2(s))
        t = d + d                                    # no residual add
        return self.relu(self.bn3(self.c3(t)) + self.bn4(s))      # two BatchNorms, one add


class InPlace(nn.Module):
    """Overwrites tracked tensors in place: an in-place ReLU module, ``+=`` and ``relu_``."""

    def __init__(self):
        super().__init__()
        self.c1, self.c2 = nn.Conv2d(3, 4, 3, padding=1), nn.Conv2d(4, 4, 3, padding=1)
        self.act = nn.ReLU(inplace=True)

    def forward(self, x):
        a = self.act(self.c1(x))
        b = self.c2(a)
        b += a
        return b.relu_()


# name -> _build_twin's keyword arguments; "streams" / "derived" stand for the stand-in objects made per graph
TWIN_CONFIGS = {
    "interleaved": (),
    "interleaved_keep": ("keep_inputs",),
    "split": ("keep_inputs", "streams"),
    "split_fuse": ("keep_inputs", "streams", "fuse_bn"),
    "split_fuse_derive": ("keep_inputs", "streams", "fuse_bn", "derived"),
}


class Streams:
    """Stand-in for the twin's stream fork / join helper on a machine without a GPU."""

    def __init__(self):
        def fork(x):
            return x

        def back():
            pass

        def join():
            pass

        self.fork, self.back, self.join = fork, back, join


def _named(name):
    def fn(*args):
        return None

    fn.__name__ = fn.__qualname__ = name
    return fn


def channel_axes(model, sf):
    """Axis 1 of every convolution, BatchNorm, add and ReLU node of ``model``'s graph."""
    from pleas_merging_amd.core.utils import Axis

    mods = dict(model.named_modules())
    graph = torch.fx.Tracer().trace(model)
    return [Axis(n.name, 1) for n in graph.nodes
            if (n.op == "call_module" and isinstance(mods[n.target], (nn.Conv2d, nn.BatchNorm2d)))
            or sf._is_add(n) or (n.op.startswith("call_") and sf._is_relu(n, mods))]


def twin_graph(am, model, axes, train, config):
    m1, m2 = copy.deepcopy(model).train(train), copy.deepcopy(model).train(train)
    flags = TWIN_CONFIGS[config]
    return am._build_twin(
        m1, m2, axes, lambda g, name, a, n1, n2: g.call_function(_named("sink_" + name), (n1, n2, a)),
        keep_inputs="keep_inputs" in flags, side_stream=Streams() if "streams" in flags else None, fuse_bn="fuse_bn" in flags,
        emit_derived=(lambda g, name, src, a, f1, f2: g.call_function(_named("derived_%s_from_%s" % (name, src)),
                                                                      (f1[0], f1[1], f2[0], f2[1], a)))
        if "derived" in flags else None)


def _arg(a):
    if isinstance(a, torch.fx.Node):
        return a.name
    if isinstance(a, (tuple, list)):
        return [_arg(v) for v in a]
    return repr(a)


def _target(node):
    t = node.target
    return t if isinstance(t, str) else getattr(t, "__name__", type(t).__name__)


def node_list(graph):
    return [[n.op, _target(n), [_arg(a) for a in n.args], n.name] for n in graph.nodes]


def record(models, twin_axes=None):
    """``models``: fixture name -> eval-mode model (left as it was).  ``twin_axes``: model name -> tracked axes, for the
    models whose twin graphs are recorded (None: ``channel_axes``); ``in_place`` is added to those."""
    import importlib

    am = importlib.import_module("pleas_merging_amd.methods.activation_matching")      # the package exports a function of that name
    sf = importlib.import_module("pleas_merging_amd.methods.source_forward")

    out = {"fuse_bn_act": {}, "twin_chains": {}, "twin_graphs": {}}
    before = sf.SOURCE_CONV_BN
    try:
        for name, model in models.items():
            for setting, (train, conv_bn, kwargs) in SETTINGS.items():
                m = copy.deepcopy(model).train(train)
                sf.SOURCE_CONV_BN = conv_bn
                gm = sf.fuse_bn_act(m, **kwargs)
                out["fuse_bn_act"]["%s/%s" % (name, setting)] = None if gm is None else node_list(gm.graph)
            for train in (False, True):
                m1, m2 = copy.deepcopy(model).train(train), copy.deepcopy(model).train(train)
                at, absorbed = am._bn_chains(am._Trace(m1), m1, m2)
                nm = lambda n: None if n is None else n.name
                out["twin_chains"]["%s/%s" % (name, "train" if train else "eval")] = {
                    "chains": [[last.name] + [nm(v) for v in at[last]] for last in at],      # last: bn, add, relu, residual
                    "absorbed": sorted(n.name for n in absorbed)}      # on file: the last row, behind the word "absorbed"
        for name, axes in dict(twin_axes or {}, in_place=None).items():
            model = InPlace().eval() if name == "in_place" else models[name]
            axes = channel_axes(model, sf) if axes is None else list(axes)
            for train in (False, True):
                for config in TWIN_CONFIGS:
                    key = "%s/%s/%s" % (name, "train" if train else "eval", config)
                    out["twin_graphs"][key] = node_list(twin_graph(am, model, axes, train, config).graph)
    finally:
        sf.SOURCE_CONV_BN = before
    return out


def tiny_axes(tiny):
    """The twin's tracked axes of a tiny fixture: its spec's node axes."""
    return [nax for group in tiny.spec.values() for nax in group.node]


def main():
    sys.path.insert(0, os.path.dirname(HERE))
    from conftest import Tiny

    bottleneck = Tiny("tiny_bottleneck.npz")
    pins = record({"tiny_basic": Tiny("tiny_basic.npz").m1, "tiny_bottleneck": bottleneck.m1, "add_patterns": AddPatterns().eval()},
                  {"tiny_bottleneck": tiny_axes(bottleneck), "add_patterns": None})
    with open(PINS, "w") as f:      # one node / one chain per line
        f.write("{\n")
        for i, (kind, entries) in enumerate(sorted(pins.items())):
            f.write(' %s: {\n' % json.dumps(kind))
            for j, (key, value) in enumerate(sorted(entries.items())):
                rows = value if kind != "twin_chains" else value["chains"] + [["absorbed"] + value["absorbed"]]
                f.write('  %s: [\n%s\n  ]%s\n' % (json.dumps(key), ",\n".join("   " + json.dumps(r) for r in rows),
                                                  "," if j + 1 < len(entries) else ""))
            f.write(" }%s\n" % ("," if i + 1 < len(pins) else ""))
        f.write("}\n")
    print(PINS, os.path.getsize(PINS) // 1024, "KiB")


if __name__ == "__main__":
    main()
