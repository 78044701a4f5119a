"""ReLU6 through the host side (no GPU): the spec builder's rules, the own MobileNetV2 definition, the graph rewrites with a CPU
stand-in for the fused passes, the twin graph's out-of-place activations and the wrappers' refusals."""
import copy
import os
import sys

import pytest
import torch
import torch.fx
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import relu6_cases as rc  # noqa: E402

from pleas_merging_amd import hip_ops  # noqa: E402
from pleas_merging_amd.core.compiler import get_permutation_spec  # noqa: E402
from pleas_merging_amd.core.utils import Axis, apply_perm, make_random_perm  # noqa: E402
from pleas_merging_amd.methods import source_forward as sf  # noqa: E402


def _same_spec(got, want, rename=None):
    """Group for group: keys, sizes, state axes, node names (``rename``: node names of ``want`` -> those of ``got``)."""
    rename = rename or {}
    assert list(got.keys()) == list(want.keys())
    for k in want:
        assert got[k].size == want[k].size, k
        assert set(got[k].state) == set(want[k].state), k
        assert {(a.key, a.axis) for a in got[k].node} == {(rename.get(a.key, a.key), a.axis) for a in want[k].node}, k


def _calibrated(model, shape, seed=0):
    """Eval-mode ``model`` with non-trivial BatchNorm statistics."""
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(generator=g)
            m.running_var.uniform_(0.5, 2.0, generator=g)
            with torch.no_grad():
                m.weight.normal_(1.0, 0.3, generator=g)
                m.bias.normal_(0.0, 0.5, generator=g)
    return model.eval(), torch.randn(*shape, generator=g)


# ------------------------------------------------------------------------------------------------------------------- spec
def test_spec_of_the_small_network_equals_its_relu_twins():
    torch.manual_seed(0)
    net = rc.small_mobilenet()
    spec = get_permutation_spec(net, ((2,) + rc.SMALL_INPUT[1:],))
    _same_spec(spec, get_permutation_spec(rc.relu_twin(net), ((2,) + rc.SMALL_INPUT[1:],)))
    assert len(spec) >= 5 and any(net.get_submodule(a.key.rsplit(".", 1)[0]).groups > 1
                                  for g in spec.values() for a in g.state if a.key.endswith("1.0.weight"))


class _Spelled(nn.Module):
    """conv -> bn -> activation four times, the activation spelled four ways (``six``) or as ReLU in the matching forms."""

    def __init__(self, six: bool):
        super().__init__()
        self.six = six
        self.convs = nn.ModuleList([nn.Conv2d(3 if i == 0 else 6 + i - 1, 6 + i, 3, padding=1, bias=False) for i in range(4)])
        self.bns = nn.ModuleList([nn.BatchNorm2d(6 + i) for i in range(4)])
        self.act = nn.Hardtanh(0, 6) if six else nn.ReLU()
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(9, 5)

    def forward(self, x):
        x = self.bns[0](self.convs[0](x))
        x = F.relu6(x) if self.six else F.relu(x)
        x = self.bns[1](self.convs[1](x))
        x = F.hardtanh(x, 0., 6.) if self.six else F.relu(x)
        x = self.act(self.bns[2](self.convs[2](x)))
        x = self.bns[3](self.convs[3](x))
        x = F.hardtanh_(x, min_val=0, max_val=6) if self.six else torch.relu(x)
        return self.fc(torch.flatten(self.avgpool(x), 1))


def test_spec_of_the_functional_spellings_equals_the_relu_forms():
    six, one = _Spelled(True), _Spelled(False)
    names = {b.name: a.name for a, b in zip(torch.fx.Tracer().trace(six).nodes, torch.fx.Tracer().trace(one).nodes)}
    assert any(a != b for a, b in names.items())
    _same_spec(get_permutation_spec(six, ((2, 3, 8, 8),)), get_permutation_spec(one, ((2, 3, 8, 8),)), names)
    # Hardtanh is elementwise whatever its bounds
    six.act = nn.Hardtanh(-2, 5)
    _same_spec(get_permutation_spec(six, ((2, 3, 8, 8),)), get_permutation_spec(one, ((2, 3, 8, 8),)), names)


def test_a_random_permutation_leaves_the_network_function_unchanged():
    torch.manual_seed(1)
    net, x = _calibrated(rc.small_mobilenet(), rc.SMALL_INPUT)
    spec = get_permutation_spec(net, ((2,) + rc.SMALL_INPUT[1:],))
    perm = make_random_perm(spec, torch.Generator().manual_seed(2))
    assert any(not torch.equal(p, torch.arange(len(p))) for p in perm.values())
    moved = copy.deepcopy(net)
    moved.load_state_dict(apply_perm(perm, spec, net.state_dict()))
    assert not torch.equal(moved.features[0][0].weight, net.features[0][0].weight)
    with torch.no_grad():
        assert torch.allclose(moved(x), net(x), rtol=1e-2, atol=1e-3)


# ------------------------------------------------------------------------------------------------------------- the model
def test_full_size_mobilenet_v2_counts_keys_and_spec():
    from pleas_merging_amd.mobilenet import mobilenet_v2

    torch.manual_seed(0)
    net = mobilenet_v2()
    convs = [m for m in net.modules() if isinstance(m, nn.Conv2d)]
    assert sum(p.numel() for p in net.parameters()) == 3504872
    assert len(convs) == 52 and sum(1 for m in convs if m.groups > 1) == 17
    assert all(m.groups in (1, m.in_channels) and m.bias is None for m in convs)
    bn = lambda prefix: {prefix + "." + leaf for leaf in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")}
    want = {"features.0.0.weight"} | bn("features.0.1") | {"features.1.conv.0.0.weight", "features.1.conv.1.weight"}
    want |= bn("features.1.conv.0.1") | bn("features.1.conv.2")
    for k in range(2, 18):
        base = "features.%d.conv." % k
        want |= {base + "0.0.weight", base + "1.0.weight", base + "2.weight"} | bn(base + "0.1") | bn(base + "1.1") | bn(base + "3")
    want |= {"features.18.0.weight", "classifier.1.weight", "classifier.1.bias"} | bn("features.18.1")
    assert set(net.state_dict()) == want
    assert net.features[18][0].weight.shape == (1280, 320, 1, 1) and net.classifier[1].weight.shape == (1000, 1280)
    acts = [m for m in net.modules() if isinstance(m, nn.ReLU6)]
    assert len(acts) == 35 and all(m.inplace for m in acts) and not [m for m in net.modules() if isinstance(m, nn.ReLU)]
    assert all(isinstance(net.get_submodule(k.rsplit(".", 2)[0])[2], nn.ReLU6) for k in want if k.endswith(".0.weight"))
    fresh = mobilenet_v2()
    result = fresh.load_state_dict(net.state_dict(), strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    head = net.classifier[1]
    assert float(head.bias.detach().abs().max()) == 0.0 and 0.005 < float(head.weight.detach().std()) < 0.02
    assert all(float((m.weight.detach() - 1).abs().max()) == 0.0 and float(m.bias.detach().abs().max()) == 0.0
               for m in net.modules() if isinstance(m, nn.BatchNorm2d))
    # width multiplier and rounding: torchvision's _make_divisible
    assert mobilenet_v2(width_mult=0.5).last_channel == 1280 and mobilenet_v2(width_mult=1.4).last_channel == 1792
    assert mobilenet_v2(width_mult=0.75).features[2].conv[2].out_channels == 24
    spec = get_permutation_spec(net, ((2, 3, 224, 224),))
    _same_spec(spec, get_permutation_spec(rc.relu_twin(net), ((2, 3, 224, 224),)))
    assert isinstance(torch.fx.symbolic_trace(net), torch.fx.GraphModule)


# ---------------------------------------------------------------------------------------------------------- graph rewrites
def _act(v, relu):
    """The activation of code ``relu`` with torch operators (what the kernels compute)."""
    code = hip_ops._act_code("stand-in", relu)
    return F.relu6(v) if code == hip_ops.ACT_RELU6 else torch.relu(v) if code == hip_ops.ACT_RELU else v


def _op(x, s, t, res, relu):
    y = x * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1)
    return _act(y if res is None else y + res, relu)


def _pool_op(x, s, t, kernel, stride, padding, relu):
    return F.max_pool2d(_op(x, s, t, None, relu), kernel, stride, padding)


class _Chains(nn.Module):
    """bn -> act -> maxpool, then bn -> act, then bn -> (+ identity) -> act, then a bare bn."""

    def __init__(self, act):
        super().__init__()
        self.c1, self.b1, self.a1, self.pool = nn.Conv2d(3, 6, 3, padding=1), nn.BatchNorm2d(6), act(), nn.MaxPool2d(3, 2, 1)
        self.c2, self.b2, self.a2 = nn.Conv2d(6, 6, 3, padding=1), nn.BatchNorm2d(6), act()
        self.c3, self.b3, self.a3 = nn.Conv2d(6, 6, 1), nn.BatchNorm2d(6), act()
        self.c4, self.b4 = nn.Conv2d(6, 4, 1), nn.BatchNorm2d(4)

    def forward(self, x):
        x = self.pool(self.a1(self.b1(self.c1(x))))
        y = self.a2(self.b2(self.c2(x)))
        y = self.a3(self.b3(self.c3(y)) + x)
        return self.b4(self.c4(y))


def _fused_calls(gm):
    return [(n.name, n.target, n.args) for n in gm.graph.nodes if n.op == "call_function" and n.target in (_op, _pool_op)]


@pytest.mark.parametrize("act", [lambda: nn.ReLU6(inplace=True), lambda: nn.Hardtanh(0, 6), lambda: nn.Hardtanh(0.0, 6.0, inplace=True)],
                         ids=["relu6_inplace", "hardtanh_0_6", "hardtanh_inplace"])
def test_every_chain_form_becomes_one_call_carrying_relu6(act):
    torch.manual_seed(2)
    net, x = _calibrated(_Chains(act), (2, 3, 9, 9))
    gm = sf.fuse_bn_act(net, _op, pool_op=_pool_op)
    calls = _fused_calls(gm)
    assert [(t, a[-1]) for _, t, a in calls] == [(_pool_op, hip_ops.ACT_RELU6), (_op, hip_ops.ACT_RELU6), (_op, hip_ops.ACT_RELU6), (_op, False)]
    assert calls[0][2][3:6] == ((3, 3), 2, 1) and calls[1][2][3] is None and isinstance(calls[2][2][3], torch.fx.Node)
    assert [n.target for n in gm.graph.nodes if n.op == "call_module"] == ["c1", "c2", "c3", "c4"]
    assert not [n for n in gm.graph.nodes if n.op == "call_function" and n.target not in (_op, _pool_op)]
    with torch.no_grad():
        want = net(x.clone())
        assert torch.allclose(gm(x.clone()), want, rtol=0, atol=1e-6)
        assert float(want.abs().max()) > 0
    # without a pooled stand-in the stem chain is bn -> act, the pooling a module
    plain = sf.fuse_bn_act(net, _op)
    assert [(t, a[-1]) for _, t, a in _fused_calls(plain)][0] == (_op, hip_ops.ACT_RELU6)
    with torch.no_grad():
        assert torch.allclose(plain(x.clone()), want, rtol=0, atol=1e-6)


class _Functional(nn.Module):
    def __init__(self, spelling):
        super().__init__()
        self.c, self.b, self.spelling = nn.Conv2d(3, 5, 3, padding=1), nn.BatchNorm2d(5), spelling

    def forward(self, x):
        return self.spelling(self.b(self.c(x)) + x.mean(1, keepdim=True))


SPELLINGS = {
    "relu6": (lambda v: F.relu6(v), hip_ops.ACT_RELU6),
    "relu6_inplace": (lambda v: F.relu6(v, inplace=True), hip_ops.ACT_RELU6),
    "hardtanh_positional": (lambda v: F.hardtanh(v, 0., 6.), hip_ops.ACT_RELU6),
    "hardtanh_keywords": (lambda v: F.hardtanh(v, min_val=0, max_val=6.0, inplace=True), hip_ops.ACT_RELU6),
    "hardtanh_": (lambda v: F.hardtanh_(v, 0, 6), hip_ops.ACT_RELU6),
    "relu": (lambda v: F.relu(v), True),
    "relu_method": (lambda v: v.relu_(), True),
    "hardtanh_default_bounds": (lambda v: F.hardtanh(v), None),
    "hardtanh_0_5": (lambda v: F.hardtanh(v, 0., 5.), None),
    "hardtanh_lower_bound_only": (lambda v: F.hardtanh(v, 0.), None),
    "clamp": (lambda v: torch.clamp(v, 0, 6), None),
}


@pytest.mark.parametrize("name", list(SPELLINGS))
def test_functional_spellings_recognised_exactly(name):
    spelling, code = SPELLINGS[name]
    torch.manual_seed(3)
    net, x = _calibrated(_Functional(spelling), (2, 3, 6, 6))
    gm = sf.fuse_bn_act(net, _op)
    (call,) = _fused_calls(gm)
    if code is None:      # an ordinary node: the BatchNorm stands alone, the add and the clamp stay
        assert call[2][3] is None and call[2][4] is False
        assert len([n for n in gm.graph.nodes if n.op in ("call_function", "call_method") and n.target is not _op]) >= 3
    else:
        assert isinstance(call[2][3], torch.fx.Node) and call[2][4] == code and type(call[2][4]) is type(code)
    with torch.no_grad():
        assert torch.allclose(gm(x.clone()), net(x.clone()), rtol=0, atol=1e-6)


def test_a_hardtanh_with_other_bounds_is_not_fused():
    torch.manual_seed(4)
    net, x = _calibrated(_Chains(lambda: nn.Hardtanh(0, 5)), (2, 3, 9, 9))
    gm = sf.fuse_bn_act(net, _op, pool_op=_pool_op)
    assert [(t, a[-1]) for _, t, a in _fused_calls(gm)] == [(_op, False)] * 4
    assert [n.target for n in gm.graph.nodes if n.op == "call_module" and isinstance(net.get_submodule(n.target), nn.Hardtanh)] == ["a1", "a2", "a3"]
    with torch.no_grad():
        assert torch.allclose(gm(x.clone()), net(x.clone()), rtol=0, atol=1e-6)


def _old_is_relu(node, mods):
    if node.op == "call_module":
        return isinstance(mods[node.target], nn.ReLU)
    if node.op == "call_function":
        return node.target in (F.relu, torch.relu, torch.relu_)
    if node.op == "call_method":
        return node.target in ("relu", "relu_")
    return False


def test_relu_graphs_are_what_the_old_predicate_builds(monkeypatch):
    from pleas_merging_amd import resnet as zoo

    torch.manual_seed(5)
    net, x = _calibrated(zoo.resnet18(num_classes=10), (2, 3, 64, 64))
    listing = lambda gm: [(n.op, n.name, tuple(a.name if isinstance(a, torch.fx.Node) else a for a in n.args)) for n in gm.graph.nodes]
    builds = (("cpu", dict(op=_op, pool_op=_pool_op)), ("cpu_unpooled", dict(op=_op)), ("own", {}), ("inference", dict(inference=True)))
    new = {kind: sf.fuse_bn_act(net, **kw) for kind, kw in builds}
    monkeypatch.setattr(sf, "_is_relu", _old_is_relu)
    for kind, kw in builds:
        assert listing(sf.fuse_bn_act(net, **kw)) == listing(new[kind]), kind
    monkeypatch.undo()
    calls = _fused_calls(new["cpu"])
    assert len(calls) == 20 and calls[0][1] is _pool_op
    assert all(a[-1] in (False, hip_ops.ACT_RELU) and a[-1] != hip_ops.ACT_RELU6 for _, _, a in calls)
    assert sum(1 for _, _, a in calls if a[-1] == hip_ops.ACT_RELU) == 17      # the stem, 8 x (bn1, bn2 + identity); 3 downsample bn bare
    with torch.no_grad():
        assert torch.allclose(new["cpu"](x), net(x), rtol=0, atol=1e-5)
    # the default graph (own kernels' callables) of the small MobileNetV2: every conv -> bn -> ReLU6 is one call with the code
    small = rc.small_mobilenet().eval()
    gm = sf.fuse_bn_act(small)
    fused = [n for n in gm.graph.nodes if n.op == "call_function" and isinstance(n.target, sf.HipConvBnAct)]
    assert [n.args[4] for n in fused].count(hip_ops.ACT_RELU6) == 6 and [n.args[4] for n in fused].count(False) == 5
    # depthwise layers stay modules under the vendor form, followed by one bn_act carrying the code
    rest = [n.args[4] for n in gm.graph.nodes if n.op == "call_function" and n.target is sf._bn_act]
    assert rest == [hip_ops.ACT_RELU6] * 5


# -------------------------------------------------------------------------------------------------------------- twin graph
class _HardtanhInPlace(nn.Module):
    def __init__(self):
        super().__init__()
        self.c1, self.b1, self.c2 = nn.Conv2d(3, 4, 3, padding=1), nn.BatchNorm2d(4), nn.Conv2d(4, 4, 3, padding=1)

    def forward(self, x):
        a = self.b1(self.c1(x))
        a = F.hardtanh_(a, 0., 6.)
        b = self.c2(a)
        b = F.relu6(b, inplace=True)
        return F.hardtanh(b + a, 0, 6, True)


def _inplace_nodes(gm):
    """Nodes of ``gm`` that overwrite their input: in-place activation modules, ``hardtanh_`` / ``relu_``, ``inplace=True``."""
    found = []
    for n in gm.graph.nodes:
        if n.op == "call_module" and getattr(gm.get_submodule(n.target), "inplace", False):
            found.append(n)
        elif n.op == "call_function" and (n.target in (F.hardtanh_, torch.relu_) or n.kwargs.get("inplace")
                                          or (n.target in (F.relu6, F.relu) and len(n.args) > 1 and n.args[1])
                                          or (n.target is F.hardtanh and len(n.args) > 3 and n.args[3])):
            found.append(n)
        elif n.op == "call_method" and n.target.endswith("_"):
            found.append(n)
    return found


@pytest.mark.parametrize("kind", ["modules", "functions"])
def test_twin_graph_runs_in_place_relu6_out_of_place(kind):
    from pleas_merging_amd.methods import twin_graph

    torch.manual_seed(6)
    if kind == "modules":
        (m1, x), (m2, _) = _calibrated(rc.small_mobilenet(), rc.SMALL_INPUT, 1), _calibrated(rc.small_mobilenet(), rc.SMALL_INPUT, 2)
        tracked = ["features_0_1", "features_0_2", "features_2_conv_1_1", "features_2_conv_1_2"]
    else:
        (m1, x), (m2, _) = _calibrated(_HardtanhInPlace(), (2, 3, 6, 6), 1), _calibrated(_HardtanhInPlace(), (2, 3, 6, 6), 2)
        tracked = ["b1", "hardtanh_", "c2", "relu6"]
    assert _inplace_nodes(torch.fx.symbolic_trace(m1))           # the model itself does overwrite
    seen = {}

    def emit(g, name, a, n1, n2):
        def sink(u, v, _n=name):
            seen[_n] = (u, v)          # no clone: what the deferred sinks would read after the forward
        sink.__name__ = sink.__qualname__ = "sink_" + name
        return g.call_function(sink, (n1, n2))

    gm = twin_graph._build_twin(m1, m2, [Axis(n, 1) for n in tracked], emit, keep_inputs=True)
    assert _inplace_nodes(gm) == []
    with torch.no_grad():
        out = gm(x.clone())
        want = (m1(x.clone()), m2(x.clone()))
    assert torch.equal(out[0][0], want[0]) and torch.equal(out[0][1], want[1])
    # the tracked pre-activation values survived the forward: they are not their own clamp
    pre, post = seen[tracked[0]][0], seen[tracked[1]][0]
    assert float(pre.min()) < 0 and torch.equal(post, F.relu6(pre)) and float(post.min()) == 0.0
    pre, post = seen[tracked[2]][0], seen[tracked[3]][0]
    assert float(pre.min()) < 0 and torch.equal(post, F.relu6(pre))


# --------------------------------------------------------------------------------------------------------------- wrappers
def test_wrappers_refuse_unknown_activation_codes_before_the_library(monkeypatch):
    from pleas_merging_amd import _lib

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_library)
    assert (hip_ops.ACT_NONE, hip_ops.ACT_RELU, hip_ops.ACT_RELU6) == (0, 1, 2)
    x, v, w = torch.zeros(1, 2, 4, 4), torch.ones(2), torch.zeros(2, 2, 1, 1)
    dw = torch.zeros(2, 1, 3, 3)
    for bad in (3, -1, 2.0, None, "relu6", torch.tensor(2)):
        for call in (lambda: hip_ops.bn_act(x, v, v, None, bad), lambda: hip_ops.bn_act_maxpool(x, v, v, (3, 3), 2, 1, bad),
                     lambda: hip_ops.bn_act_tracked(x, v, v, None, bad), lambda: hip_ops.conv2d_bn_act(x, w, None, 1, 0, False, v, v, None, bad),
                     lambda: hip_ops.conv2d_act(x, w, None, 1, 0, False, v, v, None, bad),
                     lambda: hip_ops.dwconv2d(x, dw, None, 1, 1, v, v, None, bad)):
            with pytest.raises(hip_ops.PleasHipError, match="activation"):
                call()
    # the accepted ones get past that check (and are then refused for being CPU tensors, still before the library)
    for good in (False, True, 0, 1, 2, hip_ops.ACT_RELU6):
        with pytest.raises(hip_ops.PleasHipError, match="GPU"):
            hip_ops.bn_act(x, v, v, None, good)
    t = torch.tensor([-1.0, -0.0, 3.0, 6.5, float("inf"), float("-inf"), float("nan")])
    assert torch.equal(_act(t, hip_ops.ACT_RELU6)[:6], torch.tensor([0.0, 0.0, 3.0, 6.0, 6.0, 0.0]))
    assert bool(_act(t, 2)[6].isnan()) and torch.equal(_act(t, True)[:4], torch.relu(t)[:4]) and _act(t, False) is t
