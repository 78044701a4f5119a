"""ReLU6 in the five fused epilogues and through the pipeline, on the GPU.

Kernel arms: self-consistency through the no-activation path, which the existing files hold against fp64.  For identical operands
the code-2 result must be bit for bit ``torch.clamp(result under code 0, 0, 6)`` with NaN in the same places, the code-1 result
bit for bit what ``relu=True`` gives, and a stored ``y`` must not depend on the code.  Operands are ``x = 6 * randn`` with randn
scale, shift and residual; every test asserts on the code-0 result that at least 5 % of the values lie above 6 and 5 % below 0.

End to end: the small inverted-residual network of tests/relu6_cases.py, built like ``test_hip_depthwise.py:_sepnet_job`` and held
to that file's gates (1e-4 rel-fro against the oracle, equal permutations, the same bits twice)."""
import copy
import functools
import os
import sys
import types

import pytest
import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depthwise_cases as dc  # noqa: E402
import relu6_cases as rc  # noqa: E402
import stream_cases as sc  # noqa: E402

from oracle import pleas_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

NONE, RELU, RELU6 = 0, 1, 2


# ------------------------------------------------------------------------------------------------------------ comparisons
def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equal values, NaN in the same places."""
    a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(nan=7.0), b.nan_to_num(nan=7.0))


def _clamped(v0: torch.Tensor) -> torch.Tensor:
    """What code 2 must give where code 0 gave ``v0``: ``torch.clamp(v0, 0, 6)`` on the CPU (a NaN stays)."""
    return torch.clamp(v0.cpu(), 0.0, 6.0)


def _spread(v0: torch.Tensor, what: str) -> None:
    """The code-0 result exercises both bounds: >= 5 % above 6, >= 5 % below 0."""
    v = v0.cpu()
    hi, lo = float((v > 6).float().mean()), float((v < 0).float().mean())
    print("%s: %.0f %% above 6, %.0f %% below 0" % (what, 100 * hi, 100 * lo))
    assert hi >= 0.05 and lo >= 0.05, (what, hi, lo)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


# ----------------------------------------------------------------------------------------------------- bn_act and tracked
# Seeds: those below give at least 5 % above 6 and below 0 on every case (checked on the CPU; each test asserts it on its result).
def _bn_operands(shape, seed, batches=1):
    n, C, inner = shape
    g = torch.Generator().manual_seed(seed)
    x, res = 6 * _randn(g, n, C, inner), _randn(g, n, C, inner)
    scale, shift = (_randn(g, C), _randn(g, C)) if batches == 1 else (_randn(g, batches, C), _randn(g, batches, C))
    return x, scale, shift, res


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("shape", rc.BN_ACT_SHAPES, ids=["scalar_2x5x63", "vec_2x8x16"])
def test_bn_act_codes(shape, with_res):
    from pleas_merging_amd import hip_ops

    x, scale, shift, res = (t.cuda() for t in _bn_operands(shape, 2))
    res = res if with_res else None
    v0 = hip_ops.bn_act(x, scale, shift, res, NONE)
    _spread(v0, "bn_act %s" % (shape,))
    assert torch.equal(v0, hip_ops.bn_act(x, scale, shift, res, False))
    assert _same(hip_ops.bn_act(x, scale, shift, res, RELU6), _clamped(v0))
    assert torch.equal(hip_ops.bn_act(x, scale, shift, res, RELU), hip_ops.bn_act(x, scale, shift, res, True))
    assert torch.equal(hip_ops.bn_act(x, scale, shift, res, RELU), torch.relu(v0))
    assert hip_ops.ACT_RELU6 == RELU6 and hip_ops.ACT_RELU == RELU and hip_ops.ACT_NONE == NONE


@pytest.mark.parametrize("batches", [1, 2], ids=["one_map", "two_batches"])
@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("shape", rc.BN_ACT_SHAPES, ids=["scalar_2x5x63", "vec_2x8x16"])
def test_bn_act_tracked_codes(shape, with_res, batches):
    from pleas_merging_amd import hip_ops

    x, scale, shift, res = (t.cuda() for t in _bn_operands(shape, 1 + batches, batches))
    res = res if with_res else None
    last = lambda out: next(t for t in reversed(out) if t is not None)
    out0 = hip_ops.bn_act_tracked(x, scale, shift, res, NONE)
    v0 = last(out0)
    _spread(v0, "bn_act_tracked %s x %d" % (shape, batches))
    assert torch.equal(v0, hip_ops.bn_act(x, scale, shift, res, NONE))            # the plain pass with [batches][C] maps
    bn6, sum6, act6 = hip_ops.bn_act_tracked(x, scale, shift, res, RELU6)
    bn1, sum1, act1 = hip_ops.bn_act_tracked(x, scale, shift, res, RELU)
    bnT, sumT, actT = hip_ops.bn_act_tracked(x, scale, shift, res, True)
    assert _same(act6, _clamped(v0)) and torch.equal(act1, actT) and torch.equal(act1, torch.relu(v0))
    assert _same(hip_ops.bn_act(x, scale, shift, res, RELU6), act6)
    # the kept values do not depend on the code
    assert torch.equal(bn6, bn1) and torch.equal(bn6, bnT) and torch.equal(bn6, out0[0])
    if with_res:
        assert torch.equal(sum6, v0) and torch.equal(sum1, v0) and torch.equal(sumT, v0)
    else:
        assert sum6 is None and sum1 is None
    # keep_bn=False: the BatchNorm value is not written, the activation is the same
    nb, _, act = hip_ops.bn_act_tracked(x, scale, shift, res, RELU6, keep_bn=False)
    assert nb is None and torch.equal(act, act6)


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("shape", rc.BN_ACT_SHAPES, ids=["scalar_2x5x63", "vec_2x8x16"])
def test_bn_act_edge_values_against_relu6_on_the_cpu(shape, with_res):
    from pleas_merging_amd import hip_ops

    six = torch.tensor(6.0)
    edge = torch.tensor(list(rc.EDGE_VALUES) + [float(torch.nextafter(six, torch.tensor(float("inf")))),
                                                float(torch.nextafter(six, torch.tensor(float("-inf"))))])
    x, scale, shift, res = _bn_operands(shape, 5)
    c = shape[1] - 2
    scale[c], shift[c] = 1.0, 0.0
    x[1, c, 3:3 + len(edge)] = edge
    res[1, c, 3:3 + len(edge)] = 0.0
    want = F.relu6(edge)
    assert torch.equal(want.nan_to_num(nan=7.0), torch.tensor([7.0, 6.0, 0.0, 0.0, 0.0, 6.0, 6.0, 0.0, 6.0, float(edge[-1])])) and float(edge[-1]) < 6.0
    xs, ss, ts, rs = x.cuda(), scale.cuda(), shift.cuda(), (res.cuda() if with_res else None)
    _spread(hip_ops.bn_act(xs, ss, ts, rs, NONE), "bn_act edge values %s" % (shape,))
    for got in (hip_ops.bn_act(xs, ss, ts, rs, RELU6), hip_ops.bn_act_tracked(xs, ss, ts, rs, RELU6)[2],
                hip_ops.bn_act_tracked(xs, torch.stack([ss, ss]), torch.stack([ts, ts]), rs, RELU6)[2]):
        assert _same(got[1, c, 3:3 + len(edge)], want), got[1, c, 3:3 + len(edge)]
        assert _same(got, F.relu6(hip_ops.bn_act(xs, ss, ts, rs, NONE).cpu()))


# ---------------------------------------------------------------------------------------------------------- bn_act_maxpool
POOL_CASES = {"stem": 1, "general": 8}      # tests/stream_cases.BN_ACT_MAXPOOL entries, one per kernel form


def _pool_operands(form):
    N, C, H, W = sc.BN_ACT_MAXPOOL[POOL_CASES[form]]["shape"]
    g = torch.Generator().manual_seed(9)
    x, scale, shift = 6 * _randn(g, N, C, H, W), _randn(g, C), _randn(g, C)
    x[1, 2, 4, 5] = float("nan")                                                  # one window's tap (several windows share it)
    return x, scale, shift


@pytest.mark.parametrize("form", list(POOL_CASES))
def test_bn_act_maxpool_codes(form):
    from pleas_merging_amd import hip_ops

    assert {p[0] for p in sc.reachable("bn_act_maxpool")} == set(POOL_CASES)      # every form the plan query reports
    c = sc.BN_ACT_MAXPOOL[POOL_CASES[form]]
    assert sc.path(sc.plan("bn_act_maxpool", c)[0])[0] == form
    k, stride, pad = c["k"], c["stride"], c["pad"]
    x, scale, shift = (t.cuda() for t in _pool_operands(form))
    v0 = hip_ops.bn_act(x, scale, shift, None, NONE)
    _spread(v0, "bn_act_maxpool %s" % form)
    want = F.max_pool2d(_clamped(v0), k, stride, pad)
    assert int(want.isnan().sum()) >= 1
    assert _same(hip_ops.bn_act_maxpool(x, scale, shift, (k, k), stride, pad, RELU6), want)
    assert _same(hip_ops.bn_act_maxpool(x, scale, shift, (k, k), stride, pad, RELU), hip_ops.bn_act_maxpool(x, scale, shift, (k, k), stride, pad, True))
    assert _same(hip_ops.bn_act_maxpool(x, scale, shift, (k, k), stride, pad, NONE), F.max_pool2d(v0.cpu(), k, stride, pad))


# ----------------------------------------------------------------------------------------------- convolutions' epilogue
def _conv_operands(name: str):
    N, Cin, H, W, Cout, K, stride, pad = rc.CONV_CASES[name]
    g = torch.Generator().manual_seed(11)
    x, w, bias = 6 * _randn(g, N, Cin, H, W), _randn(g, Cout, Cin, K, K), _randn(g, Cout)
    Ho, Wo = (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1
    scale, shift, res = _randn(g, Cout), _randn(g, Cout), _randn(g, N, Cout, Ho, Wo)
    x[0, 1, 2, 3] = float("nan")                           # every output whose window holds it is a NaN, in y and in z
    return x, w, bias, scale, shift, res


def _conv_codes(name: str, with_res: bool):
    from pleas_merging_amd import hip_ops

    N, Cin, H, W, Cout, K, stride, pad = rc.CONV_CASES[name]
    Ho, Wo = (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1
    x, w, bias, scale, shift, res = (t.cuda() for t in _conv_operands(name))
    res = res if with_res else None
    both = lambda code: hip_ops.conv2d_bn_act(x, w, bias, stride, pad, False, scale, shift, res, code)
    only = lambda code: hip_ops.conv2d_act(x, w, bias, stride, pad, False, scale, shift, res, code)
    y0, z0 = both(NONE)
    assert tuple(z0.shape) == (N, Cout, Ho, Wo) and 0 < int(z0.isnan().sum()) < z0.numel() // 2
    _spread(z0, "conv %s" % name)
    y6, z6 = both(RELU6)
    y1, z1 = both(RELU)
    yT, zT = both(True)
    assert _same(z6, _clamped(z0)) and _same(z1, zT)
    assert _same(y6, y0) and _same(y1, y0) and _same(yT, y0)                     # the stored y does not depend on the code
    assert _same(only(RELU6), z6) and _same(only(RELU), z1) and _same(only(NONE), z0) and _same(only(True), zT)
    # the header's contract: z is what the activation pass makes of the stored y, NaN included
    assert _same(z6, hip_ops.bn_act(y0, scale, shift, res, RELU6)) and _same(z0, hip_ops.bn_act(y0, scale, shift, res, NONE))
    assert float(z6.nan_to_num(nan=0.0).max()) == 6.0 and float(z6.nan_to_num(nan=0.0).min()) == 0.0


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("name", list(rc.CONV_CASES))
def test_conv2d_epilogue_codes(name, with_res):
    _conv_codes(name, with_res)


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
def test_conv2d_epilogue_codes_under_split_bf16(with_res):
    from pleas_merging_amd import hip_ops

    with hip_ops.arith(hip_ops.ARITH_SPLIT_BF16):
        _conv_codes("vector", with_res)


def _dw_operands(i: int):
    N, C, H, W, K, s, p = dc.CASES[i]
    Ho, Wo = dc.out_size(H, W, K, s, p)
    g = torch.Generator().manual_seed(20 + i)
    x, w, bias = 6 * _randn(g, N, C, H, W), _randn(g, C, 1, K, K), _randn(g, C)
    scale, shift, res = _randn(g, C), _randn(g, C), _randn(g, N, C, Ho, Wo)
    x[0, C - 1, H // 2, W // 2] = float("nan")
    return x, w, bias, scale, shift, res


@pytest.mark.parametrize("i", rc.DW_CASES, ids=[dc.case_id(dc.CASES[i]) for i in rc.DW_CASES])
def test_dwconv2d_codes_in_its_three_uses(i):
    from pleas_merging_amd import hip_ops

    N, C, H, W, K, s, p = dc.CASES[i]
    x, w, bias, scale, shift, res = (t.cuda() for t in _dw_operands(i))
    y = hip_ops.dwconv2d(x, w, bias, s, p)                                        # y alone
    for r in (res, None):
        z = {}
        for code in (NONE, RELU, RELU6, True):
            y2, z[code] = hip_ops.dwconv2d(x, w, bias, s, p, scale, shift, r, code)                     # y and z
            assert _same(y2, y)
            assert _same(hip_ops.dwconv2d(x, w, bias, s, p, scale, shift, r, code, out=False), z[code])   # z alone
        _spread(z[NONE], "dwconv2d %s" % dc.case_id(dc.CASES[i]))
        assert int(z[NONE].isnan().sum()) >= 1
        assert _same(z[RELU6], _clamped(z[NONE])) and _same(z[RELU], z[True])
        assert _same(z[RELU6], hip_ops.bn_act(y, scale, shift, r, RELU6))


# ------------------------------------------------------------------------------------------------------------- end to end
def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / (b.double().cpu().norm() + 1e-30))


STEM = "features.0.0.weight"


@functools.lru_cache(maxsize=None)
def _job():
    """Data, the two source models (BatchNorm statistics from 3 train-mode batches, then eval), the spec, and the oracle's run at
    ratio 0: assignment, costs, merged and trained state.  The BatchNorm layers in front of an activation get weights of 3 .. 5
    before the statistics are taken, so that the clamp at 6 is met (unit weights leave every activation below it)."""
    from pleas.core.compiler import get_permutation_spec

    g = torch.Generator().manual_seed(3)
    data = [(torch.randn(*rc.SMALL_INPUT, generator=g), torch.zeros(rc.SMALL_INPUT[0], dtype=torch.long)) for _ in range(7)]
    models = []
    for seed in (0, 1):
        torch.manual_seed(seed)
        m = rc.small_mobilenet()
        with torch.no_grad():
            for seq in m.modules():
                if isinstance(seq, nn.Sequential) and len(seq) == 3 and isinstance(seq[2], nn.ReLU6):
                    seq[1].weight.uniform_(3.0, 5.0, generator=g)
        m.train()
        with torch.no_grad():
            for x, _ in data[:3]:
                m(x)
        models.append(m.eval())
    m1, m2 = models
    hit = []
    hooks = [mod.register_forward_hook(lambda mod, i, o: hit.append(float((o == 6).float().mean()))) for mod in m1.modules() if isinstance(mod, nn.ReLU6)]
    with torch.no_grad():
        m1(data[3][0])
    for h in hooks:
        h.remove()
    assert len(hit) == 11 and min(hit) > 0 and sum(1 for h in hit if h > 0.01) >= 6, hit      # every activation clamps at 6 somewhere
    spec = get_permutation_spec(m1, ((2,) + rc.SMALL_INPUT[1:],))
    assert sorted(grp.size for grp in spec.values()) == [8, 8, 48, 48, 48, 48, 1280], {k: grp.size for k, grp in spec.items()}
    perm, costs = orc.activation_matching(spec, m1, m2, data, 3, accumulate=True)
    o3 = orc.partial_merge(spec, m1, m2, perm, costs, 0.0)
    merged = {k: v.clone() for k, v in o3.state_dict().items()}
    o3, _ = orc.train(data, m1, m2, o3, spec, perm, costs, 0.0, 5, num_classes=10)
    return data, m1, m2, spec, perm, costs, merged, {k: v.clone() for k, v in o3.state_dict().items()}


def _matching(m1, m2):
    from pleas.methods.activation_matching import activation_matching
    from pleas_merging_amd import hip_ops

    data, spec = _job()[0], _job()[3]
    with hip_ops.depthwise_form("hip"):
        return activation_matching(spec, copy.deepcopy(m1).cuda(), copy.deepcopy(m2).cuda(), data, 3, output_costs=True)


def _run_job():
    from pleas.methods.partial_matching import partial_merge
    from pleas.methods.pleas_merging import PleasFitter
    from pleas_merging_amd import hip_ops

    data, m1, m2, spec = _job()[:4]
    with hip_ops.depthwise_form("hip"):
        g1, g2 = copy.deepcopy(m1).cuda(), copy.deepcopy(m2).cuda()
        perm, costs = _matching(m1, m2)
        m3 = partial_merge(spec, g1, g2, perm, costs, 0.0)
        fit = PleasFitter(g1, g2, copy.deepcopy(m3), spec, perm, costs, 0.0, 5, num_classes=10)
        vendor_layers = list(fit.vendor_layers)
        n = sum(1 for _ in fit.steps([x for x, _ in data[:6]]))
        got = {k: v.cpu() for k, v in fit.finish().state_dict().items()}
    assert n == 6
    return perm, costs, vendor_layers, got


@functools.lru_cache(maxsize=None)
def _first_run():
    return _run_job()


def test_matching_merge_and_adam_fit_against_the_oracle():
    data, m1, m2, spec, want_perm, want_costs, merged, want = _job()
    perm, costs, vendor_layers, got = _first_run()
    for k in spec:
        assert _rel(costs[k], want_costs[k]) < 1e-4, (k, _rel(costs[k], want_costs[k]))
        assert torch.equal(perm[k].cpu(), want_perm[k]), k
    assert vendor_layers == [], vendor_layers
    worst, moved = 0.0, 0
    for k in want:
        if k == STEM or not want[k].dtype.is_floating_point or torch.equal(want[k], merged[k]):
            continue          # the stem sees the SAME input in both models: its residual is rounding noise (tests/test_hip_odd_layers.py)
        moved += 1
        worst = max(worst, _rel(got[k], want[k]))
        assert _rel(got[k], want[k]) < 1e-4, (k, _rel(got[k], want[k]))
    assert moved >= 15 and sum(1 for k in want if k.endswith("conv.1.0.weight") and not torch.equal(want[k], merged[k])) == 4
    travel = lambda w: float((w.double().cpu() - merged[STEM].double()).abs().max())
    assert travel(got[STEM]) <= 3 * travel(want[STEM]) + 1e-7, (travel(got[STEM]), travel(want[STEM]))
    print("worst trained tensor %.2e rel-fro from the oracle over %d tensors" % (worst, moved))
    # the same job again: the same bits
    perm2, costs2, _, got2 = _run_job()
    assert all(torch.equal(perm[k], perm2[k]) and torch.equal(costs[k], costs2[k]) for k in spec)
    assert all(torch.equal(got[k], got2[k]) for k in got)


def test_in_place_relu6_does_not_disturb_the_matching_costs():
    data, m1, m2, spec = _job()[:4]
    assert all(m.inplace for m in m1.modules() if isinstance(m, nn.ReLU6))
    perm, costs = _first_run()[:2]
    perm2, costs2 = _matching(rc.out_of_place(m1), rc.out_of_place(m2))
    for k in spec:
        assert torch.equal(costs[k], costs2[k]) and torch.equal(perm[k], perm2[k]), k


# ------------------------------------------------------------------------------------------------------------ closed form
def _merged():
    from pleas.methods.partial_matching import partial_merge

    data, m1, m2, spec, perm, costs = _job()[:6]
    g1, g2 = copy.deepcopy(m1).cuda(), copy.deepcopy(m2).cuda()
    costs = {k: v.cuda() for k, v in costs.items()}
    return data, g1, g2, spec, perm, costs, partial_merge(spec, g1, g2, perm, costs, 0.0)


def _train(solver: str):
    from pleas.methods.pleas_merging import train
    from pleas_merging_amd import hip_ops

    data, g1, g2, spec, perm, costs, m3 = _merged()
    with hip_ops.depthwise_form("hip"), hip_ops.depthwise_closed_form("hip"):
        out = train(data[:6], g1, g2, m3, spec, perm, costs, 0.0, False, 5, None, num_classes=10, solver=solver)
    return {k: v.detach().cpu().clone() for k, v in out.state_dict().items()}, out


def _oracle_solution(name: str, ridge: float = 1e-6):
    """Per-channel fp64 solution of a depthwise layer from the oracle's ``layer_targets`` activations on batches 0 .. 5: the
    regularised normal equations of the contract (tests/test_hip_dw_normal_eq.py), ``weight [C, 1, K, K]``."""
    data, m1, m2, spec, perm, costs = _job()[:6]
    blocks = orc.spread_blocks(spec, orc.get_blocks(spec, perm, costs, 0.0))
    a1, a2 = {}, {}
    hooks = orc._hook_inputs(m1, a1) + orc._hook_inputs(m2, a2)
    l1, l2 = orc.get_attr(m1, name.split(".")), orc.get_attr(m2, name.split("."))
    K, s, p = l1.kernel_size[0], l1.stride[0], l1.padding[0]
    assert l1.bias is None
    rows = []
    with torch.no_grad():
        for x, _ in data[:6]:
            m1(x)
            m2(x)
            ip, op = orc.layer_targets(l1, l2, blocks, name, a1[name], a2[name], num_classes=10, merging="perm_gradmask")
            N, C = ip.shape[:2]
            cols = F.unfold(ip.double(), K, padding=p, stride=s)
            L = cols.shape[-1]
            Umat = cols.view(N, C, K * K, L).permute(1, 0, 3, 2).reshape(C, N * L, K * K)
            t = op.double().reshape(N, C, L).permute(1, 0, 2).reshape(C, N * L, 1)
            rows.append(torch.cat([Umat, t], 2))
    for h in hooks:
        h.remove()
    V = torch.cat(rows, 1)
    T = K * K
    G, hvec = V[:, :, :T].transpose(1, 2) @ V[:, :, :T], V[:, :, :T].transpose(1, 2) @ V[:, :, -1:]
    A = G + ridge * G.diagonal(dim1=1, dim2=2).mean(1)[:, None, None] * torch.eye(T, dtype=torch.float64)
    return torch.linalg.solve(A, hvec)[:, :, 0].reshape(-1, 1, K, K)


def test_closed_form_against_the_oracle():
    """As tests/test_hip_dw_normal_eq.py::test_closed_form_of_the_sepnet_against_the_oracle: the job returns, the depthwise layers
    against the per-channel fp64 solution (gate 1e-4), the oracle objective against the Adam fit's, the same job twice."""
    from test_hip_pipeline import _layer_objective

    data, m1, m2, spec, perm, costs, merged = _job()[:7]
    got, m_neq = _train("normal_eq")
    dw = [k[:-len(".weight")] for k in merged if k.endswith("conv.1.0.weight") or k == "features.1.conv.0.0.weight"]
    assert len(dw) == 5
    worst = 0.0
    for name in dw:
        key = name + ".weight"
        assert not torch.equal(got[key], merged[key]), key
        rel = _rel(got[key], _oracle_solution(name))
        worst = max(worst, rel)
        assert rel < 1e-4, (key, rel)
    print("depthwise layers: worst tensor %.2e rel-fro from the per-channel fp64 solution (gate 1e-4)" % worst)
    m_adam = copy.deepcopy(m_neq).cpu()
    m_adam.load_state_dict(_first_run()[3])
    t = types.SimpleNamespace(spec=spec, m1=m1, m2=m2)
    f_init = _layer_objective(t, orc.partial_merge(spec, m1, m2, perm, costs, 0.0), 0.0, perm, costs, data[:6])
    f_adam = _layer_objective(t, m_adam, 0.0, perm, costs, data[:6])
    f_neq = _layer_objective(t, copy.deepcopy(m_neq).cpu(), 0.0, perm, costs, data[:6])
    print("oracle objective: merged %.6g, Adam %.6g, closed form %.6g" % (f_init, f_adam, f_neq))
    assert f_neq <= f_adam * (1 + 1e-4) and f_neq < f_init, (f_init, f_adam, f_neq)
    again, _ = _train("normal_eq")
    assert got.keys() == again.keys() and all(torch.equal(got[k], again[k]) for k in got)


# ------------------------------------------------------------------------------------------------- BN reset and inference
def _merged_cpu():
    data, m1, m2, spec, perm, costs = _job()[:6]
    return orc.partial_merge(spec, m1, m2, perm, costs, 0.0)


@pytest.mark.parametrize("backbone", ["modules", "hip"])
def test_reset_bn_stats_against_the_module_pass(backbone):
    from pleas.methods.extras import reset_bn_stats
    from pleas_merging_amd import hip_ops

    data = _job()[0]
    ref = _merged_cpu()
    ref.train()
    for mod in ref.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.reset_running_stats()
    with torch.no_grad():
        for x, _ in data[:4]:
            ref(x)
    runs = []
    with hip_ops.depthwise_form("hip"):
        for _ in range(2 if backbone == "hip" else 1):
            got = reset_bn_stats(_merged_cpu().cuda(), data, 4, backbone=backbone)
            assert got.training and next(got.parameters()).is_cuda
            runs.append({k: v.cpu() for k, v in got.state_dict().items()})
    want = ref.state_dict()
    worst, checked, zero_means = 0.0, 0, []
    for k, b in want.items():
        if "running_" in k:
            checked += 1
            std = want[k.replace("running_mean", "running_var")].sqrt().norm()
            if k.endswith("running_mean") and float(b.norm()) < 1e-6 * float(std):
                # the batch mean of a bias-free 1 x 1 convolution of train-mode BatchNorm outputs is zero: a linear bottleneck ends in
                # a BatchNorm, and from features.2 on a block's input is such an output or a sum of them (the residual add).  Both
                # sides hold rounding noise there, which is held against the channels' deviation
                zero_means.append(k)
                assert float(runs[0][k].norm()) < 1e-6 * float(std), (k, float(runs[0][k].norm()), float(std))
                continue
            worst = max(worst, _rel(runs[0][k], b))
            assert _rel(runs[0][k], b) < 2e-4, (k, _rel(runs[0][k], b))
        elif k.endswith("num_batches_tracked"):
            assert int(runs[0][k]) == int(b) == 4
    assert checked == 2 * 16 and zero_means == ["features.%s.running_mean" % k for k in ("3.conv.0.1", "4.conv.0.1", "5.conv.0.1", "6.1")], zero_means
    print("BN reset, backbone=%s: worst running statistic %.2e rel-fro from the module pass (gate 2e-4)" % (backbone, worst))
    if backbone == "hip":
        assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0])


def test_inference_backbone_fuses_every_relu6_chain():
    from pleas_merging_amd import hip_ops
    from pleas_merging_amd.methods import source_forward as sf

    data, m1 = _job()[:2]
    net = copy.deepcopy(m1).cuda().eval()
    x = torch.cat([b for b, _ in data[:4]]).cuda()
    with torch.no_grad():
        want = net(x)
    chains = sum(1 for m in net.modules() if isinstance(m, nn.Sequential) and len(m) == 3 and isinstance(m[2], nn.ReLU6))
    with hip_ops.depthwise_form("hip"):
        graph = sf.InferenceBackbone(net)
        nodes = list(graph.graph.graph.nodes)
        fused = [n for n in nodes if n.op == "call_function" and isinstance(n.target, sf.HipConvAct)]
        assert chains == 11 and sum(1 for n in fused if n.args[4] == hip_ops.ACT_RELU6) == chains
        assert sum(1 for n in fused if n.args[4] == hip_ops.ACT_RELU6 and n.target.own.dw) == 5
        assert sum(1 for n in fused if n.args[4] is False) == 5 and len(fused) == 16          # the linear bottlenecks
        left = [n for n in nodes if (n.op == "call_function" and n.target in (F.relu6, F.hardtanh, F.hardtanh_, sf._bn_act))
                or (n.op == "call_module" and isinstance(net.get_submodule(n.target), (nn.Hardtanh, nn.BatchNorm2d, nn.Conv2d)))]
        assert left == [], left
        got = graph(x)
    assert float((got - want).norm() / want.norm()) < 1e-5
    assert torch.equal(got.argmax(1), want.argmax(1))
