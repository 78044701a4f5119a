"""The BN-statistics reset on the library's own kernels (``reset_bn_stats(backbone="hip")``), on the GPU:

1. ``pleas_conv2d_bn_stats_fwd`` on every tile form, weight layout and ``pleas_arith`` mode: ``y`` bit-equal to
   ``pleas_conv2d_fwd``'s, scale / shift / running statistics against an fp64 restatement of ``bn_train_finalize_kernel`` from
   that ``y`` (one fp32 rounding allowed), the counter exact;
2. batches that share a forward, at the smallest shapes where a tile straddles a batch boundary; the refused shape through
   ``HipConvBnStats``'s two-launch path;
3. repeatability, call by call and of the whole pass;
4. the pass end to end against the drivers' loop on the CPU, on the tiny fixture and at ResNet-50 size.

Gates.  The kernel sums ``(double)y`` and ``fma(v, v, .)`` in fp64 in a fixed order; the restatement sums the same fp64 values in
another order.  With |mean| / std of a few (x ~ randn + 2) the two fp64 results agree to ~1e-13 relative, so the fp32 values
rounded from them differ by at most one rounding: |scale - ref| <= 2^-23 |ref|, |shift - ref| <= 2^-23 (|beta| + |mean * scale|),
running statistics within 2^-23 of the restated recursion (floor 2^-23 (|r0| + |stat|)).
"""
import copy

import pytest
import torch

import tile_cases as tc
from oracle import pleas_oracle as orc

pytestmark = pytest.mark.gpu

E23 = 2.0 ** -23
GUARD, SENTINEL = 256, -7.25
EPS = 1e-5


class Guarded:
    """A NaN-filled output with a guard band behind it (one allocation: a tile that writes past its ragged edge lands in it)."""

    def __init__(self, shape):
        n = 1
        for s in shape:
            n *= s
        self.n = n
        self.whole = torch.full((n + GUARD,), SENTINEL, device="cuda")
        self.t = self.whole[:n].view(shape)
        self.t.fill_(float("nan"))

    def intact(self):
        return bool((self.whole[self.n:] == SENTINEL).all())


_OPERANDS = {}


@pytest.fixture(scope="module", autouse=True)
def _operands_released():
    yield
    _OPERANDS.clear()
    torch.cuda.empty_cache()


def _operands(case):
    """x, w (both layouts), bias, BatchNorm weight / bias and starting running statistics of a table case: made once, shared by
    the arithmetics and never written (running statistics are cloned per call).  x ~ randn + 2: channel means of y of a few
    standard deviations, so that E[y^2] - mean^2 does not cancel."""
    if case not in _OPERANDS:
        N, Cout, Cin, H, W, k, stride, pad, bias = case
        g = torch.Generator().manual_seed(hash(case) % (1 << 31))
        w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
        _OPERANDS[case] = dict(
            x=(torch.randn(N, Cin, H, W, generator=g) + 2.0).cuda(), w=w.cuda(),
            wk=w.permute(0, 2, 3, 1).contiguous().cuda() if tc.kpos_legal(case) else None,
            b=(3.0 * torch.randn(Cout, generator=g)).cuda() if bias else None,
            gamma=(0.5 + torch.rand(Cout, generator=g)).cuda(), beta=torch.randn(Cout, generator=g).cuda(),
            rm0=torch.randn(Cout, generator=g).cuda(), rv0=(0.5 + torch.rand(Cout, generator=g)).cuda(),
            out=(N, Cout) + tc.out_hw(H, W, k, stride, pad))
    return _OPERANDS[case]


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _conv(o, w, y, case, kp):
    from pleas_merging_amd import _lib, hip_ops

    N, Cout, Cin, H, W, k, stride, pad = case[:8]
    _lib.check(_lib.lib().pleas_conv2d_fwd(_ptr(o["x"]), _ptr(w), _ptr(o["b"]), _ptr(y), N, Cin, H, W, Cout, k, k, stride, pad,
                                           1 if kp else 0, hip_ops._stream()), "pleas_conv2d_fwd")


class Fold:
    """One ``pleas_conv2d_bn_stats_fwd`` call into its own outputs: ``y`` guarded, running statistics from the case's start."""

    def __init__(self, o, w, case, kp, batches, momentum, seen=7, x=None, rc_only=False):
        from pleas_merging_amd import _lib, hip_ops

        N, Cout, Cin, H, W, k, stride, pad = case[:8]
        x = o["x"] if x is None else x
        N = x.shape[0]
        Ho, Wo = tc.out_hw(H, W, k, stride, pad)
        self.y = Guarded((N, Cout, Ho, Wo))
        self.maps = torch.full((2, batches, Cout), float("nan"), device="cuda")
        self.rm, self.rv = o["rm0"].clone(), o["rv0"].clone()
        self.nbt = torch.tensor(seen, dtype=torch.int64, device="cuda")
        need = int(_lib.lib().pleas_conv2d_bn_stats_ws_bytes(N, Cout, Ho, Wo, batches))
        ws = torch.full((need // 8 + 1,), float("nan"), dtype=torch.float64, device="cuda")
        self.rc = _lib.lib().pleas_conv2d_bn_stats_fwd(
            _ptr(x), _ptr(w), _ptr(o["b"]), _ptr(self.y.t), N, Cin, H, W, Cout, k, k, stride, pad, 1 if kp else 0, batches,
            _ptr(o["gamma"]), _ptr(o["beta"]), EPS, -1.0 if momentum is None else momentum, _ptr(self.rm), _ptr(self.rv),
            _ptr(self.nbt), _ptr(self.maps[0]), _ptr(self.maps[1]), _ptr(ws), need, hip_ops._stream())
        if not rc_only:
            _lib.check(self.rc, "pleas_conv2d_bn_stats_fwd")
        self.scale, self.shift = self.maps[0], self.maps[1]


def restate(y, o, batches, momentum, seen=7):
    """``bn_train_finalize_kernel``'s formulas in fp64 on the host, from ``y``: per batch scale / shift (fp64, with the terms
    their gates are made of), then the running statistics batch by batch with the module's fp32 rounding."""
    N, C = y.shape[:2]
    v = y.double().cpu().view(batches, N // batches, C, -1)
    count = v.shape[1] * v.shape[3]
    mean = v.sum((1, 3)) / count
    var = ((v * v).sum((1, 3)) / count - mean * mean).clamp_min(0.0)
    gamma, beta = o["gamma"].double().cpu(), o["beta"].double().cpu()
    scale = gamma / torch.sqrt(var + EPS)
    shift = beta - mean * scale
    unbiased = var * count / (count - 1.0) if count > 1 else var
    rm0, rv0 = o["rm0"].double().cpu(), o["rv0"].double().cpu()
    rm, rv = rm0.clone(), rv0.clone()
    for b in range(batches):
        f = momentum if momentum is not None else 1.0 / (seen + b + 1)
        rm = ((1.0 - f) * rm + f * mean[b]).float().double()
        rv = ((1.0 - f) * rv + f * unbiased[b]).float().double()
    return dict(scale=scale, shift=shift, shift_gate=E23 * (beta.abs() + (mean * scale).abs()),
                rm=rm, rv=rv, rm_gate=E23 * torch.maximum(rm.abs(), rm0.abs() + mean.abs().amax(0)),
                rv_gate=E23 * torch.maximum(rv.abs(), rv0.abs() + unbiased.abs().amax(0)), count=seen + batches)


WORST = {}      # per output: the largest |got - ref| / gate seen, printed by the tests (a figure, not a check)


def held(f, ref, tag, fails):
    """The gates of the module docstring on one call's outputs; appends (tag, what, worst excess) per miss."""
    for what, got, want, gate in (("scale", f.scale, ref["scale"], E23 * ref["scale"].abs()),
                                  ("shift", f.shift, ref["shift"], ref["shift_gate"]),
                                  ("running_mean", f.rm, ref["rm"], ref["rm_gate"]),
                                  ("running_var", f.rv, ref["rv"], ref["rv_gate"])):
        got = got.double().cpu()
        over = (got - want).abs() - gate
        WORST[what] = max(WORST.get(what, 0.0), float(((got - want).abs() / gate.clamp_min(1e-300)).max()))
        if bool(torch.isnan(got).any()) or float(over.max()) > 0.0:
            fails.append((tag, what, float((over / gate.clamp_min(1e-300)).max())))
    if int(f.nbt) != ref["count"]:
        fails.append((tag, "num_batches_tracked", int(f.nbt)))


# ------------------------------------------------------------------------------------------------ 1. every tile form
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["fp32", "split_bf16", "split_bf16_exact"])
def test_conv2d_bn_stats_on_every_form(mode):
    fails, forms, runs = [], set(), 0
    WORST.clear()
    with tc.arith(mode):
        for case, kp in tc.fwd_runs("conv2d_bn_act"):
            runs += 1
            o = _operands(case)
            w = o["wk"] if kp else o["w"]
            form = tc.fwd_form(case, kp)
            forms.add(form)
            tag = (case, "kpos" if kp else "std", "form %d" % form)
            plain = Guarded(o["out"])
            _conv(o, w, plain.t, case, kp)
            for momentum in (0.1, None):
                f = Fold(o, w, case, kp, 1, momentum)
                if not f.y.intact():
                    fails.append((tag, "guard band written"))
                if bool(torch.isnan(plain.t).any()) or not torch.equal(f.y.t, plain.t):
                    fails.append((tag, "y differs from pleas_conv2d_fwd's"))
                held(f, restate(plain.t, o, 1, momentum), tag + (momentum,), fails)
    torch.cuda.synchronize()
    print("arith %d: %d runs, forms %s, worst |got - ref| / gate %r" % (mode, runs, sorted(forms), WORST))
    assert forms == set(range(10)), forms
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ 2. batches sharing a forward
SHARED = [
    # N, Cout, Cin, H, W, k, stride, pad, batches
    (6, 136, 64, 14, 14, 3, 1, 1, 3),      # 392 pixels per batch: flat k x k form, 128 rows
    (6, 40, 64, 7, 7, 1, 1, 0, 2),         # 147 pixels per batch: scalar pixel path, a 4-pixel group straddles, 64 rows
    (6, 72, 24, 9, 11, 3, 1, 1, 2),        # general tile
    (8, 64, 3, 32, 32, 7, 2, 3, 4),        # stem geometry
]
REFUSED = (6, 40, 64, 3, 3, 1, 1, 0, 2)    # 27 pixels per batch


@pytest.mark.parametrize("shape", SHARED, ids=lambda s: "x".join(map(str, s)))
def test_batches_sharing_a_forward_are_folded_on_their_own_samples(shape):
    case, batches = shape[:8] + (True,), shape[8]
    o = _operands(case)
    n = case[0] // batches
    fails = []
    for kp in tc.fwd_layouts(case):
        w = o["wk"] if kp else o["w"]
        plain = Guarded(o["out"])
        _conv(o, w, plain.t, case, kp)
        for momentum in (0.1, None):
            tag = (kp, momentum)
            f = Fold(o, w, case, kp, batches, momentum)
            assert f.y.intact() and not bool(torch.isnan(plain.t).any()) and torch.equal(f.y.t, plain.t), tag
            ref = restate(plain.t, o, batches, momentum)
            held(f, ref, tag, fails)
            # the same batches as separate calls on their slices
            for b in range(batches):
                one = Fold(o, w, case, kp, 1, momentum, x=o["x"][b * n:(b + 1) * n].clone())
                assert torch.equal(one.y.t, plain.t[b * n:(b + 1) * n]), tag + (b,)
                for what, got, alone, gate in (("scale", f.scale[b], one.scale[0], E23 * ref["scale"][b].abs()),
                                               ("shift", f.shift[b], one.shift[0], ref["shift_gate"][b])):
                    over = (got.double().cpu() - alone.double().cpu()).abs() - gate
                    if float(over.max()) > 0.0:
                        fails.append((tag, b, what + " vs its own call", float((over / gate).max())))
    assert not fails, fails


def test_batches_of_few_pixels_take_the_two_launch_path_bit_for_bit():
    from pleas_merging_amd import hip_ops
    from pleas_merging_amd.methods.source_forward import BatchesPerForward, HipConv, HipConvBnStats

    case, batches = REFUSED[:8] + (True,), REFUSED[8]
    o = _operands(case)
    assert Fold(o, o["w"], case, False, batches, 0.1, rc_only=True).rc == -22
    assert Fold(o, o["w"], case, False, 1, 0.1, rc_only=True).rc == 0          # one batch of 81 pixels is taken
    N, Cout, Cin, H, W, k, stride, pad = case[:8]
    conv = torch.nn.Conv2d(Cin, Cout, k, stride, pad).cuda()
    bn = torch.nn.BatchNorm2d(Cout).cuda().train()
    with torch.no_grad():
        conv.weight.copy_(o["w"])
        conv.bias.copy_(o["b"])
        bn.weight.copy_(o["gamma"])
        bn.bias.copy_(o["beta"])
        bn.running_mean.copy_(o["rm0"])
        bn.running_var.copy_(o["rv0"])
    bn2 = copy.deepcopy(bn)
    state = BatchesPerForward()
    state.parts = batches
    both = HipConvBnStats(HipConv(conv, "c"), bn, "c", state)
    with torch.no_grad():
        y, scale, shift = both(o["x"])
        y2 = HipConv(conv, "c")(o["x"])
        scale2, shift2 = hip_ops.BnTrainFold(bn2)(y2, batches)
    assert both.taken == {"fused": 0, "two_launch": 1, "module": 0}
    assert scale.shape == (batches, Cout) and torch.equal(y, y2) and torch.equal(scale, scale2) and torch.equal(shift, shift2)
    assert torch.equal(bn.running_mean, bn2.running_mean) and torch.equal(bn.running_var, bn2.running_var)
    assert int(bn.num_batches_tracked) == int(bn2.num_batches_tracked) == batches
    ref = restate(y2, o, batches, 0.1, seen=0)
    assert float(((scale.double().cpu() - ref["scale"]).abs() - E23 * ref["scale"].abs()).max()) <= 0.0
    # one batch per forward: the same callable takes the fused kernel
    state.parts = 1
    with torch.no_grad():
        both(o["x"])
    assert both.taken["fused"] == 1


# ------------------------------------------------------------------------------------------------ 3. repeatability
def test_the_same_call_on_moved_operands_returns_the_same_bits():
    for shape in SHARED[:2]:
        case, batches = shape[:8] + (True,), shape[8]
        o = _operands(case)
        kp = tc.kpos_legal(case)
        a = Fold(o, o["wk"] if kp else o["w"], case, kp, batches, 0.1)
        pad_ = torch.empty(12345, device="cuda")       # what follows is allocated somewhere else
        moved = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in o.items()}
        b = Fold(moved, moved["wk"] if kp else moved["w"], case, kp, batches, 0.1)
        del pad_
        assert moved["x"].data_ptr() != o["x"].data_ptr()
        for what, p, q in (("y", a.y.t, b.y.t), ("scale", a.scale, b.scale), ("shift", a.shift, b.shift),
                           ("running_mean", a.rm, b.rm), ("running_var", a.rv, b.rv)):
            assert not bool(torch.isnan(p).any()) and torch.equal(p, q), (shape, what)


def _merged_tiny(t, ratio=0.5):
    return orc.partial_merge(t.spec, t.m1, t.m2, t.per_key("am_perm"), t.per_key("am_cost"), ratio)


def test_the_whole_pass_twice_returns_the_same_bits(tiny_bottleneck):
    from pleas.methods.extras import reset_bn_stats

    t = tiny_bottleneck
    merged = _merged_tiny(t)
    data = [(b[0].cuda(), b[1]) for b in t.batches()]
    runs = [reset_bn_stats(copy.deepcopy(merged).cuda(), data, 101, backbone="hip").state_dict() for _ in range(2)]
    assert any("running_var" in k for k in runs[0])
    for k in runs[0]:
        assert not bool(torch.isnan(runs[0][k].float()).any()) and torch.equal(runs[0][k], runs[1][k]), k


# ------------------------------------------------------------------------------------------------ 4. end to end
def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / (b.double().cpu().norm() + 1e-30))


def _drivers_loop(ref, data, n):
    """run_domainnet.py:327-341 written out: train mode, every BatchNorm reset, n forwards without gradients."""
    ref.train()
    for mod in ref.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.reset_running_stats()
    with torch.no_grad():
        for b in data[:n]:
            ref(b[0].float())
    return ref


def _paths(runner):
    from pleas_merging_amd.methods.source_forward import HipConvBnStats

    taken = {"fused": 0, "two_launch": 0, "module": 0}
    for node in runner.graph.nodes:
        if node.op == "call_function" and isinstance(node.target, HipConvBnStats):
            for k, v in node.target.taken.items():
                taken[k] += v
    return taken


@pytest.fixture
def runners(monkeypatch):
    """The runners ``reset_bn_stats`` builds while the test runs (the graph is not part of its result)."""
    from pleas_merging_amd.methods import extras

    built, make = [], extras._bn_reset_runner

    def spy(*args, **kwargs):
        built.append(make(*args, **kwargs))
        return built[-1]

    monkeypatch.setattr(extras, "_bn_reset_runner", spy)
    return built


def test_bn_reset_hip_backbone_equals_the_drivers_loop_on_the_tiny_fixture(tiny_basic, runners):
    """The recipe of test_hip_extras.test_bn_reset_on_the_merged_cuda_model_equals_the_drivers_loop with ``backbone="hip"``."""
    from pleas.methods.extras import reset_bn_stats
    from pleas.methods.partial_matching import partial_merge
    from pleas.methods.pleas_merging import train

    t = tiny_basic
    perm, costs_c = t.per_key("am_perm"), t.per_key("am_cost")
    costs = {k: v.cuda() for k, v in costs_c.items()}
    m1, m2 = copy.deepcopy(t.m1).cuda(), copy.deepcopy(t.m2).cuda()
    data = t.batches("xt")
    m3 = partial_merge(t.spec, m1, m2, perm, costs, 0.5)
    m3 = train(data, m1, m2, m3, t.spec, perm, costs, 0.5, False, 5, None, num_classes=10).cuda()
    ref = orc.partial_merge(t.spec, t.m1, t.m2, perm, costs_c, 0.5)
    ref, _ = orc.train(data, t.m1, t.m2, ref, t.spec, perm, costs_c, 0.5, 5, num_classes=10)
    with torch.no_grad():      # both sides on the oracle's stem, as in the recipe: the BN pass itself is what is compared
        m3.conv1.weight.copy_(ref.conv1.weight)
    got = reset_bn_stats(m3, data, 101, backbone="hip")
    assert got.training and next(got.parameters()).is_cuda
    taken = _paths(runners[0])
    assert taken["fused"] + taken["two_launch"] > 0 and taken["module"] == 0, taken
    ref = _drivers_loop(ref, data, 101)
    checked = 0
    for (k, a), (_, b) in zip(got.state_dict().items(), ref.state_dict().items()):
        if "running_" in k:
            assert _rel(a, b) < 2e-4, (k, _rel(a, b))
            checked += 1
        elif k.endswith("num_batches_tracked"):
            assert int(a) == int(b) == min(len(data), 101)
    assert checked >= 10


@pytest.fixture(scope="module")
def rn50_merged():
    """A merged ResNet-50 (ratio 0.5), 4 batches of 4 at 96 x 96, and the drivers' loop on the CPU: made once."""
    from pleas.core.compiler import get_permutation_spec
    from pleas.core.utils import make_identity_perm
    from pleas_merging_amd import resnet as zoo

    g = torch.Generator().manual_seed(3)
    data = [(torch.randn(4, 3, 96, 96, generator=g), None) for _ in range(4)]
    models = []
    for seed in (0, 1):
        torch.manual_seed(seed)
        m = zoo.MODELS["resnet50"](num_classes=1000)
        zoo.calibrate_bn(m, [d[0] for d in data[:2]])
        models.append(m.eval())
    spec = get_permutation_spec(models[0], ((1, 3, 96, 96),))
    perm = make_identity_perm(spec)
    costs = {k: torch.eye(grp.size) + 0.01 * torch.rand(grp.size, grp.size, generator=g) for k, grp in spec.items()}
    merged = orc.partial_merge(spec, models[0], models[1], perm, costs, 0.5)
    ref = _drivers_loop(copy.deepcopy(merged), data, 4).state_dict()
    return merged, data, ref


@pytest.mark.parametrize("per_forward", [None, 1, 3])
def test_bn_reset_hip_backbone_rn50_size_vs_the_drivers_loop(rn50_merged, runners, per_forward):
    """layer4's 3 x 3 maps hold 36 pixels per batch: batches that share a forward take the two-launch path there, while
    layer3's (144 pixels) and everything above take the fused kernel."""
    from pleas.methods.extras import reset_bn_stats

    merged, data, ref = rn50_merged
    got = reset_bn_stats(copy.deepcopy(merged).cuda(), data, 4, batches_per_forward=per_forward, backbone="hip")
    assert got.training and next(got.parameters()).is_cuda
    taken = _paths(runners[0])
    assert taken["module"] == 0 and taken["fused"] > 0, taken
    assert (taken["two_launch"] > 0) == (per_forward != 1), taken
    worst, n_bn = 0.0, 0
    for (k, a), (_, b) in zip(got.state_dict().items(), ref.items()):
        if "running_" in k:
            worst = max(worst, _rel(a, b))
        elif k.endswith("num_batches_tracked"):
            assert int(a) == int(b) == 4
            n_bn += 1
    print("rn50 merged (ratio 0.5) BN reset, backbone=hip, per forward %s: worst running-statistic rel-fro %.2e, paths %r"
          % (per_forward, worst, taken))
    assert n_bn == 53 and worst < 2e-4, worst


def test_a_hooked_convolution_still_hands_its_output_to_the_hook(tiny_bottleneck):
    from pleas_merging_amd.methods.source_forward import fuse_bn_act

    model = copy.deepcopy(tiny_bottleneck.m1).cuda().train()
    plain = copy.deepcopy(model)
    gm = fuse_bn_act(model, train_stats=True, train_convs=True)
    x = tiny_bottleneck.batches()[0][0].cuda()
    seen = {}
    handle = model.layer1[0].conv2.register_forward_hook(lambda mod, inp, out: seen.setdefault("y", out))
    with torch.no_grad():
        out = gm(x)
    handle.remove()
    taps = {}
    handle = plain.layer1[0].conv2.register_forward_hook(lambda mod, inp, out: taps.setdefault("y", out))
    with torch.no_grad():
        want = plain(x)
    handle.remove()
    assert "y" in seen and seen["y"].shape == taps["y"].shape and _rel(seen["y"], taps["y"]) < 1e-5
    assert _rel(out, want) < 1e-4
    for (k, a), (_, b) in zip(model.state_dict().items(), plain.state_dict().items()):
        if "running_" in k:
            assert _rel(a, b) < 2e-4, k
