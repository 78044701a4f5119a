"""Evaluation of merged models on the library's own kernels (``backbone="hip"`` of the helpers in methods/evaluation.py;
reference pleas/methods/pleas_merging.py:436-496, :499-586), kernel by kernel and end to end:

* ``pleas_conv2d_act_fwd`` -- the image-only epilogue -- bit-equal to the ``z`` of ``pleas_conv2d_bn_act_fwd`` on every tile
  form, weight layout and ``pleas_arith`` mode; the sample-axis split of ``hip_ops.conv2d_act`` bit-equal to one call;
* ``pleas_pool_gather`` against fp64, ``pleas_top1_count`` against ``torch.argmax`` on the CPU;
* the inference graph: hooks still get the convolution's output; a ResNet-50-sized merged model against fp64, stale constants
  caught, ``refresh()``; the three helpers on the tiny fixtures.
"""
import copy

import pytest
import torch

import tile_cases as tc
from oracle import pleas_oracle as orc

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GUARD, SENTINEL = 256, -7.25


@pytest.fixture(scope="module")
def ops():
    from pleas_merging_amd import hip_ops

    return hip_ops


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


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


# ------------------------------------------------------------------------------------------------ 1. image-only convolution
_OPERANDS = {}


@pytest.fixture(scope="module", autouse=True)
def _operands_released():
    yield
    _OPERANDS.clear()
    torch.cuda.empty_cache()


def _operands(case):
    """x, w (both layouts), bias, scale, shift and an identity of a table case: made once, shared by the three arithmetics."""
    if case not in _OPERANDS:
        N, Cout, Cin, H, W, k, stride, pad, bias = case
        Ho, Wo = tc.out_hw(H, W, k, stride, pad)
        g = torch.Generator().manual_seed(hash(case) % (1 << 31))
        w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
        _OPERANDS[case] = dict(
            x=torch.randn(N, Cin, H, W, generator=g).cuda(), w=w.cuda(),
            wk=w.permute(0, 2, 3, 1).contiguous().cuda() if tc.kpos_legal(case) else None,
            b=torch.randn(Cout, generator=g).cuda() if bias else None, scale=(0.5 + torch.rand(Cout, generator=g)).cuda(),
            shift=torch.randn(Cout, generator=g).cuda(), res=torch.randn(N, Cout, Ho, Wo, generator=g).cuda(), out=(N, Cout, Ho, Wo))
    return _OPERANDS[case]


def _launch(name, o, w, y, identity, z, relu, case, kp):
    from pleas_merging_amd import _lib, hip_ops

    N, Cout, Cin, H, W, k, stride, pad = case[:8]
    ptr = lambda t: t.data_ptr() if t is not None else None
    outs = (ptr(y),) if name == "pleas_conv2d_bn_act_fwd" else ()
    args = (ptr(o["x"]), ptr(w), ptr(o["b"])) + outs + (ptr(o["scale"]), ptr(o["shift"]), ptr(identity), ptr(z), 1 if relu else 0,
                                                        N, Cin, H, W, Cout, k, k, stride, pad, 1 if kp else 0, hip_ops._stream())
    _lib.check(getattr(_lib.lib(), name)(*args), name)


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["fp32", "split_bf16", "split_bf16_exact"])
def test_conv2d_act_is_the_z_of_conv2d_bn_act_on_every_form(mode):
    """Same arithmetic, one output fewer: no tolerance.  Fails where ``pleas_conv2d_act_fwd`` does not exist."""
    fails, forms = [], set()
    with tc.arith(mode):
        for case, kp in tc.fwd_runs("conv2d_bn_act"):
            o = _operands(case)
            w = o["wk"] if kp else o["w"]
            form = tc.fwd_form(case, kp)
            forms.add(form)
            tag = (case, "kpos" if kp else "std", "form %d" % form)
            for identity, relu in ((None, True), (o["res"], True), (None, False), (o["res"], False)):
                y, z2, z = Guarded(o["out"]), Guarded(o["out"]), Guarded(o["out"])
                _launch("pleas_conv2d_bn_act_fwd", o, w, y.t, identity, z2.t, relu, case, kp)
                _launch("pleas_conv2d_act_fwd", o, w, None, identity, z.t, relu, case, kp)
                if not z.intact():
                    fails.append((tag, "guard band written", identity is not None, relu))
                if bool(torch.isnan(z2.t).any()) or not torch.equal(z.t, z2.t):
                    fails.append((tag, "z differs from pleas_conv2d_bn_act_fwd's", identity is not None, relu))
    torch.cuda.synchronize()
    assert forms == set(range(10)), forms
    assert not fails, fails


@pytest.mark.parametrize("mode", [0, 1])
def test_conv2d_act_splits_a_batch_along_the_sample_axis(ops, mode):
    """N = 5 on a 14 x 14 layer with the wrapper's limit lowered to just over two samples: calls of 2 + 2 + 1 samples into
    one z, bit-equal to the single call."""
    case = (5, 200, 96, 14, 14, 1, 1, 0, False) if mode == 0 else (5, 136, 64, 14, 14, 3, 1, 1, False)
    assert case in tc.FWD_TABLE
    o = _operands(case)
    N, Cout, Cin, H, W, k, stride, pad, _ = case
    per = Cout * H * W
    assert ops.conv2d_sample_split(N, per, H * W, 2 * per + 1) == [(0, 2), (2, 2), (4, 1)]
    with tc.arith(mode):
        for kp in tc.fwd_layouts(case):
            w = o["wk"] if kp else o["w"]
            for identity in (None, o["res"]):
                one = ops.conv2d_act(o["x"], w, o["b"], stride, pad, kp, o["scale"], o["shift"], identity, True)
                parts = ops.conv2d_act(o["x"], w, o["b"], stride, pad, kp, o["scale"], o["shift"], identity, True, _limit=2 * per + 1)
                assert not bool(torch.isnan(one).any()) and torch.equal(one, parts), (kp, identity is not None)
                _, z = ops.conv2d_bn_act(o["x"], w, o["b"], stride, pad, kp, o["scale"], o["shift"], identity, True)
                assert torch.equal(one, z)


def test_conv2d_bn_act_refuses_a_strided_scale_before_any_launch(ops, monkeypatch):
    """The image operands are checked once for both epilogues: a ``scale`` / ``shift`` that is a strided view (every other element
    of a longer vector) would be read as if it were dense, so it is refused on the host and the entry point is never reached."""
    from pleas_merging_amd import _lib

    case = (16, 40, 64, 1, 1, 1, 1, 0, True)      # the smallest of the table
    assert case in tc.FWD_TABLE and case == min(tc.FWD_TABLE, key=lambda c: c[0] * c[1] * c[2] * c[3] * c[4] * c[5] ** 2)
    o = _operands(case)
    N, Cout, Cin, H, W, k, stride, pad, _ = case
    strided = torch.ones(2 * Cout, device="cuda")[::2]
    assert strided.numel() == Cout and not strided.is_contiguous()

    def reached(*args):
        raise AssertionError("the entry point was called")

    for name in ("pleas_conv2d_bn_act_fwd", "pleas_conv2d_act_fwd"):
        monkeypatch.setattr(_lib.lib(), name, reached, raising=True)
    for scale, shift in ((strided, o["shift"]), (o["scale"], strided)):
        with pytest.raises(ops.PleasHipError):
            ops.conv2d_bn_act(o["x"], o["w"], o["b"], stride, pad, False, scale, shift, None, True)
        with pytest.raises(ops.PleasHipError):
            ops.conv2d_act(o["x"], o["w"], o["b"], stride, pad, False, scale, shift, None, True)


# ------------------------------------------------------------------------------------------------ 2. pool_gather
@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("C", [10, 2048])
@pytest.mark.parametrize("HW", [1, 49, 64, 196])
def test_pool_gather_vs_fp64(ops, HW, C, N):
    """|got - want| <= gamma(HW + 1) * sum|x| / HW, gamma(n) = n u / (1 - n u): HW - 1 additions in any order and one
    division (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2)."""
    g = torch.Generator().manual_seed(1000 * HW + 10 * C + N)
    side = {1: (1, 1), 49: (7, 7), 64: (8, 8), 196: (14, 14)}[HW]
    x = (torch.randn(N, C, *side, generator=g) + 0.5).cuda()
    mean = x.double().flatten(2).mean(2)
    bound = (HW + 1) * U / (1 - (HW + 1) * U) * x.double().abs().flatten(2).sum(2) / HW
    order = torch.cat([torch.arange(C - 1, -1, -1), torch.tensor([0, 0, C - 1, 3, 3])])      # reversed, then repeats
    for src in (None, order.to(torch.int32).cuda(), ops.channel_map(order, C, "cuda")):
        got = ops.pool_gather(x, src)
        want, lim = (mean, bound) if src is None else (mean[:, order.cuda()], bound[:, order.cuda()])
        assert got.shape == want.shape and got.dtype == torch.float32
        assert bool(((got.double() - want).abs() <= lim).all()), float(((got.double() - want).abs() - lim).max())
        assert torch.equal(got, ops.pool_gather(x, src))          # fixed summation order: the same bits again
    if HW == 1:
        assert torch.equal(ops.pool_gather(x), x.flatten(1))
    for bad in ([0, C], [-1, 0]):
        with pytest.raises(ops.PleasHipError):
            ops.pool_gather(x, torch.tensor(bad, dtype=torch.int32).cuda())
        with pytest.raises(ops.PleasHipError):
            ops.channel_map(bad, C, "cuda")


# ------------------------------------------------------------------------------------------------ 3. top1_count
def _top1_rows(C, n, g):
    """n rows of logits [C]: the first ones planted (exact ties, all equal, NaN, -inf), the rest random."""
    rows = torch.randn(n, C, generator=g)
    a, b = C // 3, (2 * C) // 3          # a <= b; equal when C == 1
    plant = []
    tie = rows[0].clone()
    tie[a] = tie[b] = 9.0                # two exact maxima: the first index wins
    plant.append(tie)
    tie3 = rows[0].clone()
    tie3[b] = tie3[C - 1] = tie3[a] = 7.5
    plant.append(tie3)
    plant.append(torch.full((C,), 0.25))                       # every column maximal: index 0
    nan = rows[0].clone()
    nan[b] = float("nan")                                      # a NaN counts as maximal
    plant.append(nan)
    nans = rows[0].clone()
    nans[b] = nans[C - 1] = float("nan")                       # the first NaN
    nans[a] = float("inf") if a != b else nans[a]
    plant.append(nans)
    plant.append(torch.full((C,), float("-inf")))              # index 0
    low = torch.full((C,), float("-inf"))
    low[C - 1] = -3.0
    plant.append(low)
    big = rows[0].clone()
    big[C - 1] = float("inf")                                  # the maximum in the last column (a partial last stride of 64)
    plant.append(big)
    return torch.stack(plant), rows


@pytest.mark.parametrize("N", [1, 37])
@pytest.mark.parametrize("C", [1, 10, 1000, 1003])
def test_top1_count_vs_torch_argmax(ops, C, N):
    g = torch.Generator().manual_seed(7 * C + N)
    plant, rows = _top1_rows(C, 37, g)
    if N == 1:
        batches = [r[None] for r in plant] + [rows[:1]]         # every planted row as a batch of its own
    else:
        rows[:len(plant)] = plant
        batches = [rows, rows.flip(0).contiguous()]
    hits = torch.zeros(1, dtype=torch.long, device="cuda")
    total = 0
    for i, logits in enumerate(batches):
        want = logits.argmax(1)                                    # CPU
        labels = want.clone()
        wrong = torch.arange(logits.shape[0]) % 3 == 1
        labels[wrong] = (labels[wrong] + 1) % max(C, 2)            # C == 1: label 1, never predicted
        if N == 1 and i % 2:
            labels = (want + 1) % max(C, 2)
        total += int((want == labels).sum())
        pred = torch.full((logits.shape[0],), -5, dtype=torch.long, device="cuda") if i % 2 == 0 else None   # pred is optional
        out = ops.top1_count(logits.cuda(), labels.cuda(), hits, pred)
        assert out is hits
        if pred is not None:
            assert torch.equal(pred.cpu(), want), (i, pred.cpu().tolist(), want.tolist())
        assert int(hits[0]) == total, (i, int(hits[0]), total)    # calls accumulate into the same counter
    assert total > 0
    with pytest.raises(ops.PleasHipError):
        ops.top1_count(batches[0].cuda(), torch.zeros(batches[0].shape[0], dtype=torch.int32, device="cuda"), hits)


# ------------------------------------------------------------------------------------------------ 4. hooks
def test_a_hooked_convolution_still_hands_its_output_to_the_hook(ops, tiny_bottleneck):
    from pleas_merging_amd.methods.source_forward import InferenceBackbone

    model = copy.deepcopy(tiny_bottleneck.m1).cuda().eval()
    x = tiny_bottleneck.batches()[0][0].cuda()
    ib = InferenceBackbone(model)
    plain = ib(x)
    conv = model.layer2[0].conv2
    seen = []
    handle = conv.register_forward_hook(lambda mod, inp, out: seen.append((inp[0], out)))
    hooked = ib(x)
    handle.remove()
    assert len(seen) == 1
    inp, y = seen[0]
    assert torch.equal(y, ops.conv2d(inp, conv.weight.detach(), conv.bias, conv.stride[0], conv.padding[0]))
    assert torch.equal(hooked, plain)
    assert torch.equal(ib(x), plain) and len(seen) == 1           # hook removed: the image-only path again
    with torch.no_grad():
        assert _rel(plain, model(x)) < 1e-5


# ------------------------------------------------------------------------------------------------ 5. helpers, known answer
MARGIN = 1e-3


def _confident(logits64):
    """Samples whose fp64 top-2 margin exceeds MARGIN of the largest |logit|: their label does not hang on fp32 rounding."""
    top = logits64.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) > MARGIN * logits64.abs().max()


def _labelled_batches(t, source):
    """Inputs with labels from an fp64 CPU forward of ``source``, kept where the label is confident: the fixture's batches if
    the fp64 reference itself leaves out at most one sample in ten, else the first seeded draw that does (chosen on the CPU)."""
    ref = copy.deepcopy(source).double().eval()
    shape = t.batches()[0][0].shape
    draws = [[b[0] for b in t.batches()]] + [[torch.randn(shape, generator=torch.Generator().manual_seed(50 + s + i)) for i in range(4)]
                                              for s in range(0, 400, 10)]
    for xs in draws:
        with torch.no_grad():
            logits = [ref(x.double()) for x in xs]
        keep = [_confident(l) for l in logits]
        total, kept = sum(k.numel() for k in keep), sum(int(k.sum()) for k in keep)
        if 10 * (total - kept) <= total:
            return [(x[k], l.argmax(1)[k]) for x, l, k in zip(xs, logits, keep) if bool(k.any())], total, kept
    raise AssertionError("no draw with confident labels")


def test_eval_helpers_hip_backbone_known_answer(ops, tiny_bottleneck):
    """The construction of test_eval_helpers_on_a_merged_cuda_backbone_known_answer (model2 = model1 with every group permuted,
    merged at ratio 0.5, fc -> Identity) through ``backbone="hip"``: each source head gets its own feature order from ONE
    pool_gather, accuracy exactly 1 on the samples whose fp64 label is confident, features equal to the source backbone's."""
    from pleas.core.utils import apply_perm, make_random_perm
    from pleas.methods.activation_matching import activation_matching
    from pleas.methods.partial_matching import partial_merge
    from pleas.methods.pleas_merging import (InferenceBackbone, eval_perm_model, eval_whole_model, final_feature_map, get_fc_perm,
                                             permute_final_features)

    t = tiny_bottleneck
    c1 = copy.deepcopy(t.m1)
    c2 = copy.deepcopy(c1)
    apply_perm(make_random_perm(t.spec, torch.Generator().manual_seed(3)), t.spec, c2, inplace=True)
    m1, m2 = copy.deepcopy(c1).cuda().eval(), copy.deepcopy(c2).cuda().eval()
    perm, costs = activation_matching(t.spec, m1, m2, t.batches(), 2, output_costs=True)
    m3 = partial_merge(t.spec, m1, m2, perm, costs, 0.5, device="cuda")
    fc_perm = get_fc_perm(perm, t.spec, costs, 0.5)
    backbone = copy.deepcopy(m3)
    backbone.fc = torch.nn.Identity()
    width = len(fc_perm[0]) + 2 * len(fc_perm[2])
    for idx, (src, cpu_src) in enumerate(((m1, c1), (m2, c2))):
        loader, total, kept = _labelled_batches(t, cpu_src)
        print("head %d: %d of %d samples counted" % (idx, kept, total))
        assert 10 * (total - kept) <= total
        # pinned host batches: copied without blocking the host, in stream order
        loader = [(x.pin_memory(), y.pin_memory()) for x, y in loader]
        x0 = loader[0][0].cuda()
        body = copy.deepcopy(src)
        body.fc = torch.nn.Identity()
        ib = InferenceBackbone(backbone)
        assert ib.gather_features(ops.channel_map(final_feature_map(fc_perm, idx), width, "cuda"))
        feats = ib(x0)
        with torch.no_grad():
            assert feats.is_cuda and _rel(feats, body(x0)) < 1e-5, idx
            assert _rel(feats, permute_final_features(backbone(x0), fc_perm, idx)) < 1e-5, idx
        acc = eval_perm_model(backbone, src.fc, loader, 10, fc_perm, idx, backbone="hip")
        assert acc.is_cuda and acc.dim() == 0 and float(acc) == 1.0, float(acc)
        whole = eval_whole_model(src, loader, 10, backbone="hip")
        assert not whole.is_cuda and float(whole) == 1.0, float(whole)
        # and a loader that is half wrong counts half
        flipped = [(x, (y + (torch.arange(y.numel()) % 2)) % 10) for x, y in loader]
        wrong = sum(int((torch.arange(y.numel()) % 2).sum()) for _, y in loader)
        assert abs(float(eval_perm_model(backbone, src.fc, flipped, 10, fc_perm, idx, backbone="hip")) - (kept - wrong) / kept) < 1e-6


# ------------------------------------------------------------------------------------------------ 6. ResNet-50 size
def test_inference_graph_rn50_size_vs_fp64_and_refresh():
    """Merged ResNet-50 (ratio 0.5: widths 1.5x), batch 2 at 224 x 224: logits of the inference graph against an fp64 CPU
    forward of the same modules, gate max(3 x the module path's own distance from fp64 on this GPU, 2e-6); the same call twice
    gives the same bits; after ``reset_bn_stats`` a stale graph misses the gate and ``refresh()`` meets it again."""
    from pleas.core.compiler import get_permutation_spec
    from pleas.core.utils import make_identity_perm
    from pleas.methods.extras import reset_bn_stats
    from pleas_merging_amd import resnet as zoo
    from pleas_merging_amd.methods.source_forward import InferenceBackbone

    g = torch.Generator().manual_seed(3)
    data = [(torch.randn(2, 3, 224, 224, generator=g), None) for _ in range(4)]
    models = []
    for seed in (0, 1):
        torch.manual_seed(seed)
        m = zoo.MODELS["resnet50"](num_classes=1000)
        zoo.calibrate_bn(m, [d[0] for d in data[:2]])
        models.append(m.eval())
    spec = get_permutation_spec(models[0], ((1, 3, 224, 224),))
    perm = make_identity_perm(spec)
    costs = {k: torch.eye(grp.size) + 0.01 * torch.rand(grp.size, grp.size, generator=g) for k, grp in spec.items()}
    merged = orc.partial_merge(spec, models[0], models[1], perm, costs, 0.5).eval()
    x = data[0][0]

    def fp64(model):
        ref = copy.deepcopy(model).cpu().double().eval()
        with torch.no_grad():
            return ref(x.double())

    def gate(model, want):
        with torch.no_grad():
            own = _rel(model(x.cuda()), want)
        return max(3 * own, 2e-6), own

    got = copy.deepcopy(merged).cuda().eval()
    want = fp64(got)
    ib = InferenceBackbone(got)
    assert ib.graph is not None
    logits = ib(x.cuda())
    lim, own = gate(got, want)
    print("rn50 merged, inference graph %.3e from fp64 (modules %.3e, gate %.3e)" % (_rel(logits, want), own, lim))
    assert logits.shape == (2, 1000) and _rel(logits, want) <= lim
    assert torch.equal(ib(x.cuda()), logits)
    # new running statistics: the graph's constants are those of the day it was built
    reset_bn_stats(got, data[2:], 2)
    got.eval()
    want2 = fp64(got)
    lim2, own2 = gate(got, want2)
    stale = ib(x.cuda())
    print("after reset_bn_stats: stale graph %.3e from the new fp64 logits (gate %.3e)" % (_rel(stale, want2), lim2))
    assert _rel(stale, want2) > lim2
    fresh = ib.refresh()(x.cuda())
    print("refreshed graph %.3e (modules %.3e)" % (_rel(fresh, want2), own2))
    assert not torch.equal(fresh, logits) and _rel(fresh, want2) <= lim2


# ------------------------------------------------------------------------------------------------ 7. linear probe
class _Run:
    def __init__(self):
        self.logs = []

    def log(self, metrics):
        self.logs.append(dict(metrics))


def test_linear_probe_hip_backbone_vs_modules(tiny_bottleneck):
    from pleas.methods.pleas_merging import InferenceBackbone, train_eval_linear_probe

    t = tiny_bottleneck
    cpu = copy.deepcopy(t.m1)
    cpu.fc = torch.nn.Identity()
    model = copy.deepcopy(cpu).cuda().eval()
    g = torch.Generator().manual_seed(5)
    train = [(b[0], torch.randint(0, 10, (b[0].shape[0],), generator=g)) for b in t.batches()]
    test = train[:2]
    # the features either backbone hands the head, against fp64 (the gate of the ResNet-50 test)
    ref = copy.deepcopy(cpu).double().eval()
    ib = InferenceBackbone(model)
    for x, _ in train[:2]:
        with torch.no_grad():
            want = ref(x.double())
            own = _rel(model(x.cuda()), want)
        rel = _rel(ib(x.cuda()), want)
        print("probe features: hip %.3e, modules %.3e from fp64" % (rel, own))
        assert rel <= max(3 * own, 2e-6)
    heads, runs = {}, {}
    for backbone in ("modules", "hip"):
        torch.manual_seed(0)                       # the same fresh head
        runs[backbone] = _Run()
        heads[backbone] = train_eval_linear_probe(model, train, test, 10, runs[backbone], "tiny", epochs=2, backbone=backbone)
    assert [sorted(d) for d in runs["hip"].logs] == [sorted(d) for d in runs["modules"].logs] and len(runs["hip"].logs) == 3
    assert _rel(heads["hip"].weight, heads["modules"].weight) <= 1e-4
    assert _rel(heads["hip"].bias, heads["modules"].bias) <= 1e-4
    for a, b in zip(runs["hip"].logs, runs["modules"].logs):
        assert all(abs(a[k] - b[k]) <= 1e-4 * max(1.0, abs(b[k])) for k in a if k.endswith("loss")), (a, b)
