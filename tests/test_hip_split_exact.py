"""``pleas_arith(PLEAS_ARITH_SPLIT_BF16_EXACT)``: the split-bf16 kernels with all nine bf16 products of every fp32 product
(csrc/common.hpp, split3_mfma<9>).  Every bf16 x bf16 product is exact in fp32 and the three planes sum exactly to the operand,
so the only rounding left is the fp32 accumulation: the mode is held to the EXACT arithmetic's derived element-wise bound
gamma_K (tests/test_hip_tile_forms.py) wherever that is tighter than the split kernels' measured one, through every entry
point, form and variant (a), through the matching contraction (b); it is a third arithmetic that goes away again (c), also on
operands whose true result is exactly representable (d: tests/split_exact_cases.py, preconditions and the emulated nine-product
sum in tests/test_arith_exact_host.py; on the MI355X the MFMA's own adder keeps the mode from reproducing that result bit for
bit, see the test's docstring).

Measured on an MI355X (printed again on every run), worst element-wise ratio |got - want| / sum |x_i w_i| of the nine-product
kernels over the table + the random draw: see DESIGN.md 3.7."""
import pytest
import torch

import split_exact_cases as sx
import test_hip_tile_forms as tf
import tile_cases as tc
from oracle import pleas_oracle as orc

pytestmark = pytest.mark.gpu

MODE = 2
U = tf.U


@pytest.fixture(scope="module")
def ops():
    from pleas_merging_amd import hip_ops

    return hip_ops


@pytest.fixture(scope="module", autouse=True)
def _references_released():
    yield
    tf._FWD_REF.clear()
    tf._WG_REF.clear()
    torch.cuda.empty_cache()


def _split_fwd(form):
    return form in tf.SPLIT_FWD_FORMS


# ------------------------------------------------------------------------------------------------ a. every form and variant
def _fwd_batch_group(ops, runs, fails, worst):
    """tf._fwd_batch_group under mode 2: split forms within min(gamma_K, FWD_SPLIT_BOUND), the others within gamma_K."""
    from pleas_merging_amd.methods.partial_matching import block_maps

    batch = ops.FwdBatch(torch.device("cuda"))
    held = []
    for case, kp in runs:
        N, Cout, Cin, H, W, k, stride, pad, bias = case
        ref = tf.fwd_ref(case)
        Ho, Wo = tc.out_hw(H, W, k, stride, pad)
        g = torch.Generator().manual_seed(ref["seed"] + 1)
        ns = Cout // 5
        nm = Cout - 2 * ns
        Csrc = nm + ns
        pm = torch.randperm(Csrc, generator=g)
        blk = (torch.arange(nm), pm[:nm], torch.arange(nm, Csrc), pm[nm:])
        o1, o2 = torch.randn(N, Csrc, Ho, Wo, generator=g).cuda(), torch.randn(N, Csrc, Ho, Wo, generator=g).cuda()
        blkc = [t.cuda() for t in blk]
        target = torch.cat([(o1.double()[:, blkc[0]] + o2.double()[:, blkc[1]]) / 2, o1.double()[:, blkc[2]], o2.double()[:, blkc[3]]], 1)
        r1, r2, nmerged = block_maps(blk, "cuda")
        numel = ref["out"].numel()
        resid = tf.Guarded((N, Cout, Ho, Wo))
        batch.add(ref["x"], ref["wk"] if kp else ref["w"], ref["b"], o1, o2, r1, r2, nmerged, resid.t, 2.0 / numel, 1.0 / numel,
                  (k, k), stride, pad, flags=ops.FwdBatch.KPOS_MAJOR if kp else 0)
        held.append((case, kp, ref, target, resid, numel, (o1, o2, r1, r2)))
    loss = torch.full((len(held),), float("nan"), device="cuda")
    batch.flush(loss)
    torch.cuda.synchronize()
    for i, (case, kp, ref, target, resid, numel, _keep) in enumerate(held):
        form = tc.fwd_form(case, kp)
        tag = (case, "kpos" if kp else "std", "form %d" % form)
        dscale = 2.0 / numel
        want = dscale * (ref["out"] - target)
        want_loss = float(((ref["out"] - target) ** 2).mean())
        K = case[2] * case[5] * case[5]
        split = _split_fwd(form)
        c = min(tf.gamma(K), tf.FWD_SPLIT_BOUND) if split else tf.gamma(K)
        bound = dscale * ((c + 5 * U) * ref["S"] + 5 * U * target.abs())
        ok, err = tf._elementwise(resid.t, want, bound)
        ratio = float((err / (dscale * (ref["S"] + target.abs())).clamp_min(1e-300)).max())
        worst[1 if split else 0] = max(worst[1 if split else 0], ratio)
        worst[2] += 1
        rel = tf._rel(resid.t, want)
        if not resid.intact():
            fails.append((tag, "guard band written"))
        if not ok:
            fails.append((tag, "element-wise bound missed: worst ratio %.3e" % ratio))
        if not rel < 5e-6:
            fails.append((tag, "residual %.3e from fp64" % rel))
        if not abs(float(loss[i]) - want_loss) < 1e-5 * max(1.0, want_loss):
            fails.append((tag, "loss %r vs %r" % (float(loss[i]), want_loss)))


def _conv2d_case(ops, case, kp, fails, worst):
    N, Cout, Cin, H, W, k, stride, pad, bias = case
    ref = tf.fwd_ref(case)
    form = tc.fwd_form(case, kp)
    tag = (case, "kpos" if kp else "std", "form %d" % form)
    w = ref["wk"] if kp else ref["w"]
    y0 = tf.Guarded(tuple(ref["out"].shape))
    ops.conv2d(ref["x"], w, ref["b"], stride, pad, kp, out=y0.t)
    split = _split_fwd(form)
    K = Cin * k * k
    ok, err = tf._elementwise(y0.t, ref["out"], (min(tf.gamma(K), tf.FWD_SPLIT_BOUND) if split else tf.gamma(K)) * ref["S"])
    ratio = float((err / ref["S"].clamp_min(1e-300)).max())
    worst[1 if split else 0] = max(worst[1 if split else 0], ratio)
    worst[2] += 1
    rel = tf._rel(y0.t, ref["out"])
    if not y0.intact():
        fails.append((tag, "conv2d: guard band written"))
    if not ok:
        fails.append((tag, "conv2d: element-wise bound missed: worst ratio %.3e" % ratio))
    if not rel <= max(2e-6, 3 * ref["vendor"]):
        fails.append((tag, "conv2d: %.3e from fp64 (vendor %.3e)" % (rel, ref["vendor"])))
    g = torch.Generator().manual_seed(ref["seed"] + 2)
    scale = (0.5 + torch.rand(Cout, generator=g)).cuda()
    shift = torch.randn(Cout, generator=g).cuda()
    res = torch.randn(tuple(ref["out"].shape), generator=g).cuda()
    for identity, relu in ((None, True), (res, True), (None, False), (res, False)):
        y, z = tf.Guarded(tuple(ref["out"].shape)), tf.Guarded(tuple(ref["out"].shape))
        tf._conv2d_bn(ref["x"], w, ref["b"], y.t, scale, shift, identity, z.t, relu, case, kp)
        if not (y.intact() and z.intact()):
            fails.append((tag, "conv2d_bn_act: guard band written"))
        if not torch.equal(y.t, y0.t):
            fails.append((tag, "conv2d_bn_act: y differs from the plain launch"))
        if not torch.equal(z.t, ops.bn_act(y0.t, scale, shift, identity, relu)):
            fails.append((tag, "conv2d_bn_act: z differs from bn_act(y)", identity is not None, relu))


def _wgrad_group(ops, runs, fails, worst, accumulate=(False, True)):
    batch = ops.WgradBatch(torch.device("cuda"))
    held = []
    for case, fl in runs:
        k = case[5]
        ref = tf.wgrad_ref(case)
        for acc in accumulate:
            want = tf._kmajor(ref["want"]) if fl else ref["want"]
            S = tf._kmajor(ref["S"]) if fl else ref["S"]
            grad = tf.Guarded(tuple(want.shape))
            base = None
            if acc:
                base = tf._kmajor(ref["base"]) if fl else ref["base"]
                grad.t.copy_(base)
            batch.add(ref["resid"], ref["ip"], grad.t, (k, k), case[6], case[7], flags=fl | (tc.WG_ACC if acc else 0))
            held.append((case, fl, acc, ref, want, S, base, grad))
    infos = tc.wgrad_infos([tc.wgrad_geo(c, fl | (tc.WG_ACC if acc else 0)) for c, fl, acc, *_ in held])
    batch.flush()
    torch.cuda.synchronize()
    for (case, fl, acc, ref, want, S, base, grad), info in zip(held, infos):
        tag = (case[:8], "kpos" if fl else "std", "acc" if acc else "ovw", "variant %d" % info["variant"], "S=%d" % info["S"])
        split = bool(info["variant"] & 64)
        bound = (min(tf.gamma(ref["K"]), tf.WGRAD_SPLIT_BOUND) if split else tf.gamma(ref["K"])) * S
        full = want
        if acc:
            full = base.double() + want
            bound = bound + 2 * U * (base.double().abs() + want.abs())
        ok, err = tf._elementwise(grad.t, full, bound)
        ratio = float((err / S.clamp_min(1e-300)).max())
        if not acc:
            worst[1 if split else 0] = max(worst[1 if split else 0], ratio)
        worst[2] += 1
        if not grad.intact():
            fails.append((tag, "guard band written"))
        if not ok:
            fails.append((tag, "element-wise bound missed: worst ratio %.3e" % ratio))
        if not tf._rel(grad.t, full) < 3e-6:
            fails.append((tag, "gradient %.3e from fp64" % tf._rel(grad.t, full)))


@pytest.fixture
def exact_split():
    with tc.arith(MODE):
        yield


def test_fwd_batch_every_form(ops, exact_split):
    fails, worst = [], [0.0, 0.0, 0]
    for runs in tf._grouped(tc.fwd_runs("fwd_batch")):
        _fwd_batch_group(ops, runs, fails, worst)
    print("fwd_batch, pleas_arith(2), %d layers: worst ratio |got - want| / (sum|xw| + |target|) exact %.3e, nine-product split %.3e"
          % (worst[2], worst[0], worst[1]))
    assert worst[1] > 0 and worst[0] > 0
    assert not fails, fails


def test_conv2d_and_bn_act_every_form(ops, exact_split):
    fails, worst = [], [0.0, 0.0, 0]
    for case, kp in tc.fwd_runs("conv2d"):
        _conv2d_case(ops, case, kp, fails, worst)
    torch.cuda.synchronize()
    print("conv2d, pleas_arith(2), %d layers: worst ratio |got - want| / sum|xw| exact %.3e, nine-product split %.3e" % (worst[2], worst[0], worst[1]))
    assert worst[1] > 0 and worst[0] > 0
    assert not fails, fails


def test_wgrad_batch_every_variant(ops, exact_split):
    fails, worst = [], [0.0, 0.0, 0]
    for runs in tf._grouped(tc.wgrad_runs(), 24):
        _wgrad_group(ops, runs, fails, worst)
    print("wgrad_batch, pleas_arith(2), %d layers: worst ratio |got - want| / sum|xy| exact %.3e, nine-product split %.3e" % (worst[2], worst[0], worst[1]))
    assert worst[1] > 0 and worst[0] > 0
    assert not fails, fails


def test_random_general_geometries_all_entry_points(ops, exact_split):
    draw = tc.random_cases()
    fails, worst = [], [0.0, 0.0, 0]
    _fwd_batch_group(ops, [(c, False) for c in draw], fails, worst)
    for c in draw:
        _conv2d_case(ops, c, False, fails, worst)
    print("random draw, forward, pleas_arith(2), %d layers: worst ratio exact %.3e, nine-product split %.3e" % (worst[2], worst[0], worst[1]))
    worst = [0.0, 0.0, 0]
    _wgrad_group(ops, [(c, 0) for c in draw], fails, worst, accumulate=(False,))
    print("random draw, weight gradient, pleas_arith(2), %d layers: worst ratio exact %.3e, nine-product split %.3e" % (worst[2], worst[0], worst[1]))
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ b. the matching contraction
GRAM_SHAPES = [((16, 256, 14, 14), 1), ((2, 64, 28, 28), 1), ((5, 132, 6, 6), 1), ((2, 64, 112, 112), 1)]      # test_gram_split_bf16_switch


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


@pytest.mark.parametrize("shape,axis", GRAM_SHAPES)
def test_gram_under_the_nine_product_mode(ops, shape, axis):
    g = torch.Generator().manual_seed(77)
    x = torch.randn(shape, generator=g)
    y = 0.7 * x + 0.5 * torch.randn(shape, generator=g)
    xd, yd = x.cuda(), y.cuda()
    want = orc.cross_features_inner_product(x.double(), y.double(), axis)
    exact = ops.cross_features_inner_product(xd, yd, axis).cpu()
    C = shape[axis]

    def grouped_launch():                             # the grouped launch has kernels of its own, and its own cut of the K axis
        out = torch.full((C, C), float("nan"), device="cuda")
        batch = ops.GramBatch([out], 0)
        batch.add(xd, yd, axis, 0)
        batch.flush(accumulate=False)
        torch.cuda.synchronize()
        return out.cpu()

    grouped_exact = grouped_launch()
    with tc.arith(MODE):
        nine = ops.cross_features_inner_product(xd, yd, axis).cpu()
        nine_d = ops.cross_features_cdist(xd, yd, axis).cpu()
        grouped = grouped_launch()
    with tc.arith(1):
        six = ops.cross_features_inner_product(xd, yd, axis).cpu()
    assert not torch.equal(nine, exact) and not torch.equal(nine, six)      # a third arithmetic did run
    gate = max(2 * _rel(exact, want), 5e-7)
    print("gram %r: exact %.2e, six products %.2e, nine products %.2e; grouped launch: exact %.2e, nine products %.2e from fp64"
          % (shape, _rel(exact, want), _rel(six, want), _rel(nine, want), _rel(grouped_exact, want), _rel(grouped, want)))
    assert _rel(nine, want) < gate, (_rel(nine, want), _rel(exact, want))
    assert not torch.equal(grouped, grouped_exact)
    assert _rel(grouped, want) < max(2 * _rel(grouped_exact, want), 5e-7), (_rel(grouped, want), _rel(grouped_exact, want))
    assert _rel(nine_d, orc.cross_features_cdist_f64(x, y, axis)) < 2e-6
    assert torch.equal(ops.cross_features_inner_product(xd, yd, axis).cpu(), exact)


# ------------------------------------------------------------------------------------------------ c. a third arithmetic
def _three_arithmetics(run):
    exact = run()
    with tc.arith(1):
        six = run()
    with tc.arith(MODE):
        nine = run()
        assert torch.equal(run(), nine)                  # deterministic
    assert not torch.equal(nine, exact)
    assert not torch.equal(nine, six)
    assert torch.equal(run(), exact)                     # and it goes away again
    print("elements in which the nine-product result differs from the six-product one: %.1f %%, from the exact one: %.1f %%"
          % (100 * float((nine != six).double().mean()), 100 * float((nine != exact).double().mean())))
    return exact, six, nine


def test_a_third_arithmetic_in_the_weight_gradient(ops):
    g = torch.Generator().manual_seed(5)
    N, Cout, Cin, H = 8, 256, 128, 28
    ip, resid = torch.randn(N, Cin, H, H, generator=g).cuda(), torch.randn(N, Cout, H, H, generator=g).cuda()
    want = torch.ops.aten.convolution_backward(resid.double(), ip.double(), torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, device="cuda"),
                                               None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [False, True, False])[1]

    def run():
        grad = torch.full((Cout, Cin, 3, 3), float("nan"), device="cuda")
        b = ops.WgradBatch(torch.device("cuda"))
        b.add(resid, ip, grad, (3, 3), 1, 1)
        b.flush()
        return grad

    exact, six, nine = _three_arithmetics(run)
    e = [tf._rel(t, want) for t in (exact, six, nine)]
    print("3x3 weight gradient, K = %d pixels: exact %.2e, six products %.2e, nine products %.2e from fp64" % (N * H * H, *e))
    assert e[2] < max(2 * e[0], 5e-7), e


def test_a_third_arithmetic_in_the_plain_convolution(ops):
    g = torch.Generator().manual_seed(6)
    N, Cin, Cout, H = 4, 256, 128, 14
    x, w = torch.randn(N, Cin, H, H, generator=g).cuda(), (torch.randn(Cout, Cin, 1, 1, generator=g) / 16).cuda()
    want = torch.nn.functional.conv2d(x.double(), w.double())
    exact, six, nine = _three_arithmetics(lambda: ops.conv2d(x, w, None, 1, 0))
    e = [tf._rel(t, want) for t in (exact, six, nine)]
    print("1x1 convolution, K = %d channels: exact %.2e, six products %.2e, nine products %.2e from fp64" % (Cin, *e))
    assert e[2] < max(2 * e[0], 5e-7), e


# ------------------------------------------------------------------------------------------------ d. the products are all there
def _run_crafted(ops, c):
    x, w = c["x"].cuda(), c["w"].cuda()
    if c["kind"] == "conv2d":
        N, Cin, H, W, Cout, k = c["geo"]
        kp = k > 1                                       # the flat k x k forms take kernel-position-major weights
        case = (N, Cout, Cin, H, W, k, 1, k // 2, False)
        assert tc.fwd_form(case, kp) in tf.SPLIT_FWD_FORMS
        out = tf.Guarded((N, Cout, H, W))
        ops.conv2d(x, w.permute(0, 2, 3, 1).contiguous() if kp else w, None, 1, k // 2, kp, out=out.t)
    elif c["kind"] == "wgrad":
        N, Cout, Cin, H, W = c["geo"]
        split = bool(tc.wgrad_infos([(N, Cout, Cin, H, W, 1, 1, 1, 0, 0)])[0]["variant"] & 64)
        assert split == (_lib_mode() != 0)
        out = tf.Guarded((Cout, Cin, 1, 1))
        b = ops.WgradBatch(torch.device("cuda"))
        b.add(x, w, out.t, (1, 1), 1, 0)
        b.flush()
    else:
        N, C, H, W = c["geo"]
        out = tf.Guarded((C, C))
        ops.gram_accum(x, w, 1, out.t, 0, accumulate=False)
    torch.cuda.synchronize()
    assert out.intact()
    return out.t.clone()


def _lib_mode():
    from pleas_merging_amd import _lib

    return _lib.lib().pleas_arith_get()


@pytest.mark.parametrize("c", sx.cases(), ids=[c["name"] for c in sx.cases()])
def test_three_arithmetics_on_operands_with_an_exactly_representable_result(ops, c):
    """The operands of tests/split_exact_cases.py: the true result is a small integer, sum x3 * w, that an arithmetic with exact
    products AND an exact sum inside every MFMA would reproduce bit for bit (tests/test_arith_exact_host.py holds that on the
    CPU).  The MI355X does not: an MFMA whose products (up to 2^27 here) cancel pairwise loses the low bits of its accumulator
    input -- under the nine-product mode 70 % (1 x 1, Cin 32) to 100 % (3 x 3) of the outputs differ from the integer, by up to
    6 .. 20, the results come out as multiples of 2.  That is a property of the matrix unit's adder, not of the
    kernels, so what is asserted here on these operands is what holds for any: three arithmetics, three results, each
    repeatable, and the exact one back afterwards.  The distances from the true integer are printed."""
    want = c["want"].float().cuda().reshape(-1)
    got = {}
    for mode in (0, 1, 2):
        with tc.arith(mode):
            got[mode] = _run_crafted(ops, c).reshape(-1)
            assert torch.equal(_run_crafted(ops, c).reshape(-1), got[mode])      # deterministic
    wrong = {m: 100 * float((got[m] != want).double().mean()) for m in got}
    dev = {m: float((got[m] - want).abs().max()) for m in got}
    print("%s: outputs that differ from the true integer (worst deviation): fp32 %.0f %% (%.0f), six products %.0f %% (%.0f), "
          "nine products %.0f %% (%.0f)" % (c["name"], wrong[0], dev[0], wrong[1], dev[1], wrong[2], dev[2]))
    assert not torch.equal(got[2], got[0])
    assert not torch.equal(got[2], got[1])
    assert not torch.equal(got[1], got[0])
    assert torch.equal(_run_crafted(ops, c).reshape(-1), got[0])                 # and the exact arithmetic is back
