"""Every tile form of the convolution forward (csrc/conv_fwd.hip) and of the weight gradient (csrc/conv.hip) against fp64, over
the case table of tests/tile_cases.py (tests/test_tile_coverage.py holds, without a GPU, that the table reaches every form a
geometry can reach), under both arithmetics (``pleas_arith``), through all four entry points:

* ``pleas_fwd_batch``: fp64 convolution + block-merged target, residual and loss (pleas/methods/pleas_merging.py:116-147, :282);
* ``pleas_conv2d_fwd`` against ``F.conv2d`` in fp64, ``pleas_conv2d_bn_act_fwd`` bit-equal to the launches it replaces;
* ``pleas_wgrad_batch`` against ``aten.convolution_backward`` in fp64 (pleas_merging.py:287), standard and
  kernel-position-major destination, overwrite and ACCUMULATE.

Outputs are pre-filled with NaN and followed by a guard band that must stay untouched.  Beside the project's norm-wise gates
(residual 5e-6, weight gradient 3e-6, plain convolution max(2e-6, 3 x the vendor's distance from fp64)) every element is held
to a bound that a norm over a million elements would absorb (a wrong border column of one form):

* exact arithmetic: any fp32 summation order of a length-K dot product satisfies |got - want| <= gamma_K * sum |x_i w_i| with
  gamma_K = (K + 2) u / (1 - (K + 2) u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1; K + 2
  takes the bias / the accumulate add).  sum |x_i w_i| is the fp64 convolution (gradient) of the absolute values.  The fused
  forward's epilogue adds four roundings (the target's sum, the subtraction, the scale, dscale's own conversion to fp32), each
  below u (|out| + |target|), |out| <= sum |x_i w_i|; a fifth u stands for their products.
* split bf16: the constant is not derivable (six of nine partial products kept, accumulation order inside the MFMA
  unspecified): the exact kernel's worst ratio |got - want| / (sum |x_i w_i| + |target|) over the table was measured on the
  MI355X and the split kernels are allowed 4 x that (two dropped-term classes below 2^-26 |xy| each and another accumulation
  order) -- FWD_EXACT_RATIO / WGRAD_EXACT_RATIO below.
"""
import pytest
import torch
import torch.nn.functional as F

import tile_cases as tc

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GUARD, SENTINEL = 256, -7.25
GROUP = 12                       # (case, layout) runs per grouped launch: forms mixed as in a real update

# Measured on an MI355X over the whole table + the random draw with the exact arithmetic (the tests print them again on every
# run, "worst ratio ... exact"): forward 3.656e-07 (fwd_batch) / 4.031e-07 (conv2d) / 2.285e-07 (random draw), weight gradient
# 3.396e-07 (table) / 2.991e-07 (random draw).  The split kernels get 4 x the larger: 1.612e-06 and 1.358e-06.
FWD_EXACT_RATIO = 4.031e-07
WGRAD_EXACT_RATIO = 3.396e-07
FWD_SPLIT_BOUND = 4 * FWD_EXACT_RATIO
WGRAD_SPLIT_BOUND = 4 * WGRAD_EXACT_RATIO

# Forms with a split-bf16 twin -- kFwdForms[].split in csrc/conv_fwd.hip, which has no query: keep the two in step.  Every other
# form runs the exact kernel inside the same launch and is held to the exact bound under either arithmetic.
SPLIT_FWD_FORMS = (4, 6, 7, 9)


def gamma(K):
    return (K + 2) * U / (1 - (K + 2) * U)


@pytest.fixture(scope="module")
def ops():
    from pleas_merging_amd import hip_ops

    return hip_ops


@pytest.fixture(params=[0, 1], ids=["fp32", "split_bf16"])
def mode(request):
    with tc.arith(request.param):
        yield request.param


@pytest.fixture(scope="module", autouse=True)
def _references_released():
    """The cached operands and fp64 references live on the GPU for this module only."""
    yield
    _FWD_REF.clear()
    _WG_REF.clear()
    torch.cuda.empty_cache()


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


class Guarded:
    """A NaN-filled output with a guard band behind it (one allocation: a tile that writes past its ragged edge lands in it)."""

    def __init__(self, shape, fill=float("nan")):
        n = 1
        for s in shape:
            n *= s
        self.n = n
        self.whole = torch.full((n + GUARD,), SENTINEL, device="cuda")
        self.t = self.whole[:n].view(shape)
        self.t.fill_(fill)

    def poison(self):
        self.t.fill_(float("nan"))

    def intact(self):
        return bool((self.whole[self.n:] == SENTINEL).all())


def _elementwise(got, want, bound):
    """(every element within its bound -- a NaN is not --, |got - want|)."""
    err = (got.double() - want).abs()
    return bool((err <= bound).all()), err


# ------------------------------------------------------------------------------------------------ references (cached per case)
_FWD_REF, _WG_REF = {}, {}


def fwd_ref(case):
    """Operands and fp64 references of a forward case: out = conv in fp64, S = conv of the absolute values + |bias|, the vendor's
    fp32 kernel's distance from fp64."""
    if case not in _FWD_REF:
        N, Cout, Cin, H, W, k, stride, pad, bias = case
        g = torch.Generator().manual_seed(hash(case) % (1 << 31))
        x = torch.randn(N, Cin, H, W, generator=g).cuda()
        w = (torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5).cuda()
        b = torch.randn(Cout, generator=g).cuda() if bias else None
        out = F.conv2d(x.double(), w.double(), b.double() if bias else None, stride, pad)
        S = F.conv2d(x.double().abs(), w.double().abs(), b.double().abs() if bias else None, stride, pad)
        vendor = _rel(F.conv2d(x, w, b, stride, pad), out)
        _FWD_REF[case] = dict(x=x, w=w, wk=w.permute(0, 2, 3, 1).contiguous() if tc.kpos_legal(case) else None, b=b, out=out, S=S,
                              vendor=vendor, seed=hash(case) % (1 << 31))
    return _FWD_REF[case]


def wgrad_ref(case):
    if case not in _WG_REF:
        N, Cout, Cin, H, W, k, stride, pad = case[:8]
        g = torch.Generator().manual_seed(hash(case[:8]) % (1 << 31))
        Ho, Wo = tc.out_hw(H, W, k, stride, pad)
        ip = torch.randn(N, Cin, H, W, generator=g).cuda()
        resid = torch.randn(N, Cout, Ho, Wo, generator=g).cuda()
        base = torch.randn(Cout, Cin, k, k, generator=g).cuda()
        zero = torch.zeros(Cout, Cin, k, k, dtype=torch.float64, device="cuda")
        bw = lambda r, i: torch.ops.aten.convolution_backward(r, i, zero, None, [stride, stride], [pad, pad], [1, 1], False, [0, 0], 1,
                                                              [False, True, False])[1]
        _WG_REF[case] = dict(ip=ip, resid=resid, base=base, want=bw(resid.double(), ip.double()),
                             S=bw(resid.double().abs(), ip.double().abs()), K=N * Ho * Wo)
    return _WG_REF[case]


def _kmajor(t):
    """[Cout][Cin][KH][KW] -> the kernel-position-major gradient layout [Cout][KH * KW][Cin]."""
    Cout, Cin = t.shape[:2]
    return t.reshape(Cout, Cin, -1).permute(0, 2, 1).contiguous()


# ------------------------------------------------------------------------------------------------ pleas_fwd_batch
def _fwd_batch_group(ops, runs, mode, fails, worst):
    """One grouped launch over (case, kpos) runs; appends what misses a gate to `fails`, returns the worst exact ratio."""
    from pleas_merging_amd.methods.partial_matching import block_maps

    batch = ops.FwdBatch(torch.device("cuda"))
    held = []
    for case, kp in runs:
        N, Cout, Cin, H, W, k, stride, pad, bias = case
        ref = fwd_ref(case)
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
        resid = Guarded((N, Cout, Ho, Wo))
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
        denom = ref["S"] + target.abs()
        split = mode == 1 and form in SPLIT_FWD_FORMS
        bound = dscale * (FWD_SPLIT_BOUND * denom if split else (gamma(K) + 5 * U) * ref["S"] + 5 * U * target.abs())
        ok, err = _elementwise(resid.t, want, bound)
        ratio = float((err / (dscale * denom).clamp_min(1e-300)).max())
        worst[1 if split else 0] = max(worst[1 if split else 0], ratio)
        worst[2] += 1
        rel = _rel(resid.t, want)
        if not resid.intact():
            fails.append((tag, "guard band written"))
        if not ok:
            fails.append((tag, "element-wise bound missed: worst ratio %.3e" % ratio))
        if not rel < 5e-6:
            fails.append((tag, "residual %.3e from fp64" % rel))
        if not abs(float(loss[i]) - want_loss) < 1e-5 * max(1.0, want_loss):
            fails.append((tag, "loss %r vs %r" % (float(loss[i]), want_loss)))


def _grouped(runs, size=GROUP):
    # a stride through the list instead of consecutive slices: neighbours in the table share a form, a launch should mix them
    n = -(-len(runs) // size)
    return [runs[i::n] for i in range(n)]


def test_fwd_batch_every_form(ops, mode):
    fails, worst = [], [0.0, 0.0, 0]
    for runs in _grouped(tc.fwd_runs("fwd_batch")):
        _fwd_batch_group(ops, runs, mode, fails, worst)
    print("fwd_batch, pleas_arith(%d), %d layers: worst ratio |got - want| / (sum|xw| + |target|) exact %.3e, split %.3e" % (mode, worst[2], worst[0], worst[1]))
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ plain convolution (+ BatchNorm)
def _conv2d_bn(x, w, b, y, scale, shift, res, z, relu, case, kp):
    from pleas_merging_amd import _lib, hip_ops

    N, Cout, Cin, H, W, k, stride, pad = case[:8]
    _lib.check(_lib.lib().pleas_conv2d_bn_act_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr() if b is not None else None, y.data_ptr(),
                                                  scale.data_ptr(), shift.data_ptr(), res.data_ptr() if res is not None else None,
                                                  z.data_ptr(), 1 if relu else 0, N, Cin, H, W, Cout, k, k, stride, pad,
                                                  1 if kp else 0, hip_ops._stream()), "pleas_conv2d_bn_act_fwd")


def _conv2d_case(ops, case, kp, mode, fails, worst):
    N, Cout, Cin, H, W, k, stride, pad, bias = case
    ref = fwd_ref(case)
    form = tc.fwd_form(case, kp)
    tag = (case, "kpos" if kp else "std", "form %d" % form)
    w = ref["wk"] if kp else ref["w"]
    y0 = Guarded(tuple(ref["out"].shape))
    ops.conv2d(ref["x"], w, ref["b"], stride, pad, kp, out=y0.t)
    split = mode == 1 and form in SPLIT_FWD_FORMS
    K = Cin * k * k
    ok, err = _elementwise(y0.t, ref["out"], (FWD_SPLIT_BOUND if split else gamma(K)) * ref["S"])
    ratio = float((err / ref["S"].clamp_min(1e-300)).max())
    worst[1 if split else 0] = max(worst[1 if split else 0], ratio)
    worst[2] += 1
    rel = _rel(y0.t, ref["out"])
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
        y, z = Guarded(tuple(ref["out"].shape)), Guarded(tuple(ref["out"].shape))
        _conv2d_bn(ref["x"], w, ref["b"], y.t, scale, shift, identity, z.t, relu, case, kp)
        if not (y.intact() and z.intact()):
            fails.append((tag, "conv2d_bn_act: guard band written"))
        if not torch.equal(y.t, y0.t):
            fails.append((tag, "conv2d_bn_act: y differs from the plain launch"))
        if not torch.equal(z.t, ops.bn_act(y0.t, scale, shift, identity, relu)):
            fails.append((tag, "conv2d_bn_act: z differs from bn_act(y)", identity is not None, relu))


def test_conv2d_and_bn_act_every_form(ops, mode):
    fails, worst = [], [0.0, 0.0, 0]
    assert tc.fwd_runs("conv2d") == tc.fwd_runs("conv2d_bn_act")      # one pass serves both entry points
    for case, kp in tc.fwd_runs("conv2d"):
        _conv2d_case(ops, case, kp, mode, fails, worst)
    torch.cuda.synchronize()
    print("conv2d, pleas_arith(%d), %d layers: worst ratio |got - want| / sum|xw| exact %.3e, split %.3e" % (mode, worst[2], worst[0], worst[1]))
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ pleas_wgrad_batch
def _wgrad_group(ops, runs, mode, fails, worst, accumulate=(False, True)):
    """One grouped launch over (case, destination layout) runs, each overwriting and accumulating."""
    batch = ops.WgradBatch(torch.device("cuda"))
    held = []
    for case, fl in runs:
        k = case[5]
        ref = wgrad_ref(case)
        for acc in accumulate:
            want = _kmajor(ref["want"]) if fl else ref["want"]
            S = _kmajor(ref["S"]) if fl else ref["S"]
            grad = Guarded(tuple(want.shape))
            base = None
            if acc:
                base = _kmajor(ref["base"]) if fl else ref["base"]
                grad.t.copy_(base)
            batch.add(ref["resid"], ref["ip"], grad.t, (k, k), case[6], case[7], flags=fl | (tc.WG_ACC if acc else 0))
            held.append((case, fl, acc, ref, want, S, base, grad))
    infos = tc.wgrad_infos([tc.wgrad_geo(c, fl | (tc.WG_ACC if acc else 0)) for c, fl, acc, *_ in held])
    batch.flush()
    torch.cuda.synchronize()
    for (case, fl, acc, ref, want, S, base, grad), info in zip(held, infos):
        tag = (case[:8], "kpos" if fl else "std", "acc" if acc else "ovw", "variant %d" % info["variant"], "S=%d" % info["S"])
        split = bool(info["variant"] & 64)
        bound = (WGRAD_SPLIT_BOUND if split else gamma(ref["K"])) * S
        full = want
        if acc:
            full = base.double() + want
            bound = bound + 2 * U * (base.double().abs() + want.abs())
        ok, err = _elementwise(grad.t, full, bound)
        ratio = float((err / S.clamp_min(1e-300)).max())
        if not acc:
            worst[1 if split else 0] = max(worst[1 if split else 0], ratio)
        worst[2] += 1
        if not grad.intact():
            fails.append((tag, "guard band written"))
        if not ok:
            fails.append((tag, "element-wise bound missed: worst ratio %.3e" % ratio))
        if not _rel(grad.t, full) < 3e-6:
            fails.append((tag, "gradient %.3e from fp64" % _rel(grad.t, full)))


def test_wgrad_batch_every_variant(ops, mode):
    fails, worst = [], [0.0, 0.0, 0]
    for runs in _grouped(tc.wgrad_runs(), 24):
        _wgrad_group(ops, runs, mode, fails, worst)
    print("wgrad_batch, pleas_arith(%d), %d layers: worst ratio |got - want| / sum|xy| exact %.3e, split %.3e" % (mode, worst[2], worst[0], worst[1]))
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ random general geometries
def test_random_general_geometries_all_entry_points(ops, mode):
    """Property test of what had none: the general tile (stride 1-3, pad 0..k, images down to smaller than the kernel, channel
    counts of every residue) through the grouped forward, the plain / BatchNorm convolution and the weight gradient, one seeded
    draw (tests/test_tile_coverage.py holds what the draw must reach), the gates of the table."""
    draw = tc.random_cases()
    fails, worst = [], [0.0, 0.0, 0]
    _fwd_batch_group(ops, [(c, False) for c in draw], mode, fails, worst)
    for c in draw:
        _conv2d_case(ops, c, False, mode, fails, worst)
    print("random draw, forward, pleas_arith(%d), %d layers: worst ratio exact %.3e, split %.3e" % (mode, worst[2], worst[0], worst[1]))
    worst = [0.0, 0.0, 0]
    _wgrad_group(ops, [(c, 0) for c in draw], mode, fails, worst, accumulate=(False,))
    print("random draw, weight gradient, pleas_arith(%d), %d layers: worst ratio exact %.3e, split %.3e" % (mode, worst[2], worst[0], worst[1]))
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ the launches a plan goes through
def test_eight_launches_of_one_forward_plan_and_a_relaunch_on_moved_operands(ops, mode):
    """A grouped forward changes its own schedule: launches 1-2 run on static lanes, launch 3 is timed, later launches are
    re-dealt from the measured durations with long forms cut into slices (launches that start inside a form's item list), and a
    fitter re-uses the plan through ``relaunch`` with rewritten pointers.  Eight launches of one mixed-form plan whose two large
    forms do get cut (tests/tile_cases.py, SCHEDULE_CASES), outputs re-poisoned each time: every one ``torch.equal`` to the
    first and within the fp64 gates; then a relaunch on fresh copies of every operand."""
    from pleas_merging_amd.methods.partial_matching import block_maps

    runs = tc.schedule_list()
    assert len({u[0] for u in tc.fwd_units(runs)}) >= 4
    batch = ops.FwdBatch(torch.device("cuda"))
    held = []
    for case, kp in runs:
        N, Cout, Cin, H, W, k, stride, pad, bias = case
        ref = fwd_ref(case)
        Ho, Wo = tc.out_hw(H, W, k, stride, pad)
        g = torch.Generator().manual_seed(ref["seed"] + 3)
        ns = Cout // 5
        nm = Cout - 2 * ns
        pm = torch.randperm(nm + ns, generator=g)
        blk = (torch.arange(nm), pm[:nm], torch.arange(nm, nm + ns), pm[nm:])
        o1, o2 = torch.randn(N, nm + ns, Ho, Wo, generator=g).cuda(), torch.randn(N, nm + ns, Ho, Wo, generator=g).cuda()
        bc = [t.cuda() for t in blk]
        target = torch.cat([(o1.double()[:, bc[0]] + o2.double()[:, bc[1]]) / 2, o1.double()[:, bc[2]], o2.double()[:, bc[3]]], 1)
        r1, r2, nmerged = block_maps(blk, "cuda")
        numel = ref["out"].numel()
        resid = Guarded((N, Cout, Ho, Wo))
        ten = dict(ip=ref["x"], w=ref["wk"] if kp else ref["w"], bias=ref["b"], o1=o1, o2=o2, row1=r1, row2=r2, resid=resid.t)
        batch.add(ten["ip"], ten["w"], ten["bias"], o1, o2, r1, r2, nmerged, resid.t, 2.0 / numel, 1.0 / numel, (k, k), stride, pad,
                  flags=ops.FwdBatch.KPOS_MAJOR if kp else 0)
        held.append((case, ten, resid, 2.0 / numel * (ref["out"] - target), float(((ref["out"] - target) ** 2).mean())))
    loss = torch.full((len(held),), float("nan"), device="cuda")
    first = None
    for launch in range(8):
        for _, _, resid, _, _ in held:
            resid.poison()
        loss.fill_(float("nan"))
        if launch == 0:
            batch.flush(loss)
        else:
            batch.relaunch(loss)
        torch.cuda.synchronize()
        got = [resid.t.clone() for _, _, resid, _, _ in held] + [loss.clone()]
        if first is None:
            first = got
            for (case, _, resid, want, want_loss), l in zip(held, loss.tolist()):
                assert _rel(resid.t, want) < 5e-6, case
                assert abs(l - want_loss) < 1e-5 * max(1.0, want_loss), case
        for a, b, h in zip(got, first, held + [None]):
            assert torch.equal(a, b), ("launch %d differs from the first" % (launch + 1), h and h[0])
        assert all(resid.intact() for _, _, resid, _, _ in held)
    lanes = ops.fwd_plan_lanes()
    units = sum(len(str(f["lane"])) for f in lanes["forms"].values())
    print("eight launches, pleas_arith(%d): state %d, %d forms in %d launch units: %r" % (mode, lanes["state"], len(lanes["forms"]), units,
                                                                                         lanes["forms"]))
    if lanes["state"] == 0 and all(f["lane"] == 1 for f in lanes["forms"].values()):
        print("the library's side streams could not be created: no calibration launch, equality only")
    else:
        assert lanes["state"] == 2, lanes
        assert units > len(lanes["forms"]), "no form was cut into slices: the sliced launches stayed unexecuted (%r)" % (lanes,)
    # the fitter's fast path: the same table with every pointer moved to a fresh copy of its operand
    table = batch.table()
    moved = []
    for i, (_, ten, _, _, _) in enumerate(held):
        fresh = {name: (None if t is None else t.clone()) for name, t in ten.items()}
        fresh["resid"].fill_(float("nan"))
        for name, t in fresh.items():
            table[name][i] = 0 if t is None else t.data_ptr()
        moved.append(fresh)
    loss2 = torch.full_like(loss, float("nan"))
    batch.relaunch(loss2)
    torch.cuda.synchronize()
    for fresh, want in zip(moved, first):
        assert torch.equal(fresh["resid"], want)
    assert torch.equal(loss2, first[-1])


def test_eight_launches_of_a_weight_gradient_that_forks_onto_its_side_stream(ops):
    """Under the split arithmetic a list that mixes split-capable and exact-only layers runs as two grids, the exact one on a
    side stream of the library: eight launches of one plan, every one ``torch.equal`` to the first and within the fp64 gate."""
    cases = [(4, 128, 128, 14, 14, 3, 1, 1), (4, 96, 64, 7, 7, 3, 1, 1), (4, 256, 64, 14, 14, 1, 1, 0), (4, 128, 64, 28, 28, 3, 2, 1),
             (2, 64, 64, 56, 56, 3, 1, 1), (3, 70, 15, 7, 7, 3, 1, 1), (3, 96, 80, 7, 7, 1, 1, 0)]
    with tc.arith(1):
        kinds = {bool(i["variant"] & 64) for i in tc.wgrad_infos([tc.wgrad_geo(c) for c in cases])}
        assert kinds == {True, False}
        batch = ops.WgradBatch(torch.device("cuda"))
        held = []
        for case in cases:
            ref = wgrad_ref(case)
            grad = Guarded(tuple(ref["want"].shape))
            batch.add(ref["resid"], ref["ip"], grad.t, (case[5], case[5]), case[6], case[7])
            held.append((case, ref, grad))
        first = None
        for launch in range(8):
            for _, _, grad in held:
                grad.poison()
            if launch == 0:
                batch.flush()
            else:
                batch.relaunch()
            torch.cuda.synchronize()
            got = [grad.t.clone() for _, _, grad in held]
            if first is None:
                first = got
                for case, ref, grad in held:
                    assert _rel(grad.t, ref["want"]) < 3e-6, case
            for a, b, h in zip(got, first, held):
                assert torch.equal(a, b), ("launch %d differs from the first" % (launch + 1), h[0])
            assert all(grad.intact() for _, _, grad in held)
