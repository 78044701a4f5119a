"""Every path of the streaming kernels on the GPU (csrc/elementwise.hip, csrc/bn_train.hip, target_residual / loss_final in
csrc/conv.hip): one parametrised test per kernel over its table in tests/stream_cases.py, against the references and bounds of
tests/stream_ref.py.  tests/test_stream_coverage.py (no GPU) holds the tables to the paths the library reports.

Every output is a NaN-filled view with a sentinel band on both sides (``Guarded``); every input is a view inside a NaN-filled
buffer (``placed``), one float past the aligned start where the case says so: a read or a write outside an operand shows up as
a NaN in the result or a broken band, a skipped element as a NaN left behind.  The entry points are called through ``_lib``
where the ``hip_ops`` wrapper would allocate the output itself.  The wrapped cases run once each; nothing is looped."""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

import stream_cases as sc
import stream_ref as sr

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 256, -7.25
U, TINY = sr.U, sr.TINY


@pytest.fixture(scope="module")
def ops():
    from pleas_merging_amd import hip_ops

    return hip_ops


@pytest.fixture(scope="module")
def lib():
    from pleas_merging_amd import _lib

    return _lib.lib()


@pytest.fixture(autouse=True)
def _released():
    yield
    torch.cuda.empty_cache()


class Guarded:
    """An output: ``shape`` floats (or int64) filled with NaN (-1) inside one allocation, a sentinel band before and behind it;
    ``off``: the view starts one element past the aligned start (an odd offset into the buffer)."""

    def __init__(self, shape, off=False, dtype=torch.float32, fill=None):
        self.n = math.prod(shape)
        self.start = GUARD + (1 if off else 0)
        self.whole = torch.full((self.start + self.n + GUARD,), SENTINEL if dtype.is_floating_point else -7, dtype=dtype, device="cuda")
        self.t = self.whole[self.start:self.start + self.n].view(shape)
        self.t.fill_(fill if fill is not None else (float("nan") if dtype.is_floating_point else -1))
        assert self.whole.data_ptr() % 16 == 0 and (self.t.data_ptr() % 16 != 0) == bool(off and dtype == torch.float32)

    def intact(self):
        band = self.whole[0]
        return bool((self.whole[:self.start] == band).all()) and bool((self.whole[self.start + self.n:] == band).all())


def placed(t, off=False):
    """An input: ``t`` copied into the middle of a NaN-filled device buffer, one float off the aligned start if asked."""
    start = GUARD + (1 if off else 0)
    whole = torch.full((start + t.numel() + GUARD,), float("nan"), device="cuda")
    view = whole[start:start + t.numel()].view(t.shape)
    view.copy_(t)
    assert whole.data_ptr() % 16 == 0 and (view.data_ptr() % 16 != 0) == bool(off)
    return view


def ptr(t):
    return t.data_ptr() if t is not None else None


def ok(rc, lib):
    assert rc == 0, lib.pleas_last_error().decode()


def same(a, b):
    """Bit-equal as values, a NaN equal to a NaN (torch.equal says no to that)."""
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def table(kernel):
    rows = sc.KERNELS[kernel][0]
    return pytest.mark.parametrize("i", range(len(rows)), ids=["%d" % i for i in range(len(rows))])


# ------------------------------------------------------------------------------------------------ merge_blocks
@table("merge_blocks")
def test_merge_blocks(ops, lib, i):
    """Bit-equal to ``(a + b) * coef`` from index_select in fp32; a row or column an absent entry must not read holds NaN."""
    c = sc.MERGE_BLOCKS[i]
    w1, w2, r1, r2, c1, c2 = sr.merge_inputs(c, sc.seed("merge_blocks", i))
    d1, d2 = placed(w1, "w1" in c["off"]), placed(w2, "w2" in c["off"])
    maps = [m.cuda() if m is not None else None for m in (r1, r2, c1, c2)]
    want = sr.merge_ref(d1, d2, *maps, c["merged"], c["axis"])
    out = Guarded(tuple(want.shape), "out" in c["off"])
    geo = sc.merge_geo(c)
    ok(lib.pleas_merge_blocks(ptr(d1), ptr(d2), ptr(out.t), *geo[:6], *(ptr(m) for m in maps), c["merged"], ops._stream()), lib)
    assert out.intact() and not torch.isnan(out.t).any() and not torch.isnan(want).any()
    assert torch.equal(out.t, want), c
    if not c["off"]:      # the wrapper: the same launch into its own allocation
        assert torch.equal(ops.merge_blocks(d1, d2, c["axis"], maps[0], maps[1], c["merged"], maps[2], maps[3]), want)


# ------------------------------------------------------------------------------------------------ bn_act, three entry points
def _bn_act_launch(ops, lib, c, x, scale, shift, res, combo):
    with_res, relu, with_bn, with_sum = combo
    y = Guarded(x.shape, "y" in c["off"])
    y_bn = Guarded(x.shape, "y_bn" in c["off"]) if with_bn else None
    y_sum = Guarded(x.shape, "y_sum" in c["off"]) if with_sum else None
    r = res if with_res else None
    n, C, inner, _ = sc.bn_act_geo(c)
    opt = (ptr(y_bn.t) if y_bn else None, ptr(y_sum.t) if y_sum else None)
    if c["entry"] == "bn_act":
        assert opt == (None, None) and c["batches"] == 1
        ok(lib.pleas_bn_act(ptr(x), ptr(scale), ptr(shift), ptr(r), ptr(y.t), n, C, inner, relu, ops._stream()), lib)
    elif c["entry"] == "tracked":
        assert c["batches"] == 1
        ok(lib.pleas_bn_act_tracked(ptr(x), ptr(scale), ptr(shift), ptr(r), *opt, ptr(y.t), n, C, inner, relu, ops._stream()), lib)
    else:
        ok(lib.pleas_bn_act_tracked_batches(ptr(x), ptr(scale), ptr(shift), ptr(r), *opt, ptr(y.t), n // c["batches"], c["batches"],
                                            C, inner, relu, ops._stream()), lib)
    return y, y_bn, y_sum


@table("bn_act")
def test_bn_act(ops, lib, i):
    """Each written node of the chain against the fp64 module chain inside u (|x a| + |b| + |bn|) (+ u |sum|); between the
    outputs of one launch bit for bit: y_sum == y_bn + res, y == relu(last) by torch.relu's rule -- a NaN stays a NaN."""
    c = sc.BN_ACT[i]
    x, res, scale, shift = sr.bn_act_inputs(c, sc.seed("bn_act", i))
    x, res = placed(x, "x" in c["off"]), placed(res, "res" in c["off"])
    scale, shift = scale.cuda(), shift.cuda()
    refs = {}
    for combo in c["combos"]:
        with_res, relu, with_bn, with_sum = combo
        if (with_res, relu) not in refs:
            refs[(with_res, relu)] = sr.bn_chain_ref(x, scale, shift, res if with_res else None, relu)
        bn, sm, act, bound_bn, bound_sum = refs[(with_res, relu)]
        y, y_bn, y_sum = _bn_act_launch(ops, lib, c, x, scale, shift, res, combo)
        for out in (y, y_bn, y_sum):
            assert out is None or out.intact(), (c, combo)
        assert not sr.finite_close(y.t, act, bound_sum).any(), (c, combo)
        assert torch.equal(torch.isnan(y.t), torch.isnan(act)), (c, combo, "where the module chain has a NaN, and only there")
        if y_bn:
            assert not sr.finite_close(y_bn.t, bn, bound_bn).any(), (c, combo)
        if y_sum:
            assert not sr.finite_close(y_sum.t, sm, bound_sum).any(), (c, combo)
        # between the outputs of this launch, bit for bit: the sum is y_bn + res, y is relu of the value before it
        summed = (y_sum.t if y_sum else (None if relu else y.t)) if with_res else None
        if summed is not None and y_bn:
            assert same(summed, y_bn.t + res), (c, combo)
        pre = summed if with_res else (y_bn.t if y_bn else None)
        if relu and pre is not None:
            assert same(y.t, torch.relu(pre)), (c, combo)
        if not relu and not with_res and y_bn:
            assert same(y.t, y_bn.t), (c, combo)
        if not c.get("plant"):
            assert not torch.isnan(y.t).any()


def test_bn_act_wrappers_return_the_nodes_of_the_direct_launch(ops, lib):
    """``hip_ops.bn_act`` / ``bn_act_tracked`` (``keep_bn`` both ways) choose which nodes are written; their values are the direct
    launches', bit for bit, one batch and three."""
    for i, c in ((2, sc.BN_ACT[2]), (5, sc.BN_ACT[5])):
        x, res, scale, shift = (t.cuda() for t in sr.bn_act_inputs(c, sc.seed("bn_act", i)))
        maps = (scale[0], shift[0]) if c["batches"] == 1 else (scale, shift)
        for with_res in (0, 1):
            r = res if with_res else None
            for relu in (0, 1):
                y, y_bn, y_sum = _bn_act_launch(ops, lib, c, x, scale, shift, res, (with_res, relu, 1, int(with_res and relu)))
                nodes = [y_bn.t if (with_res or relu) else y.t, (y_sum.t if relu else y.t) if with_res else None, y.t if relu else None]
                got = ops.bn_act_tracked(x, *maps, r, bool(relu))
                assert all((g is None) == (w is None) and (g is None or torch.equal(g, w)) for g, w in zip(got, nodes)), (c, with_res, relu)
                lean = ops.bn_act_tracked(x, *maps, r, bool(relu), keep_bn=False)
                last_only = not (with_res or relu)
                assert (lean[0] is None) == (not last_only) and all(
                    (g is None) == (w is None) and (g is None or torch.equal(g, w)) for g, w in zip(lean[1:], nodes[1:])), (c, with_res, relu)
                assert torch.equal(ops.bn_act(x, *maps, r, bool(relu)), y.t)


# ------------------------------------------------------------------------------------------------ bn_act_maxpool
@table("bn_act_maxpool")
def test_bn_act_maxpool(ops, lib, i):
    """Bit-equal to ``max_pool2d`` of the unpooled values the bn_act kernel writes for the same operands; inside the pooled bound
    of the fp64 module chain BatchNorm2d.eval() -> relu -> max_pool2d, with a NaN exactly where that chain has one."""
    c = sc.BN_ACT_MAXPOOL[i]
    info = sc.plan("bn_act_maxpool", c)[0]
    x, scale, shift = sr.pool_inputs(c, sc.seed("bn_act_maxpool", i))
    x = placed(x, "x" in c["off"])
    scale, shift = (scale.cuda(), shift.cuda()) if c["scale"] else (None, None)
    N, C, H, W = c["shape"]
    y = Guarded(sc.pool_out(c), "y" in c["off"])
    ok(lib.pleas_bn_act_maxpool(ptr(x), ptr(scale), ptr(shift), ptr(y.t), N, C, H, W, c["k"], c["k"], c["stride"], c["pad"],
                                int(c["relu"]), ops._stream()), lib)
    assert y.intact()
    want, bound = sr.pool_ref(x, scale, shift, c)
    assert torch.equal(torch.isnan(y.t), torch.isnan(want)), (c, info, "where the module chain has a NaN, and only there")
    assert not sr.finite_close(y.t, want, bound).any(), (c, info)
    if c["scale"]:
        unpooled = ops.bn_act(x.contiguous(), scale, shift, None, c["relu"])
    else:
        unpooled = torch.relu(x) if c["relu"] else x
    assert same(y.t, F.max_pool2d(unpooled, c["k"], c["stride"], c["pad"])), (c, info)
    if not c.get("plant"):
        assert not torch.isnan(y.t).any()


# ------------------------------------------------------------------------------------------------ masked_adam
@table("masked_adam")
def test_masked_adam(ops, i):
    """Per element inside the measured bound of the fp64 Adam; the project's criterion (relative distance below 1e-6 to
    torch.optim.Adam in fp32) on the 11-step cases; where the mask is 0, p, m and v are untouched; the floats on both sides of
    a view are untouched."""
    c = sc.MASKED_ADAM[i]
    p0, mask, m0, v0, sched = sr.adam_inputs(c, sr.ADAM_SEED + i)
    p64, lr_sum, _, pt = sr.adam_ref(c, sr.ADAM_SEED + i)
    n = c["n"]
    p, m, v = Guarded((n,), c["view"]), Guarded((n,)), Guarded((n,))
    for dst, src in ((p, p0), (m, m0), (v, v0)):
        dst.t.copy_(src)
    dmask = placed(mask, c["view"]) if mask is not None else None
    for step, lr, grad in sched:
        ops.masked_adam(p.t, placed(grad, c["view"]), dmask, m.t, v.t, lr, step)
    assert p.intact() and m.intact() and v.intact()
    got = p.t.cpu()
    assert not torch.isnan(got).any() and not torch.isnan(m.t).any() and not torch.isnan(v.t).any()
    worst = float(((got.double() - p64).abs() / sr.adam_bound(p64, lr_sum)).max())
    print("masked_adam %r: worst |p - p64| / bound = %.3f" % (c, worst))
    assert worst <= 1.0, c
    if len(sched) >= 11:
        assert float((got.double() - pt.double()).norm() / pt.double().norm()) < 1e-6
    if mask is not None:          # a zero gradient on a zero state: the update is 0 / eps, m and v stay 0
        still = mask == 0
        assert still.any() and torch.equal(got[still], p0[still]) and not m.t.cpu()[still].any() and not v.t.cpu()[still].any()
        assert m.t.cpu()[~still].any() and v.t.cpu()[~still].any()


# ------------------------------------------------------------------------------------------------ sqerr
@table("sqerr")
def test_sqerr(ops, i):
    c = sc.SQERR[i]
    a, b, base = sr.sqerr_inputs(c, sc.seed("sqerr", i))
    n = c["n"]
    info = sc.plan("sqerr", c)[0]
    scale, dscale = 1.0 / n, 2.0 / n
    out = Guarded((1,), fill=base)
    diff = Guarded((n,)) if c["diff"] else None
    da, db = placed(a), placed(b)
    ops.sqerr(da, db, scale, out.t, accumulate=c["accumulate"], diff=diff.t if diff else None, dscale=dscale)
    want, bound = sr.sqerr_ref(a, b, scale, float(torch.tensor(base)) if c["accumulate"] else 0.0, info["sweeps"])
    got = float(out.t)
    print("sqerr %r: |got - want| = %.3e, bound %.3e" % (c, abs(got - want), bound))
    assert out.intact() and abs(got - want) <= bound, (c, got, want, bound)
    if diff:
        d = dscale * (a.double() - b.double())      # three roundings: dscale to the float the ABI takes, a - b, the product
        assert diff.intact() and ((diff.t.cpu().double() - d).abs() <= 3 * U / (1 - 3 * U) * d.abs() + TINY).all()


# ------------------------------------------------------------------------------------------------ target_residual, loss_final
@table("target_residual")
def test_target_residual(ops, i):
    """The residual bit-equal to ``(out - t) * dscale`` in fp32; every workgroup's partial against the fp64 sum of the pieces it
    strides over; as many partials as the library said, none written behind them; the loss they add up to."""
    c = sc.TARGET_RESIDUAL[i]
    info = sc.plan("target_residual", c)[0]
    out, o1, o2, r1, r2, merged = sr.target_inputs(c, sc.seed("target_residual", i))
    N, C, HW = out.shape
    dscale = 2.0 / out.numel()
    buf = Guarded(out.shape, "out" in c["off"] or (c["inplace"] and "resid" in c["off"]))
    buf.t.copy_(out)
    resid = buf if c["inplace"] else Guarded(out.shape, "resid" in c["off"])
    d1, d2 = placed(o1, "o1" in c["off"]), placed(o2, "o2" in c["off"])
    r1, r2 = r1.cuda(), r2.cuda()
    dout = out.cuda()
    parts = Guarded((2, ops.target_residual_max_partials()))
    cnt = ops.target_residual(buf.t, d1, d2, r1, r2, merged, dscale, parts.t[1], None if c["inplace"] else resid.t)
    assert cnt == info["blocks"] and buf.intact() and resid.intact() and parts.intact()
    t32 = sr.merge_ref(d1, d2, r1, r2, None, None, merged, 1)
    assert not torch.isnan(resid.t).any() and torch.equal(resid.t, (dout - t32) * dscale), c
    if not c["inplace"]:
        assert torch.equal(buf.t, dout)
    d64 = dout.double() - sr.merge_ref(d1.double(), d2.double(), r1, r2, None, None, merged, 1)
    want, bound = sr.target_partials_ref(d64, info["vec"], info["blocks"], info["sweeps"])
    got = parts.t[1, :cnt].double()
    assert ((got - want).abs() <= bound).all(), (c, float(((got - want).abs() / bound).max()))
    assert torch.isnan(parts.t[1, cnt:]).all() and torch.isnan(parts.t[0]).all()
    loss = Guarded((2,))
    ops.loss_final(parts.t, torch.tensor([0, cnt], dtype=torch.int32, device="cuda"), torch.tensor([1.0, 1.0 / out.numel()], device="cuda"), loss.t)
    mean = float(want.sum()) / out.numel()
    assert loss.intact() and float(loss.t[0]) == 0.0 and abs(float(loss.t[1]) - mean) <= float(bound.sum()) / out.numel() + U * mean


def test_loss_final_over_layers_of_different_counts(ops):
    """Five layers in one launch: 0, 1, 65, 130 and ``target_residual_max_partials()`` partials in rows of a stride larger than
    every count, NaN behind each count: fp64 sums of exactly the counted entries, rounded once."""
    top = ops.target_residual_max_partials()
    counts = [0, 1, 65, 130, top]
    stride = top + 7
    g = sr.gen(77)
    parts = torch.rand(len(counts), stride, generator=g) + 0.5
    for l, n in enumerate(counts):
        parts[l, n:] = float("nan")
    scale = torch.rand(len(counts), generator=g) + 0.5
    loss = Guarded((len(counts),))
    ops.loss_final(placed(parts), torch.tensor(counts, dtype=torch.int32, device="cuda"), scale.cuda(), loss.t)
    want = torch.stack([parts[l, :n].double().sum() * scale[l].double() for l, n in enumerate(counts)])
    assert loss.intact() and ((loss.t.cpu().double() - want).abs() <= U * want + TINY).all(), (loss.t, want)


# ------------------------------------------------------------------------------------------------ channel_sum, pool_gather
@table("channel_sum")
def test_channel_sum(ops, i):
    c = sc.CHANNEL_SUM[i]
    info = sc.plan("channel_sum", c)[0]
    x = torch.randn(c["shape"], generator=sr.gen(sc.seed("channel_sum", i))) + 0.25
    out = Guarded((c["shape"][1],))
    ops.channel_sum(placed(x, "x" in c["off"]), out.t)
    want, bound = sr.channel_sum_ref(x, info["vec"], info["sweeps"])
    assert out.intact() and ((out.t.cpu().double() - want).abs() <= bound).all(), (c, info)


@table("pool_gather")
def test_pool_gather(ops, lib, i):
    c = sc.POOL_GATHER[i]
    info = sc.plan("pool_gather", c)[0]
    x, src = sr.pool_gather_inputs(c, sc.seed("pool_gather", i))
    x = placed(x, "x" in c["off"])
    src = src.cuda() if src is not None else None
    K = c["K"] if c["K"] is not None else c["C"]
    y = Guarded((c["N"], K))
    ok(lib.pleas_pool_gather(ptr(x), ptr(src), ptr(y.t), c["N"], c["C"], c["HW"], K, ops._stream()), lib)
    want, bound = sr.pool_gather_ref(x, src, info["vec"])
    assert y.intact() and not torch.isnan(y.t).any() and ((y.t.double() - want).abs() <= bound).all(), (c, info)
    if c["N"] < 100 and not c["off"]:
        assert torch.equal(ops.pool_gather(x.contiguous(), src), y.t)


# ------------------------------------------------------------------------------------------------ top1_count
@table("top1_count")
def test_top1_count(ops, i):
    """Predictions equal to ``torch.argmax`` on the CPU (the first maximal index, a NaN is maximal), hits added to the counter."""
    c = sc.TOP1_COUNT[i]
    x, labels, arg = sr.top1_inputs(c, sc.seed("top1_count", i))
    hits = Guarded((1,), dtype=torch.int64, fill=5)
    pred = Guarded((c["N"],), dtype=torch.int64) if c["pred"] else None
    ops.top1_count(placed(x), labels.cuda(), hits.t, pred.t if pred else None)
    right = int((arg == labels).sum())
    assert hits.intact() and int(hits.t) == 5 + right, (c, int(hits.t), right)
    assert {"right": right == c["N"], "wrong": right == 0, "mixed": 0 < right < c["N"]}[c["labels"]]
    if pred:
        assert pred.intact() and torch.equal(pred.t.cpu(), arg), c


# ------------------------------------------------------------------------------------------------ bn_train_fold(_batches)
@table("bn_train_fold")
def test_bn_train_fold(ops, lib, i):
    """scale and shift per batch inside the fp32 rounding of the fp64 fold, running statistics and counter as after that many
    forwards of the module in fp64; one batch through ``pleas_bn_train_fold``, more through ``pleas_bn_train_fold_batches``."""
    c = sc.BN_TRAIN_FOLD[i]
    info, (n, batches, C, inner) = sc.plan("bn_train_fold", c)
    x, bn = sr.bn_train_inputs(c, sc.seed("bn_train_fold", i))
    ref = sr.bn_train_ref(x, bn, batches)
    bn = bn.cuda()
    dx = placed(x, "x" in c["off"])
    scale, shift = Guarded((batches, C)), Guarded((batches, C))
    w, b = (ptr(bn.weight), ptr(bn.bias)) if c["affine"] else (None, None)
    stats = (ptr(bn.running_mean), ptr(bn.running_var), ptr(bn.num_batches_tracked)) if c["track"] else (None, None, None)
    need = batches * int(lib.pleas_bn_train_ws_bytes(n, C))
    ws = torch.empty(need // 8, dtype=torch.float64, device="cuda")
    momentum = -1.0 if c["momentum"] is None else c["momentum"]
    tail = (w, b, float(bn.eps), momentum) + stats + (ptr(scale.t), ptr(shift.t), ptr(ws), need, ops._stream())
    if batches == 1:
        ok(lib.pleas_bn_train_fold(ptr(dx), n, C, inner, *tail), lib)
    else:
        ok(lib.pleas_bn_train_fold_batches(ptr(dx), n, batches, C, inner, *tail), lib)
    assert scale.intact() and shift.intact()
    for got, name in ((scale.t, "scale"), (shift.t, "shift")):
        err = (got.cpu().double() - ref[name]).abs()
        assert (err <= ref["bound_" + name]).all(), (c, info, name, float((err / ref["bound_" + name]).max()))
    if c["track"]:
        assert ((bn.running_mean.cpu().double() - ref["running_mean"]).abs() <= ref["bound_rm"]).all(), (c, info)
        assert ((bn.running_var.cpu().double() - ref["running_var"]).abs() <= ref["bound_rv"]).all(), (c, info)
        assert int(bn.num_batches_tracked) == ref["counter"]
    if batches == 1 and not c["off"]:        # the wrapper on a copy of the module: the same launch
        again = copy.deepcopy(sr.bn_train_inputs(c, sc.seed("bn_train_fold", i))[1]).cuda()
        s2, h2 = ops.bn_train_fold(again, dx.contiguous())
        assert torch.equal(s2, scale.t[0]) and torch.equal(h2, shift.t[0])
