"""Inputs, fp64 references and derived bounds of the streaming kernels, on whatever device the operands live
(tests/test_stream_coverage.py checks every bound against plain fp32 on the CPU before anything runs on a GPU;
tests/test_hip_stream_paths.py holds the kernels to them).  Cases: tests/stream_cases.py.

u = 2^-24.  Two kinds of comparison:

* bit-equal, where fp32 torch reproduces the kernel's arithmetic: the merges ``(a + b) * coef`` and the residual
  ``(out - t) * dscale`` (coef is 0.5 or 1: the product is exact, so a contracted multiply-add changes nothing), ``relu`` and
  ``y_bn + res`` between the outputs of one bn_act launch, pooling against ``max_pool2d`` of the unpooled values, top-1 against
  ``argmax``, masked Adam where the mask is 0;
* per element against fp64 inside a DERIVED bound: for an affine map u (|x a| + |b| + |bn|) (+ u |sum| after a residual); for
  a sum of n terms depth * u * sum |x_i|, depth = the longest chain of additions one value passes through in that kernel --
  counted beside each reference with the kernel line it was read from.  TINY (the smallest normal fp32) is added where a
  result may be subnormal.

Whether the 16-byte and the scalar path of one kernel give the same bits: yes for merge_blocks, bn_act, bn_act_maxpool (its two
kernels), target_residual's residual (each element is computed alone); no for the sums of target_residual's partials,
channel_sum, pool_gather and bn_train_fold (a thread adds four neighbours first on the 16-byte path) -- those are compared
through the bound."""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
U64 = 2.0 ** -53
TINY = 2.0 ** -126
NAN, INF = float("nan"), float("inf")

# masked_adam, per element:  |p - p64| <= ADAM_FACTOR * ADAM_FP32_VS_FP64 * (|p64| + sum of the steps' lr)
# ADAM_FP32_VS_FP64: the largest such ratio of torch.optim.Adam in fp32 against the fp64 Adam below on the inputs of every case
# of stream_cases.MASKED_ADAM, measured on the CPU by `python tests/stream_ref.py`; the factor allows for the kernel's
# different but equally valid rounding of the scalar factors (1 - b1, b2, lr / bc1, sqrt(bc2) are rounded to fp32 once).
ADAM_FP32_VS_FP64 = 3.33e-7      # the 11-step case with a mask; the others: 5e-8 .. 3.2e-7
ADAM_FACTOR = 4
ADAM_SEED = 500                  # case i of the table is seeded ADAM_SEED + i, here and on the GPU


def gen(seed):
    return torch.Generator().manual_seed(seed)


def finite_close(got, want, bound):
    """|got - want| <= bound wherever want is finite; the same inf / NaN pattern elsewhere.  Returns the failing mask."""
    got, want = got.double(), want.double()
    fin = torch.isfinite(want)
    bad = fin & ~((got - want).abs() <= bound)
    bad |= ~fin & ~(torch.isnan(want) & torch.isnan(got)) & ~(got == want)
    return bad


# ------------------------------------------------------------------------------------------------ merge_blocks
def _index_map(src, out, absent_every, phase, g):
    """``out`` entries in [1, src - 1) (rows 0 and src - 1 stay unreferenced), -1 at positions phase, phase + absent_every, ..."""
    m = torch.randint(1, max(src - 1, 2), (out,), generator=g, dtype=torch.int32)
    if absent_every:
        m[phase::absent_every] = -1
    return m


def merge_inputs(c, seed):
    """w1, w2 with NaN planted in every row / column that no present map entry names (rows 0 and the last among them: what
    an index of -1 would alias), maps as int32."""
    g = gen(seed)
    shape, a = c["shape"], c["axis"]
    w = [torch.randn(shape, generator=g) for _ in range(2)]
    rows = [_index_map(shape[a], c["rows"], 4 if "r%d" % (k + 1) in c["absent"] else 0, k + 1, g) for k in range(2)]
    cols = [None, None]
    if c["cols"] is not None:
        cols = [_index_map(shape[a + 1], c["cols"], 3 if "cross" in c["absent"] else 0, k + 1, g) for k in range(2)]
    for k in range(2):
        for axis, m in ((a, rows[k]), (a + 1, cols[k])):
            if m is None:
                continue
            unused = torch.ones(shape[axis], dtype=torch.bool)
            unused[m[m >= 0].long()] = False
            w[k].index_fill_(axis, unused.nonzero().flatten(), NAN)
    return w[0], w[1], rows[0], rows[1], cols[0], cols[1]


def _gather(w, axis, m):
    shape = [1] * w.dim()
    shape[axis] = -1
    present = (m >= 0).view(shape)
    return torch.where(present, w.index_select(axis, m.clamp_min(0).long()), torch.zeros((), dtype=w.dtype, device=w.device))


def merge_ref(w1, w2, row1, row2, col1, col2, merged, a):
    """``(a + b) * coef`` in the dtype of w1 / w2 (fp32: the kernel's bits), from index_select; an absent entry contributes 0."""
    parts = []
    for w, r, cm in ((w1, row1, col1), (w2, row2, col2)):
        t = _gather(w, a, r)
        parts.append(t if cm is None else _gather(t, a + 1, cm))
    shape = [1] * w1.dim()
    shape[a] = -1
    coef = torch.where(torch.arange(row1.numel(), device=w1.device) < merged, 0.5, 1.0).to(w1.dtype).view(shape)
    return (parts[0] + parts[1]) * coef


# ------------------------------------------------------------------------------------------------ bn_act / bn_act_maxpool
def affine(batches, C, g):
    """scale of either sign away from zero, shift: no two channels (or batches) share either"""
    scale = (0.5 + torch.rand(batches, C, generator=g)) * (1 - 2 * (torch.rand(batches, C, generator=g) < 0.3).float())
    return scale, torch.randn(batches, C, generator=g)


def plant_specials(t, g):
    """NaN, +inf, -inf at three random places each (distinct)."""
    at = torch.randperm(t.numel(), generator=g)[:9]
    t.view(-1)[at[:3]] = NAN
    t.view(-1)[at[3:6]] = INF
    t.view(-1)[at[6:]] = -INF
    return t


def bn_act_inputs(c, seed):
    g = gen(seed)
    shape = c["shape"]
    x, res = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    scale, shift = affine(c["batches"], shape[1], g)
    if c.get("plant") == "x":
        plant_specials(x, g)
    if c.get("plant") == "res":
        plant_specials(res, g)
    return x, res, scale, shift


def bn_chain_ref(x, scale, shift, res, relu):
    """The torch module chain in fp64: BatchNorm2d.eval() (running mean 0, variance 1, eps 1e-300, which 1 absorbs: weight and bias ARE the map) per
    batch -> add -> relu.  Returns (bn, sum, act, bound_bn, bound_sum): sum is bn and act is sum where the step is absent."""
    batches, C = scale.shape
    x4 = x.double().reshape(x.shape[0], C, -1, 1)
    outs, mags = [], []
    for xb, a, b in zip(x4.chunk(batches), scale.double(), shift.double()):
        bn = torch.nn.BatchNorm2d(C, eps=1e-300).double().eval().to(x.device)
        with torch.no_grad():
            bn.weight.copy_(a)
            bn.bias.copy_(b)
            outs.append(bn(xb))
        mags.append((xb * a.view(1, -1, 1, 1)).abs() + b.abs().view(1, -1, 1, 1))
    bn = torch.cat(outs).reshape(x.shape)
    bound_bn = U * (torch.cat(mags).reshape(x.shape) + bn.abs()) + TINY
    sm = bn + res.double() if res is not None else bn
    bound_sum = bound_bn + U * sm.abs() if res is not None else bound_bn
    return bn, sm, (torch.relu(sm) if relu else sm), bound_bn, bound_sum


def pool_inputs(c, seed):
    g = gen(seed)
    x = torch.randn(c["shape"], generator=g)
    scale, shift = affine(1, c["shape"][1], g)
    if c.get("plant") == "x":
        plant_specials(x, g)
        x.view(-1)[0] = NAN          # a corner: the window that also holds the padding
    return x, scale[0], shift[0]


def pool_ref(x, scale, shift, c):
    """BatchNorm2d.eval() -> relu -> max_pool2d in fp64, and the bound: |max a - max b| <= max |a - b| over the window."""
    if c["scale"]:
        _, _, act, bound, _ = bn_chain_ref(x, scale[None], shift[None], None, c["relu"])
    else:
        act = torch.relu(x.double()) if c["relu"] else x.double()
        bound = torch.zeros_like(act)
    pool = lambda t: F.max_pool2d(t, c["k"], c["stride"], c["pad"])
    return pool(act), pool(torch.nan_to_num(bound, nan=0.0, posinf=0.0))


# ------------------------------------------------------------------------------------------------ masked_adam
def adam_inputs(c, seed):
    """p, mask, (m, v) before the first listed step -- zeros when that is step 1, and always where the mask is 0 -- and per step (lr, grad): gradients span
    1e-6 .. 1 from step to step, the rate follows the project's cosine schedule."""
    g = gen(seed)
    n, steps = c["n"], c["steps"]
    p = torch.randn(n, generator=g)
    mask = (torch.rand(n, generator=g) > 0.2).float() if c["mask"] else None
    fresh = steps[0] == 1
    m = torch.zeros(n) if fresh else 0.01 * torch.randn(n, generator=g)
    v = torch.zeros(n) if fresh else 1e-4 * torch.rand(n, generator=g)
    if mask is not None:          # a masked element has had a zero gradient from the first step on: its state is zero
        m, v = m * mask, v * mask
    sched = []
    for i, s in enumerate(steps):
        grad = torch.randn(n, generator=g) * 10 ** float(torch.randint(-6, 1, (1,), generator=g))
        sched.append((s, 5e-4 * 0.5 * (1 + math.cos(math.pi * i / 10)), grad))
    return p, mask, m, v, sched


def f32(v):
    """A Python float as the fp32 value the C ABI receives for it."""
    return float(torch.tensor(v, dtype=torch.float32))


def adam_step64(p, g, mask, m, v, lr, step, b1=0.9, b2=0.999, eps=1e-8):
    """One Adam step in fp64 from its definition (torch.optim.Adam's order of operations); returns new (p, m, v).  lr, b1, b2 and
    eps are the fp32 values ``pleas_masked_adam`` is given: they ARE the operation's parameters (1 - fl32(0.999) differs from
    1e-3 by 1.3e-5 of it -- nothing once v and the bias correction share a history, plain on a state that comes from elsewhere)."""
    lr, b1, b2, eps = f32(lr), f32(b1), f32(b2), f32(eps)
    g = g.double() * mask.double() if mask is not None else g.double()
    m = m + (1 - b1) * (g - m)
    v = v * b2 + (1 - b2) * g * g
    denom = v.sqrt() / math.sqrt(1 - b2 ** step) + eps
    return p - (lr / (1 - b1 ** step)) * m / denom, m, v


def _torch_adam(p, mask, m, v, sched, **hyper):
    pt = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=1.0, **hyper)
    opt.state[pt] = {"step": torch.tensor(0.0), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    for step, lr, grad in sched:
        opt.state[pt]["step"] = torch.tensor(float(step - 1))
        opt.param_groups[0]["lr"] = f32(lr) if hyper else lr
        pt.grad = grad * mask if mask is not None else grad.clone()
        opt.step()
    return pt.detach()


def adam_ref(c, seed):
    """(p64, lr_sum, p32, p_torch): the fp64 Adam; torch.optim.Adam in fp32 (CPU) on the same fp32-valued hyper-parameters -- the
    same operation, what ADAM_FP32_VS_FP64 measures --; and torch.optim.Adam as a caller writes it (0.9, 0.999, 1e-8 as doubles)."""
    p, mask, m, v, sched = adam_inputs(c, seed)
    p64, m64, v64 = p.double(), m.double(), v.double()
    for step, lr, grad in sched:
        p64, m64, v64 = adam_step64(p64, grad, mask, m64, v64, lr, step)
    p32 = _torch_adam(p, mask, m, v, sched, betas=(f32(0.9), f32(0.999)), eps=f32(1e-8))
    return p64, sum(f32(lr) for _, lr, _ in sched), p32, _torch_adam(p, mask, m, v, sched)


def adam_bound(p64, lr_sum):
    return ADAM_FACTOR * ADAM_FP32_VS_FP64 * (p64.abs() + lr_sum)


# ------------------------------------------------------------------------------------------------ sqerr
def sqerr_inputs(c, seed):
    g = gen(seed)
    return torch.randn(c["n"], generator=g), torch.randn(c["n"], generator=g), float(torch.randn(1, generator=g))


def sqerr_ref(a, b, scale, base, sweeps):
    """(want, bound) of out = base + scale * sum (a - b)^2.
    depth (sqerr_partial_kernel): `s = fmaf(d, d, s)` once per sweep and thread, 6 levels of `s += __shfl_xor(s, off)`, 3 adds
    of `t += ws[w]` (the first is to 0); the partials are combined in fp64 (sqerr_final_kernel).  Each term: d = a - b is
    rounded (2u on d^2), the product inside the fma is not.  `scale` arrives as a float (u), the result is rounded to fp32 (u),
    and once more by `out[0] + r`."""
    d2 = (a.double() - b.double()) ** 2
    total = float(d2.sum())
    want = base + scale * total
    depth = sweeps + 6 + 3
    return want, (depth + 2) * U * abs(scale) * total + 2 * U * abs(scale * total) + (U * abs(want) if base else 0.0) + TINY


# ------------------------------------------------------------------------------------------------ target_residual / loss_final
def target_inputs(c, seed):
    """out, o1, o2, row1, row2, n_merged: NaN in every source channel no present map entry names."""
    g = gen(seed)
    N, C, Csrc, HW = c["N"], c["C"], c["Csrc"], c["HW"]
    out = torch.randn(N, C, HW, generator=g)
    o = [torch.randn(N, Csrc, HW, generator=g) for _ in range(2)]
    rows = [_index_map(Csrc, C, 4, k + 1, g) for k in range(2)]
    for k in range(2):
        unused = torch.ones(Csrc, dtype=torch.bool)
        unused[rows[k][rows[k] >= 0].long()] = False
        o[k].index_fill_(1, unused.nonzero().flatten(), NAN)
    return out, o[0], o[1], rows[0], rows[1], C // 3


def target_partials_ref(d64, vec, blocks, sweeps):
    """Per workgroup: the fp64 sum of (out - t)^2 over the pieces it strides over, and its bound.
    depth (target_residual_kernel): `s = fmaf(d[e], d[e], s)` VEC times per sweep, 6 levels of `s += __shfl_xor`, 2 levels of
    `(wsum[0] + wsum[1]) + (wsum[2] + wsum[3])`; d is rounded twice ((a + b) * coef is exact after the add, o - t): 4u on d^2."""
    d2 = (d64 * d64).flatten()
    piece = torch.arange(d2.numel(), device=d2.device) // vec
    block = piece % (blocks * 256) // 256
    sums = torch.zeros(blocks, dtype=torch.float64, device=d2.device).index_add_(0, block, d2)
    return sums, (sweeps * vec + 6 + 2 + 4) * U * sums + TINY


# ------------------------------------------------------------------------------------------------ channel_sum / pool_gather
def channel_sum_ref(x, vec, trips):
    """(want, bound).  depth (channel_sum_kernel): per sample `a += ...` once per trip -- on the 16-byte path after the two
    levels of `(v[0] + v[1]) + (v[2] + v[3])` --, `s += a` once per sample, 8 levels of `red[tid] += red[tid + off]`."""
    N, C = x.shape[:2]
    xd = x.double().reshape(N, C, -1)
    depth = (2 if vec == 4 else 0) + trips + N + 8
    return xd.sum((0, 2)), depth * U * xd.abs().sum((0, 2)) + TINY


def pool_gather_inputs(c, seed):
    g = gen(seed)
    x = torch.randn(c["N"], c["C"], c["HW"], generator=g) + 0.25
    src = torch.randint(0, c["C"], (c["K"],), generator=g, dtype=torch.int32) if c["K"] is not None else None
    return x, src


def pool_gather_ref(x, src, vec):
    """(want, bound).  depth (pool_gather_kernel): `s += ...` once per 64 pieces of the row -- after two levels of
    `(v[0] + v[1]) + (v[2] + v[3])` on the 16-byte path --, 6 levels of `s += __shfl_xor`, then the division rounds once."""
    xd = x.double()
    HW = x.shape[2]
    if src is not None:
        xd = xd.index_select(1, src.long())
    depth = (2 if vec == 4 else 0) + -(-(HW // vec) // 64) + 6
    return xd.mean(2), (depth + 1) * U * xd.abs().sum(2) / HW + TINY


# ------------------------------------------------------------------------------------------------ top1_count
def top1_inputs(c, seed):
    """logits with ties at both ends of a row and a NaN before / after the maximum planted (C >= 3), labels by the case's mode."""
    g = gen(seed)
    N, C = c["N"], c["C"]
    x = torch.randn(N, C, generator=g)
    if C >= 3:
        x[0, 0] = x[0, C - 1] = 9.0           # the maximum at both ends: the first wins
        x[1, 0] = x[1, C - 1] = -9.0          # the minimum at both ends
        x[2, 0], x[2, C - 1] = NAN, 9.0       # a NaN before the maximum
        x[3, 0], x[3, C - 1] = 9.0, NAN       # and after it
        x[4, C // 2] = x[4, C - 1] = NAN      # two: the first
        x[5] = 1.0                            # all equal
        x[N - 1, C - 1] = 9.0                 # the last column of the last row
    arg = torch.argmax(x, 1)
    if c["labels"] == "right":
        labels = arg.clone()
    elif c["labels"] == "wrong":
        labels = (arg + 1) % C if C > 1 else arg - 1
    else:
        labels = torch.where(torch.rand(N, generator=g) < 0.5, arg, torch.randint(0, C, (N,), generator=g))
    return x, labels, arg


# ------------------------------------------------------------------------------------------------ bn_train_fold
def bn_train_inputs(c, seed):
    g = gen(seed)
    C = c["shape"][1]
    per_channel = (1, C) + (1,) * (len(c["shape"]) - 2)
    if c.get("mean"):         # a mean that is large against the (unit) spread
        x = torch.randn(c["shape"], generator=g) + c["mean"]
    else:                     # every channel its own spread and mean
        x = torch.randn(c["shape"], generator=g) * (0.5 + torch.rand(per_channel, generator=g)) + torch.randn(per_channel, generator=g)
    bn = torch.nn.BatchNorm2d(C, momentum=c["momentum"], affine=c["affine"], track_running_stats=c["track"])
    with torch.no_grad():
        if c["affine"]:
            bn.weight.uniform_(0.5, 1.5, generator=g)
            bn.bias.normal_(generator=g)
        if c["track"]:
            bn.running_mean.normal_(generator=g)
            bn.running_var.uniform_(0.5, 1.5, generator=g)
            bn.num_batches_tracked.fill_(c.get("counter", 0))
    return x.reshape(c["shape"][0], C, -1, 1), bn.train()


def bn_train_ref(x, bn, batches):
    """The module chain in fp64, batch after batch.  Returns scale, shift [batches][C] with their bounds, the running statistics
    after the last batch with theirs, and the counter.
    The kernel accumulates sum x and sum x^2 in fp64 (any order: gamma = (count + 8) 2^-53 on each), forms
    var = E[x^2] - mean^2 and the fold in fp64 and rounds scale and shift to fp32 ONCE; the running statistics are rounded to
    fp32 after every batch, as the module stores them."""
    import copy

    ref = copy.deepcopy(bn).double().train()
    scales, shifts, bs, bh = [], [], [], []
    brm = brv = 0.0
    C = x.shape[1]
    for xb in x.double().chunk(batches):
        cnt = xb.numel() // C
        if ref.track_running_stats and ref.momentum is None:
            f = 1.0 / (int(ref.num_batches_tracked) + 1)
        else:
            f = ref.momentum if ref.track_running_stats else 0.0
        with torch.no_grad():
            y = ref(xb)
        mean, var = xb.mean((0, 2, 3)), xb.var((0, 2, 3), unbiased=False)
        g = ref.weight if ref.affine else torch.ones(C, dtype=torch.float64)
        b = ref.bias if ref.affine else torch.zeros(C, dtype=torch.float64)
        sc = g / torch.sqrt(var + ref.eps)
        sh = b - mean * sc
        assert torch.allclose(y, xb * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1), rtol=1e-9, atol=1e-9)      # the fold IS the module
        gam = (cnt + 8) * U64
        ex2, eabs = (xb * xb).mean((0, 2, 3)), xb.abs().mean((0, 2, 3))
        dmean = gam * eabs
        dvar = gam * ex2 + 2 * mean.abs() * dmean + 4 * U64 * (ex2 + mean * mean)
        rel = 0.5 * dvar / (var + ref.eps) + 4 * U64
        scales.append(sc.detach())
        shifts.append(sh.detach())
        bs.append(U * sc.abs() + sc.abs() * rel + TINY)
        bh.append(U * sh.abs() + (mean * sc).abs() * rel + sc.abs() * dmean + 4 * U64 * (b.abs() + (mean * sc).abs()) + TINY)
        if ref.track_running_stats:
            brm = brm + U * ref.running_mean.abs() + f * dmean + TINY
            brv = brv + U * ref.running_var.abs() + f * dvar * cnt / max(cnt - 1, 1) + TINY
    out = dict(scale=torch.stack(scales), shift=torch.stack(shifts), bound_scale=torch.stack(bs).detach(),
               bound_shift=torch.stack(bh).detach())
    if ref.track_running_stats:
        out.update(running_mean=ref.running_mean, running_var=ref.running_var, bound_rm=brm, bound_rv=brv,
                   counter=int(ref.num_batches_tracked))
    return out


if __name__ == "__main__":
    # python tests/stream_ref.py  ->  the value of ADAM_FP32_VS_FP64
    import stream_cases as sc

    worst = 0.0
    for i, c in enumerate(sc.MASKED_ADAM):
        p64, lr_sum, pt, _ = adam_ref(c, ADAM_SEED + i)
        ratio = float(((pt.double() - p64).abs() / (p64.abs() + lr_sum)).max())
        print(c, "max |p32 - p64| / (|p64| + sum lr) = %.3e" % ratio)
        worst = max(worst, ratio)
    print("ADAM_FP32_VS_FP64 = %.3e (stored: %.3e)" % (worst, ADAM_FP32_VS_FP64))
