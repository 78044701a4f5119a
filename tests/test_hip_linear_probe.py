"""The linear probe's head on the library's kernels (``head="hip"`` of ``train_eval_linear_probe``; reference
pleas/methods/pleas_merging.py:499-570), kernel by kernel and end to end:

1. ``pleas_softmax_xent`` against fp64 on every form of the kernel (a wave per row up to 1024 columns, a workgroup per row above;
   16-byte and scalar accesses), gated by the error of torch's own fp32 ``F.cross_entropy`` on the CPU;
2. its counters against ``top1_count``, labels outside ``[0, C)``, the running loss;
3. repeatability, ``N == 0`` and the argument checks;
4. one step of ``HipProbeHead`` against fp64 autograd and torch's Adam;
5. a whole probe, ``head="hip"`` against ``head="autograd"``;
6. the feature cache.

Measured on an MI355X (worst over the grid of 1., in units of 2^-24): see DESIGN.md section 3.3.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GUARD, SENTINEL = 256, -7.25
WAVE_COLS = 1024                # kXentWaveCols: a wave per row up to here, a workgroup per row above


@pytest.fixture(scope="module")
def ops():
    from pleas_merging_amd import hip_ops

    return hip_ops


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


class Guarded:
    """A NaN-filled fp32 output with a guard band behind it (one allocation: a write past the end lands in the band)."""

    def __init__(self, shape, fill=float("nan")):
        n = 1
        for s in shape:
            n *= s
        self.n = n
        self.whole = torch.full((n + GUARD,), SENTINEL, device="cuda")
        self.t = self.whole[:n].view(shape)
        self.t.fill_(fill)

    def intact(self):
        return bool((self.whole[self.n:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 1. the kernel against fp64
_REFS = {}


def _case(N, C, kind="plain"):
    """Logits, labels and the references of one shape -- fp64, and torch's fp32 ``F.cross_entropy`` on the CPU as the yardstick --
    made once and shared: ``(logits, labels, loss64 [N], dlogits64 [N, C] of the mean, yardsticks (row loss, N * dlogits, mean))``."""
    key = (N, C, kind)
    if key not in _REFS:
        g = torch.Generator().manual_seed(1000003 * N + 7 * C + len(kind))
        logits = (1e4 if kind == "huge" else 10.0) * torch.randn(N, C, generator=g)
        labels = torch.randint(0, C, (N,), generator=g)
        if kind == "neginf" and C > 1:
            drop = torch.rand(N, C, generator=g) < 0.3
            drop[torch.arange(N), labels] = False               # never the label: the loss stays finite
            logits[drop] = float("-inf")
        x64 = logits.double().requires_grad_(True)
        loss64 = F.cross_entropy(x64, labels, reduction="none")
        (d64,) = torch.autograd.grad(loss64.mean(), x64)
        x32 = logits.clone().requires_grad_(True)
        loss32 = F.cross_entropy(x32, labels, reduction="none")
        mean32 = F.cross_entropy(x32, labels)
        (d32,) = torch.autograd.grad(mean32, x32)
        loss64 = loss64.detach()
        yard = (_row_err(loss32.detach(), loss64), N * float((d32.double() - d64).abs().max()),
                _row_err(mean32.detach().reshape(1), loss64.mean().reshape(1)))
        _REFS[key] = (logits, labels, loss64, d64, yard)
    return _REFS[key]


def _row_err(got, want64):
    return float(((got.double().cpu() - want64).abs() / want64.abs().clamp_min(1.0)).max())


@pytest.fixture(scope="module", autouse=True)
def _references_released():
    yield
    _REFS.clear()
    torch.cuda.empty_cache()


def _run(ops, logits_dev, labels, with_dlogits=True):
    N, C = logits_dev.shape
    dl = Guarded((N, C)) if with_dlogits else None
    rows, loss = Guarded((N,)), Guarded((2,))
    loss.t[1] = 0.0                                             # the running sum is added to
    counts = torch.zeros(2, dtype=torch.long, device="cuda")
    out = ops.softmax_xent(logits_dev, labels.cuda(), None, dl.t if dl else None, rows.t, loss.t, counts)
    assert out is rows.t
    torch.cuda.synchronize()
    assert rows.intact() and loss.intact() and (dl is None or dl.intact())
    return (dl.t if dl else None), rows.t, loss.t, counts


def _check(N, C, kind, got, what=""):
    dl, rows, loss, counts = got
    logits, labels, loss64, d64, (y_loss, y_d, y_mean) = _case(N, C, kind)
    e_loss, e_mean = _row_err(rows, loss64), _row_err(loss[:1], loss64.mean().reshape(1))
    e_d = N * float((dl.double().cpu() - d64).abs().max()) if dl is not None else 0.0
    print("softmax_xent %s N=%d C=%d %s: row loss %.2f u (torch %.2f u), N*dlogits %.2f u (torch %.2f u), mean %.2f u (torch %.2f u)"
          % (kind, N, C, what, e_loss / U, y_loss / U, e_d / U, y_d / U, e_mean / U, y_mean / U))
    assert e_loss <= max(3 * y_loss, 8 * U), (e_loss / U, y_loss / U)
    assert e_d <= max(3 * y_d, 8 * U), (e_d / U, y_d / U)
    assert e_mean <= max(3 * y_mean, 8 * U), (e_mean / U, y_mean / U)
    assert float(loss[1]) == float(loss[0])                    # 0 + loss[0]
    assert int(counts[0]) == int((logits.argmax(1) == labels).sum()) and int(counts[1]) == 0


GRID_C = [1, 2, 3, 37, 64, 65, 200, 1000, 1001, WAVE_COLS - 1, WAVE_COLS, WAVE_COLS + 1, 2048, 4099]


@pytest.mark.parametrize("N", [1, 5, 64, 257])
@pytest.mark.parametrize("C", GRID_C)
def test_softmax_xent_vs_fp64(ops, C, N):
    logits, labels = _case(N, C)[:2]
    _check(N, C, "plain", _run(ops, logits.cuda(), labels))


def test_softmax_xent_vs_fp64_imagenet21k_row(ops):
    logits, labels = _case(4, 21841)[:2]
    _check(4, 21841, "plain", _run(ops, logits.cuda(), labels))


@pytest.mark.parametrize("N,C", [(5, 200), (64, 1001), (5, 2048), (5, 4099)])
@pytest.mark.parametrize("kind", ["huge", "neginf"])
def test_softmax_xent_large_and_infinite_logits(ops, kind, N, C):
    """``1e4 * randn``: nothing overflows under the shift by the maximum.  ``-inf`` off the label: probability 0, a zero gradient."""
    logits, labels = _case(N, C, kind)[:2]
    got = _run(ops, logits.cuda(), labels)
    _check(N, C, kind, got)
    if kind == "neginf":
        assert bool((got[0].cpu()[torch.isinf(logits)] == 0).all())


def test_softmax_xent_neg_inf_at_the_label_is_an_infinite_loss(ops):
    logits, labels = (t.clone() for t in _case(5, 37)[:2])
    logits[2, labels[2]] = float("-inf")
    dl, rows, loss, _ = _run(ops, logits.cuda(), labels)
    want = F.cross_entropy(logits, labels, reduction="none")
    assert float(rows[2]) == float("inf") == float(want[2]) and float(loss[0]) == float("inf")
    assert float(dl[2, labels[2]]) == -float(torch.tensor(1.0 / 5, dtype=torch.float32)) and bool(torch.isfinite(dl).all())


@pytest.mark.parametrize("N,C", [(5, 64), (64, 1000), (5, 2048), (5, 37)])
def test_softmax_xent_rows_misaligned_by_slicing(ops, N, C):
    """Row bases that are not 16-byte aligned although C % 4 == 0: the scalar accesses, the same values."""
    logits, labels = _case(N, C)[:2]
    big = torch.empty(N * C + 4, device="cuda")
    for shift in (1, 3):
        view = big[shift:shift + N * C].view(N, C)
        view.copy_(logits)
        assert view.data_ptr() % 16 != 0
        _check(N, C, "plain", _run(ops, view, labels), "offset %d" % shift)


@pytest.mark.parametrize("N,C", [(5, 37), (64, 1024), (5, 4099)])
def test_softmax_xent_without_dlogits(ops, N, C):
    """Evaluation: the loss and the counts only; they are the ones of the call that also writes the gradient."""
    logits, labels = _case(N, C)[:2]
    x = logits.cuda()
    full, lean = _run(ops, x, labels), _run(ops, x, labels, with_dlogits=False)
    _check(N, C, "plain", lean)
    assert all(torch.equal(a, b) for a, b in zip(full[1:], lean[1:]))


# ------------------------------------------------------------------------------------------------ 2. counts
def _tied_rows(C, n, g):
    """n rows [C] with planted ties: two exact maxima, three, all equal, a NaN, the maximum in the last column."""
    rows = 3.0 * torch.randn(n, C, generator=g)
    a, b = C // 3, (2 * C) // 3
    rows[0, a] = rows[0, b] = 40.0
    rows[1, a] = rows[1, b] = 40.0
    rows[2, a] = rows[2, b] = rows[2, C - 1] = 35.5
    rows[3] = 0.25
    rows[4, b] = float("nan")
    rows[5, C - 1] = 50.0
    return rows, a, b


@pytest.mark.parametrize("C", [10, 1000, 1003, 2048, 4099])
def test_softmax_xent_hits_are_top1_counts(ops, C):
    g = torch.Generator().manual_seed(C)
    N = 37
    rows, a, b = _tied_rows(C, N, g)
    labels = rows.argmax(1)
    labels[torch.arange(N) % 3 == 1] += 1
    labels %= C
    labels[0], labels[1] = a, b                   # tied at the label: the first maximal index is the prediction -- a hit, a miss
    labels[7] = rows[7].argmax()
    x, y = rows.cuda(), labels.cuda()
    hits = torch.zeros(1, dtype=torch.long, device="cuda")
    ops.top1_count(x, y, hits)
    counts = torch.zeros(2, dtype=torch.long, device="cuda")
    ops.softmax_xent(x, y, counts=counts, dlogits=torch.empty_like(x))
    ops.softmax_xent(x, y, counts=counts)       # counters accumulate over calls, with and without the gradient
    want = int((rows.argmax(1) == labels).sum())
    assert 0 < want < N and int(hits[0]) == want and counts.tolist() == [2 * want, 0]


@pytest.mark.parametrize("C", [37, 1024, 1025])
def test_softmax_xent_labels_out_of_range(ops, C):
    N = 9
    logits, labels = _case(64, C)[0][:N].contiguous(), _case(64, C)[1][:N].clone()
    x = logits.cuda()
    good = _run(ops, x, labels)
    bad_labels = labels.clone()
    bad_labels[1], bad_labels[6] = -1, C
    dl, rows, loss, counts = _run(ops, x, bad_labels)
    keep = torch.ones(N, dtype=torch.bool)
    keep[[1, 6]] = False
    assert int(counts[1]) == 2
    assert int(counts[0]) == int((logits.argmax(1) == labels)[keep].sum())
    assert bool((dl[~keep] == 0).all()) and bool((rows[~keep] == 0).all())
    assert torch.equal(dl[keep], good[0][keep]) and torch.equal(rows[keep], good[1][keep])
    lim = 2 ** 62
    far = labels.clone()
    far[0], far[8] = lim, -lim                    # far outside: never an address
    _, rows, _, counts = _run(ops, x, far)
    assert int(counts[1]) == 2 and float(rows[0]) == 0 and float(rows[8]) == 0


def test_probe_head_raises_on_a_label_out_of_range_at_its_readback(ops):
    from pleas_merging_amd.methods.linear_probe import HipProbeHead

    torch.manual_seed(0)
    head = HipProbeHead(torch.nn.Linear(32, 5).cuda())
    feats = torch.randn(8, 32, device="cuda")
    labels = torch.tensor([0, 1, 2, 5, 4, 3, 2, 1], device="cuda")
    head.step(feats, labels, 1e-3, 1)
    with pytest.raises(ops.PleasHipError):
        head.epoch_readback()
    head.step(feats, labels.clamp(max=4), 1e-3, 2)
    hits, bad, total, last = head.epoch_readback()         # the counters started again
    assert bad == 0 and 0 <= hits <= 8 and total == last > 0


def test_softmax_xent_running_loss_is_the_fp32_sum_in_call_order(ops):
    loss = torch.zeros(2, device="cuda")
    singles = []
    for N, C in ((5, 37), (64, 200), (5, 4099)):
        logits, labels = _case(N, C)[:2]
        ops.softmax_xent(logits.cuda(), labels.cuda(), loss=loss)
        singles.append(loss[:1].cpu().clone())
    want = torch.zeros(1)
    for s in singles:
        want = want + s
    assert torch.equal(loss[1:].cpu(), want) and float(want) > 0


# ------------------------------------------------------------------------------------------------ 3. repeatability, arguments
@pytest.mark.parametrize("N,C", [(257, 200), (64, 1001), (257, 2048), (64, 4099)])
def test_softmax_xent_twice_gives_the_same_bits(ops, N, C):
    logits, labels = _case(N, C)[:2]
    x = logits.cuda()
    first, second = _run(ops, x, labels), _run(ops, x, labels)
    assert all(torch.equal(a, b) for a, b in zip(first, second))


def test_softmax_xent_empty_batch_and_refused_arguments(ops):
    from pleas_merging_amd import _lib

    fn = _lib.lib().pleas_softmax_xent
    x = torch.randn(4, 8, device="cuda")
    y = torch.zeros(4, dtype=torch.long, device="cuda")
    dl, rows, loss = Guarded((4, 8)), Guarded((4,)), Guarded((2,))
    counts = torch.full((2,), -3, dtype=torch.long, device="cuda")
    args = lambda N, C, d: (x.data_ptr(), y.data_ptr(), N, C, 0.25, d, rows.t.data_ptr(), loss.t.data_ptr(), counts.data_ptr(), None)
    assert fn(*args(0, 8, dl.t.data_ptr())) == 0
    out = ops.softmax_xent(x[:0], y[:0], None, dl.t[:0], rows.t[:0], loss.t, counts)
    assert out.numel() == 0
    EINVAL = -22
    assert fn(*args(4, 0, dl.t.data_ptr())) == EINVAL
    assert fn(*args(4, 8, x.data_ptr())) == EINVAL                      # dlogits aliases the logits
    assert fn(*args(1 << 20, 1 << 10, dl.t.data_ptr())) == EINVAL       # N * C = 2^30: refused before anything is launched
    torch.cuda.synchronize()
    for t in (dl, rows, loss):
        assert bool(torch.isnan(t.t).all()) and t.intact()
    assert counts.tolist() == [-3, -3]
    with pytest.raises(ops.PleasHipError):
        ops.softmax_xent(x, y, dlogits=x)
    with pytest.raises(ops.PleasHipError):
        ops.softmax_xent(x, y.int())
    with pytest.raises(ops.PleasHipError):
        ops.softmax_xent(x.t(), y)
    with pytest.raises(ops.PleasHipError):
        ops.softmax_xent(x, y, loss=torch.zeros(1, device="cuda"))


# ------------------------------------------------------------------------------------------------ 4. one head step
@pytest.mark.parametrize("N,D,C", [(8, 32, 5), (16, 64, 37), (7, 33, 3)])
def test_one_head_step_vs_fp64_autograd_and_torch_adam(ops, N, D, C):
    from pleas_merging_amd.methods.linear_probe import HipProbeHead

    torch.manual_seed(N + D + C)
    fc = torch.nn.Linear(D, C)
    feats, labels = torch.randn(N, D), torch.randint(0, C, (N,))
    fc64 = copy.deepcopy(fc).double()
    loss64 = F.cross_entropy(fc64(feats.double()), labels)
    gw64, gb64 = torch.autograd.grad(loss64, [fc64.weight, fc64.bias])
    loss64 = float(loss64.detach())
    fc32 = copy.deepcopy(fc).cuda()                                      # fp32 autograd on the vendor's kernels: the yardstick
    gw32, gb32 = torch.autograd.grad(F.cross_entropy(fc32(feats.cuda()), labels.cuda()), [fc32.weight, fc32.bias])
    lr = 1e-3
    ref = copy.deepcopy(fc)                                              # torch's Adam on the fp64 gradients cast to fp32
    ref.weight.grad, ref.bias.grad = gw64.float(), gb64.float()
    torch.optim.Adam(ref.parameters(), lr=lr).step()

    head = HipProbeHead(copy.deepcopy(fc).cuda())
    head.step(feats.cuda(), labels.cuda(), lr, 1)
    for name, got, want, own in (("gW", head.gw, gw64, gw32), ("gb", head.gb, gb64, gb32)):
        rel, lim = _rel(got, want), max(3 * _rel(own, want), 2e-6)
        print("head step N=%d D=%d C=%d %s: %.3e from fp64 (autograd fp32 %.3e)" % (N, D, C, name, rel, _rel(own, want)))
        assert rel <= lim, (name, rel, lim)
    hits, bad, total, last = head.epoch_readback()
    assert bad == 0 and total == last
    # the logits are fp32 dot products of D <= 64 terms of O(1) size: their error, and so the loss's, stays below D * 2^-24 ~ 4e-6
    assert abs(last - loss64) <= 1e-5 * max(1.0, loss64)
    with torch.no_grad():
        assert hits == int((fc64(feats.double()).argmax(1) == labels).sum())
    out = head.finish()
    assert type(out) is torch.nn.Linear
    for name, got, want in (("W", out.weight, ref.weight), ("b", out.bias, ref.bias)):
        rel = _rel(got, want)
        print("head step N=%d D=%d C=%d %s after Adam: %.3e from torch's Adam" % (N, D, C, name, rel))
        assert rel <= 1e-6, (name, rel)


# ------------------------------------------------------------------------------------------------ 5. training parity
class _Run:
    def __init__(self):
        self.logs = []

    def log(self, metrics):
        self.logs.append(dict(metrics))


def _probe_setup(t):
    cpu = copy.deepcopy(t.m1)
    cpu.fc = torch.nn.Identity()
    model = copy.deepcopy(cpu).cuda().eval()
    g = torch.Generator().manual_seed(5)
    train = [(b[0], torch.randint(0, 10, (b[0].shape[0],), generator=g)) for b in t.batches()]
    return cpu, model, train, train[:2]


def _fp64_near_ties(cpu, train, epochs, lr, gap=1e-5):
    """The probe replayed in fp64 on the CPU (the same seed: the same fresh head): per epoch, how many training samples had
    their two largest logits closer than ``gap`` when they were counted."""
    ref = copy.deepcopy(cpu).double().eval()
    with torch.no_grad():
        feats = [ref(x.double()) for x, _ in train]
    torch.manual_seed(0)
    fc = torch.nn.Linear(feats[0].shape[-1], 10).double()
    opt = torch.optim.Adam(fc.parameters(), lr=lr)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, epochs * len(train), eta_min=lr / 10)
    near = []
    for _ in range(epochs):
        n = 0
        for f, (_, y) in zip(feats, train):
            logits = fc(f)
            top = logits.detach().topk(2, dim=1).values
            n += int(((top[:, 0] - top[:, 1]) < gap).sum())
            opt.zero_grad()
            F.cross_entropy(logits, y).backward()
            opt.step()
            sched.step()
        near.append(n)
    return near


def test_hip_head_trains_the_probe_as_autograd_does(tiny_bottleneck, monkeypatch):
    from pleas.methods.pleas_merging import HipProbeHead, train_eval_linear_probe

    cpu, model, train, test = _probe_setup(tiny_bottleneck)
    epochs, lr = 2, 1e-3
    readbacks = []
    original = HipProbeHead.epoch_readback
    monkeypatch.setattr(HipProbeHead, "epoch_readback", lambda self: readbacks.append(1) or original(self))
    heads, runs = {}, {}
    for head in ("autograd", "hip"):
        torch.manual_seed(0)                       # the same fresh head
        runs[head] = _Run()
        heads[head] = train_eval_linear_probe(model, train, test, 10, runs[head], "tiny", lr=lr, epochs=epochs, backbone="hip", head=head)
    assert len(readbacks) == epochs + 1           # one per epoch, one for the test loop: no read-back per step
    assert type(heads["hip"]) is torch.nn.Linear
    hip, ref = runs["hip"].logs, runs["autograd"].logs
    assert [sorted(d) for d in hip] == [sorted(d) for d in ref] and len(hip) == epochs + 1
    assert _rel(heads["hip"].weight, heads["autograd"].weight) <= 1e-4
    assert _rel(heads["hip"].bias, heads["autograd"].bias) <= 1e-4
    for a, b in zip(hip, ref):
        assert all(abs(a[k] - b[k]) <= 1e-4 * max(1.0, abs(b[k])) for k in a if k.endswith("loss")), (a, b)
        assert a.get("epoch") == b.get("epoch")
    near = _fp64_near_ties(cpu, train, epochs, lr)
    seen = sum(int(y.numel()) for _, y in train)
    for e, (a, b) in enumerate(zip(hip[:-1], ref[:-1])):
        k = "tiny_linear_probe_train_acc"
        differ = round(abs(a[k] - b[k]) * seen)
        print("probe epoch %d: train accuracy hip %.4f autograd %.4f; %d sample(s) with an fp64 top-2 gap below 1e-5"
              % (e, a[k], b[k], near[e]))
        assert differ <= min(1, near[e]), (e, a[k], b[k], near[e])
    assert hip[-1]["tiny_linear_probe_acc"] == ref[-1]["tiny_linear_probe_acc"] or _test_near_tie(cpu, heads, test)


def _test_near_tie(cpu, heads, test, gap=1e-5):
    """The final test accuracies differ: allowed for ONE sample whose fp64 top-2 gap under the trained head is below ``gap``."""
    ref = copy.deepcopy(cpu).double().eval()
    fc, fc_hip = (copy.deepcopy(heads[h]).double().cpu() for h in ("autograd", "hip"))
    near = differ = 0
    with torch.no_grad():
        for x, _ in test:
            f = ref(x.double())
            top = fc(f).topk(2, dim=1).values
            near += int(((top[:, 0] - top[:, 1]) < gap).sum())
            differ += int((fc(f).argmax(1) != fc_hip(f).argmax(1)).sum())
    print("probe test loop: %d sample(s) predicted differently, %d with an fp64 top-2 gap below 1e-5" % (differ, near))
    return differ <= min(1, near)


# ------------------------------------------------------------------------------------------------ 6. feature cache
@pytest.mark.parametrize("head", ["hip", "autograd"])
def test_feature_cache_runs_the_backbone_once(tiny_bottleneck, head):
    from pleas.methods.pleas_merging import train_eval_linear_probe

    _, model, train, test = _probe_setup(tiny_bottleneck)
    first = next(m for m in model.modules() if isinstance(m, torch.nn.Conv2d))
    epochs = 3
    heads, fired = {}, {}
    for cache in (False, True):
        count = [0]
        handle = first.register_forward_hook(lambda *_: count.__setitem__(0, count[0] + 1))
        torch.manual_seed(0)
        heads[cache] = train_eval_linear_probe(model, train, test, 10, None, "tiny", epochs=epochs, backbone="hip", head=head,
                                               cache_features=cache)
        handle.remove()
        fired[cache] = count[0]
    assert fired == {False: epochs * len(train) + len(test), True: len(train) + len(test)}
    if head == "hip":                             # the backbone and the head are bit-repeatable: no tolerance
        assert torch.equal(heads[True].weight, heads[False].weight) and torch.equal(heads[True].bias, heads[False].bias)
