"""Depthwise convolutions on the library's own kernels (csrc/dwconv.hip) against fp64 references, on the geometries of
tests/depthwise_cases.py, and a depthwise-separable network end to end against the oracle.

Bounds.  u = 2^-24 is one fp32 rounding.  The forward's ``fmaf`` chain has K*K roundings, the bias one more, so
``|y - y64| <= (K*K + 2) u (|w| conv |x| + |bias|)`` with the magnitude from an fp64 convolution of absolute values.  The grouped
forward's residual adds one rounding of the target and carries the factor ``dscale``; its loss is held to any-order summation's
``M u`` of the fp64 sum over the M outputs; the weight gradient to ``(M + 2) u sum |resid * ip|`` over its M = N * Ho * Wo terms.
None of these is a measured tolerance.  Every test prints its worst figure as a fraction of its bound."""
import copy
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depthwise_cases as dc  # noqa: E402

from oracle import pleas_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
IDS = [dc.case_id(c) for c in dc.CASES]
MAPS = ("full", "partial", "absent")


# ------------------------------------------------------------------------------------------------------------ shared data
@functools.lru_cache(maxsize=None)
def _operands(i: int):
    """Case i: fp32 operands on the CPU (never modified), and what the fp64 references share."""
    N, C, H, W, K, s, p = dc.CASES[i]
    g = torch.Generator().manual_seed(100 + i)
    Ho, Wo = dc.out_size(H, W, K, s, p)
    r = lambda *shape: torch.randn(*shape, generator=g)
    d = dict(x=r(N, C, H, W), w=r(C, 1, K, K), bias=r(C), scale=r(C), shift=r(C), res=r(N, C, Ho, Wo), resid=r(N, C, Ho, Wo),
             o1=r(N, C + 1, Ho, Wo), o2=r(N, C + 1, Ho, Wo), perm=torch.randperm(C + 1, generator=g)[:C], shape=(N, C, Ho, Wo))
    d["y64"] = F.conv2d(d["x"].double(), d["w"].double(), None, s, p, groups=C)
    d["mag"] = F.conv2d(d["x"].double().abs(), d["w"].double().abs(), None, s, p, groups=C)
    return d


def _b(d, with_bias: bool):
    """(fp64 output, its magnitude) with or without the bias."""
    if not with_bias:
        return d["y64"], d["mag"]
    b = d["bias"].double().view(1, -1, 1, 1)
    return d["y64"] + b, d["mag"] + b.abs()


def _cuda(d, *names):
    return [d[n].cuda() for n in names]


def _ratio(got: torch.Tensor, want64: torch.Tensor, bound: torch.Tensor) -> float:
    """Worst |got - want| / bound (0 / 0 counts as 0: an exact zero against a zero bound)."""
    err = (got.double().cpu() - want64).abs()
    ok = err <= bound
    frac = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(frac.max()) if frac.numel() else 0.0
    assert bool(ok.all()), "worst error is %.3f of the bound" % worst
    return worst


# ---------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("i", range(len(dc.CASES)), ids=IDS)
def test_forward_against_fp64_and_its_three_uses_agree(i, with_bias):
    from pleas_merging_amd import hip_ops

    N, C, H, W, K, s, p = dc.CASES[i]
    d = _operands(i)
    x, w, bias, scale, shift, res = _cuda(d, "x", "w", "bias", "scale", "shift", "res")
    bias = bias if with_bias else None
    y = hip_ops.dwconv2d(x, w, bias, s, p)
    assert tuple(y.shape) == d["shape"]
    y64, mag = _b(d, with_bias)
    worst = _ratio(y, y64, (K * K + 2) * U * mag)
    print("%s: worst forward error %.3f of (K*K + 2) u |w| conv |x|" % (IDS[i], worst))
    for r, relu in ((res, True), (None, True), (res, False)):
        y1, z1 = hip_ops.dwconv2d(x, w, bias, s, p, scale, shift, r, relu)                  # y and z together
        z2 = hip_ops.dwconv2d(x, w, bias, s, p, scale, shift, r, relu, out=False)           # z only
        z3 = hip_ops.bn_act(y, scale, shift, r, relu)                                       # y only, then the activation pass
        assert torch.equal(y1, y) and torch.equal(z1, z2) and torch.equal(z1, z3)
        if relu:
            assert float(z1.min()) >= 0.0
    # into the caller's tensors
    out, act = torch.full_like(y, 7.0), torch.full_like(y, 7.0)
    got = hip_ops.dwconv2d(x, w, bias, s, p, scale, shift, res, True, out=out, act_out=act)
    assert got[0] is out and got[1] is act and torch.equal(out, y) and torch.equal(act, hip_ops.bn_act(y, scale, shift, res, True))


# --------------------------------------------------------------------------------------------------------- grouped forward
def _row_maps(kind: str, C: int, perm: torch.Tensor):
    """(row1, row2, n_merged) over sources of C + 1 channels: ``full`` every output the average of a channel of each model (a random
    permutation on the second); ``partial`` n_merged < C averaged rows, then rows of the first model alone, then of the second;
    ``absent`` like partial with -1 entries on both sides (some rows lose one source, some both)."""
    idx = torch.arange(C, dtype=torch.int32)
    perm = perm.to(torch.int32)
    if kind == "full":
        return idx.clone(), perm.clone(), C
    m = C // 2
    a = (C - m + 1) // 2
    row1, row2 = idx.clone(), perm.clone()
    row2[m:m + a] = -1
    row1[m + a:] = -1
    if kind == "absent":
        row1[::2] = -1
        row2[1::3] = -1
        row2[::4] = -1
    return row1, row2, m


def _fwd_reference(i: int, kind: str):
    N, C, H, W, K, s, p = dc.CASES[i]
    d = _operands(i)
    with_bias = kind != "full"
    row1, row2, nm = _row_maps(kind, C, d["perm"])
    out64, mag = _b(d, with_bias)
    pick = lambda o, rows: torch.where((rows >= 0).view(1, -1, 1, 1), o.double()[:, rows.clamp_min(0).long()], torch.zeros((), dtype=torch.float64))
    coef = torch.where(torch.arange(C) < nm, 0.5, 1.0).double().view(1, -1, 1, 1)
    tgt64 = coef * (pick(d["o1"], row1) + pick(d["o2"], row2))
    numel = out64.numel()
    dscale, loss_scale = float(torch.tensor(2.0 / numel, dtype=torch.float32)), float(torch.tensor(1.0 / numel, dtype=torch.float32))
    diff = out64 - tgt64
    return dict(with_bias=with_bias, rows=(row1, row2, nm), dscale=dscale, loss_scale=loss_scale, resid64=dscale * diff,
                bound=dscale * ((K * K + 2) * U * mag + U * tgt64.abs()), loss64=loss_scale * float((diff * diff).sum()), M=numel)


def _queue_fwd(batch, i: int, kind: str, keep: list):
    N, C, H, W, K, s, p = dc.CASES[i]
    d, ref = _operands(i), _fwd_reference(i, kind)
    x, w, bias, o1, o2 = _cuda(d, "x", "w", "bias", "o1", "o2")
    row1, row2, nm = ref["rows"]
    resid = torch.full(d["shape"], float("nan"), device="cuda")
    batch.add(x, w, bias if ref["with_bias"] else None, o1, o2, row1.cuda(), row2.cuda(), nm, resid, ref["dscale"], ref["loss_scale"], s, p)
    keep.append(resid)


@functools.lru_cache(maxsize=None)
def _fwd_results(kind: str):
    """Every case alone, then all cases in ONE grouped launch: ``(alone, grouped)``, each a list of (resid, loss) on the CPU."""
    from pleas_merging_amd import hip_ops

    alone = []
    for i in range(len(dc.CASES)):
        batch, keep = hip_ops.DwFwdBatch(torch.device("cuda")), []
        _queue_fwd(batch, i, kind, keep)
        loss = torch.full((1,), float("nan"), device="cuda")
        batch.flush(loss)
        alone.append((keep[0].cpu(), loss.cpu()))
    batch, keep = hip_ops.DwFwdBatch(torch.device("cuda")), []
    for i in range(len(dc.CASES)):
        _queue_fwd(batch, i, kind, keep)
    loss = torch.full((len(dc.CASES),), float("nan"), device="cuda")
    batch.flush(loss)
    first = [r.cpu() for r in keep], loss.cpu()
    batch.relaunch(loss)                      # the fitter's fast path: the same table again
    torch.cuda.synchronize()
    assert all(torch.equal(a, r.cpu()) for a, r in zip(first[0], keep)) and torch.equal(first[1], loss.cpu())
    return alone, [(r, first[1][i:i + 1]) for i, r in enumerate(first[0])]


@pytest.mark.parametrize("kind", MAPS)
@pytest.mark.parametrize("i", range(len(dc.CASES)), ids=IDS)
def test_grouped_forward_residual_and_loss(i, kind):
    ref = _fwd_reference(i, kind)
    alone, grouped = _fwd_results(kind)
    resid, loss = alone[i]
    worst = _ratio(resid, ref["resid64"], ref["bound"])
    rel = abs(float(loss) - ref["loss64"]) / ref["loss64"]
    print("%s %s: worst residual error %.3f of its bound; loss off by %.3g relative, %.3f of M u (M = %d)"
          % (IDS[i], kind, worst, rel, rel / (ref["M"] * U), ref["M"]))
    assert rel <= ref["M"] * U, (float(loss), ref["loss64"], rel, ref["M"] * U)
    assert torch.equal(grouped[i][0], resid) and torch.equal(grouped[i][1], loss)      # one grouped launch == every case alone


# --------------------------------------------------------------------------------------------------------- weight gradient
def _wgrad_reference(i: int):
    N, C, H, W, K, s, p = dc.CASES[i]
    d = _operands(i)

    def grad(x, r):
        w = torch.zeros(C, 1, K, K, dtype=torch.float64, requires_grad=True)
        F.conv2d(x, w, None, s, p, groups=C).backward(r)
        return w.grad

    return grad(d["x"].double(), d["resid"].double()), grad(d["x"].double().abs(), d["resid"].double().abs())


@functools.lru_cache(maxsize=None)
def _wgrad_results():
    from pleas_merging_amd import hip_ops

    def run(cases):
        batch, grads = hip_ops.DwWgradBatch(torch.device("cuda")), []
        for i in cases:
            N, C, H, W, K, s, p = dc.CASES[i]
            resid, x = _cuda(_operands(i), "resid", "x")
            grads.append(torch.full((C, 1, K, K), float("nan"), device="cuda"))
            batch.add(resid, x, grads[-1], s, p)
        batch.flush()
        return [g.cpu() for g in grads]

    every = range(len(dc.CASES))
    return [run([i])[0] for i in every], run(every), run(every)


@pytest.mark.parametrize("i", range(len(dc.CASES)), ids=IDS)
def test_grouped_weight_gradient(i):
    N, C, H, W, K, s, p = dc.CASES[i]
    alone, grouped, again = _wgrad_results()
    g64, mag = _wgrad_reference(i)
    Ho, Wo = dc.out_size(H, W, K, s, p)
    worst = _ratio(alone[i], g64, (N * Ho * Wo + 2) * U * mag)
    print("%s: worst gradient error %.4f of (M + 2) u sum |resid * ip| (M = %d)" % (IDS[i], worst, N * Ho * Wo))
    assert torch.equal(grouped[i], alone[i]) and torch.equal(again[i], grouped[i])


# --------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_of_the_library_and_of_the_wrapper():
    from pleas_merging_amd import _lib, hip_ops
    from pleas_merging_amd._lib import PleasHipError

    lib = _lib.lib()
    N, C, H, W, K, s, p = 2, 5, 7, 9, 3, 1, 1
    x, w, vec = torch.randn(N, C, H, W, device="cuda"), torch.randn(C, 1, K, K, device="cuda"), torch.randn(C, device="cuda")
    y, z, res = torch.empty(N, C, H, W, device="cuda"), torch.empty(N, C, H, W, device="cuda"), torch.randn(N, C, H, W, device="cuda")
    good = dict(x=x.data_ptr(), w=w.data_ptr(), bias=vec.data_ptr(), y=y.data_ptr(), scale=vec.data_ptr(), shift=vec.data_ptr(),
                res=res.data_ptr(), z=z.data_ptr(), relu=1, N=N, C=C, Hin=H, Win=W, K=K, stride=s, pad=p)
    order = ("x", "w", "bias", "y", "scale", "shift", "res", "z", "relu", "N", "C", "Hin", "Win", "K", "stride", "pad")
    call = lambda **over: lib.pleas_dwconv2d_fwd(*[dict(good, **over)[k] for k in order], hip_ops._stream())
    assert call() == 0
    for over in (dict(x=None), dict(w=None), dict(y=None, z=None), dict(shift=None), dict(N=-1), dict(C=0), dict(Hin=0), dict(Win=0),
                 dict(K=2), dict(K=9), dict(stride=0), dict(stride=3), dict(pad=2), dict(x=x.data_ptr() + 4), dict(w=w.data_ptr() + 4),
                 dict(y=y.data_ptr() + 4), dict(z=z.data_ptr() + 8), dict(res=res.data_ptr() + 4), dict(N=1 << 15, C=1 << 15),
                 dict(N=64, C=64, Hin=512, Win=512)):
        assert call(**over) == -22, over
    assert call(N=0) == 0
    torch.cuda.synchronize()
    # the wrapper's own refusals come before the library is reached
    for bad in (lambda: hip_ops.dwconv2d(x.cpu(), w, None, s, p), lambda: hip_ops.dwconv2d(x.double(), w, None, s, p),
                lambda: hip_ops.dwconv2d(x, w.half(), None, s, p), lambda: hip_ops.dwconv2d(x, w.view(1, C, K, K), None, s, p),
                lambda: hip_ops.dwconv2d(x, torch.randn(C + 1, 1, K, K, device="cuda"), None, s, p),
                lambda: hip_ops.dwconv2d(x, torch.randn(C, 1, K, K + 2, device="cuda"), None, s, p),
                lambda: hip_ops.dwconv2d(x, torch.randn(C, 1, 4, 4, device="cuda"), None, s, p),
                lambda: hip_ops.dwconv2d(x, w, None, 3, p), lambda: hip_ops.dwconv2d(x, w, None, s, 2),
                lambda: hip_ops.dwconv2d(x.transpose(2, 3), w, None, s, p), lambda: hip_ops.dwconv2d(x[:, :, :, 1:], w, None, s, p),
                lambda: hip_ops.dwconv2d(x, w, vec[:-1], s, p), lambda: hip_ops.dwconv2d(x, w, None, s, p, scale=vec),
                lambda: hip_ops.dwconv2d(x, w, None, s, p, res=res), lambda: hip_ops.dwconv2d(x, w, None, s, p, vec, vec, res[:1]),
                lambda: hip_ops.dwconv2d(x, w, None, s, p, out=torch.empty(N, C, W, H, device="cuda").transpose(2, 3)),
                lambda: hip_ops.dwconv2d(x, w, None, s, p, out=torch.empty(N, C, H, W + 1, device="cuda")),
                lambda: hip_ops.dwconv2d(x, w, None, s, p, vec, vec, act_out=torch.empty(N, C, W, H, device="cuda").transpose(2, 3))):
        with pytest.raises(PleasHipError):
            bad()
    batch = hip_ops.DwFwdBatch(torch.device("cuda"))
    rows = torch.arange(C, dtype=torch.int32, device="cuda")
    with pytest.raises(PleasHipError):
        batch.add(x, w, None, res, res, rows, rows.long(), C, y, 1.0, 1.0, s, p)
    with pytest.raises(PleasHipError):
        batch.add(x, w, None, res, res, rows, rows, C, y[:, :, :-1], 1.0, 1.0, s, p)
    with pytest.raises(PleasHipError):
        hip_ops.DwWgradBatch(torch.device("cuda")).add(res, x, torch.empty(C, 1, K, K + 2, device="cuda"), s, p)
    assert batch.pending() == 0


# ------------------------------------------------------------------------------------------------------------- end to end
def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / (b.double().cpu().norm() + 1e-30))


@functools.lru_cache(maxsize=None)
def _sepnet_job():
    """Data, the two source models (BatchNorm statistics from 3 train-mode batches, then eval), the spec, and the oracle's run at
    ratio 0: assignment, costs, merged and trained state."""
    from pleas.core.compiler import get_permutation_spec

    g = torch.Generator().manual_seed(3)
    data = [(torch.randn(4, 3, 20, 22, generator=g), torch.zeros(4, dtype=torch.long)) for _ in range(7)]
    models = []
    for seed in (0, 1):
        torch.manual_seed(seed)
        m = dc.SepNet.build(10)
        m.train()
        with torch.no_grad():
            for x, _ in data[:3]:
                m(x)
        models.append(m.eval())
    m1, m2 = models
    spec = get_permutation_spec(m1, ((2, 3, 20, 22),))
    assert sorted(grp.size for grp in spec.values()) == [8, 12, 16], {k: grp.size for k, grp in spec.items()}
    perm, costs = orc.activation_matching(spec, m1, m2, data, 3, accumulate=True)
    o3 = orc.partial_merge(spec, m1, m2, perm, costs, 0.0)
    merged = {k: v.clone() for k, v in o3.state_dict().items()}
    o3, _ = orc.train(data, m1, m2, o3, spec, perm, costs, 0.0, 5, num_classes=10)
    return data, m1, m2, spec, perm, costs, merged, {k: v.clone() for k, v in o3.state_dict().items()}


def _run_job(form: str):
    from pleas.methods.activation_matching import activation_matching
    from pleas.methods.partial_matching import partial_merge
    from pleas.methods.pleas_merging import PleasFitter
    from pleas_merging_amd import hip_ops

    data, m1, m2, spec = _sepnet_job()[:4]
    with hip_ops.depthwise_form(form):
        g1, g2 = copy.deepcopy(m1).cuda(), copy.deepcopy(m2).cuda()
        perm, costs = activation_matching(spec, g1, g2, data, 3, output_costs=True)
        m3 = partial_merge(spec, g1, g2, perm, costs, 0.0)
        fit = PleasFitter(g1, g2, copy.deepcopy(m3), spec, perm, costs, 0.0, 5, num_classes=10)
        vendor_layers = list(fit.vendor_layers)
        n = sum(1 for _ in fit.steps([x for x, _ in data[:6]]))
        got = {k: v.cpu() for k, v in fit.finish().state_dict().items()}
    assert n == 6
    return perm, costs, vendor_layers, fit.fast_updates, got


def test_sepnet_end_to_end_under_the_hip_form_against_the_oracle():
    data, m1, m2, spec, want_perm, want_costs, merged, want = _sepnet_job()
    perm, costs, vendor_layers, fast, got = _run_job("hip")
    for k in spec:
        assert _rel(costs[k], want_costs[k]) < 1e-4, k
        assert torch.equal(perm[k].cpu(), want_perm[k]), k
    assert vendor_layers == [] and fast == 5, (vendor_layers, fast)
    worst, moved = 0.0, 0
    for k in want:
        if k == "conv1.weight" or not want[k].dtype.is_floating_point or torch.equal(want[k], merged[k]):
            continue          # the stem sees the SAME input in both models: its residual is rounding noise (tests/test_hip_odd_layers.py)
        moved += 1
        worst = max(worst, _rel(got[k], want[k]))
        assert _rel(got[k], want[k]) < 1e-4, (k, _rel(got[k], want[k]))
    assert moved >= 6 and not torch.equal(want["dw1.weight"], merged["dw1.weight"]) and not torch.equal(want["dw2.bias"], merged["dw2.bias"])
    travel = lambda w: float((w.double().cpu() - merged["conv1.weight"].double()).abs().max())
    assert travel(got["conv1.weight"]) <= 3 * travel(want["conv1.weight"]) + 1e-7, (travel(got["conv1.weight"]), travel(want["conv1.weight"]))
    print("worst trained tensor %.2e rel-fro from the oracle over %d tensors" % (worst, moved))
    # the same job again: the same bits
    perm2, costs2, _, fast2, got2 = _run_job("hip")
    assert fast2 == 5 and all(torch.equal(perm[k], perm2[k]) and torch.equal(costs[k], costs2[k]) for k in spec)
    assert all(torch.equal(got[k], got2[k]) for k in got)


def test_sepnet_under_the_vendor_form_is_what_it_was():
    data, m1, m2, spec, want_perm, want_costs, merged, want = _sepnet_job()
    perm, costs, vendor_layers, fast, got = _run_job("vendor")
    assert vendor_layers == ["dw1", "dw2"] and fast == 0, (vendor_layers, fast)
    for k in spec:
        assert torch.equal(perm[k].cpu(), want_perm[k]), k
    for k in want:
        if k != "conv1.weight" and want[k].dtype.is_floating_point and not torch.equal(want[k], merged[k]):
            assert _rel(got[k], want[k]) < 1e-4, (k, _rel(got[k], want[k]))


@pytest.mark.parametrize("merging", ["reg_mean", "perm_mixedls"])
def test_stacked_modes_under_the_hip_form_against_the_vendor_form(merging):
    """Two half-batches per layer: the second one's depthwise gradients land in the second arena and are added, its loss is added to the
    first one's.  The vendor form (autograd, layer by layer) is the reference here: same gate as against the oracle."""
    from pleas.methods.partial_matching import partial_merge
    from pleas.methods.pleas_merging import PleasFitter
    from pleas_merging_amd import hip_ops

    data, m1, m2, spec, perm, costs = _sepnet_job()[:6]
    g1, g2 = copy.deepcopy(m1).cuda(), copy.deepcopy(m2).cuda()
    costs = {k: v.cuda() for k, v in costs.items()}
    m3 = partial_merge(spec, g1, g2, perm, costs, 0.0)
    got, losses = {}, {}
    for form in ("vendor", "hip"):
        with hip_ops.depthwise_form(form):
            fit = PleasFitter(g1, g2, copy.deepcopy(m3), spec, perm, costs, 0.0, 5, num_classes=10, merging=merging)
            assert fit.vendor_layers == ([] if form == "hip" else ["dw1", "dw2"])
            assert sum(1 for _ in fit.steps([x for x, _ in data[:6]])) == 6
            assert fit.fast_updates == (5 if form == "hip" else 0)
            losses[form] = fit.loss_sum.cpu()
            got[form] = {k: v.cpu() for k, v in fit.finish().state_dict().items()}
    assert _rel(losses["hip"], losses["vendor"]) < 1e-4, (losses["hip"], losses["vendor"])
    moved = 0
    for k, v in got["vendor"].items():
        if k != "conv1.weight" and v.dtype.is_floating_point and not torch.equal(v, m3.state_dict()[k].cpu()):
            moved += 1
            assert _rel(got["hip"][k], v) < 1e-4, (k, _rel(got["hip"][k], v))
    assert moved >= 6


def test_closed_form_keeps_refusing_depthwise_layers():
    from pleas.methods.partial_matching import partial_merge
    from pleas.methods.pleas_merging import train
    from pleas_merging_amd import hip_ops

    data, m1, m2, spec, perm, costs = _sepnet_job()[:6]
    g1, g2 = copy.deepcopy(m1).cuda(), copy.deepcopy(m2).cuda()
    costs = {k: v.cuda() for k, v in costs.items()}
    m3 = partial_merge(spec, g1, g2, perm, costs, 0.0)
    for form in ("vendor", "hip"):
        with hip_ops.depthwise_form(form):
            with pytest.raises(NotImplementedError, match="not supported: dw1, dw2"):
                train(data[:1], g1, g2, copy.deepcopy(m3), spec, perm, costs, 0.0, False, 1, None, num_classes=10, solver="normal_eq")


def test_inference_graph_with_depthwise_layers_against_the_modules():
    from pleas_merging_amd import hip_ops
    from pleas_merging_amd.methods import source_forward as sf

    data, m1 = _sepnet_job()[:2]
    net = copy.deepcopy(m1).cuda().eval()
    x = torch.cat([b for b, _ in data[:4]]).cuda()
    with torch.no_grad():
        want = net(x)
    with hip_ops.depthwise_form("hip"):
        graph = sf.InferenceBackbone(net)
        calls = [n.target for n in graph.graph.graph.nodes if n.op == "call_function" and isinstance(n.target, sf.HipConvAct)]
        assert sum(1 for t in calls if t.own.dw) == 2
        got = graph(x)
    assert float((got - want).norm() / want.norm()) < 1e-5
    assert torch.equal(got.argmax(1), want.argmax(1))
    # hooks fire on the depthwise modules as on dense ones: the source chain hands them y, bit for bit the plain forward's
    seen = {}
    handle = net.dw2.register_forward_hook(lambda mod, inp, out: seen.update(x=inp[0], y=out))
    with hip_ops.depthwise_form("hip"):
        gm = sf.fuse_bn_act(net)
        with torch.no_grad():
            gm(x)
    handle.remove()
    assert torch.equal(seen["y"], hip_ops.dwconv2d(seen["x"].contiguous(), net.dw2.weight.detach(), net.dw2.bias.detach(), 2, 2))
