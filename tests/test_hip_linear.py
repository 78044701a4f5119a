"""The Linear forward ``pleas_linear_fwd`` (split-K NT GEMM, csrc/linear.hip), ``pleas_column_sum`` and the ``"gemm"`` form of
``hip_ops.linear`` in its two consumers (the probe's head, the inference graph's classifier):

1. the forward against fp64 under the order-independent bound ``gamma_(K+2) (|b_c| + sum_k |x_nk w_ck|)`` -- K products, the
   slab reduce and the bias are at most K + 1 additions whatever their order, so no measurement enters the gate -- on NaN-filled
   outputs with a guard band (the convention of test_hip_tile_forms.py), every case twice for the same bits;
2. the ``"conv"`` form bit-equal to the ``conv2d`` call on views that the two consumers made before the switch existed;
3. ``column_sum`` against fp64 under ``gamma_N sum_n |x_nc|``;
4. one step of ``HipProbeHead``, a two-epoch probe and the inference graph under ``linear_form("gemm")``, with the gates of
   tests/test_hip_linear_probe.py and tests/test_hip_inference.py unchanged: the tests themselves are run.
"""
import copy

import pytest
import torch

import test_hip_linear_probe as lp
from oracle import pleas_oracle as orc

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
Guarded, _rel = lp.Guarded, lp._rel


@pytest.fixture(scope="module")
def ops():
    from pleas_merging_amd import hip_ops

    return hip_ops


def gamma(n):
    return n * U / (1 - n * U)


# ------------------------------------------------------------------------------------------------ 1. forward against fp64
CASES = [
    (1, 1, 1),               # smallest possible
    (5, 3, 4099),            # scalar loads, split K, the last range ends in a ragged chunk
    (64, 64, 32),            # exactly one tile and one chunk
    (65, 65, 33),            # ragged on all three axes
    (63, 200, 2048),         # the head's shape
    (256, 200, 2048),        # the head's shape
    (257, 1000, 512),        # many tiles (S = 6 from 80 tiles and 16 chunks: printed)
    (4, 21841, 64),          # very many classes
    (7, 37, 100),            # K % 4 == 0, rows 16-byte aligned
    (7, 37, 102),            # K % 4 != 0
    (16, 10, 0),             # K = 0
]
_REFS = {}


def _case(N, C, K):
    """Operands on the device and the fp64 reference of one shape, made once and shared, never written:
    ``(x, w, b, x @ w.T in fp64, |x| @ |w|.T in fp64, b in fp64)``."""
    key = (N, C, K)
    if key not in _REFS:
        g = torch.Generator().manual_seed(1000003 * N + 1009 * C + K)
        x, w, b = torch.randn(N, K, generator=g), torch.randn(C, K, generator=g), torch.randn(C, generator=g)
        x64, w64 = x.double(), w.double()
        _REFS[key] = (x.cuda(), w.cuda(), b.cuda(), x64 @ w64.t(), x64.abs() @ w64.abs().t(), b.double())
    return _REFS[key]


@pytest.fixture(scope="module", autouse=True)
def _references_released():
    yield
    _REFS.clear()
    torch.cuda.empty_cache()


def _check_forward(ops, N, C, K, x, w, with_bias, with_out, what=""):
    _, _, b, want, mag, b64 = _case(N, C, K)
    if with_bias:
        want, mag = want + b64, mag + b64.abs()
    got = []
    with ops.linear_form("gemm"):
        for _ in range(2):
            out = Guarded((N, C)) if with_out else None
            y = ops.linear(x, w, b if with_bias else None, out=out.t if with_out else None)
            torch.cuda.synchronize()
            if with_out:
                assert y is out.t and out.intact(), "guard band written"
            assert y.shape == (N, C) and y.dtype == torch.float32 and y.is_contiguous()
            got.append(y)
    err = (got[0].double().cpu() - want).abs()
    lim = gamma(K + 2) * mag
    assert not bool(torch.isnan(got[0]).any()), "an output element was not written"
    worst = float((err / lim.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print("linear N=%d C=%d K=%d bias=%d out=%d %s: S = %d, worst |err| / bound = %.3g"
          % (N, C, K, with_bias, with_out, what, ops.linear_plan_info(N, C, K)[2], worst))
    assert bool((err <= lim).all()), (N, C, K, worst)
    assert torch.equal(got[0], got[1]), "two calls, two results"
    return got[0]


@pytest.mark.parametrize("with_out", [False, True], ids=["fresh", "out"])
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("N,C,K", CASES)
def test_linear_vs_fp64(ops, N, C, K, with_bias, with_out):
    x, w = _case(N, C, K)[:2]
    _check_forward(ops, N, C, K, x, w, with_bias, with_out)


def test_the_cases_reach_split_and_unsplit_k(ops):
    S = {case: ops.linear_plan_info(*case)[2] for case in CASES}
    print("S per case:", S)
    assert any(s > 1 for s in S.values()) and any(s == 1 for s in S.values())
    assert S[(63, 200, 2048)] > 1 and S[(256, 200, 2048)] > 1 and S[(5, 3, 4099)] > 1       # what the table says they reach
    assert S[(64, 64, 32)] == 1 and S[(16, 10, 0)] == 1


@pytest.mark.parametrize("N,C,K", [(7, 37, 100), (63, 200, 2048)])
def test_linear_operands_one_float_into_a_larger_buffer(ops, N, C, K):
    """K % 4 == 0 but neither base is 16-byte aligned: the 4-byte loads, the same bound -- and no copy of x under "gemm"."""
    x, w = _case(N, C, K)[:2]
    bx, bw = torch.empty(N * K + 4, device="cuda"), torch.empty(C * K + 4, device="cuda")
    xv, wv = bx[1:1 + N * K].view(N, K), bw[1:1 + C * K].view(C, K)
    xv.copy_(x)
    wv.copy_(w)
    assert xv.data_ptr() % 16 == 4 and wv.data_ptr() % 16 == 4
    got = _check_forward(ops, N, C, K, xv, wv, True, True, "misaligned")
    with ops.linear_form("gemm"):
        aligned = ops.linear(x, w, _case(N, C, K)[2])
    assert torch.equal(got, aligned)            # the same products in the same order, whatever the load width


def test_linear_copies_a_strided_x(ops):
    N, C, K = 7, 37, 100
    x, w = _case(N, C, K)[:2]
    wide = torch.empty(N, 2 * K, device="cuda")
    wide[:, :K] = x
    with ops.linear_form("gemm"):
        assert torch.equal(ops.linear(wide[:, :K], w), ops.linear(x, w))


# ------------------------------------------------------------------------------------------------ 2. the "conv" form
@pytest.mark.parametrize("N,C,K", [(7, 37, 100), (63, 200, 2048), (256, 200, 2048)])
def test_conv_form_is_the_conv2d_call_on_views(ops, N, C, K):
    x, w, b = _case(N, C, K)[:3]
    want = ops.conv2d(x.view(N, K, 1, 1), w.view(C, K, 1, 1), b, 1, 0).view(N, C)
    with ops.linear_form("conv"):
        assert torch.equal(ops.linear(x, w, b), want)
        out = Guarded((N, C))
        assert ops.linear(x, w, b, out=out.t) is out.t and torch.equal(out.t, want) and out.intact()
        shifted = torch.empty(N * K + 4, device="cuda")[1:1 + N * K].view(N, K)      # not 16-byte aligned: cloned, as the callers did
        shifted.copy_(x)
        assert torch.equal(ops.linear(shifted, w, b), want)


# ------------------------------------------------------------------------------------------------ 3. column_sum
@pytest.mark.parametrize("N,C", [(1, 1), (1, 200), (5, 3), (64, 200), (257, 1000), (4096, 37)])
def test_column_sum_vs_fp64(ops, N, C):
    g = torch.Generator().manual_seed(7 * N + C)
    x = torch.randn(N, C, generator=g)
    want, mag = x.double().sum(0), x.double().abs().sum(0)
    xd = x.cuda()
    got = []
    for _ in range(2):
        out = Guarded((C,))
        assert ops.column_sum(xd, out.t) is out.t
        torch.cuda.synchronize()
        assert out.intact(), "guard band written"
        got.append(out.t)
    assert not bool(torch.isnan(got[0]).any())
    err = (got[0].double().cpu() - want).abs()
    print("column_sum N=%d C=%d: worst |err| / bound = %.3g" % (N, C, float((err / (gamma(N) * mag).clamp_min(1e-300)).max())))
    assert bool((err <= gamma(N) * mag).all())
    assert torch.equal(got[0], got[1])


# ------------------------------------------------------------------------------------------------ 4. the consumers under "gemm"
class _Spy:
    """Counts the calls of ``hip_ops.linear`` / ``column_sum`` / ``channel_sum`` and the form they ran under."""

    def __init__(self, ops, monkeypatch):
        self.forms, self.calls = [], {"column_sum": 0, "channel_sum": 0}
        linear = ops.linear

        def spied_linear(*args, **kwargs):
            self.forms.append(ops.LINEAR)
            return linear(*args, **kwargs)

        monkeypatch.setattr(ops, "linear", spied_linear)
        for name in self.calls:
            monkeypatch.setattr(ops, name, self._counted(name, getattr(ops, name)))

    def _counted(self, name, fn):
        def call(*args, **kwargs):
            self.calls[name] += 1
            return fn(*args, **kwargs)

        return call


@pytest.mark.parametrize("N,D,C", [(8, 32, 5), (16, 64, 37), (7, 33, 3)])
def test_one_head_step_under_gemm(ops, monkeypatch, N, D, C):
    """tests/test_hip_linear_probe.py::test_one_head_step_vs_fp64_autograd_and_torch_adam itself, inside ``linear_form("gemm")``."""
    spy = _Spy(ops, monkeypatch)
    with ops.linear_form("gemm"):
        lp.test_one_head_step_vs_fp64_autograd_and_torch_adam(ops, N, D, C)
    assert spy.forms == ["gemm"] and spy.calls == {"column_sum": 1, "channel_sum": 0}


def test_two_epoch_probe_under_gemm(ops, tiny_bottleneck, monkeypatch):
    """tests/test_hip_linear_probe.py::test_hip_head_trains_the_probe_as_autograd_does itself -- ``head="hip"`` against
    ``head="autograd"``: the same logged accuracies up to one fp64 near-tie, losses within 1e-4, heads within 1e-4 rel-fro,
    ``epochs + 1`` read-backs -- inside ``linear_form("gemm")``."""
    spy = _Spy(ops, monkeypatch)
    with ops.linear_form("gemm"):
        lp.test_hip_head_trains_the_probe_as_autograd_does(tiny_bottleneck, monkeypatch)
    steps = 2 * len(tiny_bottleneck.batches())
    assert spy.forms and set(spy.forms) == {"gemm"} and spy.calls == {"column_sum": steps, "channel_sum": 0}


def test_inference_graph_classifier_under_gemm(ops, tiny_bottleneck, monkeypatch):
    """The merged tiny model's logits through ``InferenceBackbone`` (its classifier is a ``HipLinear``) under "gemm" against an
    fp64 forward of the same modules: the gate of tests/test_hip_inference.py, max(3 x the modules' own distance, 2e-6)."""
    from pleas.core.utils import make_identity_perm
    from pleas_merging_amd.methods.source_forward import HipLinear, InferenceBackbone

    t = tiny_bottleneck
    g = torch.Generator().manual_seed(3)
    costs = {k: torch.eye(grp.size) + 0.01 * torch.rand(grp.size, grp.size, generator=g) for k, grp in t.spec.items()}
    merged = orc.partial_merge(t.spec, copy.deepcopy(t.m1), copy.deepcopy(t.m2), make_identity_perm(t.spec), costs, 0.5).eval()
    x = t.batches()[0][0]
    with torch.no_grad():
        want = copy.deepcopy(merged).double()(x.double())
    model = copy.deepcopy(merged).cuda().eval()
    ib = InferenceBackbone(model)
    assert ib.graph is not None
    assert any(n.op == "call_function" and isinstance(n.target, HipLinear) for n in ib.graph.graph.nodes)
    spy = _Spy(ops, monkeypatch)
    with ops.linear_form("gemm"):
        logits = ib(x.cuda())
        again = ib(x.cuda())
    with torch.no_grad():
        own = _rel(model(x.cuda()), want)
    rel, lim = _rel(logits, want), max(3 * own, 2e-6)
    print("merged tiny model, inference graph under gemm %.3e from fp64 (modules %.3e, gate %.3e)" % (rel, own, lim))
    assert logits.shape == want.shape and rel <= lim
    assert torch.equal(again, logits)
    assert spy.forms == ["gemm", "gemm"]
