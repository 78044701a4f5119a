"""Host side of the depthwise kernels (csrc/dwconv.hip), no GPU: the C ABI's surface, the plan builders behind the ``*_ws_bytes``
entry points, the argument checks (all made before anything is enqueued), the ``own_dwconv_ok`` predicate and the
``depthwise_form`` switch."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depthwise_cases as dc  # noqa: E402

EINVAL, ENOMEM = -22, -12
NAMES = ("pleas_dwconv2d_fwd", "pleas_dw_fwd_batch_ws_bytes", "pleas_dw_fwd_batch", "pleas_dw_wgrad_batch_ws_bytes",
         "pleas_dw_wgrad_batch")
A = 1 << 20      # a 16-byte aligned address that is never dereferenced: every call below is refused on the host


def _lib():
    from pleas_merging_amd import _lib

    return _lib, _lib.lib()


def _fwd_layers(cases, **over):
    _l, _ = _lib()
    arr = (_l.DwLayer * len(cases))()
    for row, (N, C, H, W, K, s, p) in zip(arr, cases):
        row.N, row.C, row.Hin, row.Win, row.K, row.stride, row.pad = N, C, H, W, K, s, p
        row.Csrc, row.n_merged, row.dscale, row.loss_scale = C, C, 0.5, 0.25
        for k, v in over.items():
            setattr(row, k, v)
    return arr


def _wgrad_layers(cases, **over):
    _l, _ = _lib()
    arr = (_l.DwWgradLayer * len(cases))()
    for row, (N, C, H, W, K, s, p) in zip(arr, cases):
        row.N, row.C, row.Hin, row.Win, row.K, row.stride, row.pad = N, C, H, W, K, s, p
        for k, v in over.items():
            setattr(row, k, v)
    return arr


def test_symbols_are_exported_and_bound():
    _l, lib = _lib()
    raw = ctypes.CDLL(_l.LIB_PATH)
    for name in NAMES:
        assert name in _l.SIGNATURES and hasattr(raw, name), name
        assert getattr(lib, name).argtypes == _l.SIGNATURES[name][1], name
    for struct, fields in ((_l.DwLayer, 19), (_l.DwWgradLayer, 10)):
        assert len(struct._fields_) == fields
    # the structs as the header lays them out: 8 (3) pointers, then 4-byte fields
    assert ctypes.sizeof(_l.DwLayer) == 8 * 8 + 11 * 4 + 4 and ctypes.sizeof(_l.DwWgradLayer) == 3 * 8 + 7 * 4 + 4


def test_ws_bytes_answers_on_the_case_list_and_refuses_with_a_message():
    _l, lib = _lib()
    one_by_one = [int(lib.pleas_dw_fwd_batch_ws_bytes(_fwd_layers([c]), 1)) for c in dc.CASES]
    assert all(v > 0 and v % 256 == 0 for v in one_by_one), one_by_one
    whole = int(lib.pleas_dw_fwd_batch_ws_bytes(_fwd_layers(dc.CASES), len(dc.CASES)))
    assert max(one_by_one) < whole <= sum(one_by_one)
    one_by_one = [int(lib.pleas_dw_wgrad_batch_ws_bytes(_wgrad_layers([c]), 1)) for c in dc.CASES]
    assert all(v > 0 and v % 256 == 0 for v in one_by_one), one_by_one
    whole = int(lib.pleas_dw_wgrad_batch_ws_bytes(_wgrad_layers(dc.CASES), len(dc.CASES)))
    assert max(one_by_one) < whole <= sum(one_by_one)
    # the gradient's partials grow with the slabs: (5, 3, 37, 41) has 185 output rows of 41 -> 4 slabs of 49 rows per channel
    small, large = (int(lib.pleas_dw_wgrad_batch_ws_bytes(_wgrad_layers([(n, 3, 37, 41, 3, 1, 1)]), 1)) for n in (1, 50))
    assert large > small
    bad = [dict(K=4), dict(K=9), dict(K=0), dict(stride=3), dict(stride=0), dict(pad=2), dict(pad=-1), dict(C=0), dict(N=0), dict(N=-1),
           dict(Hin=0), dict(Win=-3), dict(Hin=1, Win=1, pad=0), dict(N=1 << 20, C=1 << 12)]
    for over in bad:
        for fn, make in ((lib.pleas_dw_fwd_batch_ws_bytes, _fwd_layers), (lib.pleas_dw_wgrad_batch_ws_bytes, _wgrad_layers)):
            assert fn(make([dc.CASES[0]], **over), 1) == 0, over
            assert b"invalid argument" in lib.pleas_last_error(), (over, lib.pleas_last_error())
    assert lib.pleas_dw_fwd_batch_ws_bytes(_fwd_layers([dc.CASES[0]], n_merged=6), 1) == 0
    assert lib.pleas_dw_fwd_batch_ws_bytes(_fwd_layers([dc.CASES[0]], Csrc=0), 1) == 0
    assert lib.pleas_dw_fwd_batch_ws_bytes(None, 1) == 0 and lib.pleas_dw_wgrad_batch_ws_bytes(_wgrad_layers([dc.CASES[0]]), 0) == 0


def test_argument_errors_return_einval_without_a_device():
    _l, lib = _lib()
    good = dict(x=A, w=A, bias=A, y=A, scale=A, shift=A, res=A, z=A, relu=1, N=2, C=5, Hin=7, Win=9, K=3, stride=1, pad=1)
    order = ("x", "w", "bias", "y", "scale", "shift", "res", "z", "relu", "N", "C", "Hin", "Win", "K", "stride", "pad")

    def call(**over):
        args = dict(good, **over)
        return lib.pleas_dwconv2d_fwd(*[args[k] for k in order], None)

    refused = [dict(x=None), dict(w=None), dict(y=None, z=None), dict(shift=None), dict(scale=None), dict(N=-1), dict(C=0), dict(Hin=0),
               dict(Win=-1), dict(K=2), dict(K=4), dict(K=9), dict(K=0), dict(stride=0), dict(stride=3), dict(pad=2), dict(pad=-1),
               dict(Hin=2, Win=2, pad=0), dict(x=A + 4), dict(w=A + 8), dict(y=A + 4), dict(z=A + 12), dict(res=A + 4),
               dict(bias=A + 2), dict(z=None), dict(z=None, scale=None, shift=None),            # z == NULL: scale / res have no use
               dict(N=1 << 15, C=1 << 15), dict(N=64, C=64, Hin=512, Win=512), dict(N=1, C=1 << 20, Hin=32, Win=32)]
    for over in refused:
        assert call(**over) == EINVAL, over
        assert lib.pleas_last_error().startswith(b"invalid argument"), over
    assert call(N=0) == 0                                             # nothing to do: PLEAS_OK, nothing enqueued
    assert call(N=0, K=4) == EINVAL                                   # ... but the geometry is still checked
    # grouped: lists, pointers, alignment -- then the workspace, still on the host
    fwd = dict(ip=A, w=A, o1=A, o2=A, row1=A, row2=A, resid=A)
    loss = ctypes.c_void_p(A)
    assert lib.pleas_dw_fwd_batch(None, 1, loss, None, 0, 1, None) == EINVAL
    assert lib.pleas_dw_fwd_batch(_fwd_layers([dc.CASES[0]], **fwd), 0, loss, None, 0, 1, None) == EINVAL
    assert lib.pleas_dw_fwd_batch(_fwd_layers([dc.CASES[0]], **fwd), 1, None, None, 0, 1, None) == EINVAL
    for name in fwd:
        assert lib.pleas_dw_fwd_batch(_fwd_layers([dc.CASES[0]], **dict(fwd, **{name: None})), 1, loss, None, 0, 1, None) == EINVAL, name
    for name in ("ip", "w", "o1", "o2", "resid"):
        assert lib.pleas_dw_fwd_batch(_fwd_layers([dc.CASES[0]], **dict(fwd, **{name: A + 4})), 1, loss, None, 0, 1, None) == EINVAL, name
    assert lib.pleas_dw_fwd_batch(_fwd_layers([dc.CASES[0]], **dict(fwd, K=4)), 1, loss, None, 0, 1, None) == EINVAL
    assert lib.pleas_dw_fwd_batch(_fwd_layers(dc.CASES, **fwd), len(dc.CASES), loss, None, 0, 1, None) == ENOMEM
    assert lib.pleas_dw_fwd_batch(_fwd_layers(dc.CASES, **fwd), len(dc.CASES), loss, A, 256, 1, None) == ENOMEM
    assert b"workspace too small" in lib.pleas_last_error()
    wg = dict(resid=A, ip=A, grad=A)
    assert lib.pleas_dw_wgrad_batch(None, 1, None, 0, 1, None) == EINVAL
    for name in wg:
        assert lib.pleas_dw_wgrad_batch(_wgrad_layers([dc.CASES[0]], **dict(wg, **{name: None})), 1, None, 0, 1, None) == EINVAL, name
        assert lib.pleas_dw_wgrad_batch(_wgrad_layers([dc.CASES[0]], **dict(wg, **{name: A + 8})), 1, None, 0, 1, None) == EINVAL, name
    assert lib.pleas_dw_wgrad_batch(_wgrad_layers([dc.CASES[0]], **dict(wg, stride=4)), 1, None, 0, 1, None) == EINVAL
    assert lib.pleas_dw_wgrad_batch(_wgrad_layers(dc.CASES, **wg), len(dc.CASES), None, 0, 1, None) == ENOMEM
    assert lib.pleas_dw_wgrad_batch(_wgrad_layers(dc.CASES, **wg), len(dc.CASES), A, 256, 1, None) == ENOMEM


MODULES = [      # (what, module, taken under "hip")
    ("dense", lambda: nn.Conv2d(8, 8, 3, padding=1), False),
    ("depthwise 3x3", lambda: nn.Conv2d(8, 8, 3, padding=1, groups=8), True),
    ("depthwise 5x5 stride 2, bias", lambda: nn.Conv2d(16, 16, 5, stride=2, padding=2, groups=16, bias=True), True),
    ("depthwise 7x7 unpadded", lambda: nn.Conv2d(4, 4, 7, groups=4, bias=False), True),
    ("depthwise 1x1", lambda: nn.Conv2d(4, 4, 1, groups=4), True),
    ("grouped, not depthwise", lambda: nn.Conv2d(8, 8, 3, padding=1, groups=4), False),
    ("channel multiplier 2", lambda: nn.Conv2d(8, 16, 3, padding=1, groups=8), False),
    ("dilated", lambda: nn.Conv2d(8, 8, 3, padding=2, dilation=2, groups=8), False),
    ("even K", lambda: nn.Conv2d(8, 8, 4, padding=1, groups=8), False),
    ("K = 9", lambda: nn.Conv2d(8, 8, 9, padding=4, groups=8), False),
    ("stride 3", lambda: nn.Conv2d(8, 8, 3, stride=3, padding=1, groups=8), False),
    ("padding above K // 2", lambda: nn.Conv2d(8, 8, 3, padding=2, groups=8), False),
    ("rectangular kernel", lambda: nn.Conv2d(8, 8, (1, 3), padding=(0, 1), groups=8), False),
    ("two strides", lambda: nn.Conv2d(8, 8, 3, stride=(1, 2), padding=1, groups=8), False),
    ("padding='same'", lambda: nn.Conv2d(8, 8, 3, padding="same", groups=8), False),
    ("reflect padding", lambda: nn.Conv2d(8, 8, 3, padding=1, padding_mode="reflect", groups=8), False),
    ("fp64 weight", lambda: nn.Conv2d(8, 8, 3, padding=1, groups=8).double(), False),
    ("a Linear", lambda: nn.Linear(8, 8), False),
]


class _Sub(nn.Conv2d):
    pass


def test_own_dwconv_ok_over_a_table_of_modules_under_both_forms():
    from pleas_merging_amd import hip_ops
    from pleas_merging_amd.methods.source_forward import own_conv_ok, own_dwconv_ok

    for what, make, taken in MODULES:
        mod = make()
        with hip_ops.depthwise_form("vendor"):
            assert own_dwconv_ok(mod) is False, what
        with hip_ops.depthwise_form("hip"):
            assert own_dwconv_ok(mod) is taken, what
            assert not (taken and own_conv_ok(mod, "all")), what       # never both kernels
    with hip_ops.depthwise_form("hip"):
        assert own_dwconv_ok(_Sub(8, 8, 3, padding=1, groups=8)) is False      # a plain nn.Conv2d only
        assert own_conv_ok(nn.Conv2d(8, 8, 3, padding=1), "all")               # the dense predicate does not depend on the form


def test_graphs_take_depthwise_layers_under_the_hip_form_only():
    """fx level, no GPU: the eval-mode graph swaps the depthwise modules for the own callables under "hip" and keeps them under
    "vendor" (the graph of every release so far); a train-mode graph keeps them under both."""
    from pleas_merging_amd import hip_ops
    from pleas_merging_amd.methods import source_forward as sf

    def depthwise_calls(gm):
        own = [n.target for n in gm.graph.nodes if n.op == "call_function" and isinstance(n.target, (sf.HipConv, sf.HipConvBnAct))]
        dw = sum(1 for t in own if (t.own if isinstance(t, sf.HipConvBnAct) else t).dw)
        mods = dict(gm.named_modules())
        kept = sum(1 for n in gm.graph.nodes if n.op == "call_module" and isinstance(mods[n.target], nn.Conv2d) and mods[n.target].groups > 1)
        return dw, kept

    torch.manual_seed(0)
    net = dc.SepNet.build().eval()
    with hip_ops.depthwise_form("hip"):
        assert depthwise_calls(sf.fuse_bn_act(net)) == (2, 0)
        assert depthwise_calls(sf.fuse_bn_act(net, inference=True)) == (2, 0)
        net.train()
        assert depthwise_calls(sf.fuse_bn_act(net, train_stats=True, train_convs=True)) == (0, 2)
        net.eval()
    assert depthwise_calls(sf.fuse_bn_act(net)) == (0, 2)
    assert depthwise_calls(sf.fuse_bn_act(net, inference=True)) == (0, 2)


def test_depthwise_form_default_nesting_restore_and_bad_values():
    from pleas_merging_amd import hip_ops as ops

    assert ops.DEPTHWISE_FORMS == ("vendor", "hip")
    if "PLEAS_DEPTHWISE" not in os.environ:
        assert ops.DEPTHWISE == "vendor"
    before = ops.DEPTHWISE
    with ops.depthwise_form("hip"):
        assert ops.DEPTHWISE == "hip"
        with ops.depthwise_form("vendor"):
            assert ops.DEPTHWISE == "vendor"
            with ops.depthwise_form("hip"):
                assert ops.DEPTHWISE == "hip"
            assert ops.DEPTHWISE == "vendor"
        assert ops.DEPTHWISE == "hip"
    assert ops.DEPTHWISE == before
    with pytest.raises(RuntimeError, match="boom"):
        with ops.depthwise_form("hip"):
            raise RuntimeError("boom")
    assert ops.DEPTHWISE == before
    for bad in ("HIP", "", None, 1, "gemm"):
        with pytest.raises(ValueError):
            with ops.depthwise_form(bad):
                pytest.fail("entered the block")
        assert ops.DEPTHWISE == before


def test_the_default_form_follows_the_environment_variable():
    """A fresh interpreter per value (the variable is read at import): ``PLEAS_DEPTHWISE`` overrides the default, a bad value raises."""
    code = "from pleas_merging_amd import hip_ops; print(hip_ops.DEPTHWISE)"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for value, want in ((None, "vendor"), ("hip", "hip"), ("nope", None)):
        env = {k: v for k, v in os.environ.items() if k != "PLEAS_DEPTHWISE"}
        if value is not None:
            env["PLEAS_DEPTHWISE"] = value
        p = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True)
        if want is None:
            assert p.returncode != 0 and "ValueError" in p.stderr, p.stderr
        else:
            assert p.returncode == 0 and p.stdout.strip() == want, (p.stdout, p.stderr)


def test_the_wrapper_refuses_before_the_library_is_reached():
    """CPU tensors, dtypes and shapes are the wrapper's own refusals (``PleasHipError``), raised without a device."""
    from pleas_merging_amd import hip_ops
    from pleas_merging_amd._lib import PleasHipError

    x, w = torch.zeros(1, 4, 5, 5), torch.zeros(4, 1, 3, 3)
    with pytest.raises(PleasHipError, match="GPU"):
        hip_ops.dwconv2d(x, w, None, 1, 1)
    with pytest.raises(PleasHipError, match="GPU"):
        hip_ops.dwconv2d(x, w, None, 1, 1, scale=torch.ones(4), shift=torch.zeros(4), relu=True, out=False)
    assert hip_ops.dwconv_geometry_ok(3, 1, 1) and hip_ops.dwconv_geometry_ok(7, 2, 0) and hip_ops.dwconv_geometry_ok(1, 1, 0)
    for k, s, p in ((2, 1, 0), (9, 1, 4), (3, 3, 1), (3, 0, 1), (3, 1, 2), (3, 1, -1), (0, 1, 0)):
        assert not hip_ops.dwconv_geometry_ok(k, s, p), (k, s, p)
