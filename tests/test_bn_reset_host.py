"""The BN-statistics reset on the library's own kernels (``reset_bn_stats(backbone="hip")``), the parts that need no GPU:

* ``pleas_conv2d_bn_stats_fwd`` refuses what it must before any HIP call, ``pleas_conv2d_bn_stats_ws_bytes`` sizes the workspace;
* ``fuse_bn_act(train_convs=True)`` pairs every convolution of a train-mode graph with its BatchNorm fold, and builds the graph
  it always built without the argument;
* ``reset_bn_stats``'s ``backbone`` argument: default, refusal, and a CPU model under either value.
"""
import copy
import inspect

import pytest
import torch
from torch import nn

EINVAL, ENOMEM = -22, -12
P = 0x10000      # a non-null, 16-byte aligned address that nothing may dereference: every refusal comes before a HIP call


def _stats(**kw):
    """``pleas_conv2d_bn_stats_fwd`` on a legal 3 x 3 layer (6 samples in 3 batches of 392 pixels) with ``kw`` changed."""
    from pleas_merging_amd import _lib

    a = dict(x=P, w=P, bias=None, y=P, N=6, Cin=64, Hin=14, Win=14, Cout=136, KH=3, KW=3, stride=1, pad=1, flags=0, batches=3,
             gamma=None, beta=None, eps=1e-5, momentum=0.1, running_mean=None, running_var=None, num_batches_tracked=None,
             scale=P, shift=P, ws=P, ws_bytes=1 << 30, stream=None)
    assert set(kw) <= set(a), set(kw) - set(a)
    a.update(kw)
    return _lib.lib().pleas_conv2d_bn_stats_fwd(*a.values())


@pytest.mark.parametrize("kw", [dict(x=None), dict(w=None), dict(y=None), dict(scale=None), dict(shift=None), dict(batches=0),
                                dict(batches=-2), dict(batches=4), dict(running_mean=P), dict(running_var=P), dict(ws=P + 4),
                                # one value per channel and batch
                                dict(N=1, Hin=1, Win=1, KH=1, KW=1, pad=0, batches=1),
                                dict(N=2, Hin=1, Win=1, KH=1, KW=1, pad=0, batches=2),
                                # 27 and 98 pixels per batch, several batches: a tile would touch more than two of them
                                dict(N=6, Cout=40, Hin=3, Win=3, KH=1, KW=1, pad=0, batches=2),
                                dict(N=4, Hin=7, Win=7, batches=2),
                                # geometry, as pleas_conv2d_fwd
                                dict(stride=0), dict(KH=9, KW=9), dict(Hin=1, Win=1, pad=0)],
                         ids=lambda kw: ",".join("%s=%s" % (k, "P" if v == P else v) for k, v in kw.items()))
def test_conv2d_bn_stats_refusals_need_no_device(kw):
    assert _stats(**kw) == EINVAL, kw


def test_conv2d_bn_stats_workspace_refusals_and_size():
    from pleas_merging_amd import _lib

    size = _lib.lib().pleas_conv2d_bn_stats_ws_bytes
    need = size(6, 136, 14, 14, 3)
    assert need > 0
    assert _stats(ws=None) == ENOMEM and _stats(ws_bytes=need - 1) == ENOMEM and _stats(ws_bytes=0) == ENOMEM
    # a legal single batch of few pixels is no refusal of the argument checks: it gets as far as the workspace check
    assert _stats(N=6, Cout=40, Hin=3, Win=3, KH=1, KW=1, pad=0, batches=1, ws=None) == ENOMEM
    for empty in ((0, 384, 56, 56, 4), (16, 0, 56, 56, 4), (16, 384, 0, 56, 4), (16, 384, 56, 0, 4), (16, 384, 56, 56, 0),
                  (-1, 384, 56, 56, 1)):
        assert size(*empty) == 0, empty
    # two segments of (sum, sum of squares) per pixel tile and channel, the sums per (batch, channel), and the finalize
    # kernel's moments tail of the same size; the partials do not grow with the batch count
    N, C, H, W, batches = 16, 384, 56, 56, 4
    tiles = -(-N * H * W // 128)
    assert size(N, C, H, W, batches) >= (2 * tiles + 2 * batches) * C * 2 * 8
    assert size(N, C, H, W, batches) - size(N, C, H, W, 1) == 2 * (batches - 1) * C * 2 * 8


def _targets(gm):
    return [n.target if isinstance(n.target, str) else getattr(n.target, "__name__", repr(n.target)) for n in gm.graph.nodes]


def test_train_graph_pairs_every_convolution_with_its_fold(tiny_bottleneck):
    from pleas_merging_amd.methods.source_forward import HipConvBnStats, fuse_bn_act, own_conv_ok

    model = copy.deepcopy(tiny_bottleneck.m1).train()
    bns = [m for m in model.modules() if isinstance(m, nn.BatchNorm2d)]
    gm = fuse_bn_act(model, train_stats=True, train_convs=True)
    assert gm is not None and gm.training and gm.all_batch_statistics_folded
    paired = [n.target for n in gm.graph.nodes if n.op == "call_function" and isinstance(n.target, HipConvBnStats)]
    assert len(paired) == len(bns) and {id(p.bn) for p in paired} == {id(b) for b in bns}
    mods = dict(model.named_modules())
    assert not [n.target for n in gm.graph.nodes if n.op == "call_module" and own_conv_ok(mods[n.target], "all")]
    assert not [t for t in _targets(gm) if t.startswith("bn_train_fold_")]
    # every pairing feeds ONE activation pass with its three results
    for n in gm.graph.nodes:
        if n.op == "call_function" and isinstance(n.target, HipConvBnStats):
            acts = {u for item in n.users for u in item.users}
            assert len(n.users) == 3 and len(acts) == 1, n


def test_train_graph_without_the_argument_is_the_graph_it_was(tiny_bottleneck):
    from pleas_merging_amd.methods.source_forward import HipConv, HipConvBnStats, fuse_bn_act

    model = copy.deepcopy(tiny_bottleneck.m1).train()
    n_bn = sum(isinstance(m, nn.BatchNorm2d) for m in model.modules())
    convs = [k for k, m in model.named_modules() if isinstance(m, nn.Conv2d)]
    assert "train_convs" in inspect.signature(fuse_bn_act).parameters
    assert inspect.signature(fuse_bn_act).parameters["train_convs"].default is False
    for gm in (fuse_bn_act(model, train_stats=True), fuse_bn_act(model, train_stats=True, train_convs=False)):
        targets = _targets(gm)
        assert sum(t.startswith("bn_train_fold_") for t in targets) == n_bn
        assert [n.target for n in gm.graph.nodes if n.op == "call_module" and n.target in convs] == convs
        assert not [n for n in gm.graph.nodes if n.op == "call_function" and isinstance(n.target, (HipConv, HipConvBnStats))]
        # node for node: x, then conv -> fold -> scale -> shift -> activation pass per BatchNorm
        assert targets[:6] == ["x", "conv1", "bn_train_fold_bn1", "getitem", "getitem", "_bn_act_pool"], targets[:6]
    # an eval-mode model takes no notice of the argument
    model.eval()
    assert _targets(fuse_bn_act(model, train_convs=True)) == _targets(fuse_bn_act(model))


def test_reset_bn_stats_backbone_argument(tiny_bottleneck):
    from pleas_merging_amd.methods.extras import reset_bn_stats

    assert inspect.signature(reset_bn_stats).parameters["backbone"].default == "modules"
    t = tiny_bottleneck
    data = t.batches()[:3]
    with pytest.raises(ValueError):
        reset_bn_stats(copy.deepcopy(t.m1), data, 2, backbone="bogus")
    with pytest.raises(ValueError):
        reset_bn_stats(copy.deepcopy(t.m1), data, 2, backbone=None)
    a = reset_bn_stats(copy.deepcopy(t.m1), data, 3, backbone="hip").state_dict()
    b = reset_bn_stats(copy.deepcopy(t.m1), data, 3, backbone="modules").state_dict()
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    assert any(k.endswith("num_batches_tracked") and int(v) == 3 for k, v in a.items())
