"""The host side of evaluation on the library's own kernels, without a GPU: the inference rewrite of
``source_forward.fuse_bn_act`` (graph shape; the default graph untouched), the channel map that stands for
``permute_final_features`` (reference pleas/methods/pleas_merging.py:436-466), and the sample-axis split of
``hip_ops.conv2d_act`` at the convolution kernels' per-call limits."""
import copy

import pytest
import torch
from torch import nn

from pleas_merging_amd import hip_ops
from pleas_merging_amd import resnet as zoo
from pleas_merging_amd.methods import evaluation
from pleas_merging_amd.methods import source_forward as sf

# node names of fuse_bn_act(tiny_resnet("bottleneck", (1, 1, 1, 1), 10, 4).eval()) before the inference rewrite existed
TINY_BOTTLENECK_DEFAULT = (
    "x conv1_hip bn_scale bn_shift bn_act_pool bn_scale_1 bn_shift_1 layer1_0_conv1_hip_bn_act bn_scale_2 bn_shift_2 "
    "layer1_0_conv2_hip_bn_act bn_scale_4 bn_shift_4 layer1_0_downsample_0_hip_bn_act bn_scale_3 bn_shift_3 "
    "layer1_0_conv3_hip_bn_act bn_scale_5 bn_shift_5 layer2_0_conv1_hip_bn_act bn_scale_6 bn_shift_6 layer2_0_conv2_hip_bn_act "
    "bn_scale_8 bn_shift_8 layer2_0_downsample_0_hip_bn_act bn_scale_7 bn_shift_7 layer2_0_conv3_hip_bn_act bn_scale_9 "
    "bn_shift_9 layer3_0_conv1_hip_bn_act bn_scale_10 bn_shift_10 layer3_0_conv2_hip_bn_act bn_scale_12 bn_shift_12 "
    "layer3_0_downsample_0_hip_bn_act bn_scale_11 bn_shift_11 layer3_0_conv3_hip_bn_act bn_scale_13 bn_shift_13 "
    "layer4_0_conv1_hip_bn_act bn_scale_14 bn_shift_14 layer4_0_conv2_hip_bn_act bn_scale_16 bn_shift_16 "
    "layer4_0_downsample_0_hip_bn_act bn_scale_15 bn_shift_15 layer4_0_conv3_hip_bn_act avgpool flatten fc output").split()


def _models(tiny_basic, tiny_bottleneck):
    torch.manual_seed(0)
    return {"tiny_basic": copy.deepcopy(tiny_basic.m1), "tiny_bottleneck": copy.deepcopy(tiny_bottleneck.m1),
            "resnet50": zoo.MODELS["resnet50"](num_classes=10).eval()}


def _names(gm):
    return [n.name for n in gm.graph.nodes]


def _targets(gm, kind):
    return [n for n in gm.graph.nodes if n.op == "call_function" and isinstance(n.target, kind)]


def test_inference_graph_shape(tiny_basic, tiny_bottleneck):
    for name, model in _models(tiny_basic, tiny_bottleneck).items():
        for identity_head in (False, True):
            if identity_head:
                model.fc = nn.Identity()
            gm = sf.fuse_bn_act(model, inference=True)
            assert gm is not None, name
            mods = dict(gm.named_modules())
            called = [mods[n.target] for n in gm.graph.nodes if n.op == "call_module"]
            assert not [m for m in called if sf.own_conv_ok(m)], name
            assert not [m for m in called if isinstance(m, (nn.Identity, nn.AdaptiveAvgPool2d, nn.BatchNorm2d))], name
            assert len(_targets(gm, sf.PoolGather)) == 1, name
            # every fused convolution is image-only; none of the two-output callables is left
            assert _targets(gm, sf.HipConvAct) and all(type(n.target) is sf.HipConvAct for n in _targets(gm, sf.HipConvBnAct)), name
            assert len(_targets(gm, sf.HipLinear)) == (0 if identity_head else 1), name
            # the stem stays what it is today: own convolution, then BatchNorm + ReLU + max pooling in one pass
            assert _names(gm)[1] == "conv1_hip" and "bn_act_pool" in _names(gm), name
            out = next(n for n in gm.graph.nodes if n.op == "output").args[0]
            assert isinstance(out.target, sf.PoolGather if identity_head else sf.HipLinear), name


def test_default_graph_is_what_it_was(tiny_basic, tiny_bottleneck):
    torch.manual_seed(0)
    fresh = zoo.tiny_resnet("bottleneck", (1, 1, 1, 1), 10, 4).eval()
    assert _names(sf.fuse_bn_act(fresh)) == TINY_BOTTLENECK_DEFAULT
    for name, model in _models(tiny_basic, tiny_bottleneck).items():
        default, explicit, inference = sf.fuse_bn_act(model), sf.fuse_bn_act(model, inference=False), sf.fuse_bn_act(model, inference=True)
        assert _names(default) == _names(explicit), name
        for gm in (default, explicit):
            assert not _targets(gm, (sf.HipConvAct, sf.PoolGather, sf.HipLinear)), name
            assert _names(gm)[-4:] == ["avgpool", "flatten", "fc", "output"], name
        # the inference graph is the default one with its convolutions renamed and the three head nodes folded into two
        want = [n[:-len("_bn_act")] + "_act" if n.endswith("_hip_bn_act") else n for n in _names(default)[:-4]]
        assert _names(inference) == want + ["pool_gather", "fc_hip", "output"], name


def test_untraceable_model_gives_no_graph_and_the_backbone_runs_the_modules():
    class Branchy(nn.Module):
        def __init__(self):
            super().__init__()
            self.bn = nn.BatchNorm2d(3)

        def forward(self, x):
            return self.bn(x) if x.sum() > 0 else x

    model = Branchy().eval()
    assert sf.fuse_bn_act(model, inference=True) is None
    ib = sf.InferenceBackbone(model)
    x = torch.ones(1, 3, 2, 2)
    assert ib.graph is None and not ib.gather_features(None) and torch.equal(ib(x), model(x))


def test_refresh_takes_the_constants_again(tiny_bottleneck):
    model = copy.deepcopy(tiny_bottleneck.m1).train()
    ib = sf.InferenceBackbone(model)
    assert not model.training                      # an evaluation forward: the wrapper puts the model in eval mode
    before = ib.graph._pleas_scale_layer1_0_bn1.clone()
    with torch.no_grad():
        model.layer1[0].bn1.running_var.mul_(4.0)
    assert torch.equal(ib.graph._pleas_scale_layer1_0_bn1, before)       # constants are taken when the graph is built
    ib.refresh()
    assert torch.allclose(ib.graph._pleas_scale_layer1_0_bn1, sf.fold_bn(model.layer1[0].bn1)[0]) and not torch.equal(
        ib.graph._pleas_scale_layer1_0_bn1, before)


def test_final_feature_map_is_permute_final_features():
    g = torch.Generator().manual_seed(11)
    for _ in range(40):
        ni, mi = (int(v) for v in torch.randint(0, 9, (2,), generator=g))
        if ni + mi == 0:
            continue
        p1, p2 = torch.randperm(ni + mi, generator=g), torch.randperm(ni + mi, generator=g)
        fc_perm = (p1[:ni], p2[:ni], p1[ni:], p2[ni:])
        index = torch.arange(ni + 2 * mi, dtype=torch.float32).repeat(3, 1)
        for idx in (0, 1):
            src = evaluation.final_feature_map(fc_perm, idx)
            want = evaluation.permute_final_features(index, fc_perm, idx)
            assert src.dtype == torch.int64 and torch.equal(want, index[:, src]), (ni, mi, idx)
            assert src.numel() == ni + mi and int(src.min()) >= 0 and int(src.max()) < ni + 2 * mi


def test_channel_map_refuses_entries_out_of_range():
    assert hip_ops.channel_map([2, 0, 0, 1], 3, "cpu").tolist() == [2, 0, 0, 1]
    for bad in ([0, 3], [-1, 0], []):
        with pytest.raises(hip_ops.PleasHipError):
            hip_ops.channel_map(bad, 3, "cpu")


def _check_split(parts, N, per_out, pixels, limit):
    assert parts[0][0] == 0 and sum(n for _, n in parts) == N
    assert all(a[0] + a[1] == b[0] for a, b in zip(parts, parts[1:]))
    assert all(0 < n and n * per_out < limit and n * pixels < (1 << 31) for _, n in parts)
    most = min((limit - 1) // per_out, ((1 << 31) - 1) // pixels)
    assert len(parts) == -(-N // most)                                   # the fewest calls
    assert max(n for _, n in parts) - min(n for _, n in parts) <= 1      # as equal as possible


def test_sample_axis_split_at_the_limits():
    split, limit = hip_ops.conv2d_sample_split, 1 << 30
    # one output element per sample: 2^30 - 1 is the largest single call, 2^30 the first batch that splits
    assert split(limit - 1, 1, 1) == [(0, limit - 1)]
    assert split(limit, 1, 1) == [(0, limit // 2), (limit // 2, limit // 2)]
    # a ResNet's stem at 224 x 224: 64 x 112 x 112 outputs per sample, 1337 samples fit one call
    per = 64 * 112 * 112
    assert 1337 * per < limit <= 1338 * per
    assert split(1337, per, 112 * 112) == [(0, 1337)]
    assert split(1338, per, 112 * 112) == [(0, 669), (669, 669)]
    # the pixel limit alone (few channels): N * Ho * Wo < 2^31
    assert split(1 << 31, 1, 1, limit=1 << 40) == [(0, 1 << 30), (1 << 30, 1 << 30)]
    assert split((1 << 31) - 1, 1, 1, limit=1 << 40) == [(0, (1 << 31) - 1)]
    for N, per_out, pixels, lim in ((5, 128 * 196, 196, 2 * 128 * 196 + 1), (7, 10, 10, 25), (1000, 3, 1, 100), (9, 100, 100, 101)):
        _check_split(split(N, per_out, pixels, lim), N, per_out, pixels, lim)
    assert split(5, 128 * 196, 196, 2 * 128 * 196 + 1) == [(0, 2), (2, 2), (4, 1)]
    # groups of `align` samples (slices that must start 16-byte aligned): sizes are multiples of it but for the last
    assert split(10, 10, 1, 45, align=2) == [(0, 4), (4, 4), (8, 2)]
    assert split(0, 10, 1) == []
    with pytest.raises(hip_ops.PleasHipError):
        split(3, limit, 1)                        # one sample alone crosses the limit


def test_hip_backbone_refuses_cpu_models_and_unknown_names(tiny_bottleneck):
    model = copy.deepcopy(tiny_bottleneck.m1)
    fc_perm = (torch.arange(2), torch.arange(2), torch.arange(2, 4), torch.arange(2, 4))
    with pytest.raises(hip_ops.PleasHipError):
        evaluation.eval_whole_model(model, [], 10, backbone="hip")
    with pytest.raises(hip_ops.PleasHipError):
        evaluation.eval_perm_model(model, model.fc, [], 10, fc_perm, 0, backbone="hip")
    with pytest.raises(hip_ops.PleasHipError):
        evaluation.train_eval_linear_probe(model, [], [], 10, None, "d", backbone="hip")
    with pytest.raises(ValueError):
        evaluation.eval_whole_model(model, [], 10, backbone="vendor")
