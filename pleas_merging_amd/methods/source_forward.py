"""Frozen source forwards with BatchNorm / residual add / ReLU or ReLU6 folded into one HIP pass.

The PLeaS loop runs ``model1(x); model2(x)`` under forward hooks on every Conv2d / Linear
(reference pleas/methods/pleas_merging.py:267-268; both models in ``eval()``, :352-353).  Only the
hooked layers' inputs and outputs are consumed, so everything between two hooked layers is free to
be fused.  ``fuse_bn_act`` rewrites an fx trace of the model:

    bn(x) -> relu                      =>  bn_act(x, scale, shift, None, relu=True)
    bn(x) -> (+ identity) -> relu      =>  bn_act(x, scale, shift, identity, relu=True)
    bn(x)                              =>  bn_act(x, scale, shift, None, relu=False)
    bn(x) -> relu -> MaxPool2d         =>  bn_act_maxpool(x, scale, shift, kernel, stride, padding, relu=True)
                                           (the stem: the full-resolution ReLU output is never written)
    ... -> relu6 in place of relu          =>  the same calls with ``relu=hip_ops.ACT_RELU6`` (``_is_relu`` lists the spellings)

    (train mode, ``train_convs=True``)
    HipConv(conv)(x) -> bn_train_fold  =>  HipConvBnStats: ONE call that stores the convolution's output and folds its batch statistics,
                      + bn_act(...)        taken in the convolution's epilogue (``hip_ops.ConvBnStats``); the activation pass follows

    Conv2d (k x k, dense, undilated)   =>  HipConv(conv)(x): ``hip_ops.conv2d`` -- the grouped forward's tile forms as a plain
                                           convolution, bit-for-bit repeatable (``SOURCE_CONV``)
    Conv2d (depthwise, eval mode)      =>  the same three callables on ``hip_ops.dwconv2d`` under ``hip_ops.depthwise_form("hip")``
                                           (``own_dwconv_ok``); the module on the vendor's kernel otherwise
    HipConv(conv)(x) -> bn_act(...)    =>  HipConvBnAct: ONE launch that stores the convolution's output (the hooks' tensor) and
                                           its activated image from the same registers (``SOURCE_CONV_BN``)

``scale = weight / sqrt(running_var + eps)`` and ``shift = bias - running_mean * scale`` are computed
once in fp64.  The hooked modules are the SAME objects in the rewritten GraphModule, so hooks
registered on the original model keep firing; conv outputs are never written in place.
Values differ from the vendor BN kernel by fp32 rounding only (one fma instead of sub-mul-mul-add).
"""
from __future__ import annotations

import contextlib
import operator
import os
from typing import Callable, Optional

import torch
import torch.fx
import torch.nn.functional as F
from torch import nn

from .. import hip_ops


# Which convolutions of the frozen source / twin forwards run on the library's own kernel instead of the vendor's:
#   "all"    (default) every dense, undilated, square Conv2d.  Two reasons.  (1) Repeatability: MIOpen's immediate-mode picks for
#            k x k layers split K with atomics on small images / batches -- the SAME forward differs from itself run to run from
#            the first 3 x 3 layer on (ResNet-101: layer4's at 128 samples, layer2's at 16, layer1's at 4), which flipped near-tie
#            assignments between two runs of one job (GPUTEST_r04); its deterministic solvers (torch.backends.cudnn.deterministic)
#            are 6-15x slower per 3 x 3 layer.  (2) Time: layer by layer in isolation the vendor's 1 x 1 GEMMs are as fast or
#            faster (profiles/r05_probe_conv_classes_128.txt), but IN THE JOB -- two models on two streams beside each other,
#            no layout transposes, one dispatch path -- the own kernel for every layer is the fastest arrangement: 6.07 s per job
#            against 6.18 s with the 1 x 1 layers on the vendor's GEMM (same box; under the split-bf16 arithmetic 4.90 against
#            5.27 s; profiles/r05_exp_source_conv.txt).
#   "kxk"    only the layers with k > 1 (the 1 x 1 layers on the vendor's GEMM: measured repeatable);  "vendor"  none (rounds 1-4).
SOURCE_CONV = os.environ.get("PLEAS_SOURCE_CONV", "all")
# "1" (default): an own convolution whose only consumer is an eval-mode BatchNorm chain takes that chain into its epilogue
# (``hip_ops.conv2d_bn_act``: same bits as the two launches, the convolution's output is not read back); "0": two launches.
SOURCE_CONV_BN = os.environ.get("PLEAS_SOURCE_CONV_BN", "1")


def own_conv_ok(mod: nn.Module, mode: Optional[str] = None) -> bool:
    """Does ``mod`` go through ``hip_ops.conv2d`` under ``mode`` (default: ``SOURCE_CONV``)?"""
    mode = SOURCE_CONV if mode is None else mode
    if mode == "vendor" or type(mod) is not nn.Conv2d:
        return False
    if not (mod.groups == 1 and mod.dilation == (1, 1) and mod.padding_mode == "zeros" and isinstance(mod.padding, tuple)
            and mod.stride[0] == mod.stride[1] and mod.padding[0] == mod.padding[1] and mod.kernel_size[0] == mod.kernel_size[1]):
        return False
    k = mod.kernel_size[0]
    return mod.weight.dtype == torch.float32 and k * k <= 64 and (k > 1 or mode == "all")


def own_dwconv_ok(mod: nn.Module) -> bool:
    """Does ``mod`` go through ``hip_ops.dwconv2d``?  Under ``hip_ops.depthwise_form("hip")`` only: a plain ``nn.Conv2d`` with
    ``groups == in_channels == out_channels`` (one filter per channel), zeros padding, no dilation, fp32, a square odd kernel up to
    7 x 7, one stride of 1 or 2 and one padding of at most K // 2 for both axes (csrc/dwconv.hip).  A one-channel layer
    (``groups == 1``) is a dense layer: ``own_conv_ok`` has it."""
    if hip_ops.DEPTHWISE != "hip" or type(mod) is not nn.Conv2d:
        return False
    if not (mod.groups == mod.in_channels == mod.out_channels and mod.groups > 1 and mod.weight.dim() == 4 and mod.weight.shape[1] == 1
            and mod.weight.shape[0] == mod.groups and mod.padding_mode == "zeros" and isinstance(mod.padding, tuple)
            and mod.dilation == (1, 1) and mod.weight.dtype == torch.float32):
        return False
    if not (mod.stride[0] == mod.stride[1] and mod.padding[0] == mod.padding[1] and mod.kernel_size[0] == mod.kernel_size[1]):
        return False
    return hip_ops.dwconv_geometry_ok(mod.kernel_size[0], mod.stride[0], mod.padding[0])


def _own_input(x, w, dims: int = 4):
    """``x``, made contiguous, when the library's own kernel takes this call -- a CUDA fp32 tensor of ``dims`` dimensions, the weight on
    the GPU, no autograd; None otherwise (the caller then runs the module)."""
    if (not x.is_cuda or x.dtype != torch.float32 or x.dim() != dims or not w.is_cuda
            or (torch.is_grad_enabled() and (x.requires_grad or w.requires_grad))):
        return None
    return x if x.is_contiguous() else x.contiguous()


def _aligned16(x):
    """``x``, or a copy of it when its first element is not 16-byte aligned (a slice of a larger tensor)."""
    return x.clone() if x.data_ptr() % 16 else x


def _fire_hooks(mod: nn.Module, x, y):
    """``mod``'s forward hooks, called as its own ``__call__`` would: ``(the output they leave, did one of them return it)``."""
    replaced = False
    for hook in list(mod._forward_hooks.values()):
        out = hook(mod, (x,), y)
        if out is not None:
            y, replaced = out, True
    return y, replaced


class HipConv:
    """Graph callable standing in for a frozen ``nn.Conv2d``: ``hip_ops.conv2d`` on CUDA fp32 inputs without autograd, the
    module itself otherwise.  ``fire_hooks``: the module's forward hooks are called as its own ``__call__`` would (the
    PLeaS taps sit on the ORIGINAL modules, pleas_merging.py:197-231).  k x k weights with Cin % 32 == 0 are kept
    kernel-position-major (the flat-shift tile forms); the copy follows the parameter's version counter."""

    def __init__(self, conv: nn.Conv2d, tag: str, fire_hooks: bool = True):
        self.conv, self.fire_hooks = conv, fire_hooks
        self.k, self.stride, self.pad = conv.kernel_size[0], conv.stride[0], conv.padding[0]
        self.dw = conv.groups > 1      # a depthwise layer (``own_dwconv_ok``): ``hip_ops.dwconv2d``, the weight as it is
        self.kpos = not self.dw and self.k > 1 and conv.weight.shape[1] % 32 == 0
        self._w = self._stamp = None
        self.__name__ = self.__qualname__ = "hip_conv_%s" % tag

    def weight(self) -> torch.Tensor:
        w = self.conv.weight
        stamp = (w.data_ptr(), w._version)
        if self._stamp != stamp:
            with torch.no_grad():
                self._w = (w.detach().permute(0, 2, 3, 1) if self.kpos else w.detach()).contiguous()
            self._stamp = stamp
        return self._w

    def __call__(self, x):
        conv = self.conv
        xc = _own_input(x, conv.weight)
        if xc is None:
            return conv(x)                      # the module's own path, hooks included
        if self.dw:
            y = hip_ops.dwconv2d(_aligned16(xc), self.weight(), conv.bias, self.stride, self.pad)
        else:
            y = hip_ops.conv2d(xc, self.weight(), conv.bias, self.stride, self.pad, self.kpos)
        if self.fire_hooks and conv._forward_hooks:
            y, _ = _fire_hooks(conv, x, y)
        return y


def _bn_act(x, scale, shift, res, relu):
    return hip_ops.bn_act(x, scale, shift, res, relu)


class HipConvBnAct:
    """``bn_act(HipConv(conv)(x), scale, shift, res, relu)`` as ONE launch (``hip_ops.conv2d_bn_act``): the convolution's
    output is still written -- the module's forward hooks get it, it is a regression target of the PLeaS loop -- and the
    activated image is stored beside it from the same registers.  Anything the fused kernel does not take (CPU tensors,
    autograd, an identity that is a strided view) goes through the two calls it replaces, as does the activation after a
    hook that RETURNS another output."""

    suffix = "_bn_act"

    def __init__(self, own: HipConv):
        self.own = own
        self.__name__ = self.__qualname__ = own.__name__ + self.suffix

    def _fused_input(self, x, scale, res):
        """``x`` for the fused kernel (``_own_input``), or None when it does not take the call."""
        if scale.dim() != 1 or (res is not None and (not res.is_contiguous() or res.dtype != torch.float32 or res.data_ptr() % 16)):
            return None
        return _own_input(x, self.own.conv.weight)

    def __call__(self, x, scale, shift, res, relu):
        own, conv = self.own, self.own.conv
        xc = self._fused_input(x, scale, res)
        if xc is None:
            return _bn_act(own(x), scale, shift, res, relu)
        if own.dw:
            y, z = hip_ops.dwconv2d(_aligned16(xc), own.weight(), conv.bias, own.stride, own.pad, scale, shift, res, relu)
        else:
            y, z = hip_ops.conv2d_bn_act(xc, own.weight(), conv.bias, own.stride, own.pad, own.kpos, scale, shift, res, relu)
        if own.fire_hooks and conv._forward_hooks:
            y, replaced = _fire_hooks(conv, x, y)
            if replaced:
                return _bn_act(y, scale, shift, res, relu)
        return z


class HipConvAct(HipConvBnAct):
    """The image-only form of ``HipConvBnAct`` for forwards nobody taps (evaluation): ``hip_ops.conv2d_act`` stores the
    activated image and nothing else.  A convolution that carries forward hooks AT CALL TIME still owes them its output:
    that call takes the two-output path of the parent class, as does everything the fused kernel does not take."""

    suffix = "_act"

    def __call__(self, x, scale, shift, res, relu):
        own, conv = self.own, self.own.conv
        xc = None if own.fire_hooks and conv._forward_hooks else self._fused_input(x, scale, res)
        if xc is None:
            return super().__call__(x, scale, shift, res, relu)
        if own.dw:
            return hip_ops.dwconv2d(_aligned16(xc), own.weight(), conv.bias, own.stride, own.pad, scale, shift, res, relu, out=False)
        return hip_ops.conv2d_act(xc, own.weight(), conv.bias, own.stride, own.pad, own.kpos, scale, shift, res, relu)


class PoolGather:
    """Graph callable of the head: ``AdaptiveAvgPool2d((1, 1))`` -> ``flatten(1)`` as ONE ``hip_ops.pool_gather``.  ``src`` (a
    ``hip_ops.channel_map``, or None) also gathers / reorders the pooled channels in the same pass -- what
    ``permute_final_features`` does to the merged backbone's features.  CPU tensors take the two calls it replaces."""

    def __init__(self):
        self.src = None
        self.__name__ = self.__qualname__ = "pool_gather"

    def __call__(self, x):
        if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
            y = torch.flatten(F.adaptive_avg_pool2d(x, 1), 1)
            return y if self.src is None else y[:, self.src.long()]
        return hip_ops.pool_gather(x, self.src)


class HipLinear:
    """Graph callable standing in for an ``nn.Linear`` on 2-D features: ``hip_ops.linear`` (``conv2d`` with H = W = KH = KW = 1
    on views, or the GEMM form under ``hip_ops.linear_form("gemm")``; no copy of the weight: the parameter is read where it is).
    The module itself for anything else."""

    def __init__(self, fc: nn.Linear, tag: str):
        self.fc = fc
        self.__name__ = self.__qualname__ = "hip_linear_%s" % tag

    def __call__(self, x):
        fc, w = self.fc, self.fc.weight
        xc = _own_input(x, w, 2) if w.dtype == torch.float32 and w.is_contiguous() and not w.data_ptr() % 16 else None
        return fc(x) if xc is None else hip_ops.linear(xc, w.detach(), fc.bias)


def _is_global_avgpool(node: torch.fx.Node, mods) -> bool:
    one = lambda v: v in (1, (1, 1), [1, 1])
    if node.op == "call_module" and len(node.args) == 1 and not node.kwargs:
        m = mods.get(node.target)
        return type(m) is nn.AdaptiveAvgPool2d and one(m.output_size)
    if node.op == "call_function" and node.target is F.adaptive_avg_pool2d and isinstance(node.args[0], torch.fx.Node):
        size = node.args[1] if len(node.args) > 1 else node.kwargs.get("output_size")
        return len(node.args) + len(node.kwargs) == 2 and one(size)
    return False


def _is_flatten1(node: torch.fx.Node, mods) -> bool:
    """``flatten(x, 1)`` in one of its three spellings (on a [N, C, 1, 1] tensor an end_dim of -1 or 3 is the same)."""
    if node.op == "call_module" and len(node.args) == 1 and not node.kwargs:
        m = mods.get(node.target)
        return type(m) is nn.Flatten and m.start_dim == 1 and m.end_dim in (-1, 3)
    if (node.op == "call_function" and node.target is torch.flatten) or (node.op == "call_method" and node.target == "flatten"):
        rest = tuple(node.args[1:])
        start = rest[0] if rest else node.kwargs.get("start_dim", 0)
        end = rest[1] if len(rest) > 1 else node.kwargs.get("end_dim", -1)
        return start == 1 and end in (-1, 3) and len(rest) + len(node.kwargs) <= 2
    return False


def _inference_passes(graph: torch.fx.Graph, mods) -> None:
    """The rewrites of ``fuse_bn_act(.., inference=True)`` on top of the default graph: image-only convolutions, the fused
    head, the own Linear behind it, no ``nn.Identity``."""
    for node in list(graph.nodes):
        if node.op == "call_function" and type(node.target) is HipConvBnAct:
            own = node.target.own
            with graph.inserting_before(node):
                image = graph.create_node("call_function", HipConvAct(own), node.args, {}, name=own.__name__[len("hip_conv_"):] + "_hip_act")
            node.replace_all_uses_with(image)
            graph.erase_node(node)
        elif node.op == "call_module" and type(mods.get(node.target)) is nn.Identity and len(node.args) == 1 and not node.kwargs:
            node.replace_all_uses_with(node.args[0])
            graph.erase_node(node)
    for node in list(graph.nodes):
        if not (_is_global_avgpool(node, mods) and len(node.users) == 1):
            continue
        flat = next(iter(node.users))
        if not _is_flatten1(flat, mods) or flat.args[0] is not node:
            continue
        with graph.inserting_before(flat):
            head = graph.create_node("call_function", PoolGather(), (node.args[0],), {}, name="pool_gather")
        flat.replace_all_uses_with(head)
        graph.erase_node(flat)
        graph.erase_node(node)
        for user in list(head.users):
            fc = mods.get(user.target) if user.op == "call_module" else None
            if type(fc) is nn.Linear and len(user.args) == 1 and not user.kwargs and fc.weight.dtype == torch.float32:
                with graph.inserting_before(user):
                    own = graph.create_node("call_function", HipLinear(fc, user.name), (head,), {}, name=user.name + "_hip")
                user.replace_all_uses_with(own)
                graph.erase_node(user)


def _bn_act_pool(x, scale, shift, kernel, stride, padding, relu):
    if scale is not None and scale.dim() == 2 and scale.shape[0] > 1:
        # several batches with their own maps in one forward (BN-statistics reset): the pooled pass takes one map
        return F.max_pool2d(hip_ops.bn_act(x, scale, shift, None, relu), kernel, stride, padding)
    if scale is not None and scale.dim() == 2:
        scale, shift = scale[0], shift[0]
    return hip_ops.bn_act_maxpool(x, scale, shift, kernel, stride, padding, relu)


class BatchesPerForward:
    """How many batches lie back to back in the tensor a rewritten graph is forwarding right now (read by its train-mode
    BatchNorm folds); the caller sets ``parts`` around the call: ``with state.of(k): graph(torch.cat(k batches))``."""
    parts = 1

    @contextlib.contextmanager
    def of(self, parts: int):
        self.parts = parts
        try:
            yield self
        finally:
            self.parts = 1


def batch_runs(batches, per_forward: Optional[int] = None, single: bool = False):
    """Which batches share a forward: lists of consecutive ``batches`` of equal shape, at most ``per_forward`` long
    (``single``: one).  Default: forwards of up to 64 samples, at most 4 batches -- ``max(1, min(4, 64 // N))``, fixed when
    the first batch shows its size N.  A run is yielded only once the batch after it has been pulled (or the input has
    ended): an iterable that enqueues each batch's host-to-device copy does so beside the previous run's forward."""
    limit = 1 if single else None if per_forward is None else max(1, int(per_forward))
    run = []
    for x in batches:
        if limit is None:
            limit = max(1, min(4, 64 // max(1, int(x.shape[0]))))
        if run and (x.shape != run[0].shape or len(run) == limit):
            yield run
            run = []
        run.append(x)
    if run:
        yield run


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _pool_window(node: torch.fx.Node, mods):
    """``(kernel, stride, padding)`` when ``node`` is an ``nn.MaxPool2d`` call that ``bn_act_maxpool`` computes exactly
    (floor mode, dilation 1, no indices, one stride and one padding for both axes); None otherwise."""
    if node.op != "call_module" or len(node.args) != 1 or node.kwargs:
        return None
    m = mods.get(node.target)
    if not isinstance(m, nn.MaxPool2d) or m.ceil_mode or m.return_indices or _pair(m.dilation) != (1, 1):
        return None
    kernel, stride, padding = _pair(m.kernel_size), _pair(m.stride if m.stride is not None else m.kernel_size), _pair(m.padding)
    if stride[0] != stride[1] or padding[0] != padding[1] or 2 * padding[0] > min(kernel):
        return None
    return kernel, stride[0], padding[0]


def _hardtanh_bounds(node: torch.fx.Node):
    """``(min_val, max_val)`` of an ``F.hardtanh`` / ``F.hardtanh_`` call as the graph states them (defaults -1, 1); anything
    that is not a constant stays what it is and equals no number."""
    rest = tuple(node.args[1:])
    return (rest[0] if rest else node.kwargs.get("min_val", -1.0), rest[1] if len(rest) > 1 else node.kwargs.get("max_val", 1.0))


def _is_const(v, want: float) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool) and v == want


def _is_relu(node: torch.fx.Node, mods) -> int:
    """Which activation of the fused epilogues ``node`` is, in place or not: ``hip_ops.ACT_RELU`` (``nn.ReLU``, ``F.relu``,
    ``torch.relu``, ``torch.relu_``, ``.relu()``, ``.relu_()``), ``hip_ops.ACT_RELU6`` (``nn.ReLU6``, ``nn.Hardtanh`` with bounds
    (0, 6), ``F.relu6``, ``F.hardtanh`` / ``F.hardtanh_`` with constant bounds 0 and 6), or ``hip_ops.ACT_NONE`` (0: anything
    else -- a Hardtanh with other bounds and a ``clamp`` call included -- stays an ordinary node)."""
    if node.op == "call_module":
        m = mods[node.target]
        if isinstance(m, nn.ReLU):
            return hip_ops.ACT_RELU
        if isinstance(m, nn.Hardtanh) and _is_const(m.min_val, 0) and _is_const(m.max_val, 6):      # nn.ReLU6 is one
            return hip_ops.ACT_RELU6
    elif node.op == "call_function":
        if node.target in (F.relu, torch.relu, torch.relu_):
            return hip_ops.ACT_RELU
        if node.target is F.relu6:
            return hip_ops.ACT_RELU6
        if node.target in (F.hardtanh, F.hardtanh_):
            lo, hi = _hardtanh_bounds(node)
            if _is_const(lo, 0) and _is_const(hi, 6):
                return hip_ops.ACT_RELU6
    elif node.op == "call_method" and node.target in ("relu", "relu_"):
        return hip_ops.ACT_RELU
    return hip_ops.ACT_NONE


def _act_arg(relu: Optional[torch.fx.Node], mods):
    """The ``relu`` operand a fused call carries for the chain's activation node: ``False`` without one, ``True`` for a ReLU (as
    ever), ``hip_ops.ACT_RELU6`` for a ReLU6."""
    if relu is None:
        return False
    code = int(_is_relu(relu, mods))
    return True if code == hip_ops.ACT_RELU else code


def _is_add(node: torch.fx.Node) -> bool:
    named = ((node.op == "call_function" and node.target in (operator.add, operator.iadd, torch.add))
             or (node.op == "call_method" and node.target in ("add", "add_")))
    return named and not node.kwargs and len(node.args) == 2 and all(isinstance(a, torch.fx.Node) for a in node.args)


def _foldable(bn: nn.Module) -> bool:
    return (isinstance(bn, nn.BatchNorm2d) and not bn.training and bn.running_mean is not None
            and bn.running_var is not None and bn.running_mean.dtype == torch.float32)


def _foldable_train(bn: nn.Module) -> bool:
    """A BatchNorm2d that normalises with the BATCH's statistics (train mode, or no running statistics at all): still
    one affine map per channel, computed per batch on the device (``hip_ops.bn_train_fold``)."""
    if not isinstance(bn, nn.BatchNorm2d) or not (bn.training or bn.running_mean is None):
        return False
    tensors = [t for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var) if t is not None]
    return all(t.dtype == torch.float32 for t in tensors)


def fold_bn(bn: nn.BatchNorm2d):
    """``(scale, shift)`` fp32 tensors with ``bn(x) == x * scale + shift`` in eval mode (computed in fp64)."""
    with torch.no_grad():
        var = bn.running_var.double()
        w = bn.weight.double() if bn.weight is not None else torch.ones_like(var)
        b = bn.bias.double() if bn.bias is not None else torch.zeros_like(var)
        scale64 = w / torch.sqrt(var + bn.eps)
        shift64 = b - bn.running_mean.double() * scale64
    return scale64.float().contiguous(), shift64.float().contiguous()


def _train_fold(bn: nn.BatchNorm2d, tag: str, state=None) -> Callable:
    """Graph callable of a train-mode BatchNorm: ``x -> (scale, shift)`` of THIS batch; the module's running statistics
    and batch counter move on exactly as in the module's own forward (``hip_ops.bn_train_fold``: one streaming pass).
    ``state`` (an object with ``parts``, or None), ``parts`` > 1: the tensor holds that many batches back to back, each folded on
    its own samples, in order, by the same launch (``[parts, C]`` maps)."""
    folder = hip_ops.BnTrainFold(bn)      # workspace / output vectors / addresses looked up once per input shape

    def fold(x):
        return folder(x, state.parts if state is not None else 1)

    fold.__name__ = fold.__qualname__ = "bn_train_fold_%s" % tag
    fold.train_fold_of = (bn, folder, state)      # read by the pass that pairs the fold with its convolution
    return fold


class HipConvBnStats:
    """Graph callable ``x -> (y, scale, shift)`` for an own convolution whose only consumers are ONE train-mode BatchNorm fold and
    that chain's ``bn_act`` / ``bn_act_pool``: ``hip_ops.ConvBnStats`` -- the convolution leaves its output's batch statistics from
    its epilogue, the running statistics and the counter move as in the module's forward, ``y`` is not read back for them.
    ``state.parts`` batches share the tensor, each folded on its own samples.  Taken apart again, call by call:

    * CPU tensors, autograd on, a shape over the kernels' per-call limits: the convolution MODULE, then the fold of its output;
    * batches of fewer than 128 pixels sharing a forward (a tile would touch more than two), or forward hooks on the convolution
      (they get ``y`` and may replace it before it is normalised): ``HipConv`` then ``BnTrainFold`` -- two launches.

    ``taken`` counts the calls per path ("fused" / "two_launch" / "module")."""

    def __init__(self, own: HipConv, bn: nn.BatchNorm2d, tag: str, state: Optional[BatchesPerForward] = None,
                 folder: Optional["hip_ops.BnTrainFold"] = None):
        self.own, self.bn, self.state = own, bn, state
        self.folder = folder if folder is not None else hip_ops.BnTrainFold(bn)
        self.fused = hip_ops.ConvBnStats(bn)
        self.taken = {"fused": 0, "two_launch": 0, "module": 0}
        self.__name__ = self.__qualname__ = "hip_conv_%s_bn_stats" % tag

    def _path(self, shape, parts: int) -> str:
        """Of a call the own kernels take (``_own_input``), by the input's shape: "fused", "two_launch", or "module" over the limits."""
        own, conv = self.own, self.own.conv
        N, _, H, W = shape
        Ho, Wo = (H + 2 * own.pad - own.k) // own.stride + 1, (W + 2 * own.pad - own.k) // own.stride + 1
        takes = hip_ops.conv2d_bn_stats_takes(N, conv.weight.shape[0], Ho, Wo, parts)
        if takes == "limits":
            return "module"
        return "two_launch" if takes == "straddle" or (own.fire_hooks and conv._forward_hooks) else "fused"

    def __call__(self, x):
        own, conv = self.own, self.own.conv
        parts = self.state.parts if self.state is not None else 1
        xc = _own_input(x, conv.weight)
        path = "module" if xc is None else self._path(xc.shape, parts)
        self.taken[path] += 1
        if path != "fused":
            y = conv(x) if path == "module" else own(x)
            return (y,) + tuple(self.folder(y, parts))
        return self.fused(xc, own.weight(), conv.bias, own.stride, own.pad, own.kpos, parts)


def _own_convs(graph: torch.fx.Graph, mods, conv: Optional[str], depthwise: bool = True) -> int:
    """Every Conv2d call that ``own_conv_ok`` -- or, with ``depthwise``, ``own_dwconv_ok`` -- takes becomes a ``HipConv`` call;
    returns how many."""
    swapped = 0
    for node in list(graph.nodes):
        mod = mods.get(node.target) if node.op == "call_module" else None
        if len(node.args) == 1 and not node.kwargs and (own_conv_ok(mod, conv) or (depthwise and own_dwconv_ok(mod))):
            with graph.inserting_before(node):
                own = graph.create_node("call_function", HipConv(mods[node.target], node.name), (node.args[0],), {}, name=node.name + "_hip")
            node.replace_all_uses_with(own)
            graph.erase_node(node)
            swapped += 1
    return swapped


def _conv_stats_pairs(graph: torch.fx.Graph, op: Callable, pool_op: Optional[Callable]) -> None:
    """``HipConv(x)`` consumed by one train-mode fold and by that fold's ``op`` / ``pool_op`` call, and by nothing else, becomes
    ONE ``HipConvBnStats`` call whose three results feed the activation pass."""
    for stats in list(graph.nodes):
        if not (stats.op == "call_function" and hasattr(stats.target, "train_fold_of") and isinstance(stats.args[0], torch.fx.Node)):
            continue
        src = stats.args[0]
        if not (src.op == "call_function" and type(src.target) is HipConv):
            continue
        maps = set(stats.users)                                     # the getitem nodes: scale, shift
        acts = [u for u in src.users if u is not stats]
        if not (len(acts) == 1 and acts[0].op == "call_function" and acts[0].target in (op, pool_op) and acts[0].args[0] is src
                and all(m.op == "call_function" and m.target is operator.getitem and set(m.users) == {acts[0]} for m in maps)
                and src not in acts[0].args[1:]):
            continue
        bn, folder, state = stats.target.train_fold_of
        tag = src.target.__name__[len("hip_conv_"):]
        with graph.inserting_before(src):
            both = graph.create_node("call_function", HipConvBnStats(src.target, bn, tag, state, folder), (src.args[0],), {},
                                     name=src.name + "_bn_stats")
            y = graph.create_node("call_function", operator.getitem, (both, 0), {}, name=src.name + "_y")
        for m in maps:                                              # (scale, shift) move one place up
            m.args = (both, m.args[1] + 1)
        acts[0].replace_input_with(src, y)
        graph.erase_node(stats)
        graph.erase_node(src)


def bn_chain(node: torch.fx.Node, mods, bare_add: bool, claimed: Optional[set] = None):
    """``(add, relu, residual)`` of the chain ``node -> [+ other] -> [ReLU / ReLU6]`` behind BatchNorm call ``node`` whose links have no
    other consumer (None where absent); ``x + x`` is no residual add.  ``bare_add``: an add that no sole ReLU follows is taken too
    (else the BatchNorm stands alone).  ``claimed``: the adds taken so far -- none is taken twice, the one taken here joins them."""
    users = list(node.users)
    if len(users) != 1:
        return None, None, None
    if _is_relu(users[0], mods):
        return None, users[0], None
    add = users[0]
    if not _is_add(add) or add.args[0] is add.args[1] or (claimed is not None and add in claimed):
        return None, None, None
    after = list(add.users)
    relu = after[0] if len(after) == 1 and _is_relu(after[0], mods) else None
    if relu is None and not bare_add:
        return None, None, None
    if claimed is not None:
        claimed.add(add)
    return add, relu, add.args[1] if add.args[0] is node else add.args[0]


def _fold_chains(graph: torch.fx.Graph, mods, op: Callable, pool_op: Optional[Callable], train_stats: bool,
                 state: BatchesPerForward, constants: dict) -> int:
    """Every foldable BatchNorm2d call with its chain (``bn_chain``; an add only before a sole ReLU; a max pooling behind
    BN -> ReLU for ``pool_op``) becomes one ``op`` / ``pool_op`` call; eval-mode maps go to ``constants``.  Returns how many."""
    folded = 0
    for node in list(graph.nodes):
        if node.op != "call_module" or len(node.args) != 1 or node.kwargs:
            continue
        bn = mods.get(node.target)
        per_batch = train_stats and _foldable_train(bn)
        if not (per_batch or _foldable(bn)):
            continue
        tag = node.name
        if not per_batch:
            constants["_pleas_scale_%s" % tag], constants["_pleas_shift_%s" % tag] = fold_bn(bn)
        add, relu, res = bn_chain(node, mods, bare_add=False)
        pool = next(iter(relu.users)) if pool_op is not None and relu is not None and res is None and len(relu.users) == 1 else None
        window = _pool_window(pool, mods) if pool is not None else None
        chain = [n for n in (node, add, relu, pool if window is not None else None) if n is not None]
        last = chain[-1]
        with graph.inserting_before(last):
            # explicit base names: fx would otherwise derive them from the targets character by character
            if per_batch:
                stats = graph.create_node("call_function", _train_fold(bn, tag, state), (node.args[0],), {}, name="bn_stats")
                s = graph.create_node("call_function", operator.getitem, (stats, 0), {}, name="bn_scale")
                t = graph.create_node("call_function", operator.getitem, (stats, 1), {}, name="bn_shift")
            else:
                s = graph.create_node("get_attr", "_pleas_scale_%s" % tag, (), {}, name="bn_scale")
                t = graph.create_node("get_attr", "_pleas_shift_%s" % tag, (), {}, name="bn_shift")
            if window is not None:
                fused = graph.create_node("call_function", pool_op, (node.args[0], s, t) + window + (_act_arg(relu, mods),), {}, name="bn_act_pool")
            else:
                fused = graph.create_node("call_function", op, (node.args[0], s, t, res, _act_arg(relu, mods)), {}, name="bn_act")
        last.replace_all_uses_with(fused)
        for dead in reversed(chain):
            graph.erase_node(dead)
        folded += 1
    return folded


def _conv_chain_pairs(graph: torch.fx.Graph, op: Callable) -> None:
    """An own convolution consumed by one eval-mode chain only (constants, not per-batch statistics): ONE ``HipConvBnAct`` call."""
    for node in list(graph.nodes):
        if not (node.op == "call_function" and node.target is op and isinstance(node.args[0], torch.fx.Node)):
            continue
        src, s = node.args[0], node.args[1]
        if not (src.op == "call_function" and isinstance(src.target, HipConv) and len(src.users) == 1
                and isinstance(s, torch.fx.Node) and s.op == "get_attr"):
            continue
        with graph.inserting_before(node):
            both = graph.create_node("call_function", HipConvBnAct(src.target), (src.args[0],) + tuple(node.args[1:]), {},
                                     name=src.name + "_bn_act")
        node.replace_all_uses_with(both)
        graph.erase_node(node)
        graph.erase_node(src)


def _graph_module(model: nn.Module, graph: torch.fx.Graph, mods, constants: dict, state: BatchesPerForward) -> torch.fx.GraphModule:
    """Attributes: every submodule the graph calls (the SAME objects: hooks keep firing), what else it reads, the constants."""
    graph.lint()
    root = dict(constants)
    for node in graph.nodes:
        if node.op == "call_module":
            root[node.target] = mods[node.target]
        elif node.op == "get_attr" and node.target not in root:
            obj = model
            for part in node.target.split("."):
                obj = getattr(obj, part)
            root[node.target] = obj
    gm = torch.fx.GraphModule(root, graph, class_name=type(model).__name__)
    gm.train(model.training)
    gm.batches_per_forward = state      # reset_bn_stats: `with gm.batches_per_forward.of(k):` around a k-batch forward
    # does every normalisation layer with batch statistics go through a per-batch fold?  (only then may batches share a forward)
    gm.all_batch_statistics_folded = not uses_batch_statistics(gm)
    return gm


def fuse_bn_act(model: nn.Module, op: Callable = _bn_act, train_stats: bool = False,
                pool_op: Optional[Callable] = None, conv: Optional[str] = None,
                inference: bool = False, train_convs: bool = False) -> Optional[torch.fx.GraphModule]:
    """fx copy of ``model`` (sharing its submodules) with every eval-mode BatchNorm2d chain replaced by
    ``op(x, scale, shift, residual_or_None, relu)`` -- the HIP kernel ``hip_ops.bn_act`` unless a test
    passes its own; ``relu`` is ``False``, ``True`` (a ReLU) or ``hip_ops.ACT_RELU6``.  Returns None when the model cannot be traced or holds nothing to fold; the caller
    then runs the model as it is (vendor kernels).

    ``train_stats=True``: BatchNorm2d modules that normalise with the BATCH's statistics (train mode -- the BN-reset pass
    after merging, run_domainnet.py:327-341) are folded as well: ``scale, shift = bn_train_fold(bn, x)`` per batch,
    then the same single ``op`` pass -- x is read twice and written once, where the vendor's train-mode BatchNorm + add +
    ReLU read or write it seven times.

    ``pool_op(x, scale, shift, kernel, stride, padding, relu)`` takes a BN -> ReLU chain whose only consumer is a max
    pooling (``hip_ops.bn_act_maxpool`` with the default ``op``; with a caller's ``op`` only when passed too).

    ``conv`` ("kxk" / "all" / "vendor", default ``SOURCE_CONV``): which Conv2d calls become ``HipConv`` calls -- only with
    the default ``op`` (a test's CPU ``op`` keeps the modules) and, unless ``train_convs`` asks for it, never for a model in train mode (autograd may be on).

    ``inference=True`` (default ``op``, model in eval mode): the graph of a forward that nobody taps -- every ``HipConvBnAct``
    becomes the image-only ``HipConvAct`` (a convolution that carries hooks when it is called still hands them its output),
    ``AdaptiveAvgPool2d((1, 1))`` -> ``flatten(1)`` becomes one ``PoolGather``, an ``nn.Linear`` on its result the own
    ``HipLinear``, and ``nn.Identity`` calls are dropped.  The stem and whatever is not recognised stay as in the default graph.

    ``train_convs=True`` (default ``op``, model in TRAIN mode, with ``train_stats``; an explicit opt-in -- the BN-statistics reset
    with ``backbone="hip"``): the Conv2d calls of a train-mode graph become ``HipConv`` calls too -- ``HipConv`` declines under
    autograd call by call -- and a convolution consumed by one train-mode fold and that chain's activation pass alone becomes ONE
    ``HipConvBnStats`` call.  Without it the function builds the graph it always built."""
    if pool_op is None and op is _bn_act:
        pool_op = _bn_act_pool
    try:
        graph = torch.fx.Tracer().trace(model)      # the graph alone: one code generation at the end, not two
    except Exception:  # noqa: BLE001 -- untraceable control flow: nothing to rewrite
        return None
    mods = dict(model.named_modules())
    constants = {}                                    # get_attr targets of the folded scale / shift vectors
    state = BatchesPerForward()                       # train_stats: batches per forwarded tensor, set by the caller
    folded = _fold_chains(graph, mods, op, pool_op, train_stats, state, constants)
    if op is _bn_act and (train_convs or not model.training):
        # a train-mode graph (the BN-statistics reset) keeps depthwise layers on the module: no statistics epilogue for them
        folded += _own_convs(graph, mods, conv, depthwise=not model.training)
        if model.training and train_stats:
            _conv_stats_pairs(graph, op, pool_op)
        if not model.training and SOURCE_CONV_BN == "1":
            _conv_chain_pairs(graph, op)
        if not model.training and inference:
            _inference_passes(graph, mods)
    return _graph_module(model, graph, mods, constants, state) if folded else None


def uses_batch_statistics(gm) -> bool:
    """Does ``gm``'s graph still CALL something that normalises with the statistics of the batch it is given -- a BatchNorm /
    InstanceNorm module in train mode (or without running statistics), a functional ``batch_norm`` / ``instance_norm`` with
    ``training`` / ``use_input_stats`` not provably off, or a module outside ``torch.nn`` that has such a submodule?
    Several batches may share a forward only when the answer is no (the fused chains fold train-mode BatchNorm per batch)."""
    norm = (nn.modules.batchnorm._BatchNorm, nn.modules.instancenorm._InstanceNorm)
    stat = lambda m: isinstance(m, norm) and (m.training or getattr(m, "running_mean", None) is None)
    for n in gm.graph.nodes:
        if n.op == "call_module":
            m = gm.get_submodule(n.target)
            if stat(m) or any(stat(c) for c in m.modules()):
                return True
        elif n.op == "call_function" and n.target in (F.batch_norm, torch.batch_norm):
            training = n.kwargs.get("training", n.args[5] if len(n.args) > 5 else False)
            if training is not False:
                return True
        elif n.op == "call_function" and n.target in (F.instance_norm, torch.instance_norm):
            use_input = n.kwargs.get("use_input_stats", n.args[5] if len(n.args) > 5 else True)
            if use_input is not False:
                return True
    return False


class InferenceBackbone:
    """A frozen model as its inference graph (``fuse_bn_act(model, inference=True)``), called under ``no_grad``.  The folded
    BatchNorm constants and the kernel-position-major weight copies are taken when the graph is built: after
    ``reset_bn_stats``, ``load_state_dict`` or ``.data`` edits call ``refresh()``.  The model is put in eval mode (the graph is
    an evaluation forward).  A model that cannot be traced runs as its modules."""

    def __init__(self, model: nn.Module, conv: Optional[str] = None):
        self.model, self.conv = model, conv
        self.refresh()

    def refresh(self) -> "InferenceBackbone":
        self.model.eval()
        self.graph = fuse_bn_act(self.model, conv=self.conv, inference=True)
        self._head = None
        if self.graph is not None:
            heads = [n for n in self.graph.graph.nodes if n.op == "call_function" and isinstance(n.target, PoolGather)]
            out = next(n for n in self.graph.graph.nodes if n.op == "output")
            # the pooled features ARE the result (a backbone whose fc is Identity): a channel map may ride in the pooling pass
            if len(heads) == 1 and out.args[0] is heads[0]:
                self._head = heads[0].target
        return self

    def gather_features(self, src: Optional[torch.Tensor]) -> bool:
        """Let the graph's pooling pass emit channels ``src`` (a ``hip_ops.channel_map``; None: all, in order).  False when
        the graph does not end in its pooling pass -- the caller then gathers the result itself."""
        if self._head is None:
            return False
        self._head.src = src
        return True

    @torch.no_grad()
    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        return (self.graph if self.graph is not None else self.model)(x)
