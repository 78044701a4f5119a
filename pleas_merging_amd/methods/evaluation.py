"""Evaluation helpers for merged models with separate heads: the first consumers of
the block layout ``[merged | separate-of-model-1 | separate-of-model-2]`` that ``partial_merge`` gives every axis.

Reference: pleas/methods/pleas_merging.py:408-496 (``get_fc_perm``, ``permute_final_features``, ``eval_perm_model``)
and :575-586 (``eval_whole_model``).  Accuracy is counted directly (torchmetrics is not a dependency here).

``backbone="modules"`` (default) is ``model(x)`` on the vendor's modules, as the reference runs it.  ``backbone="hip"`` runs the
model as its inference graph on the library's own kernels (``source_forward.InferenceBackbone``: image-only convolutions with
the BatchNorm / add / ReLU chain in their epilogue, one ``pool_gather`` for pooling + ``permute_final_features``, the head as an
own Linear) and counts with ``hip_ops.top1_count`` into one device counter read back once after the loop; host batches are
copied on the current stream without blocking the host.  It needs the model on the GPU (``PleasHipError`` otherwise) and a forward that no
hook has to observe bit-for-bit in the vendor's arithmetic; hooks on convolutions still receive their outputs.

``train_eval_linear_probe`` also takes ``head="hip"`` (default ``"autograd"``): the probe's head trained on the library's kernels
without a read-back per step (methods/linear_probe.py), and ``cache_features=True``: the frozen backbone run once instead of
once per epoch.
"""
from __future__ import annotations

from typing import Iterable

import torch
from torch import nn

from .. import hip_ops
from ..core.utils import Axis, Permutation, PermutationSpec
from .partial_matching import get_blocks
from .linear_probe import HipProbeHead, cosine_lrs_eta_min
from .source_forward import HipLinear, InferenceBackbone

BACKBONES = ("modules", "hip")
HEADS = ("autograd", "hip")


def get_fc_perm(perm: Permutation, spec: PermutationSpec, costs, budget_ratios):
    """Blocks ``(merged idx 1, merged idx 2, separate idx 1, separate idx 2)`` of the group that feeds the classifier
    (the one whose state holds ``fc.weight:1``).  Reference :408-433."""
    blocks = get_blocks(spec, perm, costs, budget_ratios, False)
    for key, group in spec.items():
        if Axis("fc.weight", 1) in group.state:
            return blocks[key]
    raise ValueError("No fc perm found")


def permute_final_features(features: torch.Tensor, fc_perm, idx: int) -> torch.Tensor:
    """Backbone features of the merged model ``[N, n_merged + 2 n_separate]`` -> the feature order source model
    ``idx`` (0 or 1) was trained with, so that its own classifier applies.  Reference :436-466."""
    b1, b2, b1c, b2c = fc_perm
    ni, mi = len(b1), len(b1c)
    merged = features[:, :ni]
    if idx == 0:
        own, order = features[:, ni:ni + mi], torch.cat([b1, b1c], 0)
    else:
        own, order = features[:, ni + mi:ni + 2 * mi], torch.cat([b2, b2c], 0)
    return torch.cat([merged, own], 1)[:, torch.argsort(order).to(features.device)]


def final_feature_map(fc_perm, idx: int) -> torch.Tensor:
    """``permute_final_features`` as ONE gather: the int64 CPU vector ``src`` with
    ``permute_final_features(f, fc_perm, idx) == f[:, src]`` for every feature matrix ``f`` of the merged backbone."""
    b1, b2, b1c, b2c = (b.cpu() for b in fc_perm)
    ni, mi = len(b1), len(b1c)
    own = torch.arange(ni, ni + mi) + (0 if idx == 0 else mi)           # where the [merged | own] columns sit in f
    order = torch.cat([b1, b1c], 0) if idx == 0 else torch.cat([b2, b2c], 0)
    return torch.cat([torch.arange(ni), own], 0)[torch.argsort(order)]


def _hip_backbone(model: nn.Module, backbone: str):
    """``(device, InferenceBackbone or None)`` for the ``backbone`` keyword of the helpers."""
    if backbone not in BACKBONES:
        raise ValueError("backbone must be one of %r, got %r" % (BACKBONES, backbone))
    device = next(iter(model.parameters())).device
    if backbone == "modules":
        return device, None
    if device.type != "cuda":
        raise hip_ops.PleasHipError('backbone="hip" needs the model on the GPU (got %s); no CPU fallback' % device)
    return device, InferenceBackbone(model)


def _device_batches(dataloader: Iterable, device: torch.device):
    """``(x, y)`` on ``device``, copied on the CURRENT stream without blocking the host (``non_blocking``: asynchronous for
    pinned host tensors, in stream order with the kernels that read them)."""
    move = lambda t: t.to(device, non_blocking=True) if isinstance(t, torch.Tensor) else t
    for x, y in dataloader:
        yield move(x), move(y)


def _labels(y: torch.Tensor) -> torch.Tensor:
    return y.reshape(-1).to(torch.int64).contiguous()


@torch.no_grad()
def eval_perm_model(model: nn.Module, fc: nn.Module, dataloader: Iterable, num_classes: int, fc_perm, idx: int,
                    backbone: str = "modules") -> torch.Tensor:
    """Top-1 accuracy of the merged backbone under the classifier of source model ``idx``.  Reference :469-496
    (``num_classes`` is kept for the signature; the count does not need it)."""
    device, hip = _hip_backbone(model, backbone)
    model.eval()
    if hip is not None:
        src = final_feature_map(fc_perm, idx)
        head = HipLinear(fc, "fc") if type(fc) is nn.Linear else fc
        # the merged backbone emits [merged | separate-1 | separate-2]; the map is checked against that width on the host, once
        smap = hip_ops.channel_map(src, len(fc_perm[0]) + 2 * len(fc_perm[2]), device)
        in_graph = hip.gather_features(smap)      # else: a graph that does not end in its pooling pass -- gathered below
        hit = torch.zeros(1, dtype=torch.long, device=device)
        seen = 0
        for x, y in _device_batches(dataloader, device):
            feats = hip(x)
            if not in_graph:
                feats = hip_ops.pool_gather(feats.reshape(feats.shape[0], -1, 1), smap)
            hip_ops.top1_count(head(feats).contiguous(), _labels(y), hit)
            seen += int(y.numel())
        return hit[0].float() / max(seen, 1)
    hit = torch.zeros((), dtype=torch.long, device=device)
    seen = 0
    for x, y in dataloader:
        x, y = x.to(device), y.to(device)
        logits = fc(permute_final_features(model(x), fc_perm, idx))
        hit += (logits.argmax(1) == y).sum()
        seen += int(y.numel())
    return hit.float() / max(seen, 1)


@torch.no_grad()
def eval_whole_model(model: nn.Module, dataloader: Iterable, num_classes: int, backbone: str = "modules") -> torch.Tensor:
    """Top-1 accuracy of a model with its own head.  Reference :575-586."""
    device, hip = _hip_backbone(model, backbone)
    model.eval()
    hit, seen = 0, 0
    if hip is not None:
        hits = torch.zeros(1, dtype=torch.long, device=device)
        for x, y in _device_batches(dataloader, device):
            hip_ops.top1_count(hip(x).contiguous(), _labels(y), hits)
            seen += int(y.numel())
        acc = torch.tensor(int(hits[0]) / max(seen, 1))       # the loop's one read-back
        print(acc)
        return acc
    for x, y in dataloader:
        pred = model(x.to(device)).argmax(1).cpu()
        hit += int((pred == y.cpu()).sum())
        seen += int(y.numel())
    acc = torch.tensor(hit / max(seen, 1))
    print(acc)
    return acc


def _probe_batches(features, dataloader, device: torch.device, non_blocking: bool = False):
    """``(features(x), y)`` per batch of ``dataloader`` on ``device``, the frozen backbone under ``no_grad``."""
    for x, y in dataloader:
        x, y = x.to(device, non_blocking=non_blocking), y.to(device, non_blocking=non_blocking)
        with torch.no_grad():
            feats = features(x)
        yield feats, y


def _recorded(batches, store: list):
    for item in batches:
        store.append(item)
        yield item


def train_eval_linear_probe(model: nn.Module, train_dataloader, test_dataloader, num_classes: int, wandb_run, dataset_name: str,
                            lr: float = 1e-3, epochs: int = 10, device=None, backbone: str = "modules", head: str = "autograd",
                            cache_features: bool = False) -> nn.Module:
    """Linear probe on a frozen (merged) backbone, as the different-label-space driver evaluates merged models
    (reference :499-570; run_torchvision.py:276-290).  Same recipe: Adam(``lr``) on a fresh ``Linear`` head, cosine
    schedule over ``epochs * len(train_dataloader)`` steps down to ``lr / 10``, cross entropy, backbone in eval mode
    under ``no_grad``; per-epoch train accuracy / loss and the final test accuracy go to ``wandb_run.log`` under the
    reference's keys (``wandb_run=None`` skips logging).  Returns the trained head.  The backbone stays where it is
    (``device`` defaults to its device) -- the reference hard-codes ``.cuda()`` and a 224x224 probe input; here the
    feature width is read from the first training batch.  ``backbone="hip"`` moves the frozen backbone's forwards to the
    library's kernels.

    ``head="autograd"`` (default) trains the head as the reference does: ``nn.Linear``, ``CrossEntropyLoss``, ``torch.optim.Adam``
    and ``CosineAnnealingLR`` on autograd, one ``float(loss)`` read-back per step.  ``head="hip"`` trains the same head by the
    same recipe on the library's kernels (``linear_probe.HipProbeHead``: own Linear forward, ``softmax_xent``, one grouped weight
    gradient, ``channel_sum``, one ``masked_adam``; the test accuracy by ``top1_count``): five launches per step, ONE read-back per
    epoch and one for the test loop; batches are copied without blocking the host.  It needs the model on the GPU
    (``PleasHipError`` otherwise, no CPU fallback), works with either ``backbone`` and returns an ``nn.Linear`` as well.

    ``cache_features=True`` (either head) runs the backbone ONCE over the training loader, during epoch 0, and keeps every
    feature and label batch on the device (``N_total * D * 4`` bytes); epochs 1, 2, ... replay epoch 0's batches in epoch 0's
    order.  THIS CHANGES THE RECIPE: a loader that reshuffles or augments per epoch no longer does so after epoch 0, the head
    sees the same batches in the same order every epoch.  It is therefore opt-in; with a deterministic, unshuffled loader the
    result is the one of ``cache_features=False``."""
    if head not in HEADS:
        raise ValueError("head must be one of %r, got %r" % (HEADS, head))
    own_device, hip = _hip_backbone(model, backbone)
    if device is None:
        device = own_device
    device = torch.device(device)
    if head == "hip" and (own_device.type != "cuda" or device.type != "cuda"):
        raise hip_ops.PleasHipError('head="hip" needs the model on the GPU (got %s); no CPU fallback' % own_device)
    model.eval()
    features = hip if hip is not None else model
    n_batches = len(train_dataloader)
    log = wandb_run.log if wandb_run is not None else (lambda _metrics: None)
    cached = [] if cache_features else None

    def train_batches(epoch: int):
        if cached is not None and epoch > 0:
            return cached
        batches = _probe_batches(features, train_dataloader, device, non_blocking=head == "hip")
        return batches if cached is None else _recorded(batches, cached)

    if head == "hip":
        return _hip_probe(features, train_batches, test_dataloader, num_classes, log, dataset_name, lr, epochs, device, n_batches)
    fc = opt = sched = None
    loss_fn = nn.CrossEntropyLoss()
    for epoch in range(epochs):
        hit = torch.zeros((), dtype=torch.long, device=device)
        seen, total, loss = 0, 0.0, None
        for feats, y in train_batches(epoch):
            if fc is None:
                fc = nn.Linear(feats.shape[-1], num_classes).to(device)
                opt = torch.optim.Adam(fc.parameters(), lr=lr)
                sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, epochs * n_batches, eta_min=lr / 10)
            fc.train()
            logits = fc(feats)
            loss = loss_fn(logits, y)
            opt.zero_grad()
            loss.backward()
            opt.step()
            sched.step()
            hit += (logits.argmax(1) == y).sum()
            seen += int(y.numel())
            total += float(loss)
        log({"%s_linear_probe_train_acc" % dataset_name: float(hit) / max(seen, 1),
             "%s_linear_probe_train_loss" % dataset_name: float(loss) if loss is not None else float("nan"),
             "epoch": epoch, "%s_total_loss" % dataset_name: total / max(n_batches, 1)})
    if fc is None:
        raise ValueError("train_eval_linear_probe: empty training loader")
    fc.eval()
    hit, seen = torch.zeros((), dtype=torch.long, device=device), 0
    with torch.no_grad():
        for feats, y in _probe_batches(features, test_dataloader, device):
            hit += (fc(feats).argmax(1) == y).sum()
            seen += int(y.numel())
    log({"%s_linear_probe_acc" % dataset_name: float(hit) / max(seen, 1)})
    return fc


def _hip_probe(features, train_batches, test_dataloader, num_classes: int, log, dataset_name: str, lr: float, epochs: int,
               device: torch.device, n_batches: int) -> nn.Linear:
    """``train_eval_linear_probe`` with ``head="hip"``: the same loop, every step enqueued without a read-back."""
    lrs = cosine_lrs_eta_min(lr, lr / 10, max(epochs * n_batches, 1), epochs * n_batches)
    probe, t = None, 0
    for epoch in range(epochs):
        seen = 0
        for feats, y in train_batches(epoch):
            if probe is None:
                probe = HipProbeHead(nn.Linear(feats.shape[-1], num_classes).to(device))
            if t >= len(lrs):
                raise ValueError("train_eval_linear_probe: the training loader yields more batches than its len() = %d" % n_batches)
            probe.step(feats, _labels(y), lrs[t], t + 1)
            t += 1
            seen += int(y.numel())
        if probe is None:
            break
        hits, _bad, total, last = probe.epoch_readback()      # the epoch's one read-back
        log({"%s_linear_probe_train_acc" % dataset_name: hits / max(seen, 1),
             "%s_linear_probe_train_loss" % dataset_name: last if seen else float("nan"),
             "epoch": epoch, "%s_total_loss" % dataset_name: total / max(n_batches, 1)})
    if probe is None:
        raise ValueError("train_eval_linear_probe: empty training loader")
    seen = 0
    for feats, y in _probe_batches(features, test_dataloader, device, non_blocking=True):
        hip_ops.top1_count(probe.logits(feats), _labels(y), probe.counts[:1])
        seen += int(y.numel())
    hits = probe.epoch_readback()[0]                          # the test loop's one read-back
    log({"%s_linear_probe_acc" % dataset_name: hits / max(seen, 1)})
    return probe.finish()
