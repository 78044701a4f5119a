"""The linear probe's head on the library's own kernels (``head="hip"`` of ``evaluation.train_eval_linear_probe``).

Reference: pleas/methods/pleas_merging.py:499-570 trains a fresh ``nn.Linear`` on frozen features with Adam, a cosine schedule
and cross entropy on autograd: about fifteen small launches per step and one ``float(loss)`` read-back.  Here one step is five
launches of kernels the library owns -- the head's forward (``hip_ops.linear``: ``conv2d`` with H = W = 1, or the split-K GEMM
under ``hip_ops.linear_form("gemm")``, which adds a slab-reduce launch), ``hip_ops.softmax_xent`` (loss, ``dlogits`` and the hit
count from one pass), one ``WgradBatch`` with the single Linear layer, ``channel_sum`` (``column_sum`` under "gemm") for the bias
gradient and one ``masked_adam`` over the whole parameter arena -- and nothing is read back before the epoch ends.
"""
from __future__ import annotations

import math
from typing import List, Tuple

import torch
from torch import nn

from .. import hip_ops


def cosine_lrs_eta_min(base_lr: float, eta_min: float, t_max: int, n: int) -> List[float]:
    """Learning rate used by update 0..n-1 under ``CosineAnnealingLR(T_max=t_max, eta_min=eta_min)`` stepped once per update,
    evaluated with torch's recursive form so the doubles match the reference's scheduler (:525, :547).  ``cosine_lrs`` of pleas_merging.py is the ``eta_min = 0`` schedule of the PLeaS fit."""
    lrs, lr = [], base_lr
    for t in range(n):
        if t > 0:
            if (t - 1 - t_max) % (2 * t_max) == 0:
                lr = lr + (base_lr - eta_min) * (1 - math.cos(math.pi / t_max)) / 2
            else:
                lr = (1 + math.cos(math.pi * t / t_max)) / (1 + math.cos(math.pi * (t - 1) / t_max)) * (lr - eta_min) + eta_min
        lrs.append(lr)
    return lrs


class HipProbeHead:
    """A Linear head trained by Adam on mean cross entropy, on the current stream, without read-backs.

    ``fc``: a freshly constructed ``nn.Linear`` on the GPU (built exactly as the autograd path builds it, so the same seed gives
    the same initial head).  ``[W | b]``, their gradients and Adam's two moments live in flat fp32 arenas, every tensor 16-byte
    aligned, so the update of the whole head is ONE ``masked_adam`` launch.  The epoch's counters -- hits, bad labels, the
    running and the last loss -- share one 24-byte device buffer: ``epoch_readback`` is one copy."""

    def __init__(self, fc: nn.Linear):
        w = fc.weight
        if type(fc) is not nn.Linear or not w.is_cuda or w.dtype != torch.float32:
            raise hip_ops.PleasHipError("HipProbeHead needs an fp32 nn.Linear on the GPU (got %s on %s); no CPU fallback"
                                        % (type(fc).__name__, w.device))
        self.fc = fc
        self.device = dev = w.device
        C, D = w.shape
        self.C, self.D = C, D
        off_b = (C * D + 3) // 4 * 4                      # the bias starts 16-byte aligned inside the arenas
        size = off_b + ((C + 3) // 4 * 4 if fc.bias is not None else 0)
        self.p, self.g, self.m, self.v = (torch.zeros(size, dtype=torch.float32, device=dev) for _ in range(4))
        self.w, self.gw = self.p[:C * D].view(C, D), self.g[:C * D].view(C, D)
        self.b = self.gb = None
        if fc.bias is not None:
            self.b, self.gb = self.p[off_b:off_b + C], self.g[off_b:off_b + C]
            self.b.copy_(fc.bias.detach())
        self.w.copy_(w.detach())
        state = torch.zeros(3, dtype=torch.int64, device=dev)
        self._state = state
        self.counts = state[:2]                           # hits, labels outside [0, C)
        self.loss = state[2:].view(torch.float32)         # the last step's loss, the sum since the last read-back
        self.readbacks = 0
        self._shapes = {}                                 # N -> (logits, dlogits, row_loss, WgradBatch): a ragged batch is one more

    def _features(self, feats: torch.Tensor) -> torch.Tensor:
        if not feats.is_cuda or feats.dtype != torch.float32 or feats.dim() != 2 or feats.shape[1] != self.D:
            raise hip_ops.PleasHipError("HipProbeHead: fp32 [N, %d] features on the GPU expected, got %s %s on %s"
                                        % (self.D, feats.dtype, tuple(feats.shape), feats.device))
        if feats.is_contiguous() and feats.data_ptr() % 16 == 0:
            return feats
        return feats.clone(memory_format=torch.contiguous_format)

    def _forward(self, feats: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        return hip_ops.linear(feats, self.w, self.b, out=out)

    def logits(self, feats: torch.Tensor) -> torch.Tensor:
        """``feats @ W.T + b`` as a fresh [N, C] tensor (the test loop: ``top1_count(head.logits(f), y, head.counts[:1])``)."""
        feats = self._features(feats)
        return self._forward(feats, torch.empty((feats.shape[0], self.C), dtype=torch.float32, device=self.device))

    def step(self, feats: torch.Tensor, labels: torch.Tensor, lr: float, t: int) -> None:
        """Adam update number ``t`` (1, 2, ...) at learning rate ``lr`` on the batch's mean cross entropy; the batch's hits and loss
        join the epoch's counters on the device."""
        feats = self._features(feats)
        N = feats.shape[0]
        if N == 0:
            return
        bufs = self._shapes.get(N)
        if bufs is None:
            new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.device)
            bufs = self._shapes[N] = (new(N, self.C), new(N, self.C), new(N), hip_ops.WgradBatch(self.device))
        logits, dlogits, row_loss, wgrad = bufs
        self._forward(feats, logits)
        hip_ops.softmax_xent(logits, labels, 1.0 / N, dlogits, row_loss, self.loss, self.counts)
        wgrad.add(dlogits, feats, self.gw)
        wgrad.flush()
        if self.gb is not None:
            (hip_ops.column_sum if hip_ops.LINEAR == "gemm" else hip_ops.channel_sum)(dlogits, self.gb)
        hip_ops.masked_adam(self.p, self.g, None, self.m, self.v, lr, t)

    def epoch_readback(self) -> Tuple[int, int, float, float]:
        """``(hits, bad labels, sum of the losses, last loss)`` since the previous call, from ONE device-to-host copy; the
        counters start again from zero.  A label outside ``[0, C)`` raises."""
        host = self._state.cpu()
        self.readbacks += 1
        self._state.zero_()
        hits, bad = int(host[0]), int(host[1])
        last, total = (float(v) for v in host[2:].view(torch.float32))
        if bad:
            raise hip_ops.PleasHipError("linear probe: %d label(s) outside [0, %d)" % (bad, self.C))
        return hits, bad, total, last

    def finish(self) -> nn.Linear:
        """The trained parameters back in the ``nn.Linear`` this head was made from, which is returned."""
        with torch.no_grad():
            self.fc.weight.copy_(self.w)
            if self.b is not None:
                self.fc.bias.copy_(self.b)
        return self.fc
