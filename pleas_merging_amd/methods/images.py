"""uint8 image batches as a ``dataloader`` of the entry points: ``DeviceImages`` wraps a loader whose batches hold uint8 images
and yields what ``activation_matching``, ``train``, ``reset_bn_stats``, ``eval_*`` and ``train_eval_linear_probe`` take -- fp32
``[N, C, Ho, Wo]`` on the GPU -- with the normalisation, the crop and the flip done by ``hip_ops.image_batch``.

The reference's drivers run ``ToTensor`` / ``Normalize`` (and, for training data, ``RandomCrop`` / ``RandomHorizontalFlip``) per
image on CPU workers and ship fp32 (pleas/methods/activation_matching.py:121, pleas/methods/pleas_merging.py:266 move the result
with ``x.cuda()``): 12 bytes per pixel over PCIe.  Here the loader only decodes: uint8 travels (3 bytes per pixel), the table of
``hip_ops.image_table`` fixes the arithmetic, and the augmentation PARAMETERS are drawn on the host from a seeded generator, so
they do not depend on timing.
"""
from __future__ import annotations

from collections import deque
from typing import Optional, Tuple

import torch

from .. import hip_ops

_MIX = 1000003      # (seed, epoch, batch) -> one generator seed


class DeviceImages:
    """Iterable over ``loader`` that yields ``(x, *rest)``: ``x`` fp32 ``[N, C, Ho, Wo]`` on ``device``, the other items of each
    batch untouched.  ``len()`` is the loader's; every ``iter()`` walks the loader again (and starts a new epoch of draws).

    Per batch, by what the loader yields first:
      uint8 on the host    copied into one of ``depth`` pinned staging buffers the wrapper owns (a batch that is already pinned
                           is used where it lies), sent on the "h2d" copy stream (``hip_ops.h2d_start`` / ``h2d_finish``),
                           converted by ``hip_ops.image_batch`` on the consumer's current stream; the copies of the next
                           ``depth - 1`` batches are started before the current one is yielded;
      uint8 on the device  converted where it lies, no copy;
      fp32, host or device through ``hip_ops.to_device_async`` unchanged (no crop, no flip): one wrapper serves mixed pipelines.

    ``layout``: ``"nhwc"`` (what decoders produce) or ``"nchw"`` uint8 batches.  ``mean`` / ``std``: ``hip_ops.image_table``'s.
    ``crop=(Ho, Wo)`` draws one origin per sample and ``flip=True`` one flag per sample (probability 1/2), both from a CPU
    ``torch.Generator`` seeded with ``(seed, epoch, batch index)``; the epoch counts ``iter()`` calls.  ``crop`` with
    ``flip=False`` and ``seed=None`` is the centre crop of evaluation (torchvision's rounding).  Staging memory: ``depth`` pinned
    buffers of the largest uint8 batch seen (16 x 224 x 224 x 3: 2.4 MB each), allocated on first use."""

    def __init__(self, loader, mean, std, device, layout: str = "nhwc", crop: Optional[Tuple[int, int]] = None,
                 flip: bool = False, seed: Optional[int] = 0, depth: int = 2):
        if layout not in hip_ops.IMAGE_LAYOUTS:
            raise ValueError("DeviceImages: layout must be one of %r, got %r" % (tuple(hip_ops.IMAGE_LAYOUTS), layout))
        if depth < 1:
            raise ValueError("DeviceImages: depth must be at least 1, got %r" % (depth,))
        if flip and seed is None:
            raise ValueError("DeviceImages: flip=True draws flags and needs a seed")
        self.loader, self.mean, self.std = loader, mean, std
        self.device = torch.device(device)
        self.layout, self.flip, self.seed, self.depth = layout, bool(flip), seed, int(depth)
        self.crop = None if crop is None else (int(crop[0]), int(crop[1]))
        self.epoch = 0                  # iter() calls so far
        self._tables = {}               # channels -> device table
        self._staging = [None] * self.depth      # [pinned uint8 buffer, event of the last copy out of it]

    def __len__(self) -> int:
        return len(self.loader)

    def augmentation(self, epoch: int, index: int, n: int, height: int, width: int):
        """``(origin, flip)`` of batch ``index`` of epoch ``epoch`` for ``n`` images of ``height`` x ``width``: int64 ``[n, 2]``
        ``(y0, x0)`` or None (no crop), uint8 ``[n]`` or None (no flip).  A pure function of ``(seed, epoch, index)`` and the sizes."""
        origin = flags = None
        if self.crop is not None:
            ho, wo = self.crop
            if ho > height or wo > width:
                raise ValueError("DeviceImages: crop %s does not fit %d x %d images" % (self.crop, height, width))
        if self.seed is None:
            if self.crop is not None:       # centre crop, rounded as torchvision's CenterCrop does
                origin = torch.tensor([[int(round((height - ho) / 2.0)), int(round((width - wo) / 2.0))]]).repeat(n, 1)
            return origin, None
        g = torch.Generator().manual_seed(((int(self.seed) * _MIX + int(epoch)) * _MIX + int(index)) % (1 << 63))
        if self.crop is not None:
            origin = torch.stack([torch.randint(0, height - ho + 1, (n,), generator=g),
                                  torch.randint(0, width - wo + 1, (n,), generator=g)], 1)
        if self.flip:
            flags = (torch.rand(n, generator=g) < 0.5).to(torch.uint8)
        return origin, flags

    def _table(self, channels: int) -> torch.Tensor:
        t = self._tables.get(channels)
        if t is None:
            t = self._tables[channels] = hip_ops.image_table(self.mean, self.std, channels).to(self.device)
        return t

    def _stage(self, slot: int, x: torch.Tensor) -> torch.Tensor:
        """``x`` (uint8, host) in pinned memory: itself when pinned, else a copy in staging buffer ``slot`` (whose entry then
        waits for the event of the copy that is about to read it)."""
        if x.is_pinned() and x.is_contiguous():
            return x
        entry = self._staging[slot]
        if entry is not None and entry[1]:
            entry[1].synchronize()      # the previous copy out of this buffer has left the host
        if entry is None or entry[0].numel() < x.numel():
            entry = self._staging[slot] = [torch.empty(max(x.numel(), 1), dtype=torch.uint8).pin_memory(), None]
        buf = entry[0][:x.numel()].view(x.shape)
        buf.copy_(x)
        entry[1] = False                # set to the copy's event by _start
        return buf

    def _start(self, index: int, batch):
        """Begin the host-to-device copy of a batch (uint8 host images only); returns the batch's pending state."""
        items = tuple(batch) if isinstance(batch, (tuple, list)) else (batch,)
        x = items[0]
        if torch.is_tensor(x) and x.dtype == torch.uint8 and not x.is_cuda:
            slot = index % self.depth
            d, ev = hip_ops.h2d_start(self._stage(slot, x), self.device)
            if self._staging[slot] is not None and self._staging[slot][1] is False:
                self._staging[slot][1] = ev
            return index, items, (d, ev)
        return index, items, None

    def _finish(self, epoch: int, pending):
        index, items, copy = pending
        x = items[0]
        if not torch.is_tensor(x) or x.dtype != torch.uint8:
            return (hip_ops.to_device_async(x, self.device),) + items[1:]
        u8 = hip_ops.h2d_finish(copy[0], copy[1], self.device) if copy is not None else x
        if u8.dim() != 4:
            raise hip_ops.PleasHipError("DeviceImages: uint8 batches must be 4-d (%s), got shape %s" % (self.layout, tuple(u8.shape)))
        h, w = (u8.shape[1], u8.shape[2]) if self.layout == "nhwc" else (u8.shape[2], u8.shape[3])
        channels = u8.shape[3] if self.layout == "nhwc" else u8.shape[1]
        origin, flags = self.augmentation(epoch, index, u8.shape[0], h, w)
        out = hip_ops.image_batch(u8.contiguous(), self._table(channels), origin=origin, flip=flags, size=self.crop, layout=self.layout)
        if copy is None and u8.is_cuda:
            u8.record_stream(torch.cuda.current_stream(self.device))      # the loader's buffer, read on the consumer's stream
        return (out,) + items[1:]

    def __iter__(self):
        epoch = self.epoch
        self.epoch += 1
        source = enumerate(self.loader)
        pending = deque()
        while True:
            while len(pending) < self.depth:
                nxt = next(source, None)
                if nxt is None:
                    break
                pending.append(self._start(*nxt))
            if not pending:
                return
            yield self._finish(epoch, pending.popleft())
