"""uint8 image batches as a ``dataloader`` of the entry points: ``DeviceImages`` wraps a loader whose batches hold uint8 images
and yields what ``activation_matching``, ``train``, ``reset_bn_stats``, ``eval_*`` and ``train_eval_linear_probe`` take -- fp32
``[N, C, Ho, Wo]`` on the GPU -- with the normalisation, the crop and the flip done by ``hip_ops.image_batch``.

The reference's drivers run ``ToTensor`` / ``Normalize`` (and, for training data, ``RandomCrop`` / ``RandomHorizontalFlip``) per
image on CPU workers and ship fp32 (pleas/methods/activation_matching.py:121, pleas/methods/pleas_merging.py:266 move the result
with ``x.cuda()``): 12 bytes per pixel over PCIe.  Here the loader only decodes: uint8 travels (3 bytes per pixel), the table of
``hip_ops.image_table`` fixes the arithmetic, and the augmentation PARAMETERS are drawn on the host from a seeded generator, so
they do not depend on timing.

Decoded images come in every size, and the drivers' loaders resample them per image on the CPU (``RandomResizedCrop(224)`` for
training, ``Resize(256)`` + ``CenterCrop(224)`` for evaluation: experiments/shared_label_space/run_domainnet.py:204-214).  With
``collate_fn=ragged_collate`` a loader hands the images over as a list of uint8 ``[H, W, C]`` tensors; ``DeviceImages`` packs
them, with the plan of ``hip_ops.image_resample``, into one staging buffer and resamples on the GPU in PIL's own integer
arithmetic, so the batch has the bits the CPU chain would have produced.  The datasets' shared train transform is a chain,
``Resize(256)`` -> ``RandomResizedCrop(224)`` (experiments/datasets/interface.py): ``pre_resize=`` with ``resized_crop=`` runs
both resamplings on the GPU through ``hip_ops.image_resample_chain``.
"""
from __future__ import annotations

import math
from collections import deque
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from .. import hip_ops

_MIX = 1000003      # (seed, epoch, batch) -> one generator seed


def _as_image(x) -> torch.Tensor:
    """One decoded image as a ``[H, W, C]`` tensor: tensors as they are, arrays and PIL images through numpy."""
    t = x if torch.is_tensor(x) else torch.from_numpy(np.array(x))
    return t.unsqueeze(-1) if t.dim() == 2 else t


def ragged_collate(samples):
    """``collate_fn`` of a loader whose images differ in size: the first item of every sample (a uint8 ``[H, W, C]`` or ``[H, W]``
    tensor, array or PIL image) stays a LIST, one tensor per sample; the other items are stacked as ``default_collate`` does.
    ``DeviceImages`` takes the result with ``resized_crop=`` or ``resize=`` + ``crop=``."""
    from torch.utils.data import default_collate

    if not isinstance(samples[0], (tuple, list)):
        return ([_as_image(x) for x in samples],)
    images = [_as_image(sample[0]) for sample in samples]
    return (images,) + tuple(default_collate([sample[k] for sample in samples]) for k in range(1, len(samples[0])))


def _pad16(v: int) -> int:
    return (v + 15) // 16 * 16


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
    buffers of the largest uint8 batch seen (16 x 224 x 224 x 3: 2.4 MB each), allocated on first use.

    Images of mixed sizes: a batch whose first item is a LIST of uint8 ``[H, W, C]`` host tensors (``ragged_collate``) is
    resampled to one size by ``hip_ops.image_resample`` -- bit for bit what PIL's ``BILINEAR`` gives -- under one of
      ``resized_crop=(Ho, Wo)``   torchvision's ``RandomResizedCrop``: per sample a box drawn by its ``get_params`` rule from
                           ``scale`` and ``ratio`` (ten attempts, then the centred box with the ratio clamped), resampled to
                           ``(Ho, Wo)``; needs a ``seed``.  Boxes are drawn sample after sample from the generator of
                           ``(seed, epoch, batch index)``, the flip flags after all boxes;
      ``resize=s`` + ``crop=(Ho, Wo)``   ``Resize(s)`` (shorter side to ``s``) then ``CenterCrop``: the window is the centre one
                           whatever ``seed`` is (the seed only feeds ``flip``); only the window is computed.
      ``pre_resize=s`` + ``resized_crop=(Ho, Wo)``   ``Resize(s)`` then ``RandomResizedCrop``, the train transform of most of the
                           reference's datasets (experiments/datasets/interface.py): two PIL resamplings with an 8-bit image
                           in between, by ``hip_ops.image_resample_chain``.  The box is drawn on the resized size ``(H1, W1)``
                           -- shorter side ``s``, longer ``int(s * long / short)`` -- in the order above; only the box of the
                           first resize is computed.
    The images, the flags and the plan travel in ONE staging buffer and one copy on the "h2d" stream, ``depth`` batches ahead
    as above.  With either argument set, a uniform uint8 ``[N, H, W, C]`` host batch takes the same path (one wrapper, one
    output size); uint8 batches on the device and ``"nchw"`` ones are refused then.  fp32 batches still pass through."""

    def __init__(self, loader, mean, std, device, layout: str = "nhwc", crop: Optional[Tuple[int, int]] = None,
                 flip: bool = False, seed: Optional[int] = 0, depth: int = 2, resized_crop: Optional[Tuple[int, int]] = None,
                 scale: Tuple[float, float] = (0.08, 1.0), ratio: Tuple[float, float] = (3.0 / 4.0, 4.0 / 3.0),
                 resize: Optional[int] = None, pre_resize: Optional[int] = None):
        if layout not in hip_ops.IMAGE_LAYOUTS:
            raise ValueError("DeviceImages: layout must be one of %r, got %r" % (tuple(hip_ops.IMAGE_LAYOUTS), layout))
        if depth < 1:
            raise ValueError("DeviceImages: depth must be at least 1, got %r" % (depth,))
        if flip and seed is None:
            raise ValueError("DeviceImages: flip=True draws flags and needs a seed")
        if resized_crop is not None and (resize is not None or crop is not None):
            raise ValueError("DeviceImages: resized_crop excludes resize and crop (it is the crop)")
        if resized_crop is not None and seed is None:
            raise ValueError("DeviceImages: resized_crop draws boxes and needs a seed")
        if resize is not None and crop is None:
            raise ValueError("DeviceImages: resize needs crop=(Ho, Wo), the centre window all samples share")
        if resized_crop is not None and not (0 < scale[0] <= scale[1] and 0 < ratio[0] <= ratio[1]):
            raise ValueError("DeviceImages: scale and ratio must be positive, increasing pairs, got %r %r" % (scale, ratio))
        if resize is not None and int(resize) < 1:
            raise ValueError("DeviceImages: resize must be positive, got %r" % (resize,))
        if pre_resize is not None and resized_crop is None:
            raise ValueError("DeviceImages: pre_resize is the Resize in front of resized_crop=(Ho, Wo); Resize + CenterCrop is "
                             "resize=s with crop=(Ho, Wo)")
        if pre_resize is not None and int(pre_resize) < 1:
            raise ValueError("DeviceImages: pre_resize must be positive, got %r" % (pre_resize,))
        self.loader, self.mean, self.std = loader, mean, std
        self.device = torch.device(device)
        self.layout, self.flip, self.seed, self.depth = layout, bool(flip), seed, int(depth)
        self.crop = None if crop is None else (int(crop[0]), int(crop[1]))
        self.resized_crop = None if resized_crop is None else (int(resized_crop[0]), int(resized_crop[1]))
        self.scale, self.ratio = (float(scale[0]), float(scale[1])), (float(ratio[0]), float(ratio[1]))
        self.resize = None if resize is None else int(resize)
        self.pre_resize = None if pre_resize is None else int(pre_resize)
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

    def _generator(self, epoch: int, index: int) -> torch.Generator:
        return torch.Generator().manual_seed(((int(self.seed) * _MIX + int(epoch)) * _MIX + int(index)) % (1 << 63))

    def _box(self, g: torch.Generator, height: int, width: int):
        """One box ``(y0, x0, h, w)`` by the rule of torchvision's ``RandomResizedCrop.get_params``."""
        area = height * width
        lo, hi = math.log(self.ratio[0]), math.log(self.ratio[1])
        for _ in range(10):
            target = area * torch.empty(1).uniform_(self.scale[0], self.scale[1], generator=g).item()
            aspect = math.exp(torch.empty(1).uniform_(lo, hi, generator=g).item())
            w, h = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
            if 0 < w <= width and 0 < h <= height:
                y0 = int(torch.randint(0, height - h + 1, (1,), generator=g).item())
                x0 = int(torch.randint(0, width - w + 1, (1,), generator=g).item())
                return y0, x0, h, w
        w, h = width, height                 # the centred box, its ratio clamped
        if width / height < self.ratio[0]:
            h = min(height, max(1, int(round(width / self.ratio[0]))))
        elif width / height > self.ratio[1]:
            w = min(width, max(1, int(round(height * self.ratio[1]))))
        return (height - h) // 2, (width - w) // 2, h, w

    @property
    def resamples(self) -> bool:
        return self.resized_crop is not None or self.resize is not None

    @property
    def out_size(self) -> Optional[Tuple[int, int]]:
        return self.resized_crop if self.resized_crop is not None else self.crop

    def ragged_augmentation(self, epoch: int, index: int, sizes: Sequence[Tuple[int, int]]):
        """``(geom, flip)`` of batch ``index`` of epoch ``epoch`` for images of ``sizes`` = ``[(H, W), ...]``: int32 ``[n, 10]``
        descriptors of ``hip_ops.image_resample_plan`` (``H, W, y0, x0, h, w, Hv, Wv, oy, ox``), uint8 ``[n]`` or None (no flip).
        A pure function of ``(seed, epoch, index)`` and the sizes."""
        if not self.resamples:
            raise ValueError("DeviceImages: images of mixed sizes need resized_crop=(Ho, Wo), or resize=s with crop=(Ho, Wo)")
        n = len(sizes)
        g = self._generator(epoch, index) if self.seed is not None else None
        rows = []
        if self.resized_crop is not None:
            ho, wo = self.resized_crop
            for height, width in sizes:
                y0, x0, h, w = self._box(g, int(height), int(width))
                rows.append((height, width, y0, x0, h, w, ho, wo, 0, 0))
        else:
            ho, wo = self.crop
            for height, width in sizes:
                height, width = int(height), int(width)
                if width <= height:          # Resize(s): the shorter side becomes s
                    hv, wv = int(self.resize * height / width), self.resize
                else:
                    hv, wv = self.resize, int(self.resize * width / height)
                if ho > hv or wo > wv:
                    raise ValueError("DeviceImages: crop %s does not fit a %d x %d image resized to %d x %d"
                                     % (self.crop, height, width, hv, wv))
                rows.append((height, width, 0, 0, height, width, hv, wv, int(round((hv - ho) / 2.0)), int(round((wv - wo) / 2.0))))
        geom = torch.tensor(rows, dtype=torch.int32).reshape(n, hip_ops.RESAMPLE_GEOM)
        flags = (torch.rand(n, generator=g) < 0.5).to(torch.uint8) if self.flip else None
        return geom, flags

    def chain_augmentation(self, epoch: int, index: int, sizes: Sequence[Tuple[int, int]]):
        """``(geom, flip)`` of batch ``index`` of epoch ``epoch`` under ``pre_resize`` + ``resized_crop``: int32 ``[n, 8]``
        descriptors of ``hip_ops.image_resample_chain_plan`` (``H, W, H1, W1, y0, x0, h, w``), uint8 ``[n]`` or None (no flip).
        ``(H1, W1)`` is ``Resize(pre_resize)``'s size of the image, the box is drawn on it.  A pure function of ``(seed, epoch,
        index)`` and the sizes."""
        if self.pre_resize is None:
            raise ValueError("DeviceImages: chain_augmentation needs pre_resize=s with resized_crop=(Ho, Wo)")
        n, s = len(sizes), self.pre_resize
        g = self._generator(epoch, index)
        rows = []
        for height, width in sizes:
            height, width = int(height), int(width)
            if width <= height:              # Resize(s): the shorter side becomes s
                h1, w1 = int(s * height / width), s
            else:
                h1, w1 = s, int(s * width / height)
            rows.append((height, width, h1, w1) + self._box(g, h1, w1))
        geom = torch.tensor(rows, dtype=torch.int32).reshape(n, hip_ops.RESAMPLE_CHAIN_GEOM)
        flags = (torch.rand(n, generator=g) < 0.5).to(torch.uint8) if self.flip else None
        return geom, flags

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
        buf = self._buffer(slot, x.numel()).view(x.shape)
        buf.copy_(x)
        return buf

    def _buffer(self, slot: int, nbytes: int) -> torch.Tensor:
        """``nbytes`` of pinned staging buffer ``slot``, free to write: the previous copy out of it has left the host."""
        entry = self._staging[slot]
        if entry is not None and entry[1]:
            entry[1].synchronize()
        if entry is None or entry[0].numel() < nbytes:
            entry = self._staging[slot] = [torch.empty(max(nbytes, 1), dtype=torch.uint8).pin_memory(), None]
        entry[1] = False                # set to the copy's event by _start
        return entry[0][:nbytes]

    def _start_ragged(self, epoch: int, index: int, items, images):
        """Pack a list of uint8 ``[H, W, C]`` host images, their flip flags and the plan into staging buffer ``index % depth``
        (plan | flags | images, the first two padded to 16 bytes) and begin its copy.  The plan is the chain's under
        ``pre_resize``."""
        images = [_as_image(im) for im in images]
        for im in images:
            if not torch.is_tensor(im) or im.dtype != torch.uint8:
                raise hip_ops.PleasHipError("DeviceImages: images of mixed sizes must be uint8 (got %s): resample fp32 images on the "
                                            "host, or hand over what the decoder produced" % (im.dtype,))
            if im.is_cuda or im.dim() != 3:
                raise hip_ops.PleasHipError("DeviceImages: a list of images holds uint8 [H, W, C] HOST tensors, got %s on %s"
                                            % (tuple(im.shape), im.device))
        channels = images[0].shape[2] if images else 3
        if any(im.shape[2] != channels for im in images):
            raise hip_ops.PleasHipError("DeviceImages: the images of a batch must share their channel count")
        chain = self.pre_resize is not None
        draw = self.chain_augmentation if chain else self.ragged_augmentation
        plan_size, plan_of = ((hip_ops.image_resample_chain_plan_bytes, hip_ops.image_resample_chain_plan) if chain else
                              (hip_ops.image_resample_plan_bytes, hip_ops.image_resample_plan))
        geom, flags = draw(epoch, index, [(im.shape[0], im.shape[1]) for im in images])
        n, size = len(images), self.out_size
        sizes = [im.numel() for im in images]
        offsets = [0] * n
        for i in range(1, n):
            offsets[i] = offsets[i - 1] + sizes[i - 1]
        src_bytes = sum(sizes)
        plan_bytes = plan_size(geom, size)
        at_flags = _pad16(plan_bytes)
        at_src = at_flags + _pad16(n)
        slot = index % self.depth
        buf = self._buffer(slot, at_src + src_bytes)
        plan = plan_of(geom, offsets, channels, size, src_bytes, out=buf)
        if flags is not None:
            buf[at_flags:at_flags + n].copy_(flags)
        for im, o, nb in zip(images, offsets, sizes):
            buf[at_src + o:at_src + o + nb].copy_(im.reshape(-1))
        d, ev = hip_ops.h2d_start(buf, self.device)
        self._staging[slot][1] = ev
        where = (plan_bytes, at_flags if flags is not None else None, at_src, src_bytes, n, channels)
        return index, items, (d, ev, plan, where)

    def _start(self, index: int, batch, epoch: int = 0):
        """Begin the host-to-device copy of a batch (uint8 host images only); returns the batch's pending state."""
        items = tuple(batch) if isinstance(batch, (tuple, list)) else (batch,)
        x = items[0]
        if isinstance(x, (list, tuple)):
            return self._start_ragged(epoch, index, items, x)
        if self.resamples and torch.is_tensor(x) and x.dtype == torch.uint8:
            if x.is_cuda or self.layout != "nhwc" or x.dim() != 4:
                raise hip_ops.PleasHipError("DeviceImages: with resized_crop / resize, uint8 batches are lists of images or 4-d "
                                            "nhwc HOST tensors (got shape %s on %s, layout %s)" % (tuple(x.shape), x.device, self.layout))
            return self._start_ragged(epoch, index, items, list(x))
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
        if copy is not None and len(copy) == 4:      # a resampled batch: plan | flags | images in one buffer
            (d, ev, plan, (plan_bytes, at_flags, at_src, src_bytes, n, channels)) = copy
            u8 = hip_ops.h2d_finish(d, ev, self.device)
            resample = hip_ops.image_resample if self.pre_resize is None else hip_ops.image_resample_chain
            out = resample(u8[at_src:at_src + src_bytes], u8[:plan_bytes], plan, self._table(channels),
                           flip=None if at_flags is None else u8[at_flags:at_flags + n])
            return (out,) + items[1:]
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
                pending.append(self._start(*nxt, epoch))
            if not pending:
                return
            yield self._finish(epoch, pending.popleft())
