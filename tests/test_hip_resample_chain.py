"""``pleas_image_resample_chain`` (csrc/image.hip) through ``hip_ops.image_resample_chain``, and ``DeviceImages(pre_resize=...,
resized_crop=...)`` on loaders whose images differ in size.  The references are the PIL fixture
tests/golden/resample_chain_pil.npz directly, and ``hip_ops.image_resample_chain_host`` -- the same plan executed on the CPU,
which tests/test_resample_chain_host.py holds to PIL bit for bit.  Every comparison is ``torch.equal``.

Shapes (tests/resample_chain_cases.py): the smallest that cover down / up in either stage, many taps, one tap, an unchanged
first stage, a 1 x 1 box, boxes at the far corner, packed offsets that are no multiple of 4; one batch near 300 x 300 to
224 x 224 for several work items per sample."""
import os

import numpy as np
import pytest
import torch

import resample_chain_cases as cc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406, 0.45), (0.229, 0.224, 0.225, 0.25)


@pytest.fixture(scope="module")
def ops():
    from pleas_merging_amd import hip_ops

    return hip_ops


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "resample_chain_pil.npz"))


def _pack(srcs, gap):
    """uint8 [H, W, C] arrays ``gap`` bytes apart in one buffer (the first at ``gap``): ``(buffer, offsets)``."""
    offsets, at = [], gap
    for s in srcs:
        offsets.append(at)
        at += s.size + gap
    buf = torch.zeros(at, dtype=torch.uint8)
    for s, o in zip(srcs, offsets):
        buf[o:o + s.size] = torch.from_numpy(np.ascontiguousarray(s).reshape(-1))
    return buf, offsets


def _images(loader, **kw):
    from pleas_merging_amd.methods import DeviceImages

    return DeviceImages(loader, MEAN[:3], STD[:3], "cuda", **kw)


@pytest.mark.parametrize("channels", cc.CHANNELS)
def test_kernels_equal_the_pil_fixture(ops, golden, channels):
    """All cases of a channel count in one ragged batch at the common output size, every other sample flipped."""
    flip = [i % 2 for i in range(len(cc.CASES))]
    table = ops.image_table(MEAN[:channels], STD[:channels], channels)
    for fill in cc.FILLS:
        buf, offsets = _pack([cc.source(c, channels, fill) for c in cc.CASES], 3)
        assert any(o % 4 for o in offsets)
        plan = ops.image_resample_chain_plan([cc.geom_row(c) for c in cc.CASES], offsets, channels, cc.BATCH_SIZE, buf.numel())
        got = ops.image_resample_chain(buf.cuda(), plan.cuda(), plan, table.cuda(), flip=flip)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (len(cc.CASES), channels) + cc.BATCH_SIZE
        got = got.cpu()
        for i, c in enumerate(cc.CASES):
            want = torch.from_numpy(golden[cc.key(c, channels, fill) + "/want_batch"])
            want = want.flip(1) if flip[i] else want
            assert torch.equal(got[i], torch.stack([table[ch][want[..., ch].long()] for ch in range(channels)], 0)), cc.key(c, channels, fill)


@pytest.mark.parametrize("channels", cc.CHANNELS)
def test_kernels_equal_the_pil_fixture_at_each_cases_own_size(ops, golden, channels):
    table = ops.image_table(MEAN[:channels], STD[:channels], channels)
    table_d = table.cuda()
    for case in cc.CASES:
        src = cc.source(case, channels, "random")
        buf, offsets = _pack([src], 1)
        plan = ops.image_resample_chain_plan([cc.geom_row(case)], offsets, channels, case[5:7], buf.numel())
        got = ops.image_resample_chain(buf.cuda(), plan.cuda(), plan, table_d).cpu()
        want = torch.from_numpy(golden[cc.key(case, channels, "random") + "/want"])
        assert torch.equal(got[0], torch.stack([table[ch][want[..., ch].long()] for ch in range(channels)], 0)), case[0]


def _seeded_batch():
    """16 images with sides U(5..60), boxes drawn by ``DeviceImages`` on their ``Resize(24)`` sizes."""
    rng = np.random.RandomState(16)
    srcs = [rng.randint(0, 256, (int(rng.randint(5, 61)), int(rng.randint(5, 61)), 3)).astype(np.uint8) for _ in range(16)]
    wrapper = _images([], pre_resize=24, resized_crop=(16, 16), flip=True, seed=9, scale=(0.08, 1.0))
    geom, flip = wrapper.chain_augmentation(0, 0, [s.shape[:2] for s in srcs])
    return srcs, geom, flip, (16, 16)


def _large_batch():
    """3 images with sides near 300 to 224 x 224: the many-tap path and several items per sample in all four launches."""
    rng = np.random.RandomState(3)
    sizes = [(301, 333), (350, 297), (299, 299)]
    srcs = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    geom = torch.tensor([[301, 333, 256, 283, 7, 11, 240, 260], [350, 297, 301, 256, 40, 0, 261, 256], [299, 299, 256, 256, 100, 90, 37, 41]])
    return srcs, geom, torch.tensor([0, 1, 1], dtype=torch.uint8), (224, 224)


@pytest.mark.parametrize("batch", [_seeded_batch, _large_batch], ids=["seeded16", "near300"])
def test_kernels_equal_the_host_executor(ops, batch):
    srcs, geom, flip, size = batch()
    buf, offsets = _pack(srcs, 1)
    plan = ops.image_resample_chain_plan(geom, offsets, 3, size, buf.numel())
    info = ops.image_resample_chain_plan_info(plan)
    if batch is _large_batch:
        assert all(i > 3 for i in info["items"]), info["items"]
    table = ops.image_table(MEAN[:3], STD[:3], 3)
    want, _, _ = ops.image_resample_chain_host(buf, plan, table, flip=flip)
    got = ops.image_resample_chain(buf.cuda(), plan.cuda(), plan, table.cuda(), flip=flip)
    assert tuple(got.shape) == (len(srcs), 3) + size
    assert torch.equal(got.cpu(), want)


def test_no_scratch_byte_is_read_before_it_is_written(ops):
    """Two calls on the same inputs, the workspace pre-filled with two different byte patterns, ``out`` honoured."""
    srcs, geom, flip, size = _seeded_batch()
    buf, offsets = _pack(srcs, 3)
    plan = ops.image_resample_chain_plan(geom, offsets, 3, size, buf.numel())
    info = ops.image_resample_chain_plan_info(plan)
    table = ops.image_table(MEAN[:3], STD[:3], 3).cuda()
    d_buf, d_plan = buf.cuda(), plan.cuda()
    scratch = torch.full((info["ws_bytes"] + 16,), 0x00, dtype=torch.uint8, device="cuda")
    a = ops.image_resample_chain(d_buf, d_plan, plan, table, flip=flip, scratch=scratch)
    assert bool((scratch[info["ws_bytes"]:] == 0).all())                          # nothing is written past the plan's workspace
    scratch.fill_(0xFF)
    out = torch.full((16, 3, 16, 16), float("nan"), device="cuda")
    b = ops.image_resample_chain(d_buf, d_plan, plan, table, flip=flip.cuda(), out=out, scratch=scratch)
    assert b is out and torch.equal(a, b) and not bool(torch.isnan(b).any())
    assert bool((scratch[info["ws_bytes"]:] == 0xFF).all())
    c = ops.image_resample_chain(d_buf, d_plan, plan, table, flip=flip)            # and from the stream's own workspace
    assert torch.equal(a, c)
    want, _, mid = ops.image_resample_chain_host(buf, plan, ops.image_table(MEAN[:3], STD[:3], 3), flip=flip)
    assert torch.equal(a.cpu(), want)


# ------------------------------------------------------------------------------------------------ DeviceImages end to end
def _samples():
    """Fourteen (image, label) samples of mixed sizes: the case images twice, as a decoder would leave them."""
    return [(torch.from_numpy(cc.source(c, 3, "random")), i) for i, c in enumerate(cc.CASES + cc.CASES[::-1])]


def _loader(samples, batch_size=5):
    from pleas_merging_amd.methods import ragged_collate

    return [ragged_collate(samples[i:i + batch_size]) for i in range(0, len(samples), batch_size)]


def _host(ops, images, geom, size, flip):
    buf, offsets = _pack([im.numpy() for im in images], 0)
    plan = ops.image_resample_chain_plan(geom, offsets, 3, size, buf.numel())
    return ops.image_resample_chain_host(buf, plan, ops.image_table(MEAN[:3], STD[:3], 3), flip=flip)[0]


def test_device_images_chain_equals_the_host_executor_under_its_own_draws(ops):
    loader = _loader(_samples())
    wrapped = _images(loader, pre_resize=24, resized_crop=(16, 16), flip=True, seed=3)
    assert len(wrapped) == 3
    epochs = [list(wrapped), list(wrapped)]
    for epoch, got in enumerate(epochs):
        assert len(got) == 3
        for index, ((x, labels), (images, want_labels)) in enumerate(zip(got, loader)):
            geom, flip = wrapped.chain_augmentation(epoch, index, [(im.shape[0], im.shape[1]) for im in images])
            assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (len(images), 3, 16, 16)
            assert torch.equal(x.cpu(), _host(ops, images, geom, (16, 16), flip)), (epoch, index)
            assert labels is want_labels                                          # the other items pass through untouched
    assert not any(torch.equal(a[0], b[0]) for a, b in zip(*epochs))              # epoch 1 draws differ from epoch 0
    # a uniform uint8 [N, H, W, C] host batch takes the same path
    g = torch.Generator().manual_seed(11)
    uniform = (torch.randint(0, 256, (4, 32, 27, 3), dtype=torch.uint8, generator=g), torch.arange(4))
    wrapped = _images([uniform], pre_resize=24, resized_crop=(16, 16), flip=True, seed=3)
    (x, labels), = list(wrapped)
    geom, flip = wrapped.chain_augmentation(0, 0, [(32, 27)] * 4)
    assert torch.equal(x.cpu(), _host(ops, list(uniform[0]), geom, (16, 16), flip)) and labels is uniform[1]


def test_refused_inputs_raise_before_anything_is_enqueued(ops):
    from pleas_merging_amd._lib import PleasHipError

    g = torch.Generator().manual_seed(11)
    uniform = (torch.randint(0, 256, (4, 32, 27, 3), dtype=torch.uint8, generator=g), torch.arange(4))
    with pytest.raises(PleasHipError, match="HOST"):                               # uint8 already on the device
        list(_images([(uniform[0].cuda(), uniform[1])], pre_resize=24, resized_crop=(16, 16), seed=3))
    with pytest.raises(PleasHipError, match="nchw"):
        list(_images([(uniform[0].permute(0, 3, 1, 2).contiguous(), uniform[1])], layout="nchw", pre_resize=24, resized_crop=(16, 16), seed=3))
    srcs, geom, flip, size = _seeded_batch()
    buf, offsets = _pack(srcs, 3)
    plan = ops.image_resample_chain_plan(geom, offsets, 3, size, buf.numel())
    table = ops.image_table(MEAN[:3], STD[:3], 3).cuda()
    d_buf, d_plan = buf.cuda(), plan.cuda()
    out = torch.full((16, 3, 16, 16), 7.0, device="cuda")
    with pytest.raises(PleasHipError, match="no CPU fallback"):
        ops.image_resample_chain(buf, d_plan, plan, table, out=out)
    with pytest.raises(PleasHipError, match="plan_dev"):                           # the device plan on the host
        ops.image_resample_chain(d_buf, plan, plan, table, out=out)
    with pytest.raises(PleasHipError, match="plan_dev"):                           # of the wrong dtype
        ops.image_resample_chain(d_buf, d_plan.view(torch.int32), plan, table, out=out)
    room = torch.zeros(plan.numel() + 8, dtype=torch.uint8, device="cuda")
    room[2:2 + plan.numel()].copy_(plan)
    with pytest.raises(PleasHipError, match="plan_dev"):                           # not on a 4-byte boundary
        ops.image_resample_chain(d_buf, room[2:2 + plan.numel()], plan, table, out=out)
    with pytest.raises(PleasHipError, match="plan_dev"):                           # shorter than the host plan
        ops.image_resample_chain(d_buf, d_plan[:-4], plan, table, out=out)
    with pytest.raises(PleasHipError, match="host plan"):                          # the host plan on the device, or of the wrong dtype
        ops.image_resample_chain(d_buf, d_plan, d_plan, table, out=out)
    with pytest.raises(PleasHipError, match="host plan"):
        ops.image_resample_chain(d_buf, d_plan, plan.view(torch.int32), table, out=out)
    with pytest.raises(PleasHipError, match="not a chain plan"):
        ops.image_resample_chain(d_buf, d_plan, torch.zeros_like(plan), table, out=out)
    with pytest.raises(PleasHipError, match="scratch"):
        ops.image_resample_chain(d_buf, d_plan, plan, table, out=out, scratch=torch.zeros(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(PleasHipError, match="table"):
        ops.image_resample_chain(d_buf, d_plan, plan, table[:2], out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                                # nothing ran
    empty = ops.image_resample_chain_plan(torch.empty(0, 8, dtype=torch.int32), [], 3, (4, 4), 0)
    got = ops.image_resample_chain(torch.empty(0, dtype=torch.uint8, device="cuda"), empty.cuda(), empty, table)
    assert tuple(got.shape) == (0, 3, 4, 4) and got.is_cuda
