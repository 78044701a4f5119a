"""``pleas_image_resample`` (csrc/image.hip) through ``hip_ops.image_resample``, and ``DeviceImages`` on loaders whose images differ
in size.  The reference is ``hip_ops.image_resample_host`` -- the same plan executed on the CPU, which tests/test_resample_host.py
holds to PIL bit for bit -- and the PIL fixture tests/golden/resample_pil.npz directly.  Every comparison is ``torch.equal``.

Shapes (tests/resample_cases.py): the smallest that cover one tap, two to three taps, many taps, clamped edges, an unchanged
axis, a box, a window, and packed offsets that are no multiple of 4."""
import os

import numpy as np
import pytest
import torch

import resample_cases as rc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406, 0.45), (0.229, 0.224, 0.225, 0.25)
TRAIN = ["down", "pixel", "mixed", "box", "up"]          # five samples of mixed sizes, each resampled to 16 x 16
EVAL = ["eval_tall", "eval_wide"]


@pytest.fixture(scope="module")
def ops():
    from pleas_merging_amd import hip_ops

    return hip_ops


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "resample_pil.npz"))


def _case(name):
    return next(c for c in rc.CASES if c[0] == name)


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


def _train_batch(channels):
    """The TRAIN samples, every one as a box of its image resampled to 16 x 16; sizes H * W * C are mostly odd, so with a gap of
    1 or 3 bytes the offsets are no multiple of 4."""
    cases = [_case(n) for n in TRAIN]
    srcs = [rc.source(c, channels, "random") for c in cases]
    geoms = []
    for c in cases:
        g = rc.geom_row(c)
        g[6:10] = [16, 16, 0, 0]
        geoms.append(g)
    return srcs, geoms, (16, 16)


def _eval_batch(channels):
    cases = [_case(n) for n in EVAL]
    cases = [cases[0], cases[1], cases[0], cases[1], cases[0]]
    return [rc.source(c, channels, "random") for c in cases], [rc.geom_row(c) for c in cases], (20, 20)


def _both(ops, srcs, geoms, size, channels, flip, gap=3):
    buf, offsets = _pack(srcs, gap)
    assert any(o % 4 for o in offsets)
    plan = ops.image_resample_plan(geoms, offsets, channels, size, buf.numel())
    table = ops.image_table(MEAN[:channels], STD[:channels], channels)
    want, want_u8 = ops.image_resample_host(buf, plan, table, flip=flip)
    got = ops.image_resample(buf.cuda(), plan.cuda(), plan, table.cuda(), flip=flip)
    return got, want, want_u8, table


@pytest.mark.parametrize("flip", [None, [1, 0, 1, 1, 0]], ids=["plain", "flipped"])
@pytest.mark.parametrize("batch", [_train_batch, _eval_batch], ids=["resized_crop", "resize_window"])
@pytest.mark.parametrize("channels", rc.CHANNELS)
def test_kernels_equal_the_host_executor(ops, channels, batch, flip):
    srcs, geoms, size = batch(channels)
    got, want, _, _ = _both(ops, srcs, geoms, size, channels, flip)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (5, channels) + size
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("channels", rc.CHANNELS)
def test_kernels_equal_the_pil_fixture(ops, golden, channels):
    """Every case of the fixture, one sample per launch (each case has its own output size), straight against PIL's bytes."""
    for case in rc.CASES:
        for fill in rc.FILLS:
            src = rc.source(case, channels, fill)
            got, _, _, table = _both(ops, [src], [rc.geom_row(case)], case[3:5], channels, None, gap=1)
            want = torch.from_numpy(golden[rc.key(case, channels, fill) + "/want"])
            planes = torch.stack([table[c][want[..., c].long()] for c in range(channels)], 0)
            assert torch.equal(got[0].cpu(), planes), rc.key(case, channels, fill)
    # and the evaluation window of a ragged batch
    srcs, geoms, size = _eval_batch(channels)
    got, _, _, table = _both(ops, srcs, geoms, size, channels, None)
    for i, name in enumerate([EVAL[0], EVAL[1], EVAL[0], EVAL[1], EVAL[0]]):
        want = torch.from_numpy(golden[rc.key(_case(name), channels, "random") + "/want"])
        assert torch.equal(got[i].cpu(), torch.stack([table[c][want[..., c].long()] for c in range(channels)], 0))


def test_two_runs_give_equal_bits_and_out_is_honoured(ops):
    srcs, geoms, size = _train_batch(3)
    buf, offsets = _pack(srcs, 3)
    plan = ops.image_resample_plan(geoms, offsets, 3, size, buf.numel())
    table = ops.image_table(MEAN[:3], STD[:3], 3).cuda()
    d_buf, d_plan = buf.cuda(), plan.cuda()
    a = ops.image_resample(d_buf, d_plan, plan, table, flip=[0, 1, 0, 1, 0])
    out = torch.full((5, 3, 16, 16), float("nan"), device="cuda")
    b = ops.image_resample(d_buf, d_plan, plan, table, flip=torch.tensor([0, 1, 0, 1, 0], dtype=torch.uint8, device="cuda"), out=out)
    assert b is out and torch.equal(a, b) and not bool(torch.isnan(b).any())


def test_many_items_and_a_wide_output(ops):
    """More work items than one per sample (rows of a sample spread over workgroups), an output wider than a team's lanes x 4,
    and a downscaling with hundreds of taps."""
    rng = np.random.RandomState(5)
    sizes = [(257, 300), (40, 1031), (513, 64)]
    srcs = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    geoms = [[h, w, 0, 0, h, w, 70, 1100, 3, 37] for h, w in sizes]
    buf, offsets = _pack(srcs, 1)
    plan = ops.image_resample_plan(geoms, offsets, 3, (61, 1029), buf.numel())
    info = ops.image_resample_plan_info(plan)
    assert info["items"][0] > 3 and info["items"][1] > 3
    table = ops.image_table(None, None, 3)
    want, _ = ops.image_resample_host(buf, plan, table)
    got = ops.image_resample(buf.cuda(), plan.cuda(), plan, table.cuda())
    assert torch.equal(got.cpu(), want)


def test_empty_batch_and_host_tensors(ops):
    from pleas_merging_amd._lib import PleasHipError

    table = ops.image_table(None, None, 3).cuda()
    plan = ops.image_resample_plan(torch.empty(0, 10, dtype=torch.int32), [], 3, (4, 4), 0)
    got = ops.image_resample(torch.empty(0, dtype=torch.uint8, device="cuda"), plan.cuda(), plan, table)
    assert tuple(got.shape) == (0, 3, 4, 4) and got.is_cuda
    srcs, geoms, size = _train_batch(3)
    buf, offsets = _pack(srcs, 3)
    plan = ops.image_resample_plan(geoms, offsets, 3, size, buf.numel())
    with pytest.raises(PleasHipError, match="no CPU fallback"):
        ops.image_resample(buf, plan.cuda(), plan, table)
    with pytest.raises(PleasHipError, match="plan_dev"):
        ops.image_resample(buf.cuda(), plan, plan, table)


# ------------------------------------------------------------------------------------------------ DeviceImages end to end
def _samples(channels=3):
    """Twelve (image, label) samples of mixed sizes: a dataset as a decoder would leave it."""
    names = TRAIN + EVAL + TRAIN
    return [(torch.from_numpy(rc.source(_case(n), channels, "random")), i) for i, n in enumerate(names)]


def _loader(samples, batch_size=4):
    from pleas_merging_amd.methods import ragged_collate

    return [ragged_collate(samples[i:i + batch_size]) for i in range(0, len(samples), batch_size)]


def _images(loader, **kw):
    from pleas_merging_amd.methods import DeviceImages

    return DeviceImages(loader, MEAN[:3], STD[:3], "cuda", **kw)


def _host(ops, images, geom, size, flip):
    buf, offsets = _pack([im.numpy() for im in images], 0)
    plan = ops.image_resample_plan(geom, offsets, 3, size, buf.numel())
    return ops.image_resample_host(buf, plan, ops.image_table(MEAN[:3], STD[:3], 3), flip=flip)[0]


def test_device_images_resized_crop_equals_the_host_executor_under_its_own_draws(ops):
    loader = _loader(_samples())
    wrapped = _images(loader, resized_crop=(16, 16), flip=True, seed=3)
    assert len(wrapped) == 3
    epochs = [list(wrapped), list(wrapped)]
    for epoch, got in enumerate(epochs):
        assert len(got) == 3
        for index, ((x, labels), (images, want_labels)) in enumerate(zip(got, loader)):
            geom, flip = wrapped.ragged_augmentation(epoch, index, [(im.shape[0], im.shape[1]) for im in images])
            assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (4, 3, 16, 16)
            assert torch.equal(x.cpu(), _host(ops, images, geom, (16, 16), flip)), (epoch, index)
            assert torch.equal(labels, want_labels)
    assert not any(torch.equal(a[0], b[0]) for a, b in zip(*epochs))              # epoch 1 draws differ from epoch 0


def test_device_images_resize_and_centre_crop_equals_the_fixture(ops, golden):
    samples = [(torch.from_numpy(rc.source(_case(n), 3, "random")), i) for i, n in enumerate(EVAL + EVAL[::-1])]
    table = ops.image_table(MEAN[:3], STD[:3], 3)
    got = list(_images(_loader(samples, 2), resize=24, crop=(20, 20), seed=None))
    assert len(got) == 2
    flat = torch.cat([x for x, _ in got]).cpu()
    for i, name in enumerate(EVAL + EVAL[::-1]):
        want = torch.from_numpy(golden[rc.key(_case(name), 3, "random") + "/want"])
        assert torch.equal(flat[i], torch.stack([table[c][want[..., c].long()] for c in range(3)], 0)), name


def test_device_images_mixed_pipeline_and_depth(ops):
    """One wrapper, a ragged batch, a uniform uint8 batch and an fp32 batch; ``depth`` does not change a bit."""
    from pleas_merging_amd._lib import PleasHipError

    ragged = _loader(_samples())
    g = torch.Generator().manual_seed(11)
    uniform = (torch.randint(0, 256, (4, 32, 27, 3), dtype=torch.uint8, generator=g), torch.arange(4))
    fp32 = (torch.randn(4, 3, 16, 16, generator=g), torch.arange(4))
    loader = [ragged[0], uniform, fp32, ragged[1], ragged[2]]
    runs = {}
    for depth in (1, 2, 3):
        wrapped = _images(loader, resized_crop=(16, 16), flip=True, seed=3, depth=depth)
        runs[depth] = [x for x, _ in wrapped]
        assert all(x.is_cuda and tuple(x.shape) == (4, 3, 16, 16) for x in runs[depth])
    for depth in (1, 3):
        assert all(torch.equal(a, b) for a, b in zip(runs[depth], runs[2])), depth
    wrapped = _images(loader, resized_crop=(16, 16), flip=True, seed=3)
    geom, flip = wrapped.ragged_augmentation(0, 1, [(32, 27)] * 4)                # the uniform batch: resampled like a ragged one
    assert torch.equal(runs[2][1].cpu(), _host(ops, list(uniform[0]), geom, (16, 16), flip))
    assert torch.equal(runs[2][2].cpu(), fp32[0])                                 # fp32 passes through
    # the uniform path of a wrapper without resampling is what it was, and refuses a ragged batch
    plain = [x for x, _ in _images([uniform], crop=(16, 16), seed=None)]
    assert torch.equal(plain[0].cpu(), ops.image_batch(uniform[0].cuda(), ops.image_table(MEAN[:3], STD[:3], 3).cuda(),
                                                       origin=[[8, 6]] * 4, size=(16, 16)).cpu())
    with pytest.raises(ValueError, match="mixed sizes"):
        list(_images([ragged[0]], crop=(16, 16), seed=None))
    floats = ([im.float() for im in ragged[0][0]], ragged[0][1])
    with pytest.raises(PleasHipError, match="uint8"):
        list(_images([floats], resized_crop=(16, 16), seed=3))
    with pytest.raises(PleasHipError, match="HOST"):
        list(_images([(uniform[0].cuda(), uniform[1])], resized_crop=(16, 16), seed=3))
