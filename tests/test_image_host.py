"""Host side of the uint8 image path (no GPU): the exported symbol and its binding, ``hip_ops.image_table`` bit for bit against
the ``ToTensor`` / ``Normalize`` chain, what ``pleas_image_batch`` and ``hip_ops.image_batch`` refuse before any device is
touched, and the augmentation draws of ``DeviceImages``."""
import ctypes

import pytest
import torch

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)      # ImageNet's
EINVAL = -22
P = 4096          # a non-NULL, 16-byte aligned address that is never dereferenced: every call below is refused (or N == 0)


@pytest.fixture(scope="module")
def lib():
    from pleas_merging_amd import _lib, build

    build.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def ops():
    from pleas_merging_amd import hip_ops

    return hip_ops


def test_symbol_is_exported_and_bound(lib):
    from pleas_merging_amd import _lib

    assert "pleas_image_batch" in _lib.SIGNATURES
    restype, argtypes = _lib.SIGNATURES["pleas_image_batch"]
    assert restype is ctypes.c_int and len(argtypes) == 13 and argtypes[5] is ctypes.c_int64
    assert lib.pleas_image_batch.argtypes == argtypes
    assert (_lib.IMAGE_NHWC, _lib.IMAGE_NCHW) == (0, 1)


@pytest.mark.parametrize("mean,std", [(MEAN, STD), (None, None)])
def test_image_table_is_the_torch_chain_bitwise(ops, mean, std):
    table = ops.image_table(mean, std, 3)
    assert table.dtype == torch.float32 and tuple(table.shape) == (3, 256) and table.device.type == "cpu"
    # all 256 values as an image of 256 pixels: ToTensor (float, / 255), then Normalize (sub mean, div std)
    src = torch.arange(256, dtype=torch.uint8).view(1, 1, 256, 1).expand(1, 1, 256, 3).contiguous()      # [N, H, W, C]
    want = src.permute(0, 3, 1, 2).float().div(255)
    if mean is not None:
        want = want.sub(torch.tensor(mean).view(1, 3, 1, 1)).div(torch.tensor(std).view(1, 3, 1, 1))
    assert torch.equal(table, want[0, :, 0, :])
    assert torch.isfinite(table).all()


def test_image_table_refuses_bad_channel_counts(ops):
    from pleas_merging_amd._lib import PleasHipError

    for channels in (0, 5):
        with pytest.raises(PleasHipError):
            ops.image_table(None, None, channels)
    with pytest.raises(PleasHipError):
        ops.image_table((0.5, 0.5), None, 3)


def _call(lib, src=P, dst=P, lut=P, N=1, C=3, H=4, W=4, Ho=4, Wo=4, layout=0):
    return lib.pleas_image_batch(src, dst, lut, None, None, N, C, H, W, Ho, Wo, layout, None)


@pytest.mark.parametrize("bad", [dict(src=None), dict(dst=None), dict(lut=None), dict(C=0), dict(C=5), dict(Ho=5), dict(Wo=5),
                                 dict(H=0, Ho=0), dict(W=0, Wo=0), dict(Ho=0), dict(Wo=-1), dict(N=-1), dict(dst=P + 4),
                                 dict(dst=P + 8), dict(layout=2), dict(layout=-1)],
                         ids=lambda b: ",".join("%s=%s" % kv for kv in b.items()))
def test_abi_refuses_before_anything_is_enqueued(lib, bad):
    assert _call(lib, **bad) == EINVAL
    assert b"invalid argument" in lib.pleas_last_error()


def test_abi_takes_an_empty_batch(lib):
    assert _call(lib, N=0) == 0
    assert _call(lib, N=0, src=None, dst=None, lut=None) == 0
    assert _call(lib, N=0, C=5) == EINVAL          # the other refusals do not depend on N


def test_wrapper_refusals(ops):
    from pleas_merging_amd._lib import PleasHipError

    table = ops.image_table(MEAN, STD, 3)
    u8 = torch.zeros(2, 8, 6, 3, dtype=torch.uint8)
    with pytest.raises(PleasHipError, match="uint8"):                       # a wrong dtype
        ops.image_batch(u8.float(), table)
    with pytest.raises(PleasHipError, match="out must be"):                 # a CPU out
        ops.image_batch(u8, table, out=torch.empty(2, 3, 8, 6))
    with pytest.raises(PleasHipError, match="origin outside"):              # one past the last legal position, either axis
        ops.image_batch(u8, table, size=(5, 4), origin=[[3, 2], [4, 2]])
    with pytest.raises(PleasHipError, match="origin outside"):
        ops.image_batch(u8, table, size=(5, 4), origin=[[3, 2], [3, 3]])
    with pytest.raises(PleasHipError, match="origin outside"):
        ops.image_batch(u8, table, size=(5, 4), origin=[[-1, 0], [0, 0]])
    with pytest.raises(PleasHipError, match="5 channels"):                  # C = 5
        ops.image_batch(torch.zeros(2, 8, 6, 5, dtype=torch.uint8), table)
    with pytest.raises(PleasHipError, match="window"):
        ops.image_batch(u8, table, size=(9, 6))
    with pytest.raises(PleasHipError, match="layout"):
        ops.image_batch(u8, table, layout="hwcn")
    with pytest.raises(PleasHipError, match="contiguous"):
        ops.image_batch(u8.permute(0, 3, 1, 2), table, layout="nchw")
    with pytest.raises(PleasHipError, match="flip"):
        ops.image_batch(u8, table, flip=[1, 0, 1])
    with pytest.raises(PleasHipError, match="no CPU fallback"):             # legal arguments, but on the host: still no fallback
        ops.image_batch(u8, table, size=(5, 4), origin=[[3, 2], [0, 0]], flip=[1, 0])


def _images(loader=(), **kw):
    from pleas_merging_amd.methods import DeviceImages

    return DeviceImages(loader, MEAN, STD, "cpu", **kw)


def test_device_images_is_exported_and_forwards_len():
    import pleas.methods
    import pleas_merging_amd.methods as methods

    assert pleas.methods.DeviceImages is methods.DeviceImages
    assert len(_images([1, 2, 3, 4, 5])) == 5
    with pytest.raises(ValueError):
        _images(layout="hwc")
    with pytest.raises(ValueError):
        _images(flip=True, seed=None)
    with pytest.raises(ValueError):
        _images(crop=(9, 4)).augmentation(0, 0, 2, 8, 8)


def test_augmentation_draws_repeat_per_seed_epoch_batch():
    a, b = _images(crop=(24, 20), flip=True, seed=7), _images(crop=(24, 20), flip=True, seed=7)
    n, H, W = 64, 32, 32
    draws = {}
    for epoch in range(2):
        for index in range(3):
            o, f = a.augmentation(epoch, index, n, H, W)
            o2, f2 = b.augmentation(epoch, index, n, H, W)
            assert torch.equal(o, o2) and torch.equal(f, f2)                      # same (seed, epoch, batch): same draws
            assert tuple(o.shape) == (n, 2) and tuple(f.shape) == (n,) and f.dtype == torch.uint8
            assert int(o.min()) >= 0 and int(o[:, 0].max()) <= H - 24 and int(o[:, 1].max()) <= W - 20
            assert 0 < int(f.sum()) < n
            draws[epoch, index] = (o, f)
    keys = list(draws)
    for i, k in enumerate(keys):                                                  # across epochs and batches: different draws
        for k2 in keys[i + 1:]:
            assert not torch.equal(draws[k][0], draws[k2][0]) and not torch.equal(draws[k][1], draws[k2][1]), (k, k2)
    other, _ = _images(crop=(24, 20), flip=True, seed=8).augmentation(0, 0, n, H, W)
    assert not torch.equal(other, draws[0, 0][0])


def test_augmentation_without_draws():
    assert _images().augmentation(0, 0, 4, 32, 32) == (None, None)
    o, f = _images(crop=(24, 21), seed=None).augmentation(3, 5, 4, 32, 32)       # centre crop: torchvision's rounding
    assert f is None and o.tolist() == [[4, int(round(11 / 2.0))]] * 4
    o, f = _images(flip=True, seed=1).augmentation(0, 0, 4, 32, 32)
    assert o is None and tuple(f.shape) == (4,)


def test_epoch_counts_iterations():
    d = _images([])
    assert d.epoch == 0
    assert list(d) == [] and list(d) == []
    assert d.epoch == 2
