"""``pleas_image_batch`` (csrc/image.hip) through ``hip_ops.image_batch``, and ``DeviceImages`` in front of the entry points.

Every comparison is ``torch.equal`` against the chain the reference's drivers run on the CPU,
``src.permute(0, 3, 1, 2)[:, :, y0:y0 + Ho, x0:x0 + Wo].float().div(255).sub(mean).div(std)`` with ``.flip(-1)`` for flipped
samples: the kernel is a table lookup and the table is built with that arithmetic, so there is no tolerance to choose.

Per shape: the base pointer of src moved by 0 .. 3 bytes (a view into a larger buffer), canaries in front of and behind dst,
windows at origin (0, 0), at the last legal origin and at an odd x0 (a row start off every 16-byte boundary), flips mixed
inside a batch on odd and even widths, ``out=`` reuse, and every call twice for the same bits."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25)
CANARY = -12345.0


@pytest.fixture(scope="module")
def ops():
    from pleas_merging_amd import hip_ops

    return hip_ops


def _mean_std(C):
    return torch.tensor(MEAN[:C]).view(1, C, 1, 1), torch.tensor(STD[:C]).view(1, C, 1, 1)


def chain(src, layout, size, origin, flip):
    """The CPU chain, per sample (origins differ inside a batch).  ``src`` uint8 on the CPU in ``layout``."""
    planar = src if layout == "nchw" else src.permute(0, 3, 1, 2)
    mean, std = _mean_std(planar.shape[1])
    Ho, Wo = size
    out = []
    for n in range(planar.shape[0]):
        y0, x0 = origin[n] if origin is not None else (0, 0)
        x = planar[n:n + 1, :, y0:y0 + Ho, x0:x0 + Wo].float().div(255).sub(mean).div(std)
        out.append(x.flip(-1) if flip is not None and flip[n] else x)
    return torch.cat(out, 0) if out else torch.empty(0, planar.shape[1], Ho, Wo)


def _table(ops, C):
    return ops.image_table(MEAN[:C], STD[:C], C).cuda()


def _windows(N, H, W):
    """(size, origin per sample) of a shape: the whole image; a window three columns and a row short whose origins walk (0, 0),
    the last legal position and an odd x0; for wide images a window 16 columns short (x0 = 0 and 16 keep a row start on a
    16-byte boundary after the crop, the odd x0 does not)."""
    yield (H, W), None
    sizes = [(max(1, H - 1), max(1, W - 3))] + ([(H, W - 16)] if W > 16 else [])
    for Ho, Wo in sizes:
        odd = max([x for x in range(W - Wo + 1) if x % 2] or [0])
        spots = [(0, 0), (H - Ho, W - Wo), (min(1, H - Ho), odd), (0, W - Wo)]
        yield (Ho, Wo), [spots[(n + 1) % len(spots)] for n in range(N)] if N > 1 else [spots[1]]
        yield (Ho, Wo), [spots[n % len(spots)] for n in range(N)]


def _run(ops, src_cpu, layout, shift, size, origin, flip, table, out=None):
    """One call on a src whose base pointer is ``shift`` bytes past an aligned allocation; dst sits between two canaries."""
    buf = torch.zeros(src_cpu.numel() + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    src = buf[shift:shift + src_cpu.numel()].view(src_cpu.shape)
    src.copy_(src_cpu)
    N, C = src_cpu.shape[0], (src_cpu.shape[1] if layout == "nchw" else src_cpu.shape[3])
    numel = N * C * size[0] * size[1]
    if out is None:
        out = torch.full((numel + 8,), CANARY, device="cuda")
    view = out[4:4 + numel].view(N, C, *size)
    got = ops.image_batch(src, table, out=view, origin=origin, flip=flip, size=size, layout=layout)
    assert got.data_ptr() == view.data_ptr()
    assert bool((out[:4] == CANARY).all()) and bool((out[-4:] == CANARY).all()), "a canary next to dst was overwritten"
    return out, view


SHAPES = [
    ((1, 1, 1, 3), "nhwc"),
    ((2, 5, 7, 3), "nhwc"),          # ragged: a row shorter than 16 pixels, one lane per row
    ((3, 8, 16, 3), "nhwc"),         # rows of exactly 16 pixels, 16-byte aligned
    ((2, 4, 48, 3), "nhwc"),         # rows of three times 16 pixels: teams of four lanes, one idle
    ((2, 9, 35, 3), "nhwc"),         # whole 16-pixel runs plus a tail; dst rows off the 16-byte grid
    ((2, 9, 13, 1), "nhwc"),
    ((2, 6, 10, 4), "nhwc"),
    ((2, 3, 8, 16), "nchw"),         # planar, C = 3
]


@pytest.mark.parametrize("shape,layout", SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_image_batch_equals_the_cpu_chain(ops, shape, layout):
    g = torch.Generator().manual_seed(sum(shape) * 1009 + shape[2])
    src = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
    N = shape[0]
    C, H, W = (shape[1], shape[2], shape[3]) if layout == "nchw" else (shape[3], shape[1], shape[2])
    table = _table(ops, C)
    calls = 0
    for size, origin in _windows(N, H, W):
        for flip in (None, [(n + 1) % 2 for n in range(N)], [n % 2 for n in range(N)]):
            want = chain(src, layout, size, origin, flip)          # once per variant, shared by the four base pointers
            assert bool(torch.isfinite(want).all())
            for shift in range(4):
                out, view = _run(ops, src, layout, shift, size, origin, flip, table)
                tag = (shape, layout, size, origin, flip, shift)
                assert torch.equal(view.cpu(), want), tag
                first = out.clone()
                _run(ops, src, layout, shift, size, origin, flip, table, out=out)          # out= reuse; the same bits
                assert torch.equal(out, first), tag
                calls += 2
    print("%s %s: %d calls" % (shape, layout, calls))


def test_out_reuse_across_different_calls(ops):
    """One dst buffer, written by calls with different parameters in turn: each result is the chain's, nothing lingers."""
    g = torch.Generator().manual_seed(5)
    src = torch.randint(0, 256, (3, 12, 40, 3), dtype=torch.uint8, generator=g)
    table, size = _table(ops, 3), (10, 32)
    out = None
    for origin, flip in (([(0, 0)] * 3, None), ([(2, 8), (1, 3), (0, 0)], [1, 0, 1]), ([(2, 0), (2, 8), (1, 5)], [0, 1, 1])):
        out, view = _run(ops, src, "nhwc", 0, size, origin, flip, table, out=out)
        assert torch.equal(view.cpu(), chain(src, "nhwc", size, origin, flip)), (origin, flip)


def test_allocated_out_and_plain_table(ops):
    g = torch.Generator().manual_seed(6)
    src = torch.randint(0, 256, (2, 6, 20, 3), dtype=torch.uint8, generator=g)
    got = ops.image_batch(src.cuda(), ops.image_table(None, None, 3).cuda())
    assert got.dtype == torch.float32 and got.is_contiguous()
    assert torch.equal(got.cpu(), src.permute(0, 3, 1, 2).float().div(255))


def test_empty_batch(ops):
    got = ops.image_batch(torch.empty(0, 8, 8, 3, dtype=torch.uint8, device="cuda"), _table(ops, 3), size=(4, 4))
    assert tuple(got.shape) == (0, 3, 4, 4) and got.is_cuda


def test_workload_shape_once(ops):
    """The workload's own shape (teams of 16 lanes, 14 pixels each, the last of four load groups half empty), flipped and not."""
    g = torch.Generator().manual_seed(7)
    src = torch.randint(0, 256, (4, 224, 224, 3), dtype=torch.uint8, generator=g)
    flip = [0, 1, 1, 0]
    _, view = _run(ops, src, "nhwc", 0, (224, 224), None, flip, _table(ops, 3))
    assert torch.equal(view.cpu(), chain(src, "nhwc", (224, 224), None, flip))


def test_offsets_past_2_31(ops):
    """A src of more than 2^31 bytes: the samples at its far end are read through 64-bit offsets (8 x 8 windows keep dst small)."""
    N, H, W = 40000, 134, 134
    assert N * H * W * 3 > 2 ** 31
    src = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
    g = torch.Generator().manual_seed(8)
    ends = {n: torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g) for n in (0, 1, N - 3, N - 2, N - 1)}
    for n, img in ends.items():
        src[n].copy_(img)
    origin = torch.stack([torch.randint(0, H - 8 + 1, (N,), generator=g), torch.randint(0, W - 8 + 1, (N,), generator=g)], 1)
    flip = torch.randint(0, 2, (N,), generator=g)
    got = ops.image_batch(src, _table(ops, 3), origin=origin, flip=flip, size=(8, 8))
    for n, img in ends.items():
        want = chain(img[None], "nhwc", (8, 8), [tuple(origin[n].tolist())], [int(flip[n])])
        assert torch.equal(got[n:n + 1].cpu(), want), n


# ------------------------------------------------------------------------------------------------ DeviceImages end to end
@pytest.fixture(scope="module")
def pair():
    from pleas_merging_amd import resnet as zoo
    from pleas_merging_amd.core.compiler import get_permutation_spec

    torch.manual_seed(0)
    m1 = zoo.tiny_resnet("bottleneck", (1, 1, 1, 1), 10, 8).eval()
    torch.manual_seed(1)
    m2 = zoo.tiny_resnet("bottleneck", (1, 1, 1, 1), 10, 8).eval()
    spec = get_permutation_spec(m1, ((2, 3, 32, 32),))
    g = torch.Generator().manual_seed(9)
    u8 = [(torch.randint(0, 256, (4, 32, 32, 3), dtype=torch.uint8, generator=g), torch.full((4,), i)) for i in range(3)]
    # the CPU chain, once, shared; made contiguous (the chain's permute leaves channels-last strides: how the entry points treat
    # strided fp32 batches is not what these tests are about)
    fp32 = [(chain(x, "nhwc", (32, 32), None, None).contiguous().cuda(), y) for x, y in u8]
    return spec, m1.cuda(), m2.cuda(), u8, fp32


def _images(loader, **kw):
    from pleas_merging_amd.methods import DeviceImages

    return DeviceImages(loader, MEAN[:3], STD[:3], "cuda", **kw)


def _kinds(u8):
    return {"pageable": u8, "pinned": [(x.pin_memory(), y) for x, y in u8], "device": [(x.cuda(), y) for x, y in u8]}


def test_device_images_yields_the_chain_and_passes_the_rest_through(pair):
    _, _, _, u8, fp32 = pair
    for kind, loader in _kinds(u8).items():
        wrapped = _images(loader)
        assert len(wrapped) == 3
        for _ in range(2):                                          # re-iterable
            got = list(wrapped)
            assert len(got) == 3
            for (x, y), (want, label) in zip(got, fp32):
                assert x.is_cuda and x.dtype == torch.float32 and torch.equal(x, want), kind
                assert y is label or torch.equal(y, label)
    mixed = [u8[0], (fp32[1][0].cpu(), fp32[1][1]), fp32[2]]         # uint8, fp32 on the host, fp32 on the device
    for (x, _), (want, _) in zip(_images(mixed), fp32):
        assert x.is_cuda and torch.equal(x, want)


def test_matching_and_bn_reset_on_uint8_loaders_equal_fp32_batches(pair):
    from pleas_merging_amd.methods import activation_matching, partial_merge, reset_bn_stats

    spec, g1, g2, u8, fp32 = pair
    want_perm, want_costs = activation_matching(spec, g1, g2, fp32, 3, output_costs=True)
    merged = partial_merge(spec, g1, g2, want_perm, want_costs, 0.5).cuda()
    assert next(merged.parameters()).is_cuda
    want_sd = reset_bn_stats(copy.deepcopy(merged), fp32, 3, backbone="hip").state_dict()
    assert any("running_var" in k for k in want_sd)
    for kind, loader in _kinds(u8).items():
        perm, costs = activation_matching(spec, g1, g2, _images(loader), 3, output_costs=True)
        for k in spec:
            assert torch.equal(costs[k], want_costs[k]), (kind, k)
            assert torch.equal(torch.as_tensor(perm[k]), torch.as_tensor(want_perm[k])), (kind, k)
        sd = reset_bn_stats(copy.deepcopy(merged), _images(loader), 3, backbone="hip").state_dict()
        for k, v in want_sd.items():
            assert not bool(torch.isnan(v.float()).any()) and torch.equal(sd[k], v), (kind, k)


def test_augmented_passes_differ_and_repeat_under_the_same_seed(pair):
    _, _, _, u8, _ = pair
    a = _images(u8, crop=(24, 24), flip=True, seed=3)
    first, second = [x for x, _ in a], [x for x, _ in a]
    assert all(tuple(x.shape) == (4, 3, 24, 24) for x in first + second)
    assert not any(torch.equal(x, y) for x, y in zip(first, second))              # epoch 1 draws differ from epoch 0
    b = _images(u8, crop=(24, 24), flip=True, seed=3)
    again_first, again_second = [x for x, _ in b], [x for x, _ in b]
    assert all(torch.equal(x, y) for x, y in zip(first, again_first))
    assert all(torch.equal(x, y) for x, y in zip(second, again_second))
    for i, (x, _) in enumerate(u8):                                               # and each is the chain under its draws
        origin, flip = b.augmentation(1, i, 4, 32, 32)
        assert torch.equal(second[i].cpu(), chain(x, "nhwc", (24, 24), origin.tolist(), flip.tolist()))
    centre = _images(u8, crop=(24, 20), seed=None)
    for (x, _), (src, _) in zip(centre, u8):
        assert torch.equal(x.cpu(), chain(src, "nhwc", (24, 20), [(4, 6)] * 4, None))
