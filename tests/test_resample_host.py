"""Host side of the resampling path (no GPU): the exported symbols and their bindings, every refusal of the plan builder and of
the wrappers, ``pleas_image_resample_host`` bit for bit against PIL -- the committed fixture tests/golden/resample_pil.npz
(written by tests/golden/make_golden_resample.py) and, where PIL imports, the two PIL chains run live on fresh geometries --
the stand-alone sanitizer check of csrc/resample_plan.hpp, and the box / flip draws of ``DeviceImages``.  Every comparison is
equality."""
import ctypes
import os
import subprocess
import zlib

import numpy as np
import pytest
import torch

import resample_cases as rc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406, 0.45), (0.229, 0.224, 0.225, 0.25)
EINVAL, ENOMEM = -22, -12
OK_GEOM = [8, 6, 1, 1, 5, 4, 4, 4, 0, 0]      # an 8 x 6 image, the box (1, 1, 5, 4) to 4 x 4


@pytest.fixture(scope="module")
def lib():
    from pleas_merging_amd import _lib, build

    build.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def ops():
    from pleas_merging_amd import hip_ops

    return hip_ops


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "resample_pil.npz"))


def test_symbols_are_exported_and_bound(lib):
    from pleas_merging_amd import _lib

    want = {"pleas_resample_plan_bytes": (ctypes.c_size_t, 4), "pleas_resample_plan": (ctypes.c_int, 9),
            "pleas_resample_plan_info": (ctypes.c_int, 3), "pleas_image_resample_host": (ctypes.c_int, 7),
            "pleas_image_resample": (ctypes.c_int, 10)}
    for name, (restype, nargs) in want.items():
        assert name in _lib.SIGNATURES, name
        got_restype, argtypes = _lib.SIGNATURES[name]
        assert got_restype is restype and len(argtypes) == nargs, name
        assert getattr(lib, name).argtypes == argtypes


# ------------------------------------------------------------------------------------------------ refusals of the C ABI
def _plan(lib, geom=OK_GEOM, offset=0, N=1, C=3, Ho=4, Wo=4, src_bytes=8 * 6 * 3, plan_bytes=None, null=()):
    g = (ctypes.c_int32 * len(geom))(*geom)
    o = (ctypes.c_int64 * 1)(offset)
    buf = (ctypes.c_int32 * 16384)()
    rc_ = lib.pleas_resample_plan(None if "geom" in null else g, None if "offset" in null else o, N, C, Ho, Wo, src_bytes,
                                  None if "plan" in null else buf, len(buf) * 4 if plan_bytes is None else plan_bytes)
    return rc_, buf


def _geom(**kw):
    names = ["H", "W", "y0", "x0", "h", "w", "Hv", "Wv", "oy", "ox"]
    g = list(OK_GEOM)
    for k, v in kw.items():
        g[names.index(k)] = v
    return g


BAD_PLANS = [
    dict(geom=_geom(y0=4)), dict(geom=_geom(x0=3)), dict(geom=_geom(y0=-1)), dict(geom=_geom(x0=-1)),          # the box and its image
    dict(geom=_geom(h=0)), dict(geom=_geom(w=0)), dict(geom=_geom(h=9, y0=0)),
    dict(geom=_geom(oy=1)), dict(geom=_geom(ox=1)), dict(geom=_geom(oy=-1)), dict(geom=_geom(Hv=3)),              # the window and its output
    dict(geom=_geom(Wv=0)), dict(geom=_geom(H=0)), dict(geom=_geom(W=-3)),                                        # sizes
    dict(geom=_geom(H=16385), src_bytes=16385 * 6 * 3), dict(geom=_geom(W=16385), src_bytes=16385 * 8 * 3),
    dict(geom=_geom(Hv=16385)), dict(geom=_geom(Wv=16385)),
    dict(Ho=0), dict(Wo=0), dict(Ho=-1), dict(Ho=16385, geom=_geom(Hv=16384)),
    dict(C=0), dict(C=5), dict(N=-1),
    dict(src_bytes=8 * 6 * 3 - 1), dict(offset=1), dict(offset=-1), dict(src_bytes=-1),                           # the source buffer
    dict(plan_bytes=64), dict(plan_bytes=0), dict(null=("plan",)), dict(null=("geom",)), dict(null=("offset",)),
]


@pytest.mark.parametrize("bad", BAD_PLANS, ids=lambda b: ",".join("%s=%s" % kv for kv in b.items())[:60])
def test_plan_refuses(lib, bad):
    rc_, buf = _plan(lib, **bad)
    assert rc_ == EINVAL
    assert b"invalid argument" in lib.pleas_last_error()
    if "plan" not in bad.get("null", ()) and bad.get("plan_bytes", 64) >= 64:
        assert buf[0] == 0                                             # no magic word: nothing a launch would accept


def test_plan_bytes_and_info(lib):
    g = (ctypes.c_int32 * 10)(*OK_GEOM)
    n = lib.pleas_resample_plan_bytes(g, 1, 4, 4)
    assert n > 0 and n % 4 == 0
    rc_, buf = _plan(lib, plan_bytes=n)                                # exactly the bytes asked for
    assert rc_ == 0
    assert _plan(lib, plan_bytes=n - 4)[0] == EINVAL
    info = (ctypes.c_int64 * 8)()
    assert lib.pleas_resample_plan_info(buf, n, info) == 0
    assert list(info)[:5] == [1, 3, 4, 4, 8 * 6 * 3] and info[5] > 0 and info[6] >= 1 and info[7] >= 1
    assert lib.pleas_resample_plan_info(buf, n - 4, info) == EINVAL    # the plan is longer than the bytes handed over
    assert lib.pleas_resample_plan_bytes((ctypes.c_int32 * 10)(*_geom(y0=4)), 1, 4, 4) == 0
    assert b"box" in lib.pleas_last_error()
    assert lib.pleas_resample_plan_bytes(None, 0, 4, 4) > 0            # an empty batch has a plan: its header


def test_launch_refuses_on_the_host_copy(lib):
    """``pleas_image_resample`` checks the host copy of the plan, the pointers and the workspace before it enqueues: every call
    here is refused (or is the empty batch), so the fake addresses are never dereferenced and no device is touched."""
    P = 4096
    rc_, buf = _plan(lib)
    assert rc_ == 0
    n = lib.pleas_resample_plan_bytes((ctypes.c_int32 * 10)(*OK_GEOM), 1, 4, 4)
    info = (ctypes.c_int64 * 8)()
    assert lib.pleas_resample_plan_info(buf, n, info) == 0
    ws = info[5]

    def call(src=P, plan_dev=P, plan=buf, plan_bytes=n, lut=P, dst=P, w=P, ws_bytes=ws):
        return lib.pleas_image_resample(src, plan_dev, plan, plan_bytes, lut, None, dst, w, ws_bytes, None)

    for kw in (dict(src=None), dict(plan_dev=None), dict(lut=None), dict(dst=None), dict(plan=None), dict(plan_bytes=n - 4),
               dict(plan_bytes=8), dict(dst=P + 4), dict(dst=P + 8), dict(plan_dev=P + 2)):
        assert call(**kw) == EINVAL, kw
        assert b"invalid argument" in lib.pleas_last_error()
    assert call(ws_bytes=ws - 1) == ENOMEM and call(w=None) == ENOMEM
    assert str(ws).encode() in lib.pleas_last_error()
    buf[0] ^= 1                                                        # not a plan any more
    assert call() == EINVAL
    empty = (ctypes.c_int32 * 64)()
    assert lib.pleas_resample_plan(None, None, 0, 3, 4, 4, 0, empty, 256) == 0
    assert lib.pleas_image_resample(None, None, empty, 256, None, None, None, None, 0, None) == 0      # N == 0: nothing to do
    assert lib.pleas_image_resample_host(None, empty, 256, None, None, None, None) == 0


def test_wrapper_refusals(ops):
    from pleas_merging_amd._lib import PleasHipError

    table = ops.image_table(MEAN[:3], STD[:3], 3)
    src = torch.zeros(8 * 6 * 3, dtype=torch.uint8)
    plan = ops.image_resample_plan([OK_GEOM], [0], 3, (4, 4), src.numel())
    assert plan.dtype == torch.uint8 and plan.numel() == ops.image_resample_plan_bytes([OK_GEOM], (4, 4))
    info = ops.image_resample_plan_info(plan)
    assert (info["n"], info["channels"], info["size"], info["src_bytes"]) == (1, 3, (4, 4), 144)
    with pytest.raises(PleasHipError, match="box"):
        ops.image_resample_plan([_geom(y0=4)], [0], 3, (4, 4), 144)
    with pytest.raises(PleasHipError, match="window"):
        ops.image_resample_plan([_geom(oy=1)], [0], 3, (4, 4), 144)
    with pytest.raises(PleasHipError, match="source buffer"):
        ops.image_resample_plan([OK_GEOM], [1], 3, (4, 4), 144)
    with pytest.raises(PleasHipError, match="16384"):
        ops.image_resample_plan([_geom(W=16385)], [0], 3, (4, 4), 16385 * 8 * 3)
    with pytest.raises(PleasHipError, match="C must"):
        ops.image_resample_plan([OK_GEOM], [0], 5, (4, 4), 144)
    with pytest.raises(PleasHipError, match="shape"):
        ops.image_resample_plan([OK_GEOM[:9]], [0], 3, (4, 4), 144)
    with pytest.raises(PleasHipError, match="integers"):
        ops.image_resample_plan(torch.tensor([OK_GEOM]).float(), [0], 3, (4, 4), 144)
    with pytest.raises(PleasHipError, match="src_offset"):
        ops.image_resample_plan([OK_GEOM], [0, 0], 3, (4, 4), 144)
    with pytest.raises(PleasHipError, match="out must"):
        ops.image_resample_plan([OK_GEOM], [0], 3, (4, 4), 144, out=torch.zeros(16, dtype=torch.uint8))
    with pytest.raises(PleasHipError, match="uint8"):                       # a wrong dtype
        ops.image_resample(src.float(), plan, plan, table)
    with pytest.raises(PleasHipError, match="contiguous"):
        ops.image_resample(torch.zeros(288, dtype=torch.uint8)[::2], plan, plan, table)
    with pytest.raises(PleasHipError, match="144"):                         # fewer bytes than the plan was built for
        ops.image_resample(src[:100], plan, plan, table)
    with pytest.raises(PleasHipError, match="flip"):
        ops.image_resample(src, plan, plan, table, flip=[1, 0])
    with pytest.raises(PleasHipError, match="out must be"):                 # a CPU out
        ops.image_resample(src, plan, plan, table, out=torch.empty(1, 3, 4, 4))
    with pytest.raises(PleasHipError, match="host plan"):
        ops.image_resample(src, plan, plan.view(torch.int32), table)
    with pytest.raises(PleasHipError, match="no CPU fallback"):             # legal arguments, but on the host: still no fallback
        ops.image_resample(src, plan, plan, table, flip=[1])
    with pytest.raises(PleasHipError, match="table"):
        ops.image_resample_host(src, plan, ops.image_table(None, None, 4))
    damaged = plan.clone()
    damaged[0] ^= 1
    with pytest.raises(PleasHipError, match="not a plan"):
        ops.image_resample_host(src, damaged, table)


# ------------------------------------------------------------------------------------------------ the arithmetic against PIL
def _execute(ops, geoms, srcs, channels, size, flip=None, mean=None, std=None, gap=0):
    """Pack ``srcs`` (uint8 [H, W, C] arrays) ``gap`` bytes apart, plan and execute on the host."""
    offsets, at = [], gap
    for s in srcs:
        offsets.append(at)
        at += s.size + gap
    buf = torch.zeros(at, dtype=torch.uint8)
    for s, o in zip(srcs, offsets):
        buf[o:o + s.size] = torch.from_numpy(np.ascontiguousarray(s).reshape(-1))
    plan = ops.image_resample_plan(geoms, offsets, channels, size, buf.numel())
    table = ops.image_table(mean, std, channels)
    f32, u8 = ops.image_resample_host(buf, plan, table, flip=flip)
    return f32, u8, table


def _through_table(table, u8):
    """``table[c][v]`` of uint8 [N, Ho, Wo, C] bytes as fp32 [N, C, Ho, Wo]."""
    planes = [table[c][u8[..., c].long()] for c in range(u8.shape[-1])]
    return torch.stack(planes, 1)


@pytest.mark.parametrize("channels", rc.CHANNELS)
@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c[0])
def test_host_executor_equals_the_pil_fixture(ops, golden, case, channels):
    for fill in rc.FILLS:
        k = rc.key(case, channels, fill)
        src = rc.source(case, channels, fill)
        assert zlib.crc32(src.tobytes()) == int(golden[k + "/src_crc"]), "the seeded input is not the one the fixture was made from"
        geom = rc.geom_row(case)
        assert geom == golden[k + "/geom"].tolist()
        want = torch.from_numpy(golden[k + "/want"])
        f32, u8, table = _execute(ops, [geom], [src], channels, case[3:5], mean=MEAN[:channels], std=STD[:channels])
        assert torch.equal(u8[0], want), k
        assert torch.equal(f32, _through_table(table, want[None])), k
        f32, u8, table = _execute(ops, [geom], [src], channels, case[3:5], flip=[1])      # the flip mirrors the output row
        assert torch.equal(u8[0], want.flip(1)), k
        assert torch.equal(f32, _through_table(table, want.flip(1)[None])), k


def test_host_executor_on_a_ragged_batch_equals_the_fixture(ops, golden):
    """Samples of different sizes in one plan, packed 3 bytes apart (no offset a multiple of 4), some flipped."""
    for cases, flip in (([c for c in rc.CASES if c[0] in ("eval_tall", "eval_wide")], [0, 1]),):
        for channels in rc.CHANNELS:
            srcs = [rc.source(c, channels, "random") for c in cases]
            geoms = [rc.geom_row(c) for c in cases]
            _, u8, _ = _execute(ops, geoms, srcs, channels, (20, 20), flip=flip, gap=3)
            for i, c in enumerate(cases):
                want = torch.from_numpy(golden[rc.key(c, channels, "random") + "/want"])
                assert torch.equal(u8[i], want.flip(1) if flip[i] else want), (c[0], channels)


def test_host_executor_equals_pil_live(ops):
    """Where PIL imports: both chains on fresh seeded geometries, mixed into ragged batches.  (The fixture above is what the
    suite rests on; this widens it on machines that have PIL.)"""
    pytest.importorskip("PIL")
    rng = np.random.RandomState(20)
    for trial in range(24):
        channels = int(rng.choice(rc.CHANNELS))
        Ho, Wo = int(rng.randint(1, 40)), int(rng.randint(1, 40))
        geoms, srcs = [], []
        for s in range(4):
            H, W = int(rng.randint(1, 120)), int(rng.randint(1, 120))
            srcs.append(rng.randint(0, 256, (H, W, channels)).astype(np.uint8))
            if (trial + s) % 2:
                h, w = int(rng.randint(1, H + 1)), int(rng.randint(1, W + 1))
                geoms.append([H, W, int(rng.randint(0, H - h + 1)), int(rng.randint(0, W - w + 1)), h, w, Ho, Wo, 0, 0])
            else:
                Hv, Wv = Ho + int(rng.randint(0, 25)), Wo + int(rng.randint(0, 25))
                geoms.append([H, W, 0, 0, H, W, Hv, Wv, int(rng.randint(0, Hv - Ho + 1)), int(rng.randint(0, Wv - Wo + 1))])
        _, u8, _ = _execute(ops, geoms, srcs, channels, (Ho, Wo), gap=trial % 4)
        for i in range(4):
            assert np.array_equal(u8[i].numpy(), rc.pil_chain(srcs[i], geoms[i], Ho, Wo)), (trial, geoms[i])
    # the drivers' own shapes once: RandomResizedCrop(224)-like and Resize(256) + CenterCrop(224) on 375 x 500
    src = rng.randint(0, 256, (375, 500, 3)).astype(np.uint8)
    Hv, Wv = rc.resized_size(375, 500, 256)
    for geom in ([375, 500, 40, 100, 200, 260, 224, 224, 0, 0], [375, 500, 0, 0, 375, 500, Hv, Wv, (Hv - 224) // 2, int(round((Wv - 224) / 2.0))]):
        _, u8, _ = _execute(ops, [geom], [src], 3, (224, 224))
        assert np.array_equal(u8[0].numpy(), rc.pil_chain(src, geom, 224, 224)), geom


# ------------------------------------------------------------------------------------------------ the plan code under sanitizers
def test_plan_code_under_sanitizers(tmp_path):
    """csrc/resample_plan.hpp -- plan builder, header check, host executor -- compiled into the stand-alone program
    tests/resample_plan_check.cpp with AddressSanitizer + UndefinedBehaviorSanitizer and run as a child process."""
    from pleas_merging_amd import build

    exe = str(tmp_path / "resample_plan_check")
    cmd = [build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I" + build.CSRC, os.path.join(REPO, "tests", "resample_plan_check.cpp"), "-o", exe]      # host code only: a C++ program, no device code at all
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stderr[-4000:]
    assert "__asan_init" in subprocess.check_output(["nm", exe], text=True)            # the program really is instrumented
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "RESAMPLE_PLAN_OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]


# ------------------------------------------------------------------------------------------------ draws
def _images(loader=(), **kw):
    from pleas_merging_amd.methods import DeviceImages

    return DeviceImages(loader, MEAN[:3], STD[:3], "cpu", **kw)


SIZES = [(37, 53), (300, 17), (1, 1), (20, 31), (375, 500), (64, 64)]


def test_invalid_combinations_raise_at_construction():
    for kw in (dict(resized_crop=(16, 16), resize=24), dict(resized_crop=(16, 16), crop=(8, 8)), dict(resized_crop=(16, 16), seed=None),
               dict(resize=24), dict(resize=0, crop=(8, 8)), dict(resized_crop=(16, 16), scale=(0.5, 0.1)),
               dict(resized_crop=(16, 16), ratio=(0.0, 1.0))):
        with pytest.raises(ValueError):
            _images(**kw)
    with pytest.raises(ValueError, match="mixed sizes"):                  # a ragged batch needs a common output size
        _images(crop=(8, 8)).ragged_augmentation(0, 0, SIZES)
    with pytest.raises(ValueError, match="does not fit"):                 # Resize(24) of 300 x 17 is 423 x 24: no 32-wide window
        _images(resize=24, crop=(20, 32), seed=None).ragged_augmentation(0, 0, [(300, 17)])


def test_box_draws_repeat_per_seed_epoch_batch_and_stay_inside():
    a, b = _images(resized_crop=(16, 12), flip=True, seed=3), _images(resized_crop=(16, 12), flip=True, seed=3)
    seen = {}
    for epoch in range(2):
        for index in range(3):
            g, f = a.ragged_augmentation(epoch, index, SIZES)
            g2, f2 = b.ragged_augmentation(epoch, index, SIZES)
            assert torch.equal(g, g2) and torch.equal(f, f2)
            assert g.dtype == torch.int32 and tuple(g.shape) == (len(SIZES), 10) and f.dtype == torch.uint8
            for (H, W), row in zip(SIZES, g.tolist()):
                h_, w_, y0, x0, h, w, Hv, Wv, oy, ox = row
                assert (h_, w_, Hv, Wv, oy, ox) == (H, W, 16, 12, 0, 0)
                assert h >= 1 and w >= 1 and 0 <= y0 and y0 + h <= H and 0 <= x0 and x0 + w <= W
            seen[epoch, index] = g
    keys = list(seen)
    for i, k in enumerate(keys):
        for k2 in keys[i + 1:]:
            assert not torch.equal(seen[k], seen[k2]), (k, k2)
    assert not torch.equal(_images(resized_crop=(16, 12), seed=4).ragged_augmentation(0, 0, SIZES)[0], seen[0, 0])
    # the box of a sample depends on the samples before it only through the generator: a prefix of the sizes draws a prefix
    assert torch.equal(a.ragged_augmentation(0, 0, SIZES[:3])[0], seen[0, 0][:3])
    # default scale and ratio: the areas spread over (0.08, 1) of the image
    g, _ = a.ragged_augmentation(0, 0, [(375, 500)] * 64)
    area = (g[:, 4] * g[:, 5]).double() / (375 * 500)
    assert 0.07 < float(area.min()) < 0.3 and 0.7 < float(area.max()) <= 1.0


def test_fallback_box_is_the_centred_clamped_one():
    """``scale=(1, 1)`` asks for the whole area at a ratio the image does not have: all ten attempts fail."""
    d = _images(resized_crop=(16, 16), seed=3, ratio=(1.0, 1.0), scale=(1.0, 1.0))
    g, f = d.ragged_augmentation(0, 0, [(300, 17), (10, 40), (8, 8)])
    assert f is None
    assert g[:, 2:6].tolist() == [[141, 0, 17, 17], [0, 15, 10, 10], [0, 0, 8, 8]]
    d = _images(resized_crop=(16, 16), seed=3, ratio=(3 / 4, 4 / 3), scale=(1.0, 1.0))
    g, _ = d.ragged_augmentation(5, 1, [(300, 17), (10, 40)])
    assert g[:, 2:6].tolist() == [[(300 - 23) // 2, 0, int(round(17 / 0.75)), 17], [0, (40 - 13) // 2, 10, int(round(10 * 4 / 3))]]


def test_resize_window_is_the_centre_one():
    for seed in (None, 5):
        g, f = _images(resize=24, crop=(20, 20), seed=seed).ragged_augmentation(2, 1, [(50, 37), (31, 64), (24, 24)])
        assert f is None
        assert g.tolist() == [rc.geom_row(rc.CASES[8]), rc.geom_row(rc.CASES[9]), [24, 24, 0, 0, 24, 24, 24, 24, 2, 2]]
    g, f = _images(resize=24, crop=(20, 20), seed=5, flip=True).ragged_augmentation(0, 0, [(50, 37)] * 32)
    assert 0 < int(f.sum()) < 32


def test_existing_crop_and_flip_draws_are_unchanged():
    """Values recorded on the commit before the resampling path was added."""
    d = _images(crop=(24, 20), flip=True, seed=7)
    o, f = d.augmentation(0, 0, 6, 32, 32)
    assert o.tolist() == [[3, 6], [3, 8], [8, 5], [7, 10], [6, 0], [6, 3]] and f.tolist() == [1, 1, 0, 0, 1, 1]
    o, f = d.augmentation(1, 2, 6, 32, 32)
    assert o.tolist() == [[5, 10], [6, 1], [5, 8], [2, 1], [5, 5], [2, 4]] and f.tolist() == [1, 0, 1, 0, 1, 0]
    assert _images(flip=True, seed=1).augmentation(0, 0, 8, 32, 32)[1].tolist() == [1, 0, 0, 0, 1, 1, 1, 1]


def test_ragged_collate_keeps_images_apart_and_stacks_the_rest():
    import pleas.methods
    from pleas_merging_amd.methods import ragged_collate

    assert pleas.methods.ragged_collate is ragged_collate
    samples = [(torch.zeros(5, 7, 3, dtype=torch.uint8), 1, torch.ones(2)), (np.zeros((4, 9), dtype=np.uint8), 2, torch.zeros(2))]
    images, labels, extra = ragged_collate(samples)
    assert isinstance(images, list) and [tuple(i.shape) for i in images] == [(5, 7, 3), (4, 9, 1)]
    assert all(i.dtype == torch.uint8 for i in images)
    assert labels.tolist() == [1, 2] and tuple(extra.shape) == (2, 2)
    (images,) = ragged_collate([torch.zeros(2, 2, 1, dtype=torch.uint8)])
    assert len(images) == 1
