"""Host side of the chain resampling path (no GPU): the exported symbols and their bindings, every refusal of the chain plan
builder and of the wrappers, ``pleas_image_resample_chain_host`` bit for bit against PIL -- the committed fixture
tests/golden/resample_chain_pil.npz (written by tests/golden/make_golden_resample_chain.py): final bytes, the image between the
two resizes, and the fp32 output through a table --, the stand-alone sanitizer check of the chain code in csrc/resample_plan.hpp,
and the box / flip draws of ``DeviceImages(pre_resize=...)``.  Every comparison is equality.

``DeviceImages`` has no CPU path for resampled batches (its copies go through the "h2d" stream), with one stage or with two, so
the wrapper's end-to-end run is in tests/test_hip_resample_chain.py."""
import ctypes
import os
import subprocess
import zlib

import numpy as np
import pytest
import torch

import resample_chain_cases as cc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406, 0.45), (0.229, 0.224, 0.225, 0.25)
EINVAL, ENOMEM = -22, -12
CHAIN_MAGIC = 0x48435250
OK_GEOM = [8, 6, 12, 9, 1, 1, 5, 4]      # an 8 x 6 image resized to 12 x 9, its box (1, 1, 5, 4) to 4 x 4
NAMES = ["H", "W", "H1", "W1", "y0", "x0", "h", "w"]


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
    return np.load(os.path.join(REPO, "tests", "golden", "resample_chain_pil.npz"))


def test_symbols_are_exported_and_bound(lib, ops):
    from pleas_merging_amd import _lib

    want = {"pleas_resample_chain_plan_bytes": (ctypes.c_size_t, 4), "pleas_resample_chain_plan": (ctypes.c_int, 9),
            "pleas_resample_chain_plan_info": (ctypes.c_int, 3), "pleas_image_resample_chain_host": (ctypes.c_int, 8),
            "pleas_image_resample_chain": (ctypes.c_int, 10)}
    for name, (restype, nargs) in want.items():
        assert name in _lib.SIGNATURES, name
        got_restype, argtypes = _lib.SIGNATURES[name]
        assert got_restype is restype and len(argtypes) == nargs, name
        assert getattr(lib, name).argtypes == argtypes
    assert ops.RESAMPLE_CHAIN_GEOM == 8
    header = open(os.path.join(REPO, "include", "pleas_hip.h")).read()
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in want:
        assert name + "(" in header and name in integration, name


# ------------------------------------------------------------------------------------------------ refusals of the C ABI
def _plan(lib, geom=OK_GEOM, offset=0, N=1, C=3, Ho=4, Wo=4, src_bytes=8 * 6 * 3, plan_bytes=None, null=()):
    g = (ctypes.c_int32 * len(geom))(*geom)
    o = (ctypes.c_int64 * 1)(offset)
    buf = (ctypes.c_int32 * 16384)()
    buf[0] = CHAIN_MAGIC                                               # a refusal must take it away
    rc_ = lib.pleas_resample_chain_plan(None if "geom" in null else g, None if "offset" in null else o, N, C, Ho, Wo, src_bytes,
                                        None if "plan" in null else buf, len(buf) * 4 if plan_bytes is None else plan_bytes)
    return rc_, buf


def _geom(**kw):
    g = list(OK_GEOM)
    for k, v in kw.items():
        g[NAMES.index(k)] = v
    return g


BAD_PLANS = [
    dict(geom=_geom(y0=8)), dict(geom=_geom(x0=6)), dict(geom=_geom(y0=-1)), dict(geom=_geom(x0=-1)),             # a box outside H1 x W1
    dict(geom=_geom(h=13, y0=0)), dict(geom=_geom(w=10, x0=0)), dict(geom=_geom(H1=5)), dict(geom=_geom(W1=4)),
    dict(geom=_geom(h=0)), dict(geom=_geom(w=0)), dict(geom=_geom(H=0)), dict(geom=_geom(W=-3)),                  # non-positive sizes
    dict(geom=_geom(H1=0)), dict(geom=_geom(W1=0)), dict(Ho=0), dict(Wo=0), dict(Ho=-1),
    dict(geom=_geom(H=16385), src_bytes=16385 * 6 * 3), dict(geom=_geom(W=16385), src_bytes=16385 * 8 * 3),        # sides above 16384
    dict(geom=_geom(H1=16385)), dict(geom=_geom(W1=16385)), dict(Ho=16385), dict(Wo=16385),
    dict(C=0), dict(C=5), dict(N=-1),
    dict(src_bytes=8 * 6 * 3 - 1), dict(offset=1), dict(offset=-1), dict(src_bytes=-1),                           # the source buffer
    dict(plan_bytes=96), dict(plan_bytes=0), dict(null=("plan",)), dict(null=("geom",)), dict(null=("offset",)),  # plan memory
]


@pytest.mark.parametrize("bad", BAD_PLANS, ids=lambda b: ",".join("%s=%s" % kv for kv in b.items())[:60])
def test_plan_refuses(lib, bad):
    rc_, buf = _plan(lib, **bad)
    assert rc_ == EINVAL
    assert b"invalid argument" in lib.pleas_last_error()
    if "plan" not in bad.get("null", ()) and bad.get("plan_bytes", 96) >= 96:
        assert buf[0] == 0                                             # no magic word: nothing a launch would accept


def test_plan_memory_must_be_aligned(lib):
    g, o = (ctypes.c_int32 * 8)(*OK_GEOM), (ctypes.c_int64 * 1)(0)
    buf = (ctypes.c_int32 * 16384)()
    assert lib.pleas_resample_chain_plan(g, o, 1, 3, 4, 4, 144, ctypes.addressof(buf) + 2, 65000) == EINVAL
    assert b"aligned" in lib.pleas_last_error()


def test_plan_bytes_and_info(lib):
    g = (ctypes.c_int32 * 8)(*OK_GEOM)
    n = lib.pleas_resample_chain_plan_bytes(g, 1, 4, 4)
    assert n > 0 and n % 4 == 0
    rc_, buf = _plan(lib, plan_bytes=n)                                # exactly the bytes asked for
    assert rc_ == 0 and buf[0] == CHAIN_MAGIC
    assert _plan(lib, plan_bytes=n - 4)[0] == EINVAL
    info = (ctypes.c_int64 * 11)()
    assert lib.pleas_resample_chain_plan_info(buf, n, info) == 0
    assert list(info)[:5] == [1, 3, 4, 4, 8 * 6 * 3] and info[6] == 5 * 4 * 3 and list(info)[7:] == [1, 1, 1, 1]
    assert info[5] >= info[6] + 2 * 16                                 # two scratches and the intermediate
    assert lib.pleas_resample_chain_plan_info(buf, n - 4, info) == EINVAL    # the plan is longer than the bytes handed over
    assert lib.pleas_resample_chain_plan_info(buf, n, None) == EINVAL
    assert lib.pleas_resample_chain_plan_bytes((ctypes.c_int32 * 8)(*_geom(y0=8)), 1, 4, 4) == 0
    assert b"box" in lib.pleas_last_error()
    assert lib.pleas_resample_chain_plan_bytes(None, 0, 4, 4) > 0      # an empty batch has a plan: its headers


def test_launch_refuses_on_the_host_copy(lib):
    """``pleas_image_resample_chain`` checks the host copy of the plan, the pointers and the workspace before it enqueues: every
    call here is refused (or is the empty batch), so the fake addresses are never dereferenced and no device is touched."""
    P = 4096
    rc_, buf = _plan(lib)
    assert rc_ == 0
    n = lib.pleas_resample_chain_plan_bytes((ctypes.c_int32 * 8)(*OK_GEOM), 1, 4, 4)
    info = (ctypes.c_int64 * 11)()
    assert lib.pleas_resample_chain_plan_info(buf, n, info) == 0
    ws = info[5]

    def call(src=P, plan_dev=P, plan=buf, plan_bytes=n, lut=P, dst=P, w=P, ws_bytes=ws):
        return lib.pleas_image_resample_chain(src, plan_dev, plan, plan_bytes, lut, None, dst, w, ws_bytes, None)

    for kw in (dict(src=None), dict(plan_dev=None), dict(lut=None), dict(dst=None), dict(plan=None), dict(plan_bytes=n - 4),
               dict(plan_bytes=8), dict(dst=P + 4), dict(dst=P + 8), dict(plan_dev=P + 2)):
        assert call(**kw) == EINVAL, kw
        assert b"invalid argument" in lib.pleas_last_error()
    assert call(ws_bytes=ws - 1) == ENOMEM and call(w=None) == ENOMEM
    assert str(ws).encode() in lib.pleas_last_error()
    # damaged headers: the chain's, the stage-1 section's, the stage-2 plan's
    for word in (0, 9, 10, 11, 12, 24, 24 + 9, buf[11], buf[11] + 3):
        keep = buf[word]
        buf[word] ^= 1
        assert call() == EINVAL, word
        assert lib.pleas_image_resample_chain_host(P, buf, n, P, None, P, None, None) == EINVAL, word
        buf[word] = keep
    single = (ctypes.c_int32 * 16384)()                                # a single-stage plan is not a chain plan, nor the reverse
    g10 = (ctypes.c_int32 * 10)(8, 6, 1, 1, 5, 4, 4, 4, 0, 0)
    assert lib.pleas_resample_plan(g10, (ctypes.c_int64 * 1)(0), 1, 3, 4, 4, 144, single, 65536) == 0
    assert call(plan=single, plan_bytes=65536) == EINVAL
    assert lib.pleas_image_resample(P, P, buf, n, P, None, P, P, 1 << 20, None) == EINVAL
    empty = (ctypes.c_int32 * 128)()
    assert lib.pleas_resample_chain_plan(None, None, 0, 3, 4, 4, 0, empty, 512) == 0
    assert lib.pleas_image_resample_chain(None, None, empty, 512, None, None, None, None, 0, None) == 0      # N == 0: nothing to do
    assert lib.pleas_image_resample_chain_host(None, empty, 512, None, None, None, None, None) == 0


def test_wrapper_refusals(ops):
    from pleas_merging_amd._lib import PleasHipError

    table = ops.image_table(MEAN[:3], STD[:3], 3)
    src = torch.zeros(8 * 6 * 3, dtype=torch.uint8)
    plan = ops.image_resample_chain_plan([OK_GEOM], [0], 3, (4, 4), src.numel())
    assert plan.dtype == torch.uint8 and plan.numel() == ops.image_resample_chain_plan_bytes([OK_GEOM], (4, 4))
    info = ops.image_resample_chain_plan_info(plan)
    assert (info["n"], info["channels"], info["size"], info["src_bytes"], info["mid_bytes"]) == (1, 3, (4, 4), 144, 60)
    assert info["items"] == (1, 1, 1, 1)
    with pytest.raises(PleasHipError, match="box"):
        ops.image_resample_chain_plan([_geom(y0=8)], [0], 3, (4, 4), 144)
    with pytest.raises(PleasHipError, match="source buffer"):
        ops.image_resample_chain_plan([OK_GEOM], [1], 3, (4, 4), 144)
    with pytest.raises(PleasHipError, match="16384"):
        ops.image_resample_chain_plan([_geom(W1=16385)], [0], 3, (4, 4), 144)
    with pytest.raises(PleasHipError, match="C must"):
        ops.image_resample_chain_plan([OK_GEOM], [0], 5, (4, 4), 144)
    with pytest.raises(PleasHipError, match="shape"):
        ops.image_resample_chain_plan([OK_GEOM + [0, 0]], [0], 3, (4, 4), 144)      # a single-stage descriptor
    with pytest.raises(PleasHipError, match="integers"):
        ops.image_resample_chain_plan(torch.tensor([OK_GEOM]).float(), [0], 3, (4, 4), 144)
    with pytest.raises(PleasHipError, match="src_offset"):
        ops.image_resample_chain_plan([OK_GEOM], [0, 0], 3, (4, 4), 144)
    with pytest.raises(PleasHipError, match="out must"):
        ops.image_resample_chain_plan([OK_GEOM], [0], 3, (4, 4), 144, out=torch.zeros(16, dtype=torch.uint8))
    with pytest.raises(PleasHipError, match="uint8"):                       # a wrong dtype
        ops.image_resample_chain(src.float(), plan, plan, table)
    with pytest.raises(PleasHipError, match="contiguous"):
        ops.image_resample_chain(torch.zeros(288, dtype=torch.uint8)[::2], plan, plan, table)
    with pytest.raises(PleasHipError, match="144"):                         # fewer bytes than the plan was built for
        ops.image_resample_chain(src[:100], plan, plan, table)
    with pytest.raises(PleasHipError, match="flip"):
        ops.image_resample_chain(src, plan, plan, table, flip=[1, 0])
    with pytest.raises(PleasHipError, match="out must be"):                 # a CPU out
        ops.image_resample_chain(src, plan, plan, table, out=torch.empty(1, 3, 4, 4))
    with pytest.raises(PleasHipError, match="host plan"):
        ops.image_resample_chain(src, plan, plan.view(torch.int32), table)
    with pytest.raises(PleasHipError, match="no CPU fallback"):             # legal arguments, but on the host: still no fallback
        ops.image_resample_chain(src, plan, plan, table, flip=[1])
    with pytest.raises(PleasHipError, match="table"):
        ops.image_resample_chain_host(src, plan, ops.image_table(None, None, 4))
    damaged = plan.clone()
    damaged[0] ^= 1
    with pytest.raises(PleasHipError, match="not a chain plan"):
        ops.image_resample_chain_host(src, damaged, table)
    single = ops.image_resample_plan([[8, 6, 1, 1, 5, 4, 4, 4, 0, 0]], [0], 3, (4, 4), 144)
    with pytest.raises(PleasHipError, match="not a chain plan"):
        ops.image_resample_chain_host(src, single, table)
    with pytest.raises(PleasHipError, match="not a plan"):
        ops.image_resample_host(src, plan, table)


# ------------------------------------------------------------------------------------------------ the arithmetic against PIL
def _pack(srcs, gap):
    offsets, at = [], gap
    for s in srcs:
        offsets.append(at)
        at += s.size + gap
    buf = torch.zeros(at, dtype=torch.uint8)
    for s, o in zip(srcs, offsets):
        buf[o:o + s.size] = torch.from_numpy(np.ascontiguousarray(s).reshape(-1))
    return buf, offsets


def _execute(ops, geoms, srcs, channels, size, flip=None, gap=0):
    """Pack ``srcs`` (uint8 [H, W, C] arrays) ``gap`` bytes apart, plan and execute on the host; the intermediate comes back as
    one ``[h, w, C]`` tensor per sample."""
    buf, offsets = _pack(srcs, gap)
    plan = ops.image_resample_chain_plan(geoms, offsets, channels, size, buf.numel())
    table = ops.image_table(MEAN[:channels], STD[:channels], channels)
    f32, u8, mid = ops.image_resample_chain_host(buf, plan, table, flip=flip)
    mids, at = [], 0
    for g in geoms:
        nb = g[6] * g[7] * channels
        mids.append(mid[at:at + nb].view(g[6], g[7], channels))
        at += nb
    assert at == mid.numel()
    return f32, u8, mids, table


def _through_table(table, u8):
    """``table[c][v]`` of uint8 [N, Ho, Wo, C] bytes as fp32 [N, C, Ho, Wo]."""
    return torch.stack([table[c][u8[..., c].long()] for c in range(u8.shape[-1])], 1)


@pytest.mark.parametrize("flip", [0, 1], ids=["plain", "flipped"])
@pytest.mark.parametrize("channels", cc.CHANNELS)
@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c[0])
def test_host_executor_equals_the_pil_fixture_one_case_alone(ops, golden, case, channels, flip):
    for fill in cc.FILLS:
        k = cc.key(case, channels, fill)
        src = cc.source(case, channels, fill)
        assert zlib.crc32(src.tobytes()) == int(golden[k + "/src_crc"]), "the seeded input is not the one the fixture was made from"
        geom = cc.geom_row(case)
        assert geom == golden[k + "/geom"].tolist()
        want = torch.from_numpy(golden[k + "/want"])
        want = want.flip(1) if flip else want                          # the flip mirrors the output row, not the intermediate
        f32, u8, mids, table = _execute(ops, [geom], [src], channels, case[5:7], flip=[flip] if flip else None, gap=flip)
        assert torch.equal(mids[0], torch.from_numpy(golden[k + "/mid"])), k
        assert torch.equal(u8[0], want), k
        assert torch.equal(f32, _through_table(table, want[None])), k


@pytest.mark.parametrize("flipped", [False, True], ids=["plain", "flipped"])
@pytest.mark.parametrize("channels", cc.CHANNELS)
def test_host_executor_on_a_ragged_batch_of_all_cases_equals_the_fixture(ops, golden, channels, flipped):
    """Every case of a channel count in one plan, packed 3 bytes apart (no offset a multiple of 4), at the batch's common size."""
    for fill in cc.FILLS:
        srcs = [cc.source(c, channels, fill) for c in cc.CASES]
        geoms = [cc.geom_row(c) for c in cc.CASES]
        flip = [i % 2 for i in range(len(cc.CASES))] if flipped else None
        f32, u8, mids, table = _execute(ops, geoms, srcs, channels, cc.BATCH_SIZE, flip=flip, gap=3)
        for i, c in enumerate(cc.CASES):
            k = cc.key(c, channels, fill)
            want = torch.from_numpy(golden[k + "/want_batch"])
            want = want.flip(1) if flip and flip[i] else want
            assert torch.equal(mids[i], torch.from_numpy(golden[k + "/mid"])), k
            assert torch.equal(u8[i], want), k
            assert torch.equal(f32[i], _through_table(table, want[None])[0]), k


@pytest.mark.parametrize("channels", cc.CHANNELS)
def test_an_unchanged_first_stage_is_the_single_stage_resized_crop(ops, channels):
    case = next(c for c in cc.CASES if c[0] == "id")
    H, W, H1, W1, y0, x0, h, w = cc.geom_row(case)
    assert (H1, W1) == (H, W)
    for fill in cc.FILLS:
        src = cc.source(case, channels, fill)
        f32, u8, mids, table = _execute(ops, [cc.geom_row(case)], [src], channels, case[5:7], flip=[1])
        buf = torch.from_numpy(src.reshape(-1).copy())
        plan = ops.image_resample_plan([[H, W, y0, x0, h, w, case[5], case[6], 0, 0]], [0], channels, case[5:7], buf.numel())
        f32_single, u8_single = ops.image_resample_host(buf, plan, table, flip=[1])
        assert torch.equal(f32, f32_single) and torch.equal(u8, u8_single)
        assert torch.equal(mids[0], torch.from_numpy(src[y0:y0 + h, x0:x0 + w].copy()))      # the identity resize copies its box


def test_plan_is_a_pure_function_and_position_independent(ops):
    srcs = [cc.source(c, 3, "random") for c in cc.CASES]
    geoms = [cc.geom_row(c) for c in cc.CASES]
    buf, offsets = _pack(srcs, 1)
    nbytes = ops.image_resample_chain_plan_bytes(geoms, cc.BATCH_SIZE)
    a = ops.image_resample_chain_plan(geoms, offsets, 3, cc.BATCH_SIZE, buf.numel(), out=torch.full((nbytes,), 0xAA, dtype=torch.uint8))
    b = ops.image_resample_chain_plan(geoms, offsets, 3, cc.BATCH_SIZE, buf.numel(), out=torch.full((nbytes + 64,), 0x55, dtype=torch.uint8))
    assert a.numel() == nbytes and torch.equal(a, b)
    table = ops.image_table(MEAN[:3], STD[:3], 3)
    want = ops.image_resample_chain_host(buf, a, table, flip=[1, 0] * 3 + [1])
    room = torch.zeros(nbytes + 4 * 37, dtype=torch.uint8)
    moved = room[4 * 37:]                                              # the same bytes at another address
    moved.copy_(a)
    a.fill_(0)                                                         # nothing may point back into the first copy
    assert moved.data_ptr() != a.data_ptr()
    got = ops.image_resample_chain_host(buf, moved, table, flip=[1, 0] * 3 + [1])
    assert all(torch.equal(x, y) for x, y in zip(got, want))


# ------------------------------------------------------------------------------------------------ the plan code under sanitizers
def test_chain_plan_code_under_sanitizers(tmp_path):
    """The chain code of csrc/resample_plan.hpp -- plan builder, header check, host executor -- compiled into the stand-alone
    program tests/resample_chain_check.cpp with AddressSanitizer + UndefinedBehaviorSanitizer and run as a child process."""
    from pleas_merging_amd import build

    exe = str(tmp_path / "resample_chain_check")
    cmd = [build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I" + build.CSRC, os.path.join(REPO, "tests", "resample_chain_check.cpp"), "-o", exe]      # host code only: a C++ program, no device code at all
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stderr[-4000:]
    assert "__asan_init" in subprocess.check_output(["nm", exe], text=True)            # the program really is instrumented
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "RESAMPLE_CHAIN_OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]


# ------------------------------------------------------------------------------------------------ draws
def _images(loader=(), **kw):
    from pleas_merging_amd.methods import DeviceImages

    return DeviceImages(loader, MEAN[:3], STD[:3], "cpu", **kw)


SIZES = [(37, 53), (300, 17), (1, 1), (20, 31), (375, 500), (64, 64)]


def test_invalid_combinations_raise_at_construction():
    for kw in (dict(pre_resize=24), dict(pre_resize=24, resize=24, crop=(8, 8)), dict(pre_resize=24, crop=(8, 8)),      # no resized_crop
               dict(pre_resize=0, resized_crop=(16, 16)), dict(pre_resize=-3, resized_crop=(16, 16)),
               dict(pre_resize=24, resized_crop=(16, 16), resize=24), dict(pre_resize=24, resized_crop=(16, 16), crop=(8, 8)),
               dict(pre_resize=24, resized_crop=(16, 16), seed=None)):
        with pytest.raises(ValueError):
            _images(**kw)
    with pytest.raises(ValueError, match="pre_resize"):                   # without the first stage there is no chain to draw for
        _images(resized_crop=(16, 16)).chain_augmentation(0, 0, SIZES)
    assert _images(pre_resize=24, resized_crop=(16, 16)).pre_resize == 24 and _images(resized_crop=(16, 16)).pre_resize is None


def test_chain_draws_repeat_per_seed_epoch_batch_and_stay_inside_the_resized_image():
    a, b = (_images(pre_resize=24, resized_crop=(16, 12), flip=True, seed=3) for _ in range(2))
    seen = {}
    for epoch in range(2):
        for index in range(3):
            g, f = a.chain_augmentation(epoch, index, SIZES)
            g2, f2 = b.chain_augmentation(epoch, index, SIZES)
            assert torch.equal(g, g2) and torch.equal(f, f2)
            assert g.dtype == torch.int32 and tuple(g.shape) == (len(SIZES), 8) and f.dtype == torch.uint8 and tuple(f.shape) == (len(SIZES),)
            for (H, W), row in zip(SIZES, g.tolist()):
                h_, w_, H1, W1, y0, x0, h, w = row
                assert (h_, w_) == (H, W) and (H1, W1) == cc.resized_size(H, W, 24)
                assert h >= 1 and w >= 1 and 0 <= y0 and y0 + h <= H1 and 0 <= x0 and x0 + w <= W1
            seen[epoch, index] = g
    keys = list(seen)
    for i, k in enumerate(keys):
        for k2 in keys[i + 1:]:
            assert not torch.equal(seen[k], seen[k2]), (k, k2)
    assert not torch.equal(_images(pre_resize=24, resized_crop=(16, 12), seed=4).chain_augmentation(0, 0, SIZES)[0], seen[0, 0])
    assert _images(pre_resize=24, resized_crop=(16, 12), seed=3).chain_augmentation(0, 0, SIZES)[1] is None      # no flip, no flags
    # ragged_augmentation is what it was: boxes on the images themselves
    g10, _ = a.ragged_augmentation(0, 0, SIZES)
    assert torch.equal(g10, _images(resized_crop=(16, 12), flip=True, seed=3).ragged_augmentation(0, 0, SIZES)[0])


def test_chain_draws_come_in_torchvisions_order():
    """A restatement: all boxes, sample after sample on ``(H1, W1)``, then all flags, from the one generator of ``(seed, epoch,
    batch index)`` -- the order ``Resize -> RandomResizedCrop -> RandomHorizontalFlip`` consumes a generator in."""
    import math

    d = _images(pre_resize=24, resized_crop=(16, 12), flip=True, seed=5, scale=(0.08, 1.0))
    for epoch, index in ((0, 0), (1, 2)):
        g = d._generator(epoch, index)
        rows = []
        for H, W in SIZES:
            H1, W1 = cc.resized_size(H, W, 24)
            box = None
            for _ in range(10):
                target = H1 * W1 * torch.empty(1).uniform_(0.08, 1.0, generator=g).item()
                aspect = math.exp(torch.empty(1).uniform_(math.log(3 / 4), math.log(4 / 3), generator=g).item())
                w, h = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
                if 0 < w <= W1 and 0 < h <= H1:
                    y0 = int(torch.randint(0, H1 - h + 1, (1,), generator=g).item())
                    box = (y0, int(torch.randint(0, W1 - w + 1, (1,), generator=g).item()), h, w)
                    break
            if box is None:
                w, h = W1, H1
                if W1 / H1 < 3 / 4:
                    h = min(H1, max(1, int(round(W1 / (3 / 4)))))
                elif W1 / H1 > 4 / 3:
                    w = min(W1, max(1, int(round(H1 * (4 / 3)))))
                box = ((H1 - h) // 2, (W1 - w) // 2, h, w)
            rows.append([H, W, H1, W1] + list(box))
        flags = (torch.rand(len(SIZES), generator=g) < 0.5).to(torch.uint8)
        got, got_flags = d.chain_augmentation(epoch, index, SIZES)
        assert got.tolist() == rows and torch.equal(got_flags, flags)
