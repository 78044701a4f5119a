"""Host side of the Linear forward (``pleas_linear_fwd``, csrc/linear.hip) and of ``pleas_column_sum``: the exported symbols, the
split-K plan as pure arithmetic, the argument checks that answer before anything is enqueued, the wrappers' validation and the
``linear_form`` switch.  No GPU: no call here reaches a launch."""
import ctypes

import pytest
import torch

OK, EINVAL, ENOMEM = 0, -22, -12
TILE, CHUNK = 64, 32
GRID_N = [1, 63, 64, 65, 257, 4096]
GRID_C = [1, 63, 64, 65, 200, 1000, 21841]
GRID_K = [0, 1, 31, 32, 33, 2048, 4099]
FAKE = 1 << 20                  # a non-null "device pointer" for calls that must be refused before they touch memory


@pytest.fixture(scope="module")
def lib():
    from pleas_merging_amd import _lib

    return _lib.lib()


@pytest.fixture(scope="module")
def ops():
    from pleas_merging_amd import hip_ops

    return hip_ops


def _plan(lib, N, C, K):
    info = (ctypes.c_int * 5)(*[-1] * 5)
    assert lib.pleas_linear_plan_info(N, C, K, info) == OK
    return tuple(info)


def test_the_four_symbols_are_exported_and_bound(lib):
    from pleas_merging_amd import _lib

    for name in ("pleas_linear_fwd", "pleas_linear_ws_bytes", "pleas_linear_plan_info", "pleas_column_sum"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.pleas_linear_ws_bytes.restype is ctypes.c_size_t


@pytest.mark.parametrize("N", GRID_N)
def test_plan_tiles_and_k_ranges(lib, ops, N):
    for C in GRID_C:
        for K in GRID_K:
            tiles_n, tiles_c, S, per, last = plan = _plan(lib, N, C, K)
            what = (N, C, K, plan)
            assert tiles_n == -(-N // TILE) and tiles_c == -(-C // TILE), what
            chunks = -(-K // CHUNK)
            assert S >= 1 and (S - 1) * per + last == chunks, what           # ranges 0 .. S-2 of `per` chunks, then `last`: every chunk once
            if chunks:
                assert 1 <= last <= per, what                                # no range is empty
            else:
                assert (S, per, last) == (1, 0, 0), what
            ws = lib.pleas_linear_ws_bytes(N, C, K)
            assert ws == 0 if S == 1 else ws >= S * N * C * 4, what
            assert _plan(lib, N, C, K) == plan and lib.pleas_linear_ws_bytes(N, C, K) == ws      # a pure function of (N, C, K)
            assert ops.linear_plan_info(N, C, K) == plan


def test_plan_splits_k_for_the_heads_shapes_and_not_for_many_tiles(lib):
    """D = 2048, C = 200 at batch 64 / 256 gives 4 / 16 tiles: K is split.  342 class tiles fill the device by themselves."""
    for N in (64, 256):
        assert _plan(lib, N, 200, 2048)[2] > 1
    assert _plan(lib, 4, 21841, 64)[2] == 1


def test_argument_checks_answer_without_a_gpu(lib):
    fwd = lambda x, w, y, N, C, K, ws, nbytes: lib.pleas_linear_fwd(x, w, None, y, N, C, K, ws, nbytes, None)
    N, C, K = 64, 200, 2048
    need = lib.pleas_linear_ws_bytes(N, C, K)
    assert need > 0
    for x, w, y in ((None, FAKE, FAKE), (FAKE, None, FAKE), (FAKE, FAKE, None)):
        assert fwd(x, w, y, N, C, K, FAKE, need) == EINVAL
    for n, c, k in ((-1, C, K), (N, -1, K), (N, C, -1)):
        assert fwd(FAKE, FAKE, FAKE, n, c, k, FAKE, need) == EINVAL
        assert lib.pleas_linear_plan_info(n, c, k, (ctypes.c_int * 5)()) == EINVAL
        assert lib.pleas_linear_ws_bytes(n, c, k) == 0
    assert fwd(FAKE, FAKE, FAKE, N, C, K, FAKE, need - 1) == ENOMEM          # one byte short
    assert b"%d" % need in lib.pleas_last_error()
    assert fwd(FAKE, FAKE, FAKE, N, C, K, None, need) == ENOMEM
    assert fwd(FAKE, FAKE, FAKE, 0, C, K, None, 0) == OK                      # N == 0: nothing to do, nothing enqueued
    assert lib.pleas_linear_plan_info(N, C, K, None) == EINVAL
    # tensors of 2^30 elements or more: x, w, y in turn
    for n, c, k in ((1 << 20, 8, 1 << 10), (8, 1 << 20, 1 << 10), (1 << 15, 1 << 15, 8)):
        assert fwd(FAKE, FAKE, FAKE, n, c, k, FAKE, 1 << 40) == EINVAL
    col = lambda x, N, C, out: lib.pleas_column_sum(x, N, C, out, None)
    assert col(None, 4, 4, FAKE) == EINVAL and col(FAKE, 4, 4, None) == EINVAL
    assert col(FAKE, -1, 4, FAKE) == EINVAL and col(FAKE, 4, -1, FAKE) == EINVAL and col(FAKE, 0, 4, FAKE) == EINVAL
    assert col(FAKE, 1 << 20, 1 << 10, FAKE) == EINVAL


@pytest.mark.parametrize("form", ["conv", "gemm"])
def test_wrappers_refuse_cpu_tensors(ops, form):
    x, w, b = torch.randn(4, 8), torch.randn(3, 8), torch.randn(3)
    with ops.linear_form(form):
        for args in ((x, w), (x, w, b), (x, w, None, torch.empty(4, 3))):
            with pytest.raises(ops.PleasHipError):
                ops.linear(*args)
    with pytest.raises(ops.PleasHipError):
        ops.column_sum(torch.randn(4, 3), torch.empty(3))


class _OnGpu:
    """Lets the wrappers' validation be walked without a device: a CPU tensor that claims to be on the GPU.  Every malformed
    argument must be refused before ``data_ptr`` is taken, i.e. before the library is called."""

    def __init__(self, t, device="cuda:0"):
        self._t, self._device = t, torch.device(device)

    is_cuda = True

    @property
    def device(self):
        return self._device

    def data_ptr(self):
        raise AssertionError("a malformed argument reached the library")

    def __getattr__(self, name):
        return getattr(self._t, name)


def _bad_linear_args():
    x, w = torch.randn(4, 8), torch.randn(3, 8)
    g = _OnGpu
    yield "x 3-D", (g(torch.randn(4, 8, 1)), g(w))
    yield "w 1-D", (g(x), g(torch.randn(8)))
    yield "K differs", (g(x), g(torch.randn(3, 7)))
    yield "w not contiguous", (g(x), g(torch.randn(8, 3).t()))
    yield "x fp64", (g(x.double()), g(w))
    yield "w on another device", (g(x), g(w, "cuda:1"))
    yield "bias of C + 1 elements", (g(x), g(w), g(torch.randn(4)))
    yield "bias fp64", (g(x), g(w), g(torch.randn(3).double()))
    yield "bias strided", (g(x), g(w), g(torch.randn(6)[::2]))
    yield "bias on the CPU", (g(x), g(w), torch.randn(3))
    yield "out of shape (C, N)", (g(x), g(w), None, g(torch.empty(3, 4)))
    yield "out fp64", (g(x), g(w), None, g(torch.empty(4, 3).double()))
    yield "out not contiguous", (g(x), g(w), None, g(torch.empty(3, 4).t()))
    yield "out flat", (g(x), g(w), None, g(torch.empty(12)))
    yield "out on the CPU", (g(x), g(w), None, torch.empty(4, 3))


@pytest.mark.parametrize("form", ["conv", "gemm"])
def test_linear_refuses_every_malformed_argument_before_the_library(ops, form):
    with ops.linear_form(form):
        for what, args in _bad_linear_args():
            with pytest.raises(ops.PleasHipError):
                ops.linear(*args)
                pytest.fail(what)


def test_column_sum_refuses_malformed_arguments(ops):
    g = _OnGpu
    x = torch.randn(4, 3)
    for what, args in (("x 3-D", (g(torch.randn(4, 3, 1)), g(torch.empty(3)))), ("x strided", (g(torch.randn(3, 4).t()), g(torch.empty(3)))),
                       ("x empty", (g(x[:0]), g(torch.empty(3)))), ("x fp64", (g(x.double()), g(torch.empty(3)))),
                       ("out of N elements", (g(x), g(torch.empty(4)))), ("out fp64", (g(x), g(torch.empty(3).double()))),
                       ("out strided", (g(x), g(torch.empty(6)[::2]))), ("out on the CPU", (g(x), torch.empty(3)))):
        with pytest.raises(ops.PleasHipError):
            ops.column_sum(*args)
            pytest.fail(what)


def test_linear_form_default_nesting_restore_and_bad_values(ops):
    import os

    assert ops.LINEAR_FORMS == ("conv", "gemm")
    if "PLEAS_LINEAR" not in os.environ:
        assert ops.LINEAR == "conv"
    before = ops.LINEAR
    with ops.linear_form("gemm"):
        assert ops.LINEAR == "gemm"
        with ops.linear_form("conv"):
            assert ops.LINEAR == "conv"
            with ops.linear_form("gemm"):
                assert ops.LINEAR == "gemm"
            assert ops.LINEAR == "conv"
        assert ops.LINEAR == "gemm"
    assert ops.LINEAR == before
    with pytest.raises(RuntimeError, match="boom"):
        with ops.linear_form("gemm"):
            raise RuntimeError("boom")
    assert ops.LINEAR == before
    for bad in ("GEMM", "", None, 1, "vendor"):
        with pytest.raises(ValueError):
            with ops.linear_form(bad):
                pytest.fail("entered the block")
        assert ops.LINEAR == before
    # the environment variable is read when the module is imported; a bad value is refused there
    assert ops._linear_form_checked("gemm") == "gemm"
    with pytest.raises(ValueError):
        ops._linear_form_checked("nope")


def test_the_default_form_follows_the_environment_variable():
    """A fresh interpreter per value (the variable is read at import): ``PLEAS_LINEAR`` overrides the default, a bad value raises."""
    import os
    import subprocess
    import sys

    code = "from pleas_merging_amd import hip_ops; print(hip_ops.LINEAR)"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for value, want in (("gemm", "gemm"), ("nope", None)):
        env = {k: v for k, v in os.environ.items() if k != "PLEAS_LINEAR"}
        if value is not None:
            env["PLEAS_LINEAR"] = value
        p = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True)
        if want is None:
            assert p.returncode != 0 and "ValueError" in p.stderr, p.stderr
        else:
            assert p.returncode == 0 and p.stdout.strip() == want, (p.stdout, p.stderr)
