"""Bottleneck ("minimax") assignment without a GPU: the reference's solver restated (scipy_solve_minimax_assignment),
the library's host entry point (pleas_bottleneck_host) against the documented contract, its argument checks, and its
host code under ASan + UBSan."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bottleneck_cases import load_cases, masked  # noqa: E402

CASES = load_cases()


def _bits(x):
    return np.float32(x).view(np.uint32)


def test_scipy_minimax_is_the_reference_permutation():
    from pleas.core.solvers import scipy_solve_minimax_assignment

    for name, A, t, perm in CASES:
        got = scipy_solve_minimax_assignment(torch.from_numpy(A))
        assert got.dtype == torch.int64 and got.device.type == "cpu", name
        assert np.array_equal(got.numpy(), perm), name


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_host_minimax_meets_the_contract(dtype):
    from pleas.core.solvers import host_solve_minimax_assignment

    for name, A, t, _ in CASES:
        n = A.shape[0]
        for maximize in (True, False):
            X = torch.from_numpy(A if maximize else -A).to(dtype)   # the case's direction is maximize on A
            p = host_solve_minimax_assignment(X, maximize=maximize)
            assert p.dtype == torch.int64 and sorted(p.tolist()) == list(range(n)), name
            got_t = np.float32(A[np.arange(n), p.numpy()].min()) + np.float32(0)
            assert _bits(got_t) == _bits(t), (name, maximize, got_t, t)
            _, want = linear_sum_assignment(masked(A, t), maximize=True)
            assert np.array_equal(p.numpy(), want), (name, maximize)


def test_host_minimax_refuses_device_tensors_and_bad_shapes():
    from pleas_merging_amd._lib import PleasHipError
    from pleas.core.solvers import host_solve_minimax_assignment

    with pytest.raises(PleasHipError):
        host_solve_minimax_assignment(torch.zeros(3, 4))
    with pytest.raises(PleasHipError):
        host_solve_minimax_assignment(torch.full((2, 2), float("nan")))
    with pytest.raises(PleasHipError):
        host_solve_minimax_assignment(torch.zeros(4097, 4097))


def test_host_minimax_is_the_reference_t_on_ties():
    """All-equal and integer-tied matrices: t* is the reference's, and -0 counts as +0."""
    from pleas.core.solvers import host_solve_minimax_assignment, scipy_solve_minimax_assignment

    A = torch.tensor([[0.0, -0.0, -1.0], [-0.0, -2.0, 0.0], [-3.0, 0.0, -0.0]])
    p = host_solve_minimax_assignment(A)
    r = scipy_solve_minimax_assignment(A)
    assert float(A[torch.arange(3), p].min()) == float(A[torch.arange(3), r].min()) == 0.0


def test_bottleneck_argument_checks():
    from pleas_merging_amd import _lib

    lib = _lib.lib()
    out = (ctypes.c_int64 * 4)()
    good = (ctypes.c_float * 4)(1, 2, 3, 4)
    assert lib.pleas_bottleneck_host(good, 0, 2, 1, out, None) == 0
    assert lib.pleas_bottleneck_host(None, 0, 2, 1, out, None) == -22
    assert lib.pleas_bottleneck_host(good, 0, 2, 1, None, None) == -22
    assert lib.pleas_bottleneck_host(good, 0, 0, 1, out, None) == -22
    assert lib.pleas_bottleneck_host(good, 0, -3, 1, out, None) == -22
    assert lib.pleas_bottleneck_host(good, 0, _lib.LSAP_MAX_N + 1, 1, out, None) == -22
    for bad in (float("nan"), float("inf"), float("-inf")):
        m = (ctypes.c_float * 4)(1, 2, bad, 4)
        assert lib.pleas_bottleneck_host(m, 0, 2, 1, out, None) == -22
        assert lib.pleas_bottleneck_host(m, 0, 2, 0, out, None) == -22
    huge = (ctypes.c_float * 4)(3e38, -3e38, -3e38, 3e38)          # L32 below -FLT_MAX
    assert lib.pleas_bottleneck_host(huge, 0, 2, 1, out, None) == -22
    t = ctypes.c_double()
    assert lib.pleas_bottleneck_host(good, 0, 2, 1, out, ctypes.byref(t)) == 0 and t.value == 2.0   # [[1,2],[3,4]]: 2 / 3
    assert list(out[:2]) == [1, 0]
    assert lib.pleas_bottleneck_host(good, 0, 2, 0, out, ctypes.byref(t)) == 0 and t.value == 3.0
    ns = (ctypes.c_int * 2)(4, 5)
    assert lib.pleas_bottleneck_ws_bytes(ns, 2) >= 4 * (16 + 25)
    bad_ns = (ctypes.c_int * 2)(4, _lib.LSAP_MAX_N + 1)
    assert lib.pleas_bottleneck_ws_bytes(bad_ns, 2) == 0
    assert lib.pleas_bottleneck_ws_bytes(None, 2) == 0
    ptrs = (ctypes.c_void_p * 1)(None)
    one = (ctypes.c_int * 1)(4)
    assert lib.pleas_bottleneck_batched(None, one, 1, 1, ptrs, None, None, 0, None) == -22
    assert lib.pleas_bottleneck_batched(ptrs, one, 1, 1, ptrs, None, None, 0, None) == -22    # null problem pointers
    assert lib.pleas_bottleneck_batched(ptrs, one, -1, 1, ptrs, None, None, 0, None) == -22
    assert lib.pleas_bottleneck_batched(ptrs, one, 0, 1, ptrs, None, None, 0, None) == 0
    fake = (ctypes.c_void_p * 1)(0x1000)
    zero = (ctypes.c_int * 1)(0)
    assert lib.pleas_bottleneck_batched(fake, zero, 1, 1, fake, None, fake[0], 1 << 20, None) == -22      # n < 1
    assert lib.pleas_bottleneck_batched(fake, one, 1, 1, fake, None, None, 1 << 20, None) == -22         # no workspace
    assert lib.pleas_bottleneck_batched(fake, one, 1, 1, fake, None, fake[0], 8, None) == -22            # too small


def test_bottleneck_host_code_under_sanitizers():
    """pleas_bottleneck_host, the workspace sizing and the argument checks under -fsanitize=address,undefined
    (tests/sanitize_driver_bottleneck.py, a torch-free subprocess with the ASan runtime preloaded)."""
    from pleas_merging_amd import build

    lib = build.build_sanitized()
    preload = " ".join(p for p in (build.asan_runtime(), os.environ.get("LD_PRELOAD", "")) if p)
    env = dict(os.environ, LD_PRELOAD=preload, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([sys.executable, os.path.join(REPO, "tests", "sanitize_driver_bottleneck.py"), lib], env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "SANITIZE_OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
