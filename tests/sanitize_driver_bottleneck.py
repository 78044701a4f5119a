#!/usr/bin/env python3
"""Exercises the host half of csrc/bottleneck.hip (pleas_bottleneck_host, pleas_bottleneck_ws_bytes, the argument checks of
pleas_bottleneck_batched) under AddressSanitizer + UndefinedBehaviorSanitizer, WITHOUT a GPU.

Run by tests/test_bottleneck_host.py::test_bottleneck_host_code_under_sanitizers as

    LD_PRELOAD=<libclang_rt.asan> ASAN_OPTIONS=detect_leaks=0 python tests/sanitize_driver_bottleneck.py <libpleas_hip_asan.so>

No torch, no numpy: ctypes and the C-ABI only.  Prints SANITIZE_OK when every call returned what it should."""
import ctypes
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pleas_merging_amd import _lib  # noqa: E402  (ctypes only)

_lib.LIB_PATH = sys.argv[1]
lib = _lib.lib()


def expect(cond, what):
    if not cond:
        print("SANITIZE_DRIVER_FAILED:", what, "| last error:", lib.pleas_last_error())
        sys.exit(1)


def main():
    random.seed(0)
    for n, kind in [(1, "real"), (2, "int"), (3, "zero"), (17, "real"), (64, "int"), (130, "real"), (257, "int")]:
        for is_double in (0, 1):
            ct = ctypes.c_double if is_double else ctypes.c_float
            if kind == "real":
                vals = [random.gauss(0.0, 1.0) for _ in range(n * n)]
            elif kind == "int":
                vals = [float(random.randint(-3, 3)) for _ in range(n * n)]
            else:
                vals = [0.0 if random.random() < 0.5 else -0.0 for _ in range(n * n)]
            A = (ct * (n * n))(*vals)
            for maximize in (0, 1):
                out = (ctypes.c_int64 * n)()
                t = ctypes.c_double()
                rc = lib.pleas_bottleneck_host(A, is_double, n, maximize, out, ctypes.byref(t))
                expect(rc == 0, "host n=%d %s double=%d max=%d" % (n, kind, is_double, maximize))
                expect(sorted(out) == list(range(n)), "permutation n=%d" % n)
                got = [A[i * n + out[i]] for i in range(n)]
                expect((min(got) if maximize else max(got)) == t.value, "t n=%d" % n)
    out = (ctypes.c_int64 * 4)()
    bad = (ctypes.c_float * 4)(1, float("nan"), 3, 4)
    expect(lib.pleas_bottleneck_host(bad, 0, 2, 1, out, None) == -22, "nan refused")
    expect(lib.pleas_bottleneck_host(None, 0, 2, 1, out, None) == -22, "null refused")
    expect(lib.pleas_bottleneck_host(bad, 0, 4097, 1, out, None) == -22, "n > max refused")
    for ns in ([1], [4096, 1, 300], [2] * 200):
        arr = (ctypes.c_int * len(ns))(*ns)
        expect(lib.pleas_bottleneck_ws_bytes(arr, len(ns)) >= 4 * sum(x * x for x in ns), "ws bytes %s" % ns[:3])
    arr = (ctypes.c_int * 2)(3, 0)
    expect(lib.pleas_bottleneck_ws_bytes(arr, 2) == 0, "ws bytes of n = 0")
    one = (ctypes.c_int * 1)(4)
    ptrs = (ctypes.c_void_p * 1)(None)
    expect(lib.pleas_bottleneck_batched(ptrs, one, 1, 1, ptrs, None, None, 0, None) == -22, "null problem pointer")
    print("SANITIZE_OK")


if __name__ == "__main__":
    main()
