"""The cases of tests/golden/minimax_small.npz rebuilt as fp32 matrices, and the documented A_hat (numpy only).  Shared by
tests/test_bottleneck_host.py and tests/test_hip_bottleneck.py."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def seeded_matrix(n, kind, seed):
    """tests/golden/make_golden_minimax.py's larger cases, rebuilt from their seed."""
    rng = np.random.default_rng(seed)
    if kind == "normal":
        return rng.standard_normal((n, n)).astype(np.float32)
    return rng.integers(-20, 20, (n, n)).astype(np.float32)


def load_cases(max_n=None):
    """[(name, A fp32 in the direction the reference solved, t*, reference permutation)]."""
    z = np.load(os.path.join(GOLDEN, "minimax_small.npz"))
    lap = np.load(os.path.join(GOLDEN, "lap_small.npz"))
    cases = []
    for name in z["names"].tolist():
        parts = name.split("_")
        if parts[0] == "lap":
            A = lap["cost_%s" % parts[1]].astype(np.float32)
            A = A if parts[2] == "pos" else -A
        else:
            n = int(parts[1])
            if max_n is not None and n > max_n:
                continue
            A = seeded_matrix(n, parts[2], int(z[name + "/seed"]))
        cases.append((name, A, np.float32(z[name + "/t"]), z[name + "/perm"]))
    return cases


def floor_bound(t, M, m, n):
    """L32 of the contract: L = t - (n (M - m) + max(1, |t|)) in fp64, rounded toward -inf to fp32."""
    L = float(t) - (n * (float(M) - float(m)) + max(1.0, abs(float(t))))
    f = np.float32(L)
    if float(f) > L:
        f = np.nextafter(f, np.float32(-np.inf))
    return f


def masked(A, t):
    """A_hat: every entry below t replaced by L32 (A in the maximize direction)."""
    L32 = floor_bound(t, A.max(), A.min(), A.shape[0])
    assert np.isfinite(L32)
    return np.where(A >= t, A, L32).astype(A.dtype)
