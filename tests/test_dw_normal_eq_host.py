"""Host side of the depthwise closed form (csrc/dw_normal_eq.hip), no GPU: the C ABI's surface, the plan builder behind
``pleas_dw_normal_eq_ws_bytes``, the argument checks (all made before anything is enqueued), the ``depthwise_closed_form`` switch,
and the per-channel Cholesky routine through ``pleas_dw_normal_eq_solve_host`` against ``torch.linalg.solve`` in fp64.

Bound of the solve: ``|w - w64|_i <= 2^-24 |w64_i| + 3 T^2 2^-53 cond_2 ||w64||_2`` -- one rounding to fp32, and Higham's bound of a
Cholesky solve in fp64; cond_2 is computed, and ``cond_2 <= 2e6`` is asserted as a condition on the inputs
(tests/dw_normal_eq_cases.py on the ridge that takes)."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depthwise_cases as dc  # noqa: E402
import dw_normal_eq_cases as nc  # noqa: E402

EINVAL, ENOMEM = -22, -12
NAMES = ("pleas_dw_normal_eq_ws_bytes", "pleas_dw_normal_eq_accum", "pleas_dw_normal_eq_solve", "pleas_dw_normal_eq_solve_host")
A = 1 << 20      # a 16-byte aligned address that is never dereferenced: every launch below is refused on the host


def _lib():
    from pleas_merging_amd import _lib

    return _lib, _lib.lib()


def _layers(cases, **over):
    _l, _ = _lib()
    arr = (_l.DwNeqLayer * len(cases))()
    for row, (N, C, H, W, K, s, p) in zip(arr, cases):
        row.N, row.C, row.Hin, row.Win, row.K, row.stride, row.pad, row.Csrc, row.n_merged = N, C, H, W, K, s, p, C, C
        for k, v in over.items():
            setattr(row, k, v)
    return arr


def test_symbols_are_exported_and_bound():
    _l, lib = _lib()
    raw = ctypes.CDLL(_l.LIB_PATH)
    for name in NAMES:
        assert name in _l.SIGNATURES and hasattr(raw, name), name
        assert getattr(lib, name).argtypes == _l.SIGNATURES[name][1], name
    # the struct as the header lays it out: 6 pointers, then 9 4-byte fields
    assert len(_l.DwNeqLayer._fields_) == 15 and ctypes.sizeof(_l.DwNeqLayer) == 6 * 8 + 9 * 4 + 4


def test_ws_bytes_answers_on_the_case_lists_and_refuses_with_a_message():
    _l, lib = _lib()
    cases = dc.CASES + nc.SPLIT_CASES
    one_by_one = [int(lib.pleas_dw_normal_eq_ws_bytes(_layers([c]), 1)) for c in cases]
    assert all(v > 0 and v % 256 == 0 for v in one_by_one), one_by_one
    whole = int(lib.pleas_dw_normal_eq_ws_bytes(_layers(cases), len(cases)))
    assert max(one_by_one) <= whole <= sum(one_by_one)
    assert int(lib.pleas_dw_normal_eq_ws_bytes(_layers(dc.CASES), len(dc.CASES))) >= max(one_by_one[:len(dc.CASES)])
    # the partials grow with the slabs (4096 output pixels of a channel each) and with the tiles (1 / 3 / 10 for K = 3 / 5 / 7)
    ws = lambda *c: int(lib.pleas_dw_normal_eq_ws_bytes(_layers([c]), 1))
    assert ws(1, 1, 64, 64, 3, 1, 1) < ws(1, 1, 64, 65, 3, 1, 1) < ws(1, 1, 91, 91, 3, 1, 1)
    assert ws(1, 1, 64, 64, 3, 1, 1) < ws(1, 1, 64, 64, 5, 1, 2) < ws(1, 1, 64, 64, 7, 1, 3)
    bad = [dict(K=4), dict(K=2), dict(K=9), dict(K=0), dict(stride=3), dict(stride=0), dict(pad=2), dict(pad=-1), dict(C=0), dict(N=0),
           dict(N=-1), dict(Hin=0), dict(Win=-3), dict(Hin=1, Win=1, pad=0), dict(N=1 << 20, C=1 << 12), dict(n_merged=6),
           dict(n_merged=-1), dict(Csrc=0)]
    for over in bad:
        assert lib.pleas_dw_normal_eq_ws_bytes(_layers([dc.CASES[0]], **over), 1) == 0, over
        assert b"invalid argument" in lib.pleas_last_error(), (over, lib.pleas_last_error())
    assert lib.pleas_dw_normal_eq_ws_bytes(None, 1) == 0 and lib.pleas_dw_normal_eq_ws_bytes(_layers([dc.CASES[0]]), 0) == 0
    # no pointer of a layer is read: every pointer above was NULL


def test_the_launch_refuses_on_the_host_before_anything_is_enqueued():
    _l, lib = _lib()
    ptrs = dict(ip=A, o1=A, o2=A, row1=A, row2=A, S=A)
    one = lambda **over: _layers([dc.CASES[0]], **dict(ptrs, **over))
    call = lambda arr, n, ws=None, nbytes=0: lib.pleas_dw_normal_eq_accum(arr, n, ws, nbytes, 1, None)
    assert call(None, 1) == EINVAL and call(one(), 0) == EINVAL
    for name in ptrs:
        assert call(one(**{name: None}), 1) == EINVAL, name
    for name in ("ip", "o1", "o2", "S"):
        assert call(one(**{name: A + 8}), 1) == EINVAL, name
    for over in (dict(n_merged=-1), dict(n_merged=6), dict(K=4), dict(K=9), dict(stride=3), dict(pad=2), dict(N=0), dict(Csrc=0)):
        assert call(one(**over), 1) == EINVAL, over
        assert lib.pleas_last_error().startswith(b"invalid argument"), over
    assert call(one(), 1, A + 4, 1 << 20) == EINVAL                       # a misaligned workspace
    every = _layers(dc.CASES, **ptrs)
    assert call(every, len(dc.CASES)) == ENOMEM                          # no workspace
    assert call(every, len(dc.CASES), A, 256) == ENOMEM                  # a short one
    assert b"workspace too small" in lib.pleas_last_error()
    # the solve's own refusals
    solve = lambda fn, **o: fn(*[dict(dict(S=A, C=4, K=3, hb=1, ridge=1e-6, w=A, bias=A, status=A), **o)[k]
                                 for k in ("S", "C", "K", "hb", "ridge", "w", "bias", "status")], None)
    for fn in (lib.pleas_dw_normal_eq_solve, lib.pleas_dw_normal_eq_solve_host):
        for over in (dict(S=None), dict(w=None), dict(status=None), dict(bias=None), dict(C=0), dict(K=2), dict(K=9), dict(ridge=-1.0),
                     dict(ridge=float("nan")), dict(S=A + 8), dict(w=A + 2)):
            assert solve(fn, **over) == EINVAL, over


def test_the_switch_default_nesting_restore_and_bad_values():
    from pleas_merging_amd import hip_ops as ops

    assert ops.DEPTHWISE_CLOSED_FORMS == ("refuse", "hip")
    if "PLEAS_DEPTHWISE_CLOSED_FORM" not in os.environ:
        assert ops.DEPTHWISE_CLOSED_FORM == "refuse"
    before = ops.DEPTHWISE_CLOSED_FORM
    with ops.depthwise_closed_form("hip"):
        assert ops.DEPTHWISE_CLOSED_FORM == "hip"
        with ops.depthwise_closed_form("refuse"):
            assert ops.DEPTHWISE_CLOSED_FORM == "refuse"
        assert ops.DEPTHWISE_CLOSED_FORM == "hip"
    assert ops.DEPTHWISE_CLOSED_FORM == before
    with pytest.raises(RuntimeError, match="boom"):
        with ops.depthwise_closed_form("hip"):
            raise RuntimeError("boom")
    assert ops.DEPTHWISE_CLOSED_FORM == before
    for bad in ("HIP", "", None, 1, "vendor"):
        with pytest.raises(ValueError):
            with ops.depthwise_closed_form(bad):
                pytest.fail("entered the block")
        assert ops.DEPTHWISE_CLOSED_FORM == before


@pytest.mark.parametrize("has_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("K", nc.SOLVE_KS)
def test_solve_host_against_fp64(K, has_bias):
    from pleas_merging_amd import hip_ops

    S, w0, b0, w64, cond = nc.solve_case(K, has_bias)
    w, b = w0.clone(), b0.clone()
    status = hip_ops.dw_normal_eq_solve_host(S, K, has_bias, nc.SOLVE_RIDGE, w, b if has_bias else None)
    worst = nc.check_solution(K, has_bias, w, b, status, w0, b0, w64, cond)
    print("K = %d, bias %s: worst error %.3g of its bound; cond_2 up to %.3g" % (K, has_bias, worst, float(cond[cond < float("inf")].max())))
    # the wrapper's own refusals
    from pleas_merging_amd._lib import PleasHipError

    for bad in (lambda: hip_ops.dw_normal_eq_solve_host(S.float(), K, has_bias, 1e-6, w, b),
                lambda: hip_ops.dw_normal_eq_solve_host(S[:, :-1], K, has_bias, 1e-6, w, b),
                lambda: hip_ops.dw_normal_eq_solve_host(S, K, has_bias, 1e-6, w.double(), b),
                lambda: hip_ops.dw_normal_eq_solve_host(S, K, True, 1e-6, w, None),
                lambda: hip_ops.dw_normal_eq_solve(S, K, has_bias, 1e-6, w, b)):            # host tensors to the device entry
        with pytest.raises(PleasHipError):
            bad()
