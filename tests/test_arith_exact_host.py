"""``pleas_arith(PLEAS_ARITH_SPLIT_BF16_EXACT)``, the nine-product split-bf16 arithmetic, without a GPU: the switch itself, the
plans it builds (those of the six-product mode: same forms, variants, slabs, units) and the preconditions of the operands on
which tests/test_hip_split_exact.py tells the three arithmetics apart."""
import os
import subprocess
import sys

import pytest
import torch

import split_exact_cases as sx
import tile_cases as tc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from pleas_merging_amd import _lib

    return _lib.lib()


def test_mode_two_is_a_mode_of_its_own(lib):
    from pleas_merging_amd import hip_ops

    assert (hip_ops.ARITH_FP32, hip_ops.ARITH_SPLIT_BF16, hip_ops.ARITH_SPLIT_BF16_EXACT) == (0, 1, 2)
    assert lib.pleas_arith_get() == 0
    try:
        lib.pleas_arith(2)
        assert lib.pleas_arith_get() == 2
        lib.pleas_arith(1)
        assert lib.pleas_arith_get() == 1
        lib.pleas_arith(3)                      # anything else: fp32
        assert lib.pleas_arith_get() == 0
        lib.pleas_arith(2)
    finally:
        lib.pleas_arith(0)
    assert lib.pleas_arith_get() == 0


def test_the_context_manager_restores_the_previous_mode(lib):
    from pleas_merging_amd import hip_ops

    with hip_ops.arith(hip_ops.ARITH_SPLIT_BF16):
        with hip_ops.arith(hip_ops.ARITH_SPLIT_BF16_EXACT):
            assert lib.pleas_arith_get() == 2
        assert lib.pleas_arith_get() == 1
        with pytest.raises(hip_ops.PleasHipError):
            with hip_ops.arith(3):
                pass
        assert lib.pleas_arith_get() == 1
    assert lib.pleas_arith_get() == 0
    with pytest.raises(KeyError):
        with hip_ops.arith(2):
            raise KeyError("inside")
    assert lib.pleas_arith_get() == 0


@pytest.mark.parametrize("env,want", [({"PLEAS_ARITH": "split_bf16_exact"}, 2), ({"PLEAS_ARITH": "2"}, 2), ({"PLEAS_ARITH": "split_bf16"}, 1),
                                      ({"PLEAS_ARITH": "1"}, 1), ({"PLEAS_GRAM_SPLIT_BF16": "1"}, 1), ({"PLEAS_ARITH": "fp32"}, 0),
                                      ({"PLEAS_ARITH": "split_bf16_exactly"}, 0), ({}, 0)])
def test_initial_mode_from_the_environment(env, want):
    """A fresh child that loads the library through ctypes alone (no torch, no GPU)."""
    code = ("import ctypes, sys; lib = ctypes.CDLL(sys.argv[1]); lib.pleas_arith_get.restype = ctypes.c_int; "
            "print('ARITH', lib.pleas_arith_get())")
    from pleas_merging_amd import _lib

    clean = {k: v for k, v in os.environ.items() if k not in ("PLEAS_ARITH", "PLEAS_GRAM_SPLIT_BF16")}
    out = subprocess.run([sys.executable, "-c", code, _lib.LIB_PATH], env=dict(clean, **env), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "ARITH %d" % want in out.stdout, out.stdout


def _wgrad_plans():
    geos = [tc.wgrad_geo(c, fl | acc) for c, fl in tc.wgrad_runs() for acc in (0, tc.WG_ACC)]
    return geos, tc.wgrad_infos(geos)


def test_weight_gradient_plans_are_those_of_the_six_product_mode():
    geos, exact = _wgrad_plans()
    with tc.arith(1):
        _, six = _wgrad_plans()
    with tc.arith(2):
        _, nine = _wgrad_plans()
    assert len(geos) == len(six) == len(nine) > 100
    assert any(i["variant"] & 64 for i in six) and any(not i["variant"] & 64 for i in six)
    for geo, e, s, n in zip(geos, exact, six, nine):
        assert set(e) == set(s) == set(n)
        for field in s:
            assert n[field] == s[field], (geo, field, n, s)
            assert (n[field] != e[field]) == (s[field] != e[field]), (geo, field, n, s, e)
        assert not e["variant"] & 64


def test_forward_plans_are_those_of_the_six_product_mode():
    runs = tc.fwd_runs("fwd_batch")

    def plans():
        one = [tc.fwd_units([r]) for r in runs]                                       # a layer alone: its form
        mixed = [tc.fwd_units(runs[i::6]) for i in range(6)]                          # mixed lists: begin, count, lane per form
        timed = tc.fwd_units(tc.schedule_list(), form_ms=tc.SCHEDULE_MS)              # and the sliced schedule of measured durations
        return one, mixed, timed

    exact = plans()
    with tc.arith(1):
        six = plans()
    with tc.arith(2):
        nine = plans()
    assert nine == six
    assert six == exact          # the forward's forms, items and lanes do not depend on the arithmetic (its LDS sizes and kernels do)
    assert {u[0] for p in nine[0] for u in p} >= {4, 6, 7, 9}


# ------------------------------------------------------------------------------------------------ the crafted operands
def _emulate(c, products):
    """The dot products of a case from the plane products named in `products` ((i, j): x plane i times w plane j), in fp64."""
    px, pw = sx.planes(c["x"]), sx.planes(c["w"])
    return sum(c["op"](px[i], pw[j]) for i, j in products)


NINE = [(i, j) for i in range(3) for j in range(3)]
SIX = [p for p in NINE if p not in ((1, 2), (2, 1), (2, 2))]


@pytest.mark.parametrize("c", sx.cases(), ids=[c["name"] for c in sx.cases()])
def test_crafted_operands_hold_their_preconditions(c):
    x, w, want = c["x"], c["w"], c["want"]
    assert x.dtype == w.dtype == torch.float32 and want.dtype == torch.float64
    x1, x2, x3 = sx.planes(x)
    w1, w2, w3 = sx.planes(w)
    # the three planes sum exactly to the operand, every entry
    assert torch.equal(x1.double() + x2.double() + x3.double(), x.double())
    assert torch.equal(w1.double() + w2.double() + w3.double(), w.double())
    assert bool((w3 == 0).all()) and bool((w2.abs() <= 1).all())
    assert bool((w.abs() >= 256).all()) and bool((w.abs() < 512).all()) and torch.equal(w, w.round())
    # pairs: the contraction axis of x, flattened pairwise, holds (v, -(h1 + h2)(v)) with planes (-h1, -h2, 0)
    pairs = {"conv2d": lambda t: t.permute(0, 2, 3, 1), "wgrad": lambda t: t.permute(1, 0, 2, 3), "gram": lambda t: t.permute(1, 0, 2, 3)}[c["kind"]]
    ev, od = pairs(x).reshape(-1, 2).unbind(1)
    e1, e2, e3 = sx.planes(ev)
    o1, o2, o3 = sx.planes(od)
    assert bool(((ev.abs() >= 2 ** 17) & (ev.abs() < 2 ** 18)).all()) and torch.equal(ev, ev.round())
    assert torch.equal(od, -(e1 + e2)) and torch.equal(o1, -e1) and torch.equal(o2, -e2) and bool((o3 == 0).all())
    wev, wod = pairs(w).reshape(-1, 2).unbind(1)
    assert torch.equal(wev, wod)
    # the true result: a small integer, sum x3 * w, that fp32 holds
    assert torch.equal(want, want.round()) and float(want.abs().max()) < 2 ** 24
    assert torch.equal(want, c["op"](x3, w))
    assert torch.equal(want.float().double(), want)
    # all nine products give it, the six kept by PLEAS_ARITH_SPLIT_BF16 miss x3 * w2 in a majority of outputs
    assert torch.equal(_emulate(c, NINE), want)
    missing = c["op"](x3, w2)
    assert torch.equal(_emulate(c, SIX), want - missing)
    assert float((missing != 0).double().mean()) > 0.5, float((missing != 0).double().mean())
