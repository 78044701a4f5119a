"""The coverage ledger of the tile forms (no GPU): every form of the convolution forward and of the weight gradient that a
caller's geometry can reach has a case in tests/tile_cases.py, for each entry point, with the edges that go wrong in a tile.

Which form a geometry gets is decided by thresholds in ``fwd_describe`` (csrc/conv_fwd.hip) and ``build_wgrad_plan``
(csrc/conv.hip) that move from round to round.  Both sides of the comparison are therefore ASKED of the built library, through
its host-only plan queries: the set of reachable forms (a sweep over a grid of geometries) and the form of every case.  A
threshold that moves a case off its form, or a new form without a case, fails here, on a machine without a GPU, and the
printed ledger (``pytest -s``, or the captured output of a failure) shows which.

Reference semantics of the operations themselves: pleas/methods/pleas_merging.py:281-287 (layer forward, MSE, backward)."""
import pytest

import tile_cases as tc

# A reachable combination may only be left out if no tensor under 256 MB reaches it: by name, with the reason; at most two.
EXCLUSIONS = {}          # {(entry point, key): reason}

FWD_TRAITS = ("ragged_cout", "ragged_pixels", "straddles_samples", "bias")
KXK_ONLY_FORMS = (6, 9)        # k x k flat forms: every case has k > 1; the general forms 0-3 take k x k layers too


@pytest.fixture(scope="module", params=[0, 1], ids=["fp32", "split_bf16"])
def mode(request):
    with tc.arith(request.param):
        yield request.param


def _fwd_ledger(entry):
    ledger = {}
    for case, kp in tc.fwd_runs(entry):
        form = tc.fwd_form(case, kp)
        ledger.setdefault((form, kp), []).append((case, tc.fwd_traits(case, kp, form)))
    return ledger


def test_forward_table_reaches_every_reachable_form(mode):
    reach = tc.reachable_fwd()
    assert {f for f, _ in reach} == set(range(10)), "the grid itself no longer reaches all ten forms: %r" % sorted(reach)
    for entry in tc.FWD_ENTRY_POINTS:
        ledger = _fwd_ledger(entry)
        print("\n%s, pleas_arith(%d): form (kernel-position-major) -> cases" % (entry, mode))
        for key in sorted(set(ledger) | reach):
            print("  form %d%s: %s" % (key[0], " kpos" if key[1] else "", [c for c, _ in ledger.get(key, [])] or "NO CASE"))
        missing = [k for k in sorted(reach) if k not in ledger and (entry, k) not in EXCLUSIONS]
        assert not missing, "%s: reachable (form, kpos) without a case: %r" % (entry, missing)
        for form in range(10):
            have = set().union(*[t for (f, _), rows in ledger.items() if f == form for _, t in rows])
            want = set(FWD_TRAITS)
            if form < 4 or form in KXK_ONLY_FORMS:
                want.add("h_ne_w")
            assert want <= have, "%s: form %d has no case with %r" % (entry, form, sorted(want - have))
    assert len(EXCLUSIONS) <= 2


def _wgrad_ledger():
    runs = tc.wgrad_runs()
    infos = tc.wgrad_infos([tc.wgrad_geo(c, fl) for c, fl in runs])
    ledger = {}
    for (case, fl), info in zip(runs, infos):
        ledger.setdefault(tc.wgrad_key(info), []).append((case + (("kpos",) if fl else ()), tc.wgrad_traits(case, info)))
    return ledger


def test_wgrad_table_reaches_every_reachable_variant(mode):
    reach = tc.reachable_wgrad()
    ledger = _wgrad_ledger()
    print("\nwgrad_batch, pleas_arith(%d): (variant, slabs, staged rows) -> cases" % mode)
    for key in sorted(set(ledger) | reach):
        print("  %3d %-32s %-6s %-5s: %s" % (key[0], tc.variant_name(key[0]), "S>1" if key[1] else "S=1", "rows" if key[2] else "lanes",
                                            [c for c, _ in ledger.get(key, [])] or "NO CASE"))
    missing = [k for k in sorted(reach) if k not in ledger and ("wgrad_batch", k) not in EXCLUSIONS]
    assert not missing, "reachable (variant, S > 1, rows) without a case: %r" % [(k, tc.variant_name(k[0])) for k in missing]
    for v in sorted({k[0] for k in reach}):
        have = set().union(*[t for k, rows in ledger.items() if k[0] == v for _, t in rows])
        assert {"ragged_cout", "ragged_cin"} <= have, "variant %d (%s) has no case with %r" % (
            v, tc.variant_name(v), sorted({"ragged_cout", "ragged_cin"} - have))
    assert len(EXCLUSIONS) <= 2


def test_plan_info_answers_layer_by_layer_and_refuses_bad_lists():
    """``pleas_wgrad_plan_info`` runs the launch's own plan builder: a layer's answer does not depend on its neighbours, every
    layer has work, and a list the launch would refuse is refused."""
    from pleas_merging_amd import _lib, hip_ops

    geos = [tc.wgrad_geo(c) for c in tc.WGRAD_CASES]
    together = hip_ops.WgradBatch.plan_info(geos)
    assert together == [hip_ops.WgradBatch.plan_info([g])[0] for g in geos]
    for info in together:
        assert info["S"] >= 1 and info["tiles_cout"] >= 1 and info["tiles_cin"] >= 1 and info["items"] >= info["S"]
    with pytest.raises(_lib.PleasHipError):
        hip_ops.WgradBatch.plan_info([(4, 64, 64, 2, 2, 7, 7, 1, 0, 0)])          # empty output
    assert hip_ops.WgradBatch.plan_info([]) == []
    assert _lib.lib().pleas_wgrad_plan_info(None, 0, None) == -22


def test_random_draw_reaches_the_general_forms():
    """The seeded draw of the GPU property test (tests/test_hip_tile_forms.py): it must keep reaching the four general forward
    forms and six weight-gradient variants, whatever becomes of its generator."""
    draw = tc.random_cases()
    assert len(draw) == tc.RANDOM_CASES
    forms = {tc.fwd_form(c, False) for c in draw}
    variants = {i["variant"] for i in tc.wgrad_infos([tc.wgrad_geo(c) for c in draw])}
    print("random draw, seed %d: forward forms %r, weight-gradient variants %r" % (tc.RANDOM_SEED, sorted(forms), sorted(variants)))
    assert {0, 1, 2, 3} <= forms, sorted(forms)
    assert len(variants) >= 6, sorted(variants)
    assert any(c[2] % 4 for c in draw) and any(c[3] + c[4] < 2 * c[5] for c in draw)      # odd channel counts; images below the kernel


def test_schedule_list_is_cut_by_the_durations_a_launch_measured():
    """The mixed-form list of the eight-launch test: at least four forms, and the durations its calibration launch measured cut
    BOTH kinds of slices (``fwd_schedule_measured`` through ``pleas_fwd_plan_units``): the filler form into one per lane that
    wants a share and another long form into equal ones."""
    runs = tc.schedule_list()
    static = tc.fwd_units(runs)
    forms = {u[0] for u in static}
    assert len(forms) >= 4 and len(static) == len(forms)
    measured = tc.fwd_units(runs, form_ms=tc.SCHEDULE_MS)
    sliced = {f for f in forms if sum(1 for u in measured if u[0] == f) > 1}
    print("units from the measured durations: %r" % (measured,))
    assert len(sliced) >= 2, (static, measured)
    for form in forms:      # the slices of a form tile its items exactly
        whole = [u for u in static if u[0] == form][0]
        parts = sorted(u[1:3] for u in measured if u[0] == form)
        assert parts[0][0] == whole[1] and sum(c for _, c in parts) == whole[2]
        assert all(a[0] + a[1] == b[0] for a, b in zip(parts, parts[1:]))
