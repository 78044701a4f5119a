"""Closed-form fit of depthwise layers on the library's own kernels (csrc/dw_normal_eq.hip): the grouped accumulate launch against
fp64 ``unfold`` references, its grouped-launch protocol, the per-channel solve, and ``train(..., solver="normal_eq")`` on the
depthwise-separable test network against the oracle.

Bounds (derived, none measured).  Accumulate: both sides sum exact products (fp32 x fp32 in fp64) in fp64 in some order, so an entry
is within ``2 (M + L) 2^-53 sum_r |v_ri v_rj|`` of the reference, M all rows, L the launches into the S; the count entry is exact.
Solve: ``2^-24 |w64_i| + 3 T^2 2^-53 cond_2 ||w64||_2`` (tests/dw_normal_eq_cases.py).  End to end: the project's oracle gate, rel-fro
< 1e-4 -- the per-channel systems of the test network have cond_2 <= 2.2e3, fp32 forward differences of 1e-6 move their solutions by
1e-6.  Every test prints its worst figure as a fraction of its bound."""
import copy
import functools
import os
import sys
import types

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depthwise_cases as dc  # noqa: E402
import dw_normal_eq_cases as nc  # noqa: E402
from test_hip_depthwise import _rel, _row_maps, _sepnet_job  # noqa: E402
from test_hip_grouped_protocol import CountingLib, same  # noqa: E402
from test_hip_pipeline import _layer_objective  # noqa: E402

from oracle import pleas_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
CASES = dc.CASES + nc.SPLIT_CASES
IDS = [dc.case_id(c) for c in CASES]
MAPS = ("full", "partial", "absent")
NAN = float("nan")


# ------------------------------------------------------------------------------------------------------------ accumulate
@functools.lru_cache(maxsize=None)
def _operands(i: int):
    """Case i: fp32 operands on the CPU (never modified)."""
    N, C, H, W, K, s, p = CASES[i]
    g = torch.Generator().manual_seed(300 + i)
    Ho, Wo = dc.out_size(H, W, K, s, p)
    r = lambda *shape: torch.randn(*shape, generator=g)
    return dict(x=r(N, C, H, W), o1=r(N, C + 1, Ho, Wo), o2=r(N, C + 1, Ho, Wo), perm=torch.randperm(C + 1, generator=g)[:C])


def _lower(S: torch.Tensor) -> torch.Tensor:
    D = S.shape[-1]
    return S[..., torch.ones(D, D).tril().bool()]


def _fresh_S(C: int, K: int) -> torch.Tensor:
    """Zeros on and below the diagonal, a NaN sentinel above it."""
    D = K * K + 2
    S = torch.full((C, D, D), NAN, dtype=torch.float64)
    S[:, torch.ones(D, D).tril().bool()] = 0.0
    return S.cuda()


@functools.lru_cache(maxsize=None)
def _reference(i: int, kind: str):
    """(S64, magnitude, M): fp64 ``unfold`` per channel of the fp32 input and of ``hip_ops.merge_blocks``'s fp32 target."""
    from pleas_merging_amd import hip_ops

    N, C, H, W, K, s, p = CASES[i]
    d = _operands(i)
    row1, row2, nm = _row_maps(kind, C, d["perm"])
    tgt = hip_ops.merge_blocks(d["o1"].cuda(), d["o2"].cuda(), 1, row1.cuda(), row2.cuda(), nm).cpu()
    KK = K * K
    cols = F.unfold(d["x"].double(), K, padding=p, stride=s)                             # N, C * KK, L
    L = cols.shape[-1]
    Umat = cols.view(N, C, KK, L).permute(1, 0, 3, 2).reshape(C, N * L, KK)
    t = tgt.double().reshape(N, C, L).permute(1, 0, 2).reshape(C, N * L, 1)
    V = torch.cat([Umat, torch.ones(C, N * L, 1, dtype=torch.float64), t], 2)
    return V.transpose(1, 2) @ V, V.abs().transpose(1, 2) @ V.abs(), N * L


def _queue(batch, i: int, kind: str, S: torch.Tensor):
    N, C, H, W, K, s, p = CASES[i]
    d = _operands(i)
    row1, row2, nm = _row_maps(kind, C, d["perm"])
    batch.add(d["x"].cuda(), d["o1"].cuda(), d["o2"].cuda(), row1.cuda(), row2.cuda(), nm, S, s, p)


@functools.lru_cache(maxsize=None)
def _results(kind: str):
    """Every case alone (twice, each from zero), then all cases in ONE grouped launch: three lists of S on the CPU."""
    from pleas_merging_amd import hip_ops

    def run(cases):
        batch, out = hip_ops.DwNormalEqBatch(torch.device("cuda")), []
        for i in cases:
            out.append(_fresh_S(CASES[i][1], CASES[i][4]))
            _queue(batch, i, kind, out[-1])
        batch.flush()
        return [S.cpu() for S in out]

    every = range(len(CASES))
    return [run([i])[0] for i in every], [run([i])[0] for i in every], run(every)


def _check(S: torch.Tensor, S64: torch.Tensor, mag: torch.Tensor, rows: int, launches: int, K: int) -> float:
    D = K * K + 2
    upper = torch.ones(D, D).triu(1).bool()
    assert bool(torch.isnan(S[:, upper]).all()), "the strict upper triangle was written"
    err, bound = (_lower(S) - _lower(S64)).abs(), 2.0 * (rows + launches) * U53 * _lower(mag)
    frac = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(frac.max())
    assert bool((err <= bound).all()), "worst error is %.3f of the bound" % worst
    assert bool((S[:, K * K, K * K] == float(rows)).all()), "the count entry is not exact"
    return worst


@pytest.mark.parametrize("kind", MAPS)
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_accumulate_against_fp64_alone_grouped_and_again(i, kind):
    K = CASES[i][4]
    S64, mag, M = _reference(i, kind)
    alone, again, grouped = _results(kind)
    worst = _check(alone[i], S64, mag, M, 1, K)
    print("%s %s: worst entry error %.4f of 2 (M + 1) 2^-53 sum |v_i v_j| (M = %d)" % (IDS[i], kind, worst, M))
    assert torch.equal(_lower(again[i]), _lower(alone[i]))          # the same launch twice from zero
    assert torch.equal(_lower(grouped[i]), _lower(alone[i]))        # one grouped launch == every case alone


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_two_launches_into_one_S_give_the_sum(i):
    from pleas_merging_amd import hip_ops

    N, C, H, W, K, s, p = CASES[i]
    S = _fresh_S(C, K)
    batch = hip_ops.DwNormalEqBatch(torch.device("cuda"))
    for kind in ("full", "absent"):
        _queue(batch, i, kind, S)
        batch.flush()
    (a64, amag, M), (b64, bmag, _) = _reference(i, "full"), _reference(i, "absent")
    worst = _check(S.cpu(), a64 + b64, amag + bmag, 2 * M, 2, K)
    print("%s: worst entry error %.4f of 2 (2 M + 2) 2^-53 sum |v_i v_j|" % (IDS[i], worst))


def test_the_wrapper_refuses_before_the_library_is_reached():
    from pleas_merging_amd import hip_ops
    from pleas_merging_amd._lib import PleasHipError

    N, C, H, W, K, s, p = CASES[0]
    d = _operands(0)
    x, o1, o2 = d["x"].cuda(), d["o1"].cuda(), d["o2"].cuda()
    rows = torch.arange(C, dtype=torch.int32, device="cuda")
    S = _fresh_S(C, K)
    batch = hip_ops.DwNormalEqBatch(torch.device("cuda"))
    for bad in (lambda: batch.add(x.cpu(), o1, o2, rows, rows, C, S, s, p), lambda: batch.add(x.double(), o1, o2, rows, rows, C, S, s, p),
                lambda: batch.add(x, o1, o2[:, :-1], rows, rows, C, S, s, p), lambda: batch.add(x, o1[:, :, :-1], o2[:, :, :-1], rows, rows, C, S, s, p),
                lambda: batch.add(x, o1, o2, rows.long(), rows, C, S, s, p), lambda: batch.add(x, o1, o2, rows, rows[:-1], C, S, s, p),
                lambda: batch.add(x, o1, o2, rows, rows, C, S.float(), s, p), lambda: batch.add(x, o1, o2, rows, rows, C, S[:-1], s, p),
                lambda: batch.add(x, o1, o2, rows, rows, C, S[:, :-1, :-1].contiguous(), s, p),
                lambda: batch.add(x, o1, o2, rows, rows, C, S.cpu(), s, p)):
        with pytest.raises(PleasHipError):
            bad()
    assert batch.pending() == 0
    batch.add(x, o1, o2, rows, rows, C + 1, S, s, p)                 # n_merged outside 0 .. C: the library's refusal, nothing enqueued
    with pytest.raises(PleasHipError):
        batch.flush()


# ------------------------------------------------------------------------------------------------------- grouped protocol
@pytest.fixture(scope="module")
def ops():
    from pleas_merging_amd import hip_ops

    return hip_ops


@pytest.fixture
def counted(ops, monkeypatch):
    proxy = CountingLib(ops._lib.lib())
    monkeypatch.setattr(ops._lib, "lib", lambda: proxy)
    return proxy


LIST_A = [(2, 5, 7, 9, 3, 1, 1), (1, 2, 5, 5, 5, 1, 2)]
LIST_B = LIST_A + [(1, 2, 17, 241, 3, 1, 1)]       # a layer of two slabs: its partials need more workspace


class _Driver:
    """One ``DwNormalEqBatch`` over a list of layers; S starts from zero (S += ...)."""

    def __init__(self, ops):
        self.obj = ops.DwNormalEqBatch(torch.device("cuda"))

    @staticmethod
    def operands(entries, seed):
        g = torch.Generator().manual_seed(seed)
        data = []
        for N, C, H, W, K, s, p in entries:
            Ho, Wo = dc.out_size(H, W, K, s, p)
            r = lambda *shape: torch.randn(*shape, generator=g).cuda()
            data.append(dict(x=r(N, C, H, W), o1=r(N, C, Ho, Wo), o2=r(N, C, Ho, Wo), geo=(s, p), S=_fresh_S(C, K),
                             rows=(torch.arange(C, dtype=torch.int32, device="cuda"), torch.arange(C - 1, -1, -1, dtype=torch.int32, device="cuda"))))
        return data

    def run(self, data):
        for d in data:
            d["S"].copy_(_fresh_S(d["S"].shape[0], int((d["S"].shape[1] - 2) ** 0.5 + 0.5)))
            self.obj.add(d["x"], d["o1"], d["o2"], *d["rows"], d["x"].shape[1] // 2, d["S"], *d["geo"])
        self.obj.flush()
        return [_lower(d["S"]).clone() for d in data]


@functools.lru_cache(maxsize=None)
def _protocol_case(which: str, seed: int):
    from pleas_merging_amd import hip_ops

    data = _Driver.operands(LIST_A if which == "A" else LIST_B, seed)
    want = _Driver(hip_ops).run(data)
    assert all(bool(torch.isfinite(w).all()) for w in want)
    return data, want


def test_one_object_over_repeat_regrow_and_return(ops, counted):
    """A, A with new values, B (one ENOMEM answer, one new workspace, one more launch), A again: a fresh object's outputs each time;
    ``pleas_dw_normal_eq_ws_bytes`` once per workspace, the launch once per flush plus once for the regrow."""
    steps = [_protocol_case("A", 1), _protocol_case("A", 2), _protocol_case("B", 3), _protocol_case("A", 4)]
    counted.calls.clear()
    driver = _Driver(ops)
    fresh = []
    real_launch = driver.obj._launch
    driver.obj._launch = lambda f, extra: (fresh.append(f), real_launch(f, extra))[1]
    for n, (data, want) in enumerate(steps):
        assert same(driver.run(data), want), "step %d" % n
    assert counted.calls["pleas_dw_normal_eq_ws_bytes"] == 2, dict(counted.calls)
    assert counted.calls["pleas_dw_normal_eq_accum"] == len(steps) + 1, dict(counted.calls)
    assert fresh == [1, 0, 0, 1, 0], fresh          # ws_fresh with each new workspace only (the third launch is the refused one)


def test_two_objects_alternate_on_one_stream(ops):
    (data1, want1), (data2, want2) = _protocol_case("A", 1), _protocol_case("B", 3)
    one, two = _Driver(ops), _Driver(ops)
    for turn in range(3):
        assert same(one.run(data1), want1), "first object, turn %d" % turn
        assert same(two.run(data2), want2), "second object, turn %d" % turn


# ------------------------------------------------------------------------------------------------------------------ solve
@pytest.mark.parametrize("C", [5, 70])
@pytest.mark.parametrize("has_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("K", nc.SOLVE_KS)
def test_solve_against_fp64_and_the_host_routine(K, has_bias, C):
    from pleas_merging_amd import hip_ops

    S, w0, b0, w64, cond = nc.solve_case(K, has_bias, C)
    w, b = w0.cuda(), b0.cuda()
    status = hip_ops.dw_normal_eq_solve(S.cuda(), K, has_bias, nc.SOLVE_RIDGE, w, b if has_bias else None)
    worst = nc.check_solution(K, has_bias, w.cpu(), b.cpu(), status.cpu(), w0, b0, w64, cond)
    # against the host routine under the same bound (its solution in the place of the fp64 one), not bit for bit
    wh, bh = w0.clone(), b0.clone()
    sh = hip_ops.dw_normal_eq_solve_host(S, K, has_bias, nc.SOLVE_RIDGE, wh, bh if has_bias else None)
    assert torch.equal(sh, status.cpu())
    host = torch.cat([wh.reshape(C, K * K).double(), bh.double()[:, None]], 1)[:, :w64.shape[1]]
    host = torch.where(torch.isnan(w64), w64, host)
    worst_host = nc.check_solution(K, has_bias, w.cpu(), b.cpu(), status.cpu(), w0, b0, host, cond)
    print("K = %d, bias %s, C = %d: worst error %.3g of its bound against fp64, %.3g against the host routine" % (K, has_bias, C, worst, worst_host))


# ------------------------------------------------------------------------------------------------------------- end to end
def _merged(merging="perm_gradmask"):
    from pleas.methods.partial_matching import partial_merge

    data, m1, m2, spec, perm, costs = _sepnet_job()[:6]
    g1, g2 = copy.deepcopy(m1).cuda(), copy.deepcopy(m2).cuda()
    costs = {k: v.cuda() for k, v in costs.items()}
    return data, g1, g2, spec, perm, costs, partial_merge(spec, g1, g2, perm, costs, 0.0)


def _train(solver: str, merging: str = "perm_gradmask"):
    """``train`` on batches 0 .. 5 of the test network's job under both "hip" switches; the trained state on the CPU."""
    from pleas.methods.pleas_merging import train
    from pleas_merging_amd import hip_ops

    data, g1, g2, spec, perm, costs, m3 = _merged()
    with hip_ops.depthwise_form("hip"), hip_ops.depthwise_closed_form("hip"):
        out = train(data[:6], g1, g2, m3, spec, perm, costs, 0.0, False, 5, None, num_classes=10, solver=solver, merging=merging)
    return {k: v.detach().cpu().clone() for k, v in out.state_dict().items()}, out


@functools.lru_cache(maxsize=None)
def _closed_form_state(merging: str = "perm_gradmask"):
    return _train("normal_eq", merging)[0]


def _oracle_solution(name: str, merging: str, ridge: float = 1e-6):
    """Per-channel fp64 solution of a depthwise layer from the oracle's ``layer_targets`` activations on batches 0 .. 5: the
    regularised normal equations of the contract, ``(weight [C, 1, K, K], bias [C] or None)``."""
    data, m1, m2, spec, perm, costs = _sepnet_job()[:6]
    blocks = orc.spread_blocks(spec, orc.get_blocks(spec, perm, costs, 0.0))
    a1, a2 = {}, {}
    hooks = orc._hook_inputs(m1, a1) + orc._hook_inputs(m2, a2)
    l1, l2 = orc.get_attr(m1, name.split(".")), orc.get_attr(m2, name.split("."))
    K, s, p, has_bias = l1.kernel_size[0], l1.stride[0], l1.padding[0], l1.bias is not None
    rows = []
    with torch.no_grad():
        for x, _ in data[:6]:
            m1(x)
            m2(x)
            ip, op = orc.layer_targets(l1, l2, blocks, name, a1[name], a2[name], num_classes=10, merging=merging)
            N, C = ip.shape[:2]
            cols = F.unfold(ip.double(), K, padding=p, stride=s)
            L = cols.shape[-1]
            Umat = cols.view(N, C, K * K, L).permute(1, 0, 3, 2).reshape(C, N * L, K * K)
            t = op.double().reshape(N, C, L).permute(1, 0, 2).reshape(C, N * L, 1)
            rows.append(torch.cat([Umat, torch.ones(C, N * L, 1, dtype=torch.float64), t], 2))
    for h in hooks:
        h.remove()
    V = torch.cat(rows, 1)
    T = K * K + int(has_bias)
    G, hvec = V[:, :, :T].transpose(1, 2) @ V[:, :, :T], V[:, :, :T].transpose(1, 2) @ V[:, :, -1:]
    A = G + ridge * G.diagonal(dim1=1, dim2=2).mean(1)[:, None, None] * torch.eye(T, dtype=torch.float64)
    x = torch.linalg.solve(A, hvec)[:, :, 0]
    return x[:, :K * K].reshape(-1, 1, K, K), (x[:, K * K] if has_bias else None)


def _gate_against_the_oracle(got, merging: str) -> float:
    worst = 0.0
    for name in ("dw1", "dw2"):
        w64, b64 = _oracle_solution(name, merging)
        for key, want in (("%s.weight" % name, w64), ("%s.bias" % name, b64)):
            if want is not None:
                rel = _rel(got[key], want)
                worst = max(worst, rel)
                assert rel < 1e-4, (merging, key, rel)
    return worst


def test_closed_form_of_the_sepnet_against_the_oracle():
    """(a) the job returns, (b) the oracle objective against the Adam fit's, (c) the depthwise layers against the per-channel fp64
    solution, (e) the same job twice."""
    data, m1, m2, spec, perm, costs, merged = _sepnet_job()[:7]
    got, m_neq = _train("normal_eq")
    assert not torch.equal(got["dw1.weight"], merged["dw1.weight"]) and not torch.equal(got["dw2.bias"], merged["dw2.bias"])
    worst = _gate_against_the_oracle(got, "perm_gradmask")
    print("depthwise layers: worst tensor %.2e rel-fro from the per-channel fp64 solution (gate 1e-4)" % worst)
    _, m_adam = _train("adam")
    t = types.SimpleNamespace(spec=spec, m1=m1, m2=m2)
    f_init = _layer_objective(t, orc.partial_merge(spec, m1, m2, perm, costs, 0.0), 0.0, perm, costs, data[:6])
    f_adam = _layer_objective(t, m_adam.cpu(), 0.0, perm, costs, data[:6])
    f_neq = _layer_objective(t, m_neq.cpu(), 0.0, perm, costs, data[:6])
    print("oracle objective: merged %.6g, Adam %.6g, closed form %.6g" % (f_init, f_adam, f_neq))
    assert f_neq <= f_adam * (1 + 1e-4) and f_neq < f_init, (f_init, f_adam, f_neq)
    again, _ = _train("normal_eq")
    assert got.keys() == again.keys() and all(torch.equal(got[k], again[k]) for k in got)


@pytest.mark.parametrize("merging", ["reg_mean", "perm_mixedls"])
def test_stacked_modes_against_the_oracles_stacked_problem(merging):
    got = _closed_form_state(merging)
    worst = _gate_against_the_oracle(got, merging)
    print("%s: worst depthwise tensor %.2e rel-fro from the per-channel fp64 solution (gate 1e-4)" % (merging, worst))


def _fitter(batches):
    from pleas_merging_amd.methods.normal_eq import NormalEqFitter
    from pleas_merging_amd import hip_ops

    data, g1, g2, spec, perm, costs, m3 = _merged()
    with hip_ops.depthwise_form("hip"), hip_ops.depthwise_closed_form("hip"):
        fit = NormalEqFitter(g1, g2, m3, spec, perm, costs, 0.0, 5, 5e-4, False, 10, "rn50")
        assert [p.name for p in fit.plans if p.dw] == ["dw1", "dw2"] and fit.vendor_layers == []
        n = sum(1 for _ in fit.steps([data[b][0] for b in batches]))
    assert n == len(batches)
    return fit


def test_the_dense_layers_do_not_move_with_the_depthwise_ones(monkeypatch):
    """(d) the same job with the depthwise layers taken out -- nothing accumulated, nothing solved for them --: the dense layers'
    weights are the same bits, the depthwise ones keep their merged values."""
    from pleas_merging_amd import hip_ops

    fit = _fitter(range(6))
    info = fit.solve()
    assert info["dw1"] == 9.0 and info["dw2"] == 26.0 and info["dw_singular_channels"] == 0.0, info
    with_dw = {k: v.detach().cpu().clone() for k, v in fit.finish().state_dict().items()}
    monkeypatch.setattr(hip_ops.DwNormalEqBatch, "add", lambda self, *a, **k: None)
    monkeypatch.setattr(hip_ops, "dw_normal_eq_solve", lambda S, K, hb, ridge, w, b=None: torch.zeros(S.shape[0], dtype=torch.int32, device=S.device))
    fit = _fitter(range(6))
    fit.solve()
    assert float(fit.S_flat.abs().max()) == 0.0
    without = {k: v.detach().cpu().clone() for k, v in fit.finish().state_dict().items()}
    merged = _sepnet_job()[6]
    for k in with_dw:
        if k.startswith("dw"):
            assert _rel(without[k], merged[k]) < 1e-6 and not torch.equal(with_dw[k], without[k]), k
        else:
            assert torch.equal(with_dw[k], without[k]), k


def test_additivity_over_fitters():
    """(g) one fitter on batches 0 .. 5 against two on the even / odd ones whose S are added: the accumulate bound with M the rows
    of all six batches and L = 6 launches + the addition, the magnitude bounded by Cauchy-Schwarz from the diagonal
    (sum |v_i v_j| <= sqrt(S_ii S_jj))."""
    whole, even, odd = _fitter(range(6)), _fitter([0, 2, 4]), _fitter([1, 3, 5])
    assert whole.S_flat.numel() == 8 * 11 * 11 + 16 * 27 * 27 and whole.A_flat.numel() == even.A_flat.numel()
    worst = 0.0
    for idx, S in whole.S.items():
        S, parts = S.cpu(), even.S[idx].cpu() + odd.S[idx].cpu()
        D = S.shape[-1]
        M = float(S[0, D - 2, D - 2])
        diag = S.diagonal(dim1=1, dim2=2)
        bound = _lower(2.0 * (M + 7) * U53 * torch.sqrt(diag[:, :, None] * diag[:, None, :]))
        err = (_lower(S) - _lower(parts)).abs()
        assert bool((err <= bound).all())
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert bool((S[:, D - 2, D - 2] == parts[:, D - 2, D - 2]).all()) and M > 0
    print("additivity: worst entry %.4f of its bound" % worst)


def test_the_refusal_is_unchanged_without_the_switch_or_under_the_vendor_form():
    """(h)"""
    from pleas.methods.pleas_merging import train
    from pleas_merging_amd import hip_ops

    data, g1, g2, spec, perm, costs, m3 = _merged()
    message = ("solver='normal_eq' takes dense, undilated Conv2d layers with a square kernel / stride / padding; "
               "not supported: dw1, dw2 \\(solver='adam' fits them\\)")
    for form, closed in (("hip", "refuse"), ("vendor", "refuse"), ("vendor", "hip")):
        with hip_ops.depthwise_form(form), hip_ops.depthwise_closed_form(closed):
            with pytest.raises(NotImplementedError, match=message):
                train(data[:1], g1, g2, copy.deepcopy(m3), spec, perm, costs, 0.0, False, 1, None, num_classes=10, solver="normal_eq")
