"""pleas_cholesky_solve_batched (csrc/solve.hip) against fp64, problem by problem, row by row, panel by panel.

The fitter (methods/normal_eq.py) submits one system per (layer, mask pattern): K = free columns of the pattern, N = output
rows that share it -- arbitrary and unrelated across a batch.  Every table in tests/solve_cases.py is such a batch.

Inputs are seeded, built in fp64 on the CPU and rounded to fp32; the references (torch.linalg.solve / cholesky, fp64, CPU)
see the SAME rounded data, so the figures below are the solver's error alone.

Tolerance.  Every case is also solved on the CPU in fp32 by LAPACK (cholesky + cholesky_solve); the kernel's worst row may
be off by at most C_GATE times LAPACK's worst row of the same problem (the factor: worst 64-column panel against LAPACK's
worst panel).  LAPACK's figures are floored only so that a problem of two or three numbers, which can come out exact by
luck in one implementation and an ulp off in the other, does not divide by (nearly) nothing: the row figure at one fp32
epsilon, 2^-23 (only K = 1 falls under it), the panel figure at 2^-26 (LAPACK's panels are at 2.5e-8 and above from K = 2
on, 6e-8 to 1.3e-7 from K = 33 on, so the floor never binds there).  The printed ratios are kernel / floored LAPACK.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import solve_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
PANEL_FLOOR = 2.0 ** -26
# Largest kernel / LAPACK-fp32 ratio of a problem, per case, measured on an MI355X (solution rows | factor panels):
#   128x1+65x100 1.83 | 1.35   192x8+130x150 1.60 | 1.58   256x100+65x321 1.89 | 1.54   320x3+70x300+129x200 1.68 | 1.61
#   no_rhs 2.14 | 1.53   panel_edges 2.27 | 1.58   k1153 2.24 | 1.74   draw120 2.11 | 1.79   cond 1e4 1.69 | 1.58
#   info 2.31 | 1.71   ridge 1e-6 1.79 | 1.54   ridge 1e-3 1.74 | 1.45
# C_GATE = twice the largest (2 x 2.31 = 4.62), rounded up to a power of two.  8 is also the most the gate may ever be:
# a kernel that needs more is a finding, not a reason to widen it.
C_GATE = 8.0


@pytest.fixture(scope="module")
def ops():
    from pleas_merging_amd import hip_ops

    return hip_ops


# ------------------------------------------------------------------------------------------------ problems and references
class Problem:
    """One system: fp32 data (A symmetric, Bt rows = right-hand sides) and everything the CPU knows about it."""

    def __init__(self, A64, Bt64, ridge=0.0):
        self.A = A64.float()                                       # what the kernel gets; rounding keeps the symmetry
        self.Bt = Bt64.float()
        self.K, self.N = self.A.shape[0], self.Bt.shape[0]
        eye = torch.eye(self.K, dtype=torch.float64)
        self.A_ref = self.A.double() + ridge * self.A.double().diagonal().mean() * eye
        self.L_ref, bad = torch.linalg.cholesky_ex(self.A_ref)
        self.info_ref = int(bad)
        if self.info_ref:
            return
        self.X_ref = torch.cholesky_solve(self.Bt.double().t(), self.L_ref).t()
        assert row_err(torch.linalg.solve(self.A_ref, self.Bt.double().t()).t(), self.X_ref) < 1e-9
        # fp32 LAPACK on the same data: the ridge goes in the way the kernel adds it, in fp32
        A32 = self.A + (torch.tensor(ridge, dtype=torch.float32) * self.A.diagonal().mean()) * torch.eye(self.K)
        L32, bad32 = torch.linalg.cholesky_ex(A32)
        self.lapack_breaks = int(bad32) != 0
        if not self.lapack_breaks:
            self.lapack_row = row_err(torch.cholesky_solve(self.Bt.t(), L32).t(), self.X_ref)
            self.lapack_panel = panel_err(L32, self.L_ref)


def row_err(X, ref):
    """Largest relative error of a row (0 without rows)."""
    if X.shape[0] == 0:
        return 0.0
    d = (X.double() - ref).norm(dim=1) / ref.norm(dim=1)
    return float(d.max())


def panel_err(L, ref):
    """Largest relative error of a 64-column panel of the lower triangle."""
    d = torch.tril(L.double()) - ref
    return max(float(d[:, j:j + 64].norm() / ref[:, j:j + 64].norm()) for j in range(0, ref.shape[0], 64))


def lower(A):
    """The lower triangle's entries (the strict upper one holds the mirrored panels, or whatever it held before)."""
    K = A.shape[0]
    return A[torch.ones(K, K, dtype=torch.bool, device=A.device).tril()]


def spd(K, N, g, spread=1.0, ridge=0.0):
    """M M^T / (K + 8) + 0.5 I of the existing solve test (cond about 9).  ``spread`` > 1: the columns of M are scaled
    geometrically from 1 down to 1 / spread and the shift shrinks with them, which puts cond(A) near spread^2."""
    M = torch.randn(K, K + 8, generator=g, dtype=torch.float64)
    scale = spread ** -(torch.arange(K + 8, dtype=torch.float64) / (K + 7))
    M = M * scale
    A = M @ M.t() / (K + 8) + 0.5 / spread ** 2 * torch.eye(K, dtype=torch.float64)
    return Problem(A, torch.randn(N, K, generator=g, dtype=torch.float64), ridge)


def make_batch(sizes, seed, **kw):
    g = torch.Generator().manual_seed(seed)
    return [spd(K, N, g, **kw) for K, N in sizes]


def run(ops, problems, ridge=0.0, upper=None):
    """The kernel on fresh device copies; returns (info, solutions, factored A's), all on the CPU.
    ``upper``: a value for the strict upper triangle of every A in place of the symmetric copy."""
    As = []
    for p in problems:
        a = p.A.clone()
        if upper is not None:
            a[torch.ones(p.K, p.K, dtype=torch.bool).triu(1)] = upper
        As.append(a.cuda().contiguous())
    Bts = [p.Bt.cuda().contiguous() for p in problems]
    info = ops.cholesky_solve_batched(As, Bts, ridge=ridge)
    return info.cpu(), [b.cpu() for b in Bts], [a.cpu() for a in As]


class Solved:
    """A batch, the kernel's answer for it in ONE call, and its answer for every problem in a call of its own."""

    def __init__(self, ops, problems, ridge=0.0):
        self.problems, self.ridge = problems, ridge
        self.info, self.X, self.F = run(ops, problems, ridge)
        self.solo = [run(ops, [p], ridge) for p in problems]


def check_accuracy(s, what):
    """Every healthy problem: rows against fp64 at C_GATE x LAPACK, factor panels likewise.  Prints the ratios."""
    worst_row = worst_panel = 0.0
    failures = []
    for i, p in enumerate(s.problems):
        if p.info_ref:
            continue
        assert not p.lapack_breaks, (what, i, p.K)
        assert int(s.info[i]) == 0, (what, i, p.K, p.N, int(s.info[i]))
        r = row_err(s.X[i], p.X_ref) / max(p.lapack_row, EPS32)
        f = panel_err(s.F[i], p.L_ref) / max(p.lapack_panel, PANEL_FLOOR)
        worst_row, worst_panel = max(worst_row, r), max(worst_panel, f)
        if not (r <= C_GATE and f <= C_GATE):                      # NaN fails
            failures.append((i, p.K, p.N, "rows %.2f x LAPACK's %.2e" % (r, p.lapack_row),
                             "panels %.2f x LAPACK's %.2e" % (f, p.lapack_panel)))
    print("%s: kernel / LAPACK fp32, worst problem: rows %.2f, factor panels %.2f" % (what, worst_row, worst_panel))
    assert not failures, (what, failures[:8])


def check_independent(s, what):
    """Solution and factor of every problem: the bits of the same problem solved alone."""
    differ = []
    for i, (p, (info1, X1, F1)) in enumerate(zip(s.problems, s.solo)):
        assert int(info1[0]) == int(s.info[i]), (what, i)
        if p.info_ref:
            continue
        if not torch.equal(s.X[i], X1[0]):
            differ.append((i, p.K, p.N, "rows", (s.X[i] != X1[0]).any(dim=1).nonzero().flatten().tolist()[:6]))
        if not torch.equal(lower(s.F[i]), lower(F1[0])):
            differ.append((i, p.K, p.N, "factor"))
    assert not differ, (what, differ[:8])


# --------------------------------------------------------------------------------------------------- mixed-size batches
_solved = {}


def solved(ops, name):
    if name not in _solved:
        _solved[name] = Solved(ops, make_batch(sc.BATCHES[name], seed=100 + list(sc.BATCHES).index(name)))
    return _solved[name]


@pytest.mark.parametrize("name", list(sc.BATCHES))
def test_mixed_batch_rows_and_factor_against_fp64(ops, name):
    check_accuracy(solved(ops, name), name)


@pytest.mark.parametrize("name", list(sc.BATCHES))
def test_mixed_batch_equals_solo_solves(ops, name):
    """Fails on the grids sized by rows_max and the LARGEST problem's panel width: rows of the problems in their last,
    narrow panel missed that panel's forward substitution (the four MIXED_LAST_PANEL batches: 36, 22, 1 and 44 + 8 rows)."""
    check_independent(solved(ops, name), name)


def test_ill_conditioned_family(ops):
    problems = make_batch(sc.ILL_BATCH, seed=7, spread=64.0)
    for p in problems:
        if p.K >= 64:
            cond = float(torch.linalg.cond(p.A.double()))
            print("K = %d: cond %.3g" % (p.K, cond))
            assert 3e3 < cond < 3e4, (p.K, cond)
        assert not p.lapack_breaks, p.K
    s = Solved(ops, problems)
    check_accuracy(s, "cond 1e4")
    check_independent(s, "cond 1e4")


def test_only_the_lower_triangle_is_read(ops):
    problems = solved(ops, "panel_edges").problems
    s = solved(ops, "panel_edges")
    zero = run(ops, problems, upper=0.0)
    info, X, F = run(ops, problems, upper=float("nan"))
    assert torch.equal(info, zero[0]) and torch.equal(info, s.info)
    for i, p in enumerate(problems):
        for _, X0, F0 in (zero, (None, s.X, s.F)):                # zeros above the diagonal, and the symmetric copy
            assert torch.equal(X[i], X0[i]), (i, p.K, p.N)
            assert torch.equal(lower(F[i]), lower(F0[i])), (i, p.K, p.N)


def test_repeatable(ops):
    problems = solved(ops, "320x3+70x300+129x200").problems + solved(ops, "k1153").problems
    a, b = run(ops, problems), run(ops, problems)
    assert torch.equal(a[0], b[0])
    for i in range(len(problems)):
        assert torch.equal(a[1][i], b[1][i]) and torch.equal(lower(a[2][i]), lower(b[2][i])), i


# ------------------------------------------------------------------------------------------------------------------ info
def test_info_is_the_first_bad_pivot_of_that_problem_only(ops):
    """LAPACK's convention (torch.linalg.cholesky_ex): info = m + 1 for the first non-positive pivot m, at the index of
    that problem -- also behind the launch group's boundary at 96 -- and the neighbours never notice."""
    g = torch.Generator().manual_seed(31)
    bad = {i: (K, m) for i, K, m in sc.INFO_BAD}
    problems, h = [], 0
    for i in range(sc.INFO_COUNT):
        if i in bad:
            K, m = bad[i]
            p = spd(K, 6, g)
            A = p.A.double()
            A[m, m] = -1.0
            p = Problem(A, p.Bt.double())
            assert p.info_ref == m + 1
        else:
            p = spd(*sc.INFO_HEALTHY[h % len(sc.INFO_HEALTHY)], g)
            h += 1
            assert p.info_ref == 0
        problems.append(p)
    assert max(bad) >= 96
    s = Solved(ops, problems)
    assert s.info.tolist() == [p.info_ref for p in problems]
    for i, p in enumerate(problems):
        if not p.info_ref:
            assert bool(torch.isfinite(s.X[i]).all()) and bool(torch.isfinite(lower(s.F[i])).all()), i
    check_independent(s, "info")
    check_accuracy(s, "info")


# ----------------------------------------------------------------------------------------------------------------- ridge
@pytest.mark.parametrize("ridge", [1e-6, 1e-3])
def test_ridge_kernel_and_fp64_fallback_share_one_convention(ops, ridge):
    """x (A + ridge * mean(diag A) * I) = row, per problem: the kernel, and methods/normal_eq._spd_solve_fp64 that
    replaces it for a system the fp32 factorisation flags."""
    from pleas_merging_amd.methods.normal_eq import _spd_solve_fp64

    problems = make_batch(sc.RIDGE_BATCH, seed=41, ridge=ridge)
    s = Solved(ops, problems, ridge=ridge)
    check_accuracy(s, "ridge %g" % ridge)
    check_independent(s, "ridge %g" % ridge)
    for p in problems:
        got = _spd_solve_fp64(p.A, p.Bt, ridge)
        assert got.dtype == torch.float32 and got.shape == p.Bt.shape
        # computed in fp64, returned in fp32: one rounding per element (2^-24), with a factor of two to spare
        assert row_err(got, p.X_ref) < EPS32, (p.K, p.N, row_err(got, p.X_ref))
    if ridge == 1e-3:      # the convention matters: without the ridge the answer is somewhere else
        plain = make_batch(sc.RIDGE_BATCH, seed=41)
        assert all(row_err(a.X_ref, b.X_ref) > 1e-4 for a, b in zip(plain, problems) if a.N)


# ------------------------------------------------------------------------------------------------------------- refusals
def test_wrapper_refusals(ops):
    a, b = (4 * torch.eye(8)).cuda(), torch.ones(3, 8).cuda()        # a launch would leave 2 I and 0.25
    before = (a.clone(), b.clone())
    bad_calls = {
        "A not square": ([torch.ones(8, 9).cuda()], [b]),
        "Bt with another K": ([a], [torch.ones(3, 7).cuda()]),
        "A a strided view": ([torch.eye(16).cuda()[::2, ::2]], [b]),
        "Bt a transposed view": ([a], [torch.ones(8, 3).cuda().t()]),
        "A on the CPU": ([torch.eye(8)], [b]),
        "Bt on the CPU": ([a], [torch.ones(3, 8)]),
        "second problem bad": ([a, torch.ones(4, 5).cuda()], [b, torch.ones(1, 4).cuda()]),
    }
    for what, (As, Bts) in bad_calls.items():
        with pytest.raises(ops.PleasHipError):
            ops.cholesky_solve_batched(As, Bts)
            print("accepted:", what)
    torch.cuda.synchronize()
    assert torch.equal(a, before[0]) and torch.equal(b, before[1])     # refused before anything was launched
