"""Cases of the depthwise closed form's tests (csrc/dw_normal_eq.hip), shared by tests/test_dw_normal_eq_host.py and
tests/test_hip_dw_normal_eq.py.

Accumulate kernel: ``(N, C, H, W, K, stride, pad)`` as in tests/depthwise_cases.py.  Its work item is one (channel, slab of 4096
consecutive output pixels of the channel, counted over (n, oy, ox)); inside a slab the four waves take groups of four pixels in
turn.  ``SPLIT_CASES`` are the smallest shapes that straddle that split (M = N * Ho * Wo pixels per channel); groups that are not
full, steps that wrap over several rows and images, and 1 x 1 maps are in ``depthwise_cases.CASES`` already."""

SPLIT_CASES = [
    (1, 1, 64, 64, 3, 1, 1),      # M = 4096: exactly one full slab
    (1, 2, 17, 241, 3, 1, 1),     # M = 4097: a second slab of ONE pixel (three of its waves have no work), two channels
    (1, 1, 91, 91, 3, 1, 1),      # M = 8281: three slabs
    (2, 1, 33, 63, 5, 1, 2),      # M = 4158: K = 5 (three tiles) over two slabs, the slab boundary inside the second image
    (1, 1, 17, 241, 7, 1, 3),     # M = 4097: K = 7 (ten tiles) over two slabs
]

SOLVE_KS = (3, 5, 7)
SOLVE_ROWS = 64
# The rank-deficient channels below have cond_2 = T / ridge + 1 (one non-zero eigenvalue g against the shift ridge * g / T), so at
# the fitter's default ridge of 1e-6 they sit at 9e6 .. 5e7, above the 2e6 the tests require of their inputs.  5e-5 puts the worst
# one (T = 50) at 1e6.
SOLVE_RIDGE = 5e-5


def solve_case(K: int, has_bias: bool, C: int = 5, seed: int = 0):
    """``(S, w0, b0, w64, cond)`` on the CPU: ``S`` fp64 [C, D, D] (LOWER triangle; the strict upper triangle holds NaN) built in
    fp64 from ``SOLVE_ROWS`` random rows per channel; the initial fp32 weight and bias; the fp64 solution [C, T] of
    ``(G_T + ridge * mean(diag G_T) I) x = h_T`` by ``torch.linalg.solve`` (NaN rows where the system is singular: the all-zero
    channel without a bias); and cond_2 of every regularised system.  Channel C - 2 has the centre tap alone non-zero (the 1 x 1-map
    case), channel C - 1 is all zero."""
    import torch

    g = torch.Generator().manual_seed(1000 * K + 10 * C + int(has_bias) + seed)
    KK, D = K * K, K * K + 2
    T = KK + int(has_bias)
    U = torch.randn(C, SOLVE_ROWS, KK, generator=g, dtype=torch.float64)
    t = torch.randn(C, SOLVE_ROWS, generator=g, dtype=torch.float64)
    centre = torch.zeros(KK, dtype=torch.float64)
    centre[KK // 2] = 1.0
    U[C - 2] *= centre
    U[C - 1] = 0.0
    V = torch.cat([U, torch.ones(C, SOLVE_ROWS, 1, dtype=torch.float64), t[:, :, None]], 2)
    full = V.transpose(1, 2) @ V
    S = torch.where(torch.ones(D, D).tril().bool(), full, torch.full((), float("nan"), dtype=torch.float64)).contiguous()
    G, h = full[:, :T, :T], full[:, KK + 1, :T]
    A = G + SOLVE_RIDGE * G.diagonal(dim1=1, dim2=2).mean(1)[:, None, None] * torch.eye(T, dtype=torch.float64)
    w64 = torch.full((C, T), float("nan"), dtype=torch.float64)
    cond = torch.full((C,), float("inf"), dtype=torch.float64)
    for c in range(C):
        if float(A[c].diagonal().abs().max()) > 0.0:
            w64[c] = torch.linalg.solve(A[c], h[c])
            cond[c] = torch.linalg.cond(A[c], 2)
    w0 = torch.randn(C, 1, K, K, generator=g)
    b0 = torch.randn(C, generator=g)
    return S, w0, b0, w64, cond


def check_solution(K: int, has_bias: bool, w, b, status, w0, b0, w64, cond) -> float:
    """The solve's contract on one ``solve_case``; returns the worst error as a fraction of the bound
    ``2^-24 |w64_i| + 3 T^2 2^-53 cond_2 ||w64||_2`` (one rounding to fp32; Higham's bound of a Cholesky solve)."""
    import torch

    C, KK = w64.shape[0], K * K
    T = KK + int(has_bias)
    got = torch.cat([w.reshape(C, KK).double(), b.double()[:, None]], 1)[:, :T]
    worst = 0.0
    for c in range(C):
        if c == C - 1 and not has_bias:                   # all-zero system: flagged, nothing written
            assert int(status[c]) == 1
            assert torch.equal(w[c], w0[c])
            continue
        assert int(status[c]) == 0, (c, int(status[c]))
        assert float(cond[c]) <= 2e6, (c, float(cond[c]))           # a condition on the inputs, not on the code
        bound = 2.0 ** -24 * w64[c].abs() + 3 * T * T * 2.0 ** -53 * cond[c] * w64[c].norm()
        err = (got[c] - w64[c]).abs()
        assert bool((err <= bound).all()), (c, float((err / bound.clamp_min(1e-300)).max()))
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        if c == C - 1:                                    # all-zero taps beside a bias: the taps solve to 0
            assert bool((w[c] == 0).all())
    if not has_bias:
        assert torch.equal(b, b0)                         # a layer without bias: the bias argument is not touched
    return worst
