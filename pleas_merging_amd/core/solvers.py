"""Linear-assignment solvers with the reference's call signature ``solver(A) -> LongTensor[n]``.

``hip_solve_lsa`` (default of this package) runs the batched gfx950 kernel;
``scipy_solve_lsa`` keeps the reference's public symbol (pleas/core/solvers.py:18-33,
re-exported at pleas/core/__init__.py:21) for callers that pass it explicitly.
The bottleneck ("minimax") solvers: ``hip_solve_minimax_assignment`` (batched gfx950 kernels),
``host_solve_minimax_assignment`` (the same result on the host) and the reference's
``scipy_solve_minimax_assignment`` (pleas/core/solvers.py:88-115), never a default.
"""
from __future__ import annotations

import bisect

import torch


def hip_solve_lsa(A: torch.Tensor, maximize: bool = True) -> torch.Tensor:
    from ..hip_ops import hip_solve_lsa as _impl

    return _impl(A, maximize)


def host_solve_lsa(A: torch.Tensor, maximize: bool = True) -> torch.Tensor:
    """The library's own solver on a HOST cost matrix (``pleas_lsap_host``, scipy's scan order and tie rule): what a
    caller with CPU state dicts passes as ``lsa_solver`` -- explicitly; device tensors always take ``hip_solve_lsa``."""
    from ..hip_ops import host_solve_lsa as _impl

    return _impl(A, maximize)


def scipy_solve_lsa(A: torch.Tensor, maximize: bool = True) -> torch.Tensor:
    """Host solver of the reference (pleas/core/solvers.py:18-33); never a default here."""
    import scipy.optimize

    ri, ci = scipy.optimize.linear_sum_assignment(A.detach().cpu().numpy(), maximize=maximize)
    ri, ci = torch.as_tensor(ri), torch.as_tensor(ci)
    assert (ri == torch.arange(len(ri))).all()
    return ci


def hip_solve_minimax_assignment(A: torch.Tensor, maximize: bool = True) -> torch.Tensor:
    """Lexicographic bottleneck assignment on the GPU (``pleas_bottleneck_batched``): the permutation that maximises the
    smallest matched entry, then the sum; int64 on ``A``'s device.  ``activation_matching`` and ``weight_matching`` run
    all groups of a batch in one call when this is their ``lsa_solver``."""
    from ..hip_ops import hip_solve_minimax_assignment as _impl

    return _impl(A, maximize)


def host_solve_minimax_assignment(A: torch.Tensor, maximize: bool = True) -> torch.Tensor:
    """The same solver on a HOST matrix (``pleas_bottleneck_host``), same result as the device path; CPU tensors only."""
    from ..hip_ops import host_solve_minimax_assignment as _impl

    return _impl(A, maximize)


def scipy_solve_minimax_assignment(A: torch.Tensor) -> torch.Tensor:
    """Host solver of the reference (pleas/core/solvers.py:88-115): bisection over the sorted entries, each probe a
    maximum bipartite matching of ``A >= t`` in scipy; returns the matching of the highest feasible probe, as the
    reference does (whichever bottleneck-optimal matching scipy finds).  Never a default here."""
    import numpy as np
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import maximum_bipartite_matching

    B = A.detach().cpu().numpy()
    values = np.sort(B.ravel())
    best = [-float("inf"), None]

    def infeasible(t):
        matching = maximum_bipartite_matching(csr_matrix(B >= t), perm_type="column")
        ok = not (matching == -1).any()
        if ok and t > best[0]:
            best[0], best[1] = t, matching
        return not ok

    bisect.bisect_right(values, False, key=infeasible)
    return torch.from_numpy(best[1]).long().to(A.device)
