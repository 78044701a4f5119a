"""Bottleneck ("minimax") assignment on the MI355X: pleas_bottleneck_batched against the fixture of the reference's
bottleneck values (tests/golden/minimax_small.npz) and against the library's host entry point, bit for bit; the batched
solver inside activation_matching and weight_matching; refusals."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bottleneck_cases import GOLDEN, load_cases  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.float32(x).view(np.uint32)


def _host(A, maximize=True):
    from pleas.core.solvers import host_solve_minimax_assignment

    return host_solve_minimax_assignment(A.cpu(), maximize=maximize)


def test_batched_fixture_cases_both_directions():
    """Every fixture case plus an n = 1 problem in ONE launch per direction: t* bit for bit, col_ind = the host entry's."""
    from pleas_merging_amd import hip_ops

    cases = load_cases() + [("one", np.array([[-0.0]], dtype=np.float32), np.float32(0.0), np.array([0]))]
    mats = [torch.from_numpy(A).cuda() for _, A, _, _ in cases]
    want = [_host(torch.from_numpy(A)) for _, A, _, _ in cases]
    for maximize in (True, False):
        t_out = torch.empty(len(mats), dtype=torch.float32, device="cuda")
        outs = hip_ops.solve_bottleneck_batched(mats if maximize else [-m for m in mats], maximize, t_out=t_out)
        t_host = t_out.cpu().numpy()
        for (name, A, t, _), o, w, tg in zip(cases, outs, want, t_host):
            got_t = tg if maximize else np.float32(-tg) + np.float32(0)
            assert _bits(got_t) == _bits(t), (name, maximize, got_t, t)
            assert o.is_cuda and torch.equal(o.cpu(), w), (name, maximize)


def _resnet101_cdist_mats():
    """71 cdist-structured matrices with ResNet-101's group sizes, ties injected (duplicated units, rounded distances)."""
    spec = json.load(open(os.path.join(GOLDEN, "spec_resnet101.json")))["spec"]
    g = torch.Generator().manual_seed(7)
    mats = []
    for i, row in enumerate(spec):
        n = row["size"]
        x = torch.randn(n, 16, generator=g)
        y = x[torch.randperm(n, generator=g)] + 0.3 * torch.randn(n, 16, generator=g)
        y[: n // 8] = y[n // 8: 2 * (n // 8)]                  # duplicated units: tied columns
        A = -torch.cdist(x, y)
        if i % 2:
            A = torch.round(A * 4) / 4                            # coarse grid: many tied entries
        mats.append(A.float().contiguous())
    return mats


def test_resnet101_sizes_and_4096_match_host_and_repeat():
    from pleas_merging_amd import hip_ops

    mats = _resnet101_cdist_mats()
    g = torch.Generator().manual_seed(8)
    mats.append(torch.round(torch.randn(4096, 4096, generator=g) * 8) / 8)
    dev = [m.cuda() for m in mats]
    first = hip_ops.solve_bottleneck_batched(dev)
    second = hip_ops.solve_bottleneck_batched(dev)
    for i, (m, a, b) in enumerate(zip(mats, first, second)):
        assert torch.equal(a, b), i
        assert torch.equal(a.cpu(), _host(m)), (i, m.shape[0])


def test_activation_matching_with_minimax_solver(tiny_basic):
    from pleas.core.solvers import hip_solve_minimax_assignment
    from pleas.methods.activation_matching import activation_matching

    t = tiny_basic
    m1, m2 = copy.deepcopy(t.m1).cuda(), copy.deepcopy(t.m2).cuda()
    perm, costs = activation_matching(t.spec, m1, m2, t.batches(), 3, lsa_solver=hip_solve_minimax_assignment,
                                      output_costs=True)
    for k in t.spec:
        assert perm[k].dtype == torch.int64 and torch.equal(perm[k].cpu(), _host(costs[k])), k
    calls = []
    perm2, costs2 = activation_matching(t.spec, m1, m2, t.batches(), 3, lsa_solver=hip_solve_minimax_assignment,
                                        output_costs=True, while_solving=lambda: calls.append(1))
    assert calls == [1]
    for k in t.spec:
        assert torch.equal(perm2[k].cpu(), _host(costs2[k])), k


def test_weight_matching_with_minimax_solver(tiny_basic):
    from pleas.core.solvers import hip_solve_minimax_assignment
    from pleas.methods.weight_matching import weight_matching

    t = tiny_basic
    sa = {k: v.cuda() for k, v in t.m1.state_dict().items()}
    sb = {k: v.cuda() for k, v in t.m2.state_dict().items()}
    got = weight_matching(t.spec, sa, sb, max_iter=5, seed=0, verbose=False, lsa_solver=hip_solve_minimax_assignment)
    want = weight_matching(t.spec, sa, sb, max_iter=5, seed=0, verbose=False, lsa_solver=lambda A: _host(A))
    for k in t.spec:
        assert torch.equal(got[k].cpu(), want[k].cpu()), k


def test_minimax_refusals():
    from pleas.core.solvers import hip_solve_minimax_assignment
    from pleas_merging_amd import hip_ops
    from pleas_merging_amd._lib import PleasHipError

    with pytest.raises(PleasHipError):
        hip_solve_minimax_assignment(torch.randn(8, 8))                       # CPU tensor
    with pytest.raises(PleasHipError):
        hip_solve_minimax_assignment(torch.zeros(4097, 4097, device="cuda"))  # n > PLEAS_LSAP_MAX_N
    bad = torch.randn(16, 16, device="cuda")
    bad[3, 5] = float("nan")
    with pytest.raises(PleasHipError, match="NaN"):
        hip_solve_minimax_assignment(bad)
    # a refused problem does not spoil the others of its batch
    good = torch.randn(16, 16, device="cuda")
    status = []
    outs = hip_ops.solve_bottleneck_batched([good, bad], deferred=status)
    assert status[0].cpu().tolist() == [0, 1]
    assert (outs[1].cpu() == -1).all() and torch.equal(outs[0].cpu(), _host(good))
