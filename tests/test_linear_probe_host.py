"""Host side of the linear probe's ``head="hip"`` / ``cache_features`` options (methods/linear_probe.py, methods/evaluation.py):
the schedule against torch's scheduler, the argument checks, the unchanged defaults.  No GPU."""
import inspect

import pytest
import torch


@pytest.mark.parametrize("T", [1, 2, 12, 40])
def test_cosine_lrs_eta_min_is_torchs_scheduler_exactly(T):
    from pleas.methods.pleas_merging import cosine_lrs_eta_min

    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=1e-3)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T, eta_min=1e-4)
    want = []
    for _ in range(T + 1):
        want.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    assert cosine_lrs_eta_min(1e-3, 1e-4, T, T + 1) == want


def _toy():
    g = torch.Generator().manual_seed(0)
    data = [(torch.randn(4, 6, generator=g), torch.randint(0, 3, (4,), generator=g)) for _ in range(3)]
    torch.manual_seed(1)                           # the same frozen "backbone" at every call
    return torch.nn.Linear(6, 5), data


def test_hip_head_needs_the_model_on_the_gpu():
    from pleas.methods import train_eval_linear_probe
    from pleas_merging_amd.hip_ops import PleasHipError

    model, data = _toy()
    with pytest.raises(PleasHipError):
        train_eval_linear_probe(model, data, data, 3, None, "toy", epochs=1, head="hip")


def test_unknown_head_is_refused():
    from pleas.methods import train_eval_linear_probe

    model, data = _toy()
    with pytest.raises(ValueError):
        train_eval_linear_probe(model, data, data, 3, None, "toy", epochs=1, head="nope")


def test_defaults_are_unchanged_and_names_are_exported():
    import pleas.methods
    import pleas_merging_amd.methods
    from pleas.methods.pleas_merging import train_eval_linear_probe

    params = inspect.signature(train_eval_linear_probe).parameters
    assert (params["backbone"].default, params["head"].default, params["cache_features"].default) == ("modules", "autograd", False)
    for pkg in (pleas.methods, pleas_merging_amd.methods, pleas.methods.pleas_merging):
        assert callable(pkg.cosine_lrs_eta_min) and inspect.isclass(pkg.HipProbeHead)


def test_cached_features_replay_epoch_zero_on_the_cpu():
    """``cache_features=True`` with the autograd head: the backbone sees every training batch once, and with a loader that
    yields the same batches in the same order every epoch the head is the one of ``cache_features=False``, bit for bit."""
    from pleas.methods import train_eval_linear_probe

    heads, calls = [], []
    for cache in (False, True):
        model, data = _toy()
        count = [0]
        model.register_forward_hook(lambda *_: count.__setitem__(0, count[0] + 1))
        torch.manual_seed(0)
        heads.append(train_eval_linear_probe(model, data, data[:2], 3, None, "toy", epochs=3, cache_features=cache))
        calls.append(count[0])
    assert calls == [3 * 3 + 2, 3 + 2]
    assert torch.equal(heads[0].weight, heads[1].weight) and torch.equal(heads[0].bias, heads[1].bias)
