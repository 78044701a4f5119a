"""Data parallelism: who this process is among the ranks, and the exchange steps of both phases.

Rank / world discovery (``_dist_info``), the matching path's all-reduce (``allreduce_sum_``) and the fitters' ``dp_*`` steps on
their flat arenas.  Imports nothing from ``methods/``, so every module there may import it at module level.
"""
import os

import torch
import torch.distributed as dist


def _dist_info():
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return dist.get_rank(), dist.get_world_size()
    # PLEAS_EMULATE_WORLD=N (profiling aid, bench.py --emulate-world): this process does rank 0's share of an N-rank job
    # with the collectives skipped -- the per-rank critical path of a multi-GPU run, timed on one GPU.  The RESULTS of such
    # a run are partial sums and must not be used.
    emulated = int(os.environ.get("PLEAS_EMULATE_WORLD", "0") or 0)
    return (0, emulated) if emulated > 1 else (0, 1)


def _collectives_on() -> bool:
    return dist.is_available() and dist.is_initialized()


def _force_collectives() -> bool:
    """PLEAS_FORCE_COLLECTIVES=1 with ``torch.distributed`` initialised: the path's exchange steps are issued even when
    the group has ONE rank (where a sum over ranks is the identity), so that the very calls an N-rank job makes --
    ``all_reduce`` of the cost arena and of the gradient arena, ``reduce_scatter_tensor`` / ``all_gather_into_tensor``
    under ``shard_optimizer`` -- go through RCCL on a one-GPU box and can be timed there."""
    return os.environ.get("PLEAS_FORCE_COLLECTIVES", "0") not in ("", "0") and _collectives_on()


def allreduce_sum_(flat: torch.Tensor, world: int) -> torch.Tensor:
    """The one exchange step of the matching path: sum the flat cost arena over ranks
    (RCCL over xGMI under the ``nccl`` backend; gloo in the CPU tests)."""
    if (world > 1 and _collectives_on()) or _force_collectives():
        dist.all_reduce(flat, op=dist.ReduceOp.SUM)
    return flat


def dp_slice(x: torch.Tensor, rank: int, world: int) -> torch.Tensor:
    """Rank's share of one batch under data-parallel PLeaS: contiguous, equal sample chunks."""
    if world == 1:
        return x
    if x.shape[0] % world:
        raise RuntimeError("batch of %d samples does not split over %d ranks" % (x.shape[0], world))
    return x.chunk(world)[rank]


def dp_sum_(flat: torch.Tensor, world: int, share: float = 1.0) -> torch.Tensor:
    """Sum of the flat gradient arena over ranks (ONE collective per update).  Each rank scales its
    residual by 2 / (local numel * world), so the sum IS the gradient of the full-batch mean."""
    if world > 1 or _force_collectives():
        if dist.is_initialized():
            dist.all_reduce(flat, op=dist.ReduceOp.SUM)
        else:                           # PLEAS_EMULATE_WORLD (_dist_info): no peers
            _emulated_collective(flat, share)
    return flat


def dp_reduce_scatter_(flat: torch.Tensor, mine: torch.Tensor, rank: int, world: int) -> torch.Tensor:
    """Sum of ``flat`` over ranks, of which this rank needs only its ``rank``-th 1/world slice: ONE reduce-scatter into
    ``mine`` (RCCL); backends without it (gloo, the single-GPU rehearsals) all-reduce and take the slice."""
    n = flat.numel() // world
    if not dist.is_initialized():              # PLEAS_EMULATE_WORLD: no peers
        return flat[rank * n:(rank + 1) * n]
    if dist.get_backend() == "nccl":
        dist.reduce_scatter_tensor(mine, flat, op=dist.ReduceOp.SUM)
        return mine
    dist.all_reduce(flat, op=dist.ReduceOp.SUM)
    return flat[rank * n:(rank + 1) * n]


def dp_all_gather_(flat: torch.Tensor, rank: int, world: int) -> None:
    """Every rank's updated 1/world slice of ``flat`` to all ranks, in place (ONE all-gather)."""
    if not dist.is_initialized():
        return
    n = flat.numel() // world
    mine = flat[rank * n:(rank + 1) * n].clone()       # the collective must not read from its own output
    if dist.get_backend() == "nccl":
        dist.all_gather_into_tensor(flat, mine)
    else:
        dist.all_gather(list(flat.chunk(world)), mine)


_SPIN = {}


def _emulated_collective(flat: torch.Tensor, share: float = 1.0) -> None:
    """Profiling aid: with PLEAS_EMULATE_ALLREDUCE_US=T the stream is held for ``share`` * T microseconds where the
    all-reduce would run (a spin kernel on one CU; T = the whole gradient arena), so that what overlaps a collective
    can be studied on one GPU."""
    us = float(os.environ.get("PLEAS_EMULATE_ALLREDUCE_US", "0") or 0) * share
    if us <= 0 or not flat.is_cuda:
        return
    if "per_us" not in _SPIN:           # calibrate the spin kernel's cycle unit once
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1000)
        a.record()
        torch.cuda._sleep(2_000_000)
        b.record()
        b.synchronize()
        _SPIN["per_us"] = 2_000_000 / (a.elapsed_time(b) * 1e3)
    torch.cuda._sleep(int(us * _SPIN["per_us"]))
