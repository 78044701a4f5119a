"""Tensor-level wrappers over the C-ABI (include/pleas_hip.h).

PyTorch is used for device memory and streams only: every function here enqueues a
hand-written gfx950 kernel on torch's current stream via ctypes.  Inputs must be fp32
CUDA(=HIP) tensors (``image_batch`` / ``image_resample`` / ``image_resample_chain``: uint8 images); anything else raises -- there is no
eager/CPU fallback.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import os
import threading
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import ARITH_FP32, ARITH_SPLIT_BF16, ARITH_SPLIT_BF16_EXACT, EPI_INNER, EPI_NEG_CDIST, PleasHipError, check


class _Pinned(threading.local):
    """Per THREAD: torch's current stream is thread-local, so a handle pinned by one thread must never be seen by
    another (a DataLoader / collate thread, the autograd thread, a second fitter)."""

    depth = 0
    handle = 0


_PINNED = _Pinned()


def _stream() -> int:
    """Raw hipStream_t of torch's current stream.  ``torch.cuda.current_stream()`` costs ~8 us; inside a
    ``pin_stream()`` block (one PLeaS update / matching batch) the handle is looked up once -- by the thread that
    entered the block, for that thread only."""
    if _PINNED.depth > 0:
        return _PINNED.handle
    return torch.cuda.current_stream().cuda_stream


class pin_stream:
    """Context manager: all wrappers called by THIS thread inside reuse the stream handle that is current at entry
    (nested blocks re-pin and restore)."""

    def __enter__(self):
        self._saved = (_PINNED.depth, _PINNED.handle)
        _PINNED.depth += 1
        _PINNED.handle = torch.cuda.current_stream().cuda_stream
        return self

    def __exit__(self, *exc):
        _PINNED.depth, _PINNED.handle = self._saved
        return False


def _need_gpu(*tensors: torch.Tensor) -> None:
    for t in tensors:
        if not t.is_cuda:
            raise PleasHipError("HIP path needs tensors on the GPU (got device %s); no CPU fallback" % t.device)
        if t.dtype != torch.float32:
            raise PleasHipError("HIP path computes in fp32 (got %s)" % t.dtype)


_ROLE_STREAMS = {}


def role_stream(device: torch.device, role: str, priority: int = 0) -> torch.cuda.Stream:
    """ONE HIP stream per (device, role) for the life of the process.  torch's caching allocator keeps freed blocks per
    allocation stream, so a job that created fresh streams could not reuse anything an earlier job (or a warm-up) had
    left behind: it went back to hipMalloc for its ~15 GB of taps per source forward, and the pools of the abandoned
    streams stayed reserved until an out-of-memory retry released them."""
    device = torch.device(device)
    key = (device.index if device.index is not None else torch.cuda.current_device(), role)
    st = _ROLE_STREAMS.get(key)
    if st is None:
        st = _ROLE_STREAMS[key] = torch.cuda.Stream(device, priority=priority)
    return st


def to_device_async(x: torch.Tensor, device: torch.device) -> torch.Tensor:
    """``x`` on ``device``, usable on the CURRENT stream.  The reference moves every batch inside its loops with a blocking
    ``x.cuda()`` (activation_matching.py:121, pleas_merging.py:266).  A PINNED host tensor is copied on a dedicated copy
    stream ("h2d") instead: the host enqueues a loop's kernels far ahead of the GPU, so the copy of batch b + 1 runs while
    batch b computes, and the current stream only waits for the copy's event.  Pageable host tensors and device tensors
    take the ordinary path."""
    device = torch.device(device)
    if x.device == device:
        return x
    if x.is_cuda or not x.is_pinned():
        return x.to(device, non_blocking=True)
    d, ev = h2d_start(x, device)
    return h2d_finish(d, ev, device)


def h2d_start(x: torch.Tensor, device: torch.device):
    """Enqueue the copy of a PINNED host tensor on the copy stream NOW; returns ``(device tensor, event)`` for
    :func:`h2d_finish`.  A caller that knows its next batches starts their copies a whole step early: a process's streams
    share four hardware queues, so a copy enqueued right before it is needed sits behind the kernels already queued there."""
    copy = role_stream(torch.device(device), "h2d")
    with torch.cuda.stream(copy):
        d = x.to(device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(copy)
    return d, ev


def h2d_finish(d: torch.Tensor, ev, device: torch.device) -> torch.Tensor:
    """Make the CURRENT stream wait for a copy started by :func:`h2d_start` and hand the tensor over to it."""
    cur = torch.cuda.current_stream(torch.device(device))
    cur.wait_event(ev)
    d.record_stream(cur)      # allocated in the copy stream's pool, consumed on `cur`
    return d


class Workspace:
    """Grow-only device scratch buffer, one per (device, stream): two streams that run ``gram_accum`` / ``sqerr`` side
    by side must not share scratch.  Callers never see hidden allocations inside the C library."""

    _per_stream: dict = {}

    def __init__(self, device: torch.device):
        self.device = device
        self.buf = torch.empty(0, dtype=torch.uint8, device=device)

    @classmethod
    def get(cls, device: torch.device) -> "Workspace":
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device(), _stream())
        ws = cls._per_stream.get(key)
        if ws is None:
            ws = cls._per_stream[key] = cls(device)
        return ws

    def reserve(self, nbytes: int) -> torch.Tensor:
        if self.buf.numel() < nbytes:
            # the old buffer may still be in use by kernels queued on the current stream, which need not be the stream it
            # was allocated on: tell the caching allocator before dropping it
            if self.buf.numel():
                self.buf.record_stream(torch.cuda.current_stream(self.device))
            self.buf = torch.empty(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=self.device)
        return self.buf


def _as_bchw(t: torch.Tensor, axis: int) -> Tuple[int, int, int]:
    shape = t.shape
    axis = axis % t.dim()
    return math.prod(shape[:axis]), shape[axis], math.prod(shape[axis + 1:])


class _GroupedLaunch:
    """The protocol every grouped launch of the library follows (include/pleas_hip.h), written once: entries are queued by the
    subclass's ``add`` (``_queue``), ``flush`` fills the struct array, sizes a DEDICATED workspace once (the plan's tables live in
    it), launches with the ``ws_fresh`` flag, and sizes the workspace again -- once -- when the library answers
    ``PLEAS_ENOMEM`` because the list now needs more.  ``table`` / ``relaunch`` are the per-update fast path of ``PleasFitter``.

    A subclass states its ctypes struct, the names of its ``*_ws_bytes`` and launch functions, how one entry fills one struct
    row (``_fill``), and the arguments its two calls take beside the protocol's own (``_ws_args`` / ``_launch_args``)."""

    STRUCT = None
    WS_BYTES = LAUNCH = ""
    ENOMEM = -12                   # PLEAS_ENOMEM

    def __init__(self, device: torch.device):
        self.device = device
        self._keep: list = []      # per pending entry: the tensors its row points at (kept alive until the launch is queued)
        self._geo: list = []       # per pending entry: everything else of its row
        self._arr = None
        self._ws = None
        self._fresh = 1

    def _queue(self, tensors: tuple, geo: tuple) -> int:
        self._keep.append(tensors)
        self._geo.append(geo)
        return len(self._keep) - 1

    def _fill(self, row, tensors: tuple, geo: tuple) -> None:
        raise NotImplementedError

    def _ws_args(self) -> tuple:
        return ()

    def _launch_args(self, *args) -> tuple:
        return ()

    def pending(self) -> int:
        """Entries added since the last ``flush`` / ``drop``."""
        return len(self._keep)

    def drop(self) -> None:
        self._keep.clear()
        self._geo.clear()

    def _launch(self, fresh: int, extra: tuple) -> int:
        return getattr(_lib.lib(), self.LAUNCH)(self._arr, len(self._arr), *extra, self._ws.data_ptr(), self._ws.numel(), fresh,
                                                _stream())

    def _flush(self, *args, keep: bool = False) -> None:
        n = len(self._keep)
        if n == 0:
            return
        if self._arr is None or len(self._arr) != n:
            self._arr = (self.STRUCT * n)()
        for row, tensors, geo in zip(self._arr, self._keep, self._geo):
            self._fill(row, tensors, geo)
        extra = self._launch_args(*args)
        rc = self.ENOMEM
        for _ in range(2):         # the second round: the list changed shape and needs more than the workspace holds
            if self._ws is None:
                lib = _lib.lib()
                need = int(getattr(lib, self.WS_BYTES)(self._arr, n, *self._ws_args()))
                if need == 0:
                    raise PleasHipError("%s rejected the list: %s" % (self.WS_BYTES, lib.pleas_last_error().decode()))
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
                self._fresh = 1
            rc = self._launch(self._fresh, extra)
            self._fresh = 0
            if rc != self.ENOMEM:
                break
            self._ws = None
        check(rc, self.LAUNCH)
        if not keep:
            self.drop()

    def flush(self) -> None:
        """ONE grouped launch over everything added since the last flush."""
        self._flush()

    def table(self):
        """numpy view of the struct array of the latest ``flush`` (shares its memory): pointer fields may be rewritten before
        ``relaunch`` -- the per-update fast path of ``PleasFitter``, which keeps every other field as it is."""
        return None if self._arr is None else np.frombuffer(self._arr, dtype=np.dtype(self.STRUCT))

    def relaunch(self, *args) -> None:
        """The launch of the latest ``flush`` again, with the table as it is now."""
        if self._keep or self._arr is None or self._ws is None:
            raise PleasHipError("%s.relaunch: nothing flushed yet, or entries pending" % type(self).__name__)
        check(self._launch(0, self._launch_args(*args)), self.LAUNCH)


# ---------------------------------------------------------------------------------------- gram / cdist
def gram_ws_bytes(B: int, C: int, HW: int) -> int:
    return int(_lib.lib().pleas_gram_ws_bytes(B, C, HW))


def gram_accum(x: torch.Tensor, y: torch.Tensor, axis: int, acc: torch.Tensor, epilogue: int,
               accumulate: bool = True) -> torch.Tensor:
    """acc (+)= cross-features of ``x`` and ``y`` along ``axis`` (see pleas_gram_accum)."""
    _need_gpu(x, y, acc)
    if x.shape != y.shape:
        raise PleasHipError("cross features need equal shapes, got %s and %s" % (tuple(x.shape), tuple(y.shape)))
    x, y = x.contiguous(), y.contiguous()
    B, C, HW = _as_bchw(x, axis)
    if tuple(acc.shape) != (C, C) or not acc.is_contiguous():
        raise PleasHipError("acc must be a contiguous (%d, %d) tensor" % (C, C))
    need = gram_ws_bytes(B, C, HW)
    ws = Workspace.get(x.device).reserve(need)
    rc = _lib.lib().pleas_gram_accum(x.data_ptr(), y.data_ptr(), B, C, HW, epilogue, int(bool(accumulate)),
                                     acc.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    check(rc, "pleas_gram_accum")
    return acc


def cross_features_cdist(x: torch.Tensor, y: torch.Tensor, a: int) -> torch.Tensor:
    """HIP drop-in for the reference's ``cross_features_cdist`` plug point
    (pleas/methods/activation_matching.py:31-46): returns the C x C negative-distance matrix."""
    C = x.shape[a]
    out = torch.empty(C, C, dtype=torch.float32, device=x.device)
    return gram_accum(x, y, a, out, EPI_NEG_CDIST, accumulate=False)


def cross_features_inner_product(x: torch.Tensor, y: torch.Tensor, a: int) -> torch.Tensor:
    """HIP drop-in for ``cross_features_inner_product`` (activation_matching.py:14-28)."""
    C = x.shape[a]
    out = torch.empty(C, C, dtype=torch.float32, device=x.device)
    return gram_accum(x, y, a, out, EPI_INNER, accumulate=False)


class GramBatch(_GroupedLaunch):
    """Collects the tracked nodes of one forward pass and contracts them all in ONE grouped launch
    (``pleas_gram_batch``): ``add`` while the models run, ``flush`` once per batch.

    The operand tensors must stay unmodified until ``flush`` (the twin graph therefore runs ReLU
    out of place); they are released right after the launch is queued.
    """

    STRUCT, WS_BYTES, LAUNCH = _lib.GramNode, "pleas_gram_batch_ws_bytes", "pleas_gram_batch"

    def __init__(self, group_mats: Sequence[torch.Tensor], epilogue: int):
        _need_gpu(*group_mats)
        super().__init__(group_mats[0].device)
        self.mats = list(group_mats)
        self.epilogue = epilogue
        k = len(self.mats)
        self._acc = (ctypes.c_void_p * k)(*[m.data_ptr() for m in self.mats])
        self._gc = (ctypes.c_int * k)(*[m.shape[0] for m in self.mats])

    def add(self, x: torch.Tensor, y: torch.Tensor, axis: int, group: int) -> int:
        """Queue one contracted node; returns its index in this batch (the handle ``add_derived`` refers to)."""
        if x.shape != y.shape or not x.is_cuda or x.dtype != torch.float32 or y.dtype != torch.float32:
            raise PleasHipError("GramBatch.add: fp32 CUDA operands of equal shape expected")
        x, y = x.contiguous(), y.contiguous()
        return self._queue((x, y), _as_bchw(x, axis) + (group, None))

    def add_derived(self, source: int, scale_x: torch.Tensor, shift_x: torch.Tensor, scale_y: torch.Tensor,
                    shift_y: torch.Tensor, group: int) -> int:
        """Queue a node whose operands are per-channel affine images ``scale * v + shift`` of node ``source``'s operands
        (an eval-mode BatchNorm of a tracked convolution): no contraction, the reduce pass derives its contribution."""
        if not 0 <= source < len(self._keep) or self._geo[source][4] is not None:
            raise PleasHipError("GramBatch.add_derived: source must be a contracted node of this batch")
        B, C, HW = self._geo[source][:3]
        for t in (scale_x, shift_x, scale_y, shift_y):
            if not t.is_cuda or t.dtype != torch.float32 or t.numel() != C or not t.is_contiguous():
                raise PleasHipError("GramBatch.add_derived: scale / shift must be contiguous fp32 CUDA vectors of length C")
        return self._queue((scale_x, shift_x, scale_y, shift_y), (B, C, HW, group, source))

    def _fill(self, a, t, geo) -> None:
        a.B, a.C, a.HW, a.group, src = geo
        if src is None:
            a.x, a.y, a.derived, a.source = t[0].data_ptr(), t[1].data_ptr(), 0, 0
            a.scale_x = a.shift_x = a.scale_y = a.shift_y = None
        else:
            a.x = a.y = None
            a.derived, a.source = 1, src
            a.scale_x, a.shift_x, a.scale_y, a.shift_y = (v.data_ptr() for v in t)

    def _ws_args(self) -> tuple:
        return self._gc, len(self.mats)

    def _launch_args(self, accumulate: bool = True) -> tuple:
        return self._acc, self._gc, len(self.mats), self.epilogue, int(bool(accumulate))

    def flush(self, accumulate: bool = True, keep: bool = False) -> None:
        """Contract everything added since the last flush.  ``keep=True`` leaves the node list in place (a caller that
        contracts the same device tensors again)."""
        self._flush(accumulate, keep=keep)

    @staticmethod
    def plan_info(geometries, group_C=None) -> List[dict]:
        """Host-side facts about the grouped launch of a node list (``pleas_gram_batch_plan_info``; no GPU work, no tensors):
        per ``(B, C, HW)`` or ``(B, C, HW, group, source)`` -- ``source``: the index of the node a derived node is an affine
        image of, else ``None`` -- the tile form ``variant`` (0-5) the plan builder picks, the slabs ``S`` of the K axis (0 for
        a derived node), the chunks per slab, the tiles per side, the padded pixels per sample ``HWp`` and whether the node
        writes row sums.  Without ``group_C`` every node that names no group gets one of its own."""
        geometries = [tuple(g) for g in geometries]
        n = len(geometries)
        arr = (_lib.GramNode * max(n, 1))()
        held = (ctypes.c_float * 1)()
        some = ctypes.addressof(held)      # a derived node's scale / shift: checked for NULL, never read
        groups = [] if group_C is None else [int(c) for c in group_C]
        for i, (a, geo) in enumerate(zip(arr, geometries)):
            a.B, a.C, a.HW = (int(v) for v in geo[:3])
            src = geo[4] if len(geo) > 4 else None
            if len(geo) > 3:
                a.group = int(geo[3])
            else:
                a.group = len(groups)
                groups.append(a.C)
            if src is not None:
                a.derived, a.source = 1, int(src)
                a.scale_x = a.shift_x = a.scale_y = a.shift_y = some
        gc = (ctypes.c_int * max(len(groups), 1))(*groups)
        info = (ctypes.c_int * (6 * max(n, 1)))()
        check(_lib.lib().pleas_gram_batch_plan_info(arr if n else None, n, gc, len(groups), info), "pleas_gram_batch_plan_info")
        return [{"variant": info[6 * i], "S": info[6 * i + 1], "chunks_per_slab": info[6 * i + 2], "tiles": info[6 * i + 3],
                 "HWp": info[6 * i + 4], "sums": bool(info[6 * i + 5])} for i in range(n)]


def gram_plan_info(B: int, C: int, HW: int, aligned: bool = True) -> dict:
    """The plan of the single-node entry ``gram_accum`` for a shape (``pleas_gram_plan_info``; no GPU work): tile, floats per
    load ``vec``, split-K slabs ``S`` and chunks per slab, given whether both operands are 16-byte aligned."""
    info = (ctypes.c_int * 4)()
    check(_lib.lib().pleas_gram_plan_info(int(B), int(C), int(HW), int(bool(aligned)), info), "pleas_gram_plan_info")
    return {"tile": info[0], "vec": info[1], "S": info[2], "chunks_per_slab": info[3]}


# ---------------------------------------------------------------------------------------- LAP
def _square_costs(costs: Sequence[torch.Tensor], min_n: int):
    """A list of square device cost matrices as the batched solvers take it: ``(mats, outs, cost_ptrs, out_ptrs, ns)`` with
    ``mats`` kept alive by the caller, ``outs`` the int64 result vectors."""
    _need_gpu(*costs)
    mats = []
    for c in costs:
        if c.dim() != 2 or c.shape[0] != c.shape[1] or c.shape[0] < min_n:
            raise PleasHipError("square cost matrices expected, got %s" % (tuple(c.shape),))
        if c.shape[0] > _lib.LSAP_MAX_N:
            raise PleasHipError("n = %d exceeds PLEAS_LSAP_MAX_N = %d" % (c.shape[0], _lib.LSAP_MAX_N))
        mats.append(c.contiguous())
    outs = [torch.empty(m.shape[0], dtype=torch.int64, device=m.device) for m in mats]
    k = len(mats)
    cost_ptrs = (ctypes.c_void_p * k)(*[m.data_ptr() for m in mats])
    out_ptrs = (ctypes.c_void_p * k)(*[o.data_ptr() for o in outs])
    ns = (ctypes.c_int * k)(*[m.shape[0] for m in mats])
    return mats, outs, cost_ptrs, out_ptrs, ns


def _host_cost(A: torch.Tensor, name: str, device_name: str):
    """A square host cost matrix as the host solvers take it (fp32 / fp64, contiguous) and its int64 result vector."""
    if A.is_cuda:
        raise PleasHipError("%s takes a CPU tensor; use %s for device tensors" % (name, device_name))
    if A.dim() != 2 or A.shape[0] != A.shape[1] or A.shape[0] < 1:
        raise PleasHipError("square cost matrix expected, got %s" % (tuple(A.shape),))
    if A.dtype not in (torch.float32, torch.float64):
        A = A.double()
    return A.contiguous(), torch.empty(A.shape[0], dtype=torch.int64)


def solve_lsa_batched(costs: Sequence[torch.Tensor], maximize: bool = True) -> List[torch.Tensor]:
    """All assignment problems of a model pair in one launch; returns device int64 vectors."""
    if not costs:
        return []
    mats, outs, cost_ptrs, out_ptrs, ns = _square_costs(costs, 0)
    rc = _lib.lib().pleas_lsap_batched(cost_ptrs, ns, len(mats), int(bool(maximize)), out_ptrs, _stream())
    check(rc, "pleas_lsap_batched")
    return outs


def hip_solve_lsa(A: torch.Tensor, maximize: bool = True) -> torch.Tensor:
    """HIP drop-in for ``scipy_solve_lsa`` (pleas/core/solvers.py:18-33): CPU int64 ``col_ind``."""
    return solve_lsa_batched([A], maximize)[0].cpu()


def host_solve_lsa(A: torch.Tensor, maximize: bool = True) -> torch.Tensor:
    """``pleas_lsap_host``: the library's solver on a HOST cost matrix (fp32 / fp64 CPU tensor), synchronous; same
    ``col_ind`` as scipy.  For callers that keep their data on the host (weight matching of CPU state dicts); device
    tensors belong to ``hip_solve_lsa`` and are refused here -- nothing falls back from one to the other."""
    A, out = _host_cost(A, "host_solve_lsa", "hip_solve_lsa")
    check(_lib.lib().pleas_lsap_host(A.data_ptr(), int(A.dtype == torch.float64), A.shape[0], int(bool(maximize)),
                                     out.data_ptr()), "pleas_lsap_host")
    return out


# ---------------------------------------------------------------------------------------- bottleneck assignment
_BN_STATUS = {1: "a NaN or +-inf entry", 2: "an iteration cap was hit", 3: "the replacement value L32 is not finite"}


def check_bottleneck_status(status: torch.Tensor) -> None:
    """Raise ``PleasHipError`` if a status word of ``pleas_bottleneck_batched`` is not 0 (reads it: synchronises)."""
    bad = [(i, int(s)) for i, s in enumerate(status.cpu().tolist()) if s]
    if bad:
        raise PleasHipError("pleas_bottleneck_batched refused problem(s) %s" %
                            ", ".join("%d (%s)" % (i, _BN_STATUS.get(s, "status %d" % s)) for i, s in bad))


def solve_bottleneck_batched(costs: Sequence[torch.Tensor], maximize: bool = True, t_out: Optional[torch.Tensor] = None,
                             deferred: Optional[list] = None) -> List[torch.Tensor]:
    """Lexicographic bottleneck assignment of every matrix in ONE batched call (include/pleas_hip.h): per matrix the
    permutation that maximises its smallest matched entry, then the sum.  Returns device int64 vectors.  ``t_out``: an
    optional fp32 device tensor ``[len(costs)]`` that receives the bottleneck values.  The kernels' status words are
    read (one synchronisation) before returning, unless ``deferred`` is a list: then the status tensor is appended to
    it, for :func:`check_bottleneck_status` once the caller reads the results anyway."""
    if not costs:
        return []
    mats, outs, cost_ptrs, out_ptrs, ns = _square_costs(costs, 1)
    k = len(mats)
    if t_out is not None and (not t_out.is_cuda or t_out.dtype != torch.float32 or t_out.numel() != k
                              or not t_out.is_contiguous()):
        raise PleasHipError("t_out must be a contiguous fp32 device tensor of %d elements" % k)
    lib = _lib.lib()
    nbytes = lib.pleas_bottleneck_ws_bytes(ns, k)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=mats[0].device)        # caching allocator, current stream
    rc = lib.pleas_bottleneck_batched(cost_ptrs, ns, k, int(bool(maximize)), out_ptrs,
                                      t_out.data_ptr() if t_out is not None else None, ws.data_ptr(), nbytes, _stream())
    check(rc, "pleas_bottleneck_batched")
    status = ws[:4 * k].view(torch.int32)
    if deferred is None:
        check_bottleneck_status(status)
    else:
        deferred.append(status)
    return outs


def hip_solve_minimax_assignment(A: torch.Tensor, maximize: bool = True) -> torch.Tensor:
    """HIP drop-in for the reference's ``scipy_solve_minimax_assignment`` (pleas/core/solvers.py:88-115): int64
    ``col_ind`` on ``A``'s device (the reference's tie rule differs: see INTEGRATION.md)."""
    return solve_bottleneck_batched([A], maximize)[0]


def host_solve_minimax_assignment(A: torch.Tensor, maximize: bool = True) -> torch.Tensor:
    """``pleas_bottleneck_host``: the same contract on a HOST matrix (fp32 / fp64 CPU tensor), synchronous, same
    ``col_ind`` as the device path.  Device tensors are refused."""
    A, out = _host_cost(A, "host_solve_minimax_assignment", "hip_solve_minimax_assignment")
    check(_lib.lib().pleas_bottleneck_host(A.data_ptr(), int(A.dtype == torch.float64), A.shape[0], int(bool(maximize)),
                                           out.data_ptr(), None), "pleas_bottleneck_host")
    return out


# ---------------------------------------------------------------------------------------- bn + add + relu
# Activation codes of the fused epilogues (PLEAS_ACT_* of include/pleas_hip.h): the ``relu`` argument of every wrapper below.
ACT_NONE, ACT_RELU, ACT_RELU6 = 0, 1, 2


def _act_code(name: str, relu) -> int:
    """The activation code of a wrapper's ``relu`` argument: ``False`` / ``True`` as ever (none / ReLU), or one of ``ACT_NONE``,
    ``ACT_RELU``, ``ACT_RELU6``.  Anything else is refused here, before the library is reached."""
    if isinstance(relu, (bool, int)) and int(relu) in (ACT_NONE, ACT_RELU, ACT_RELU6):
        return int(relu)
    raise PleasHipError("%s: activation %r is not False, True, ACT_NONE (0), ACT_RELU (1) or ACT_RELU6 (2)" % (name, relu))


def _bn_act_args(name: str, x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, res: Optional[torch.Tensor]):
    """Checks shared by ``bn_act`` and ``bn_act_tracked``: returns ``(x, res, C, batches)``, x and res contiguous.  scale / shift
    ``[batches][C]``: x holds that many batches back to back along dim 0, each with its own affine map."""
    _need_gpu(x, scale, shift)
    if x.dim() < 2:
        raise PleasHipError("%s needs an fp32 [N, C, ...] tensor" % name)
    x = x.contiguous()
    if res is not None:
        if res.shape != x.shape or res.dtype != torch.float32:
            raise PleasHipError("%s: residual shape/dtype differs from x" % name)
        res = res.contiguous()
    C = x.shape[1]
    batches = scale.shape[0] if scale.dim() == 2 else 1
    if scale.numel() != batches * C or shift.shape != scale.shape or not scale.is_contiguous() or not shift.is_contiguous():
        raise PleasHipError("%s: scale/shift must be contiguous with one entry per channel (and batch)" % name)
    if x.shape[0] % batches:
        raise PleasHipError("%s: %d samples do not split into %d batches" % (name, x.shape[0], batches))
    return x, res, C, batches


def bn_act(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, res: Optional[torch.Tensor] = None,
           relu: bool = True) -> torch.Tensor:
    """``act(x * scale[c] + shift[c] (+ res))`` over dim 1 of a contiguous fp32 tensor: inference BatchNorm,
    residual add and activation (``relu``: a bool or an ``ACT_*`` code) of a frozen source model in one pass (``pleas_bn_act``)."""
    relu = _act_code("bn_act", relu)
    x, res, C, batches = _bn_act_args("bn_act", x, scale, shift, res)
    y = torch.empty_like(x)
    ptr = res.data_ptr() if res is not None else None
    if batches == 1:
        check(_lib.lib().pleas_bn_act(x.data_ptr(), scale.data_ptr(), shift.data_ptr(), ptr, y.data_ptr(), x.shape[0], C,
                                      math.prod(x.shape[2:]), relu, _stream()), "pleas_bn_act")
    else:      # the tracked pass without its optional outputs is this pass
        check(_lib.lib().pleas_bn_act_tracked_batches(x.data_ptr(), scale.data_ptr(), shift.data_ptr(), ptr, None, None,
                                                      y.data_ptr(), x.shape[0] // batches, batches, C,
                                                      math.prod(x.shape[2:]), relu, _stream()),
              "pleas_bn_act_tracked_batches")
    return y


def bn_act_maxpool(x: torch.Tensor, scale: Optional[torch.Tensor], shift: Optional[torch.Tensor], kernel: Tuple[int, int],
                   stride: int, padding: int, relu: bool = True) -> torch.Tensor:
    """``max_pool2d(act(x * scale[c] + shift[c]), kernel, stride, padding)`` of a contiguous fp32 NCHW tensor in one pass
    (``pleas_bn_act_maxpool``); ``scale is None``: plain max pooling.  ``relu``: a bool or an ``ACT_*`` code."""
    relu = _act_code("bn_act_maxpool", relu)
    _need_gpu(x) if scale is None else _need_gpu(x, scale, shift)
    if x.dim() != 4 or x.dtype != torch.float32:
        raise PleasHipError("bn_act_maxpool needs an fp32 [N, C, H, W] tensor")
    x = x.contiguous()
    N, C, H, W = x.shape
    if scale is not None and (scale.numel() != C or shift.numel() != C or not scale.is_contiguous() or not shift.is_contiguous()):
        raise PleasHipError("bn_act_maxpool: scale/shift must be contiguous with one entry per channel")
    KH, KW = kernel
    if stride <= 0:
        raise PleasHipError("bn_act_maxpool: stride must be positive")
    Ho, Wo = (H + 2 * padding - KH) // stride + 1, (W + 2 * padding - KW) // stride + 1
    y = torch.empty((N, C, max(Ho, 0), max(Wo, 0)), dtype=torch.float32, device=x.device)
    rc = _lib.lib().pleas_bn_act_maxpool(x.data_ptr(), scale.data_ptr() if scale is not None else None,
                                         shift.data_ptr() if scale is not None else None, y.data_ptr(), N, C, H, W, KH, KW,
                                         stride, padding, relu, _stream())
    check(rc, "pleas_bn_act_maxpool")
    return y


def bn_act_tracked(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, res: Optional[torch.Tensor], relu: bool,
                   keep_bn: bool = True):
    """One pass, every node of the chain kept: returns ``(bn, sum, act)`` = ``(x * scale + shift, bn + res, relu(sum))``;
    ``sum`` is None without a residual and ``act`` is None without ``relu`` (``pleas_bn_act_tracked``).  ``relu``: a bool or an
    ``ACT_*`` code; under ``ACT_RELU6`` ``act`` is ``F.relu6(sum)``.
    ``keep_bn=False``: the BatchNorm value itself is not needed by the caller (its matching cost is derived from the
    convolution node, ``GramBatch.add_derived``) and is not written unless it is the chain's last value."""
    relu = _act_code("bn_act_tracked", relu)
    x, res, C, batches = _bn_act_args("bn_act_tracked", x, scale, shift, res)
    # the last value of the chain goes to `y`; earlier ones to the optional outputs
    y_bn = torch.empty_like(x) if ((res is not None or relu) and keep_bn) else None
    y_sum = torch.empty_like(x) if (res is not None and relu) else None
    y = torch.empty_like(x)
    rc = _lib.lib().pleas_bn_act_tracked_batches(x.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                                 res.data_ptr() if res is not None else None,
                                                 y_bn.data_ptr() if y_bn is not None else None,
                                                 y_sum.data_ptr() if y_sum is not None else None, y.data_ptr(),
                                                 x.shape[0] // batches, batches, C, math.prod(x.shape[2:]), relu, _stream())
    check(rc, "pleas_bn_act_tracked_batches")
    if res is None:
        return (y_bn, None, y) if relu else (y, None, None)
    return (y_bn, y_sum, y) if relu else (y_bn, y, None)


def _bn_pointers(name: str, bn: "torch.nn.BatchNorm2d", device: torch.device, channels: Optional[int] = None) -> tuple:
    """Addresses of ``bn``'s weight, bias, running mean, running variance and batch counter (None where absent or untracked); the first
    four must be contiguous fp32 on ``device`` and, with ``channels``, of that length (a merged model's ``num_features`` may be stale)."""
    track = bn.track_running_stats and bn.running_mean is not None
    tensors = (bn.weight, bn.bias) + ((bn.running_mean, bn.running_var, bn.num_batches_tracked) if track else (None, None, None))
    for t in tensors[:4]:
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != device
                              or (channels is not None and t.numel() != channels)):
            raise PleasHipError("%s: BatchNorm parameters / buffers must be contiguous fp32 %son x's device"
                                % (name, "" if channels is None else "vectors of %d channels " % channels))
    return tuple(t.data_ptr() if t is not None else None for t in tensors)


def _bn_train_args(bn: "torch.nn.BatchNorm2d", x: torch.Tensor, batches: int = 1):
    """Checks and addresses shared by ``bn_train_fold`` and ``BnTrainFold``: ``(n, C, inner, pointers)`` with ``n`` samples per
    batch and ``pointers`` as ``_bn_pointers`` returns them."""
    if x.shape[0] % batches:
        raise PleasHipError("bn_train_fold: %d samples do not split into %d batches" % (x.shape[0], batches))
    n, C = x.shape[0] // batches, x.shape[1]
    inner = math.prod(x.shape[2:])
    if n * inner <= 1:
        raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (tuple(x.shape),))
    return n, C, inner, _bn_pointers("bn_train_fold", bn, x.device)


def bn_train_fold(bn: "torch.nn.BatchNorm2d", x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Train-mode ``bn`` on ``x`` as a per-channel affine map: returns fp32 device vectors ``(scale, shift)`` with
    ``F.batch_norm(x, ..., training=True) == x * scale[c] + shift[c]`` and updates ``bn``'s running statistics and
    ``num_batches_tracked`` exactly as the module's forward would (``pleas_bn_train_fold``).  The caller applies the map
    with ``bn_act`` / ``bn_act_tracked``."""
    _need_gpu(x)
    if x.dim() < 2:
        raise PleasHipError("bn_train_fold needs an [N, C, ...] tensor")
    x = x.contiguous()
    n, C, inner, (w, b, rm, rv, nbt) = _bn_train_args(bn, x)
    lib = _lib.lib()
    need = int(lib.pleas_bn_train_ws_bytes(n, C))
    ws = torch.empty(need // 8, dtype=torch.float64, device=x.device)
    out = torch.empty(2, C, dtype=torch.float32, device=x.device)
    rc = lib.pleas_bn_train_fold(x.data_ptr(), n, C, inner, w, b, float(bn.eps), -1.0 if bn.momentum is None else float(bn.momentum), rm, rv, nbt,
                                 out[0].data_ptr(), out[1].data_ptr(), ws.data_ptr(), need, _stream())
    check(rc, "pleas_bn_train_fold")
    return out[0], out[1]


class _PerModuleFold:
    """What the per-module train-mode callables share: the module, and what their cached arguments depend on."""

    def __init__(self, bn: "torch.nn.BatchNorm2d"):
        self.bn = bn
        self._shape = None

    def _addresses(self) -> tuple:
        """Compared per call: the addresses of the module's parameters / buffers (``.to()`` swaps ``.data`` under the SAME objects), and the
        last two arguments they go with: ``eps``, and the momentum (-1: the cumulative average of ``momentum=None``)."""
        bn = self.bn
        return tuple(t.data_ptr() if t is not None else 0 for t in
                     (bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked)) + (
                         float(bn.eps), -1.0 if bn.momentum is None else float(bn.momentum))


class BnTrainFold(_PerModuleFold):
    """``bn_train_fold`` for ONE BatchNorm2d called batch after batch (graph callable of the matching twin in train mode and
    of the BN-reset pass): workspace, output vectors and the module's parameter / buffer addresses are looked up once per
    input shape instead of per call -- those passes are bound by host dispatch (104 BatchNorm2d per ResNet-101 forward).
    The returned ``(scale, shift)`` are views of a buffer that the NEXT call overwrites: consume them on the same stream
    before folding the next batch (what a forward pass does)."""

    def _prepare(self, x: torch.Tensor, batches: int) -> None:
        bn = self.bn
        n, C, inner, (w, b, rm, rv, nbt) = _bn_train_args(bn, x, batches)
        need = batches * int(_lib.lib().pleas_bn_train_ws_bytes(n, C))
        self._ws = torch.empty(need // 8, dtype=torch.float64, device=x.device)
        self._out = torch.empty(2, batches, C, dtype=torch.float32, device=x.device)
        self._tensors = self._addresses()
        self._args = (n, batches, C, inner, w, b) + self._tensors[-2:] + (rm, rv, nbt,
                      self._out[0].data_ptr(), self._out[1].data_ptr(), self._ws.data_ptr(), need)
        self._shape = (tuple(x.shape), x.device, batches)

    def __call__(self, x: torch.Tensor, batches: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
        """``batches`` > 1: ``x`` is that many batches back to back along dim 0; each is folded on its own samples, in
        order (running statistics and counter as after that many forwards); returns ``[batches, C]`` scale and shift."""
        if not x.is_cuda or x.dtype != torch.float32 or x.dim() < 2:
            raise PleasHipError("bn_train_fold needs an fp32 [N, C, ...] tensor on the GPU")
        x = x.contiguous()
        if self._shape != (tuple(x.shape), x.device, batches) or self._tensors != self._addresses():
            self._prepare(x, batches)
        rc = _lib.lib().pleas_bn_train_fold_batches(x.data_ptr(), *self._args, _stream())
        check(rc, "pleas_bn_train_fold_batches")
        return (self._out[0, 0], self._out[1, 0]) if batches == 1 else (self._out[0], self._out[1])


# ---------------------------------------------------------------------------------------- merge blocks
def merge_blocks(w1: torch.Tensor, w2: torch.Tensor, row_axis: int, row1: torch.Tensor, row2: torch.Tensor,
                 n_merged_rows: int, col1: Optional[torch.Tensor] = None, col2: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Block gather/average along ``row_axis`` (and ``row_axis + 1`` when column maps are given)."""
    _need_gpu(w1, w2)
    if w1.shape != w2.shape:
        raise PleasHipError("merge_blocks needs equal source shapes")
    w1, w2 = w1.contiguous(), w2.contiguous()
    shape = list(w1.shape)
    row_axis = row_axis % w1.dim()
    outer = math.prod(shape[:row_axis])
    rows_src = shape[row_axis]
    rows_out = int(row1.numel())
    if col1 is not None:
        cols_src, cols_out = shape[row_axis + 1], int(col1.numel())
        inner = math.prod(shape[row_axis + 2:])
        out_shape = shape[:row_axis] + [rows_out, cols_out] + shape[row_axis + 2:]
    else:
        cols_src = cols_out = 1
        inner = math.prod(shape[row_axis + 1:])
        out_shape = shape[:row_axis] + [rows_out] + shape[row_axis + 1:]
    maps = [row1, row2] + ([col1, col2] if col1 is not None else [])
    for m in maps:
        if not m.is_cuda or m.dtype != torch.int32 or not m.is_contiguous():
            raise PleasHipError("index maps must be contiguous int32 CUDA tensors")
    if out is None:
        out = torch.empty(out_shape, dtype=torch.float32, device=w1.device)
    elif list(out.shape) != out_shape or not out.is_contiguous():
        raise PleasHipError("out has the wrong shape")
    rc = _lib.lib().pleas_merge_blocks(
        w1.data_ptr(), w2.data_ptr(), out.data_ptr(), outer, rows_out, cols_out, inner, rows_src, cols_src,
        row1.data_ptr(), row2.data_ptr(), col1.data_ptr() if col1 is not None else None,
        col2.data_ptr() if col2 is not None else None, int(n_merged_rows), _stream())
    check(rc, "pleas_merge_blocks")
    return out


# ---------------------------------------------------------------------------------------- Adam / loss
def masked_adam(p: torch.Tensor, g: torch.Tensor, mask: Optional[torch.Tensor], m: torch.Tensor, v: torch.Tensor,
                lr: float, step: int, b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8) -> None:
    _need_gpu(p, g, m, v)
    n = p.numel()
    for t in (g, m, v) + ((mask,) if mask is not None else ()):
        if t.numel() != n or not t.is_contiguous():
            raise PleasHipError("masked_adam operands must be contiguous and equally sized")
    rc = _lib.lib().pleas_masked_adam(p.data_ptr(), g.data_ptr(), mask.data_ptr() if mask is not None else None,
                                      m.data_ptr(), v.data_ptr(), n, lr, b1, b2, eps, step, _stream())
    check(rc, "pleas_masked_adam")


def channel_sum(x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """``out[c] = sum over n, p of x[n][c][p]`` (``x`` [N, C, ...] contiguous fp32): the bias gradient of a merged layer from
    its residual (reference: the bias node of ``total.backward()``, pleas_merging.py:287)."""
    _need_gpu(x, out)
    if not x.is_contiguous() or x.dim() < 2 or out.numel() != x.shape[1] or not out.is_contiguous():
        raise PleasHipError("channel_sum: x must be contiguous [N, C, ...] and out hold C floats")
    check(_lib.lib().pleas_channel_sum(x.data_ptr(), x.shape[0], x.shape[1], math.prod(x.shape[2:]), out.data_ptr(), _stream()),
          "pleas_channel_sum")
    return out


def sqerr(a: torch.Tensor, b: torch.Tensor, scale: float, out: torch.Tensor, accumulate: bool = False,
          diff: Optional[torch.Tensor] = None, dscale: float = 1.0) -> torch.Tensor:
    """out[0] (+)= scale * sum((a-b)^2); optionally diff = dscale * (a-b)."""
    _need_gpu(a, b, out)
    if a.shape != b.shape or not a.is_contiguous() or not b.is_contiguous():
        raise PleasHipError("sqerr operands must be contiguous and equally shaped")
    n = a.numel()
    need = int(_lib.lib().pleas_sqerr_ws_bytes(n))
    ws = Workspace.get(a.device).reserve(need)
    rc = _lib.lib().pleas_sqerr(a.data_ptr(), b.data_ptr(), n, scale, int(bool(accumulate)), out.data_ptr(), dscale,
                                diff.data_ptr() if diff is not None else None, ws.data_ptr(), ws.numel(), _stream())
    check(rc, "pleas_sqerr")
    return out


STREAM_OPS = ("merge_blocks", "bn_act", "bn_act_maxpool", "masked_adam", "sqerr", "target_residual", "channel_sum",
              "pool_gather", "top1_count", "bn_train_fold")      # PLEAS_STREAM_*, in order


def stream_plan_info(op: str, *geo: int, aligned: bool = True) -> dict:
    """The launch shape of a streaming kernel for a geometry (``pleas_stream_plan_info``; no GPU work, no tensors), computed by
    the function the launch computes it with.  ``op``: a name of ``STREAM_OPS``; ``geo``: that kernel's sizes in the order
    include/pleas_hip.h lists them; ``aligned``: whether every pointer of the launch's 16-byte predicate is 16-byte aligned.
    Returns ``vec`` (floats per load, 4 / 1), ``form`` (bn_act_maxpool: "general" / "stem"), ``blocks``, ``threads``, ``sweeps`` of
    the grid-stride loop (channel_sum / bn_train_fold: trips of a thread's loop over one slab) and, for bn_train_fold, ``S``."""
    if op not in STREAM_OPS:
        raise PleasHipError("stream_plan_info: unknown kernel %r" % (op,))
    g = (ctypes.c_int64 * max(len(geo), 1))(*(int(v) for v in geo))
    info = (ctypes.c_int * 6)()
    check(_lib.lib().pleas_stream_plan_info(STREAM_OPS.index(op), g, len(geo), int(bool(aligned)), info), "pleas_stream_plan_info")
    out = {"vec": info[0], "blocks": info[2], "threads": info[3], "sweeps": info[4]}
    if op == "bn_act_maxpool":
        out["form"] = ("general", "stem")[info[1]]
    if op == "bn_train_fold":
        out["S"] = info[5]
    return out


# ---------------------------------------------------------------------------------------- PLeaS layer fitting
def target_residual(out: torch.Tensor, o1: torch.Tensor, o2: torch.Tensor, row1: torch.Tensor, row2: torch.Tensor,
                    n_merged: int, dscale: float, partials: torch.Tensor, resid: Optional[torch.Tensor] = None) -> int:
    """resid = dscale * (out - blockmerge(o1, o2)); per-workgroup sums of squares -> ``partials``.
    ``resid`` defaults to ``out`` (in place).  Returns the number of partials written."""
    _need_gpu(out, o1, o2, partials)
    if resid is None:
        resid = out
    if not (out.is_contiguous() and o1.is_contiguous() and o2.is_contiguous() and resid.is_contiguous()):
        raise PleasHipError("target_residual operands must be contiguous")
    N, C = out.shape[0], out.shape[1]
    HW = math.prod(out.shape[2:])
    if o1.shape != o2.shape or o1.shape[0] != N or math.prod(o1.shape[2:]) != HW or row1.numel() != C:
        raise PleasHipError("target_residual: shapes of merged output, source outputs and maps disagree")
    n = ctypes.c_int(0)
    rc = _lib.lib().pleas_target_residual(out.data_ptr(), o1.data_ptr(), o2.data_ptr(), row1.data_ptr(), row2.data_ptr(),
                                          int(n_merged), N, C, o1.shape[1], HW, dscale, resid.data_ptr(),
                                          partials.data_ptr(), ctypes.byref(n), _stream())
    check(rc, "pleas_target_residual")
    return n.value


def target_residual_max_partials() -> int:
    return int(_lib.lib().pleas_target_residual_max_partials())


def loss_final(partials: torch.Tensor, n_partials: torch.Tensor, scale: torch.Tensor, loss: torch.Tensor) -> None:
    """loss[l] = scale[l] * sum(partials[l, :n_partials[l]]) for all layers in one launch."""
    L, stride = partials.shape
    rc = _lib.lib().pleas_loss_final(partials.data_ptr(), n_partials.data_ptr(), scale.data_ptr(), stride, L,
                                     loss.data_ptr(), _stream())
    check(rc, "pleas_loss_final")


class MergeBatch(_GroupedLaunch):
    """Block gather / average of many tensors along one axis in ONE grouped launch (``pleas_merge_batch``): the merged
    inputs of all layers of a PLeaS update.  ``add`` returns the output tensor (filled at ``flush``)."""

    STRUCT, WS_BYTES, LAUNCH = _lib.MergeItem, "pleas_merge_batch_ws_bytes", "pleas_merge_batch"

    def add(self, w1: torch.Tensor, w2: torch.Tensor, row_axis: int, row1: torch.Tensor, row2: torch.Tensor,
            n_merged_rows: int, out: Optional[torch.Tensor] = None, subsample: int = 1) -> torch.Tensor:
        """``subsample`` = s > 1 (``[N, C, H, W]`` sources merged along axis 1 only): the output keeps every s-th pixel of
        every s-th line, ``[N, rows, ceil(H / s), ceil(W / s)]`` -- what a 1x1 convolution with stride s reads."""
        if w1.shape != w2.shape or not w1.is_cuda or w1.dtype != torch.float32 or w2.dtype != torch.float32:
            raise PleasHipError("MergeBatch.add: fp32 CUDA sources of equal shape expected")
        w1, w2 = w1.contiguous(), w2.contiguous()
        shape = list(w1.shape)
        row_axis = row_axis % w1.dim()
        rows_out = int(row1.numel())
        want = shape[:row_axis] + [rows_out] + shape[row_axis + 1:]
        sub = (0, 0, 0)
        if subsample > 1:
            if w1.dim() != 4 or row_axis != 1:
                raise PleasHipError("MergeBatch.add: subsample needs [N, C, H, W] sources merged along axis 1")
            sub = (int(subsample), shape[2], shape[3])
            want = want[:2] + [-(-shape[2] // subsample), -(-shape[3] // subsample)]
        if out is None:
            out = torch.empty(want, dtype=torch.float32, device=w1.device)
        elif list(out.shape) != want or out.dtype != torch.float32 or not out.is_contiguous() or out.device != w1.device:
            raise PleasHipError("MergeBatch.add: out must be a contiguous fp32 tensor of shape %s" % (want,))
        self._queue((w1, w2, out, row1, row2), (math.prod(shape[:row_axis]), math.prod(want[row_axis + 1:]), rows_out,
                                                shape[row_axis], int(n_merged_rows)) + sub)
        return out

    def _fill(self, a, tensors, geo) -> None:
        a.w1, a.w2, a.out, a.row1, a.row2 = (t.data_ptr() for t in tensors)
        a.outer, a.inner, a.rows_out, a.rows_src, a.n_merged, a.sub_stride, a.sub_h, a.sub_w = geo


def fwd_plan_lanes() -> dict:
    """Per tile form of the latest grouped forward: measured duration on its lane [ms], lane, work items
    (``pleas_fwd_plan_lanes``); ``state`` 2 = the lanes were dealt from those measurements."""
    ms, lane, items = (ctypes.c_double * 10)(), (ctypes.c_int * 10)(), (ctypes.c_int * 10)()
    state = _lib.lib().pleas_fwd_plan_lanes(ms, lane, items)
    return {"state": state, "forms": {f: {"ms": round(ms[f], 4), "lane": lane[f], "items": items[f]} for f in range(10) if items[f]}}


class FwdBatch(_GroupedLaunch):
    """Forward + target + residual + loss of all merged layers of one update in ONE grouped launch
    (``pleas_fwd_batch``).  ``add`` per layer, ``flush(loss)`` once per update."""

    STRUCT, WS_BYTES, LAUNCH = _lib.FwdLayer, "pleas_fwd_batch_ws_bytes", "pleas_fwd_batch"
    KPOS_MAJOR = 1   # w is [Cout][KH][KW][Cin] (needs Cin % 32 == 0)

    def add(self, ip, w, bias, o1, o2, row1, row2, n_merged: int, resid, dscale: float, loss_scale: float,
            kernel=(1, 1), stride: int = 1, pad: int = 0, flags: int = 0) -> None:
        for t in (ip, w, o1, o2, resid):
            if not t.is_contiguous():
                raise PleasHipError("FwdBatch.add: contiguous tensors expected")
        N, Cin = ip.shape[0], ip.shape[1]
        Hin, Win = (ip.shape[2], ip.shape[3]) if ip.dim() == 4 else (1, 1)
        self._queue((ip, w, bias, o1, o2, row1, row2, resid),
                    (N, w.shape[0], Cin, Hin, Win, kernel[0], kernel[1], stride, pad, o1.shape[1], int(n_merged),
                     float(dscale), float(loss_scale), int(flags)))

    def _fill(self, a, tensors, geo) -> None:
        a.ip, a.w, a.bias, a.o1, a.o2, a.row1, a.row2, a.resid = (t.data_ptr() if t is not None else None for t in tensors)
        (a.N, a.Cout, a.Cin, a.Hin, a.Win, a.KH, a.KW, a.stride, a.pad, a.Csrc, a.n_merged, a.dscale, a.loss_scale,
         a.flags) = geo

    def _launch_args(self, loss: torch.Tensor) -> tuple:
        if loss.numel() != len(self._arr) or not loss.is_contiguous():
            raise PleasHipError("FwdBatch: loss must hold one float per layer")
        return (loss.data_ptr(),)

    def flush(self, loss: torch.Tensor) -> None:
        self._flush(loss)


def _conv_call(name: str, x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], stride: int, pad: int, kpos_major: bool, *also):
    """The argument runs every ``pleas_conv2d_*`` entry point takes for a dense square convolution of contiguous tensors (fp32 on the GPU, as
    ``also`` must be): ``(x, w, bias addresses)``, ``(N, Cin, H, W, Cout, KH, KW, stride, pad, flags)``, the output's shape ``(N, Cout, Ho, Wo)``."""
    _need_gpu(x, w, *also)
    if x.dim() != 4 or w.dim() != 4 or not x.is_contiguous() or not w.is_contiguous():
        raise PleasHipError("%s: contiguous 4-D tensors expected" % name)
    N, Cin, H, W = x.shape
    KH, KW = (w.shape[1], w.shape[2]) if kpos_major else (w.shape[2], w.shape[3])
    if (w.shape[3] if kpos_major else w.shape[1]) != Cin:
        raise PleasHipError("%s: %d input channels vs a weight of %s" % (name, Cin, tuple(w.shape)))
    return ((x.data_ptr(), w.data_ptr(), bias.data_ptr() if bias is not None else None),
            (N, Cin, H, W, w.shape[0], KH, KW, stride, pad, FwdBatch.KPOS_MAJOR if kpos_major else 0),
            (N, w.shape[0], (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1))


def _image_operands(name: str, x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, res: Optional[torch.Tensor], out_shape):
    """Addresses of the image operands: contiguous scale / shift (fp32 on the GPU: ``_conv_call``) of ``Cout`` elements, an identity like z."""
    Cout = out_shape[1]
    if scale.numel() != Cout or shift.numel() != Cout or not scale.is_contiguous() or not shift.is_contiguous():
        raise PleasHipError("%s: scale / shift must be contiguous fp32 vectors of %d channels" % (name, Cout))
    if res is not None and (tuple(res.shape) != out_shape or res.dtype != torch.float32 or not res.is_contiguous()
                            or res.device != x.device):
        raise PleasHipError("%s: the identity must be a contiguous fp32 tensor shaped like the output" % name)
    return scale.data_ptr(), shift.data_ptr(), res.data_ptr() if res is not None else None


def conv2d(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], stride: int, pad: int, kpos_major: bool = False,
           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``F.conv2d(x, w, bias, stride, pad)`` for dense, undilated, square geometries on the grouped forward's tile forms
    (``pleas_conv2d_fwd``): fp32 MFMA, a fixed summation order -- the same bits run after run, which MIOpen's 3 x 3
    kernels are not (they split K with atomics on small images / batches; tools/r05/probe_conv_classes.py).
    ``kpos_major``: ``w`` is ``[Cout][KH][KW][Cin]`` (needs Cin % 32 == 0; the flat-shift forms of stride-1 layers)."""
    operands, geometry, out_shape = _conv_call("conv2d", x, w, bias, stride, pad, kpos_major)
    if out is None:
        out = torch.empty(out_shape, dtype=torch.float32, device=x.device)
    check(_lib.lib().pleas_conv2d_fwd(*operands, out.data_ptr(), *geometry, _stream()), "pleas_conv2d_fwd")
    return out


# ---------------------------------------------------------------------------------------- depthwise convolutions
# Who runs a depthwise nn.Conv2d (groups == in_channels == out_channels) of the source / twin / evaluation forwards and of the fit:
#   "vendor"  the module on the vendor's grouped convolution, the fit by autograd layer by layer: every release so far (the default)
#   "hip"     csrc/dwconv.hip: ``dwconv2d`` in the forwards, ``DwFwdBatch`` / ``DwWgradBatch`` in the fit
# ``PLEAS_DEPTHWISE`` in the environment sets the process's form, ``depthwise_form`` a block's.
DEPTHWISE_FORMS = ("vendor", "hip")
DW_MAX_KERNEL = 7


def _depthwise_form_checked(mode) -> str:
    if mode not in DEPTHWISE_FORMS:
        raise ValueError("depthwise form %r is not one of %s" % (mode, DEPTHWISE_FORMS))
    return mode


DEPTHWISE = _depthwise_form_checked(os.environ.get("PLEAS_DEPTHWISE", "vendor"))


@contextlib.contextmanager
def depthwise_form(mode: str):
    """``DEPTHWISE = mode`` for the block, the previous form again afterwards (also when the block raises).  Process-wide, as
    ``linear_form``.  Graphs and fitters read the form when they are BUILT."""
    global DEPTHWISE
    before, DEPTHWISE = DEPTHWISE, _depthwise_form_checked(mode)
    try:
        yield
    finally:
        DEPTHWISE = before


def dwconv_geometry_ok(k: int, stride: int, pad: int) -> bool:
    """The geometries of csrc/dwconv.hip: K odd in 1 .. 7, stride 1 or 2, pad <= K // 2."""
    return 1 <= k <= DW_MAX_KERNEL and k % 2 == 1 and stride in (1, 2) and 0 <= pad <= k // 2


def _dw_image(name: str, what: str, t: Optional[torch.Tensor], shape, device) -> Optional[int]:
    if t is None:
        return None
    if (not t.is_cuda or t.device != device or t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous()
            or t.data_ptr() % 16):
        raise PleasHipError("%s: %s must be a contiguous, 16-byte aligned fp32 tensor of shape %s on the input's device"
                            % (name, what, tuple(shape)))
    return t.data_ptr()


def _dw_vector(name: str, what: str, t: Optional[torch.Tensor], C: int, device) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda or t.device != device or t.dtype != torch.float32 or t.numel() != C or not t.is_contiguous():
        raise PleasHipError("%s: %s must be a contiguous fp32 tensor of %d elements on the input's device" % (name, what, C))
    return t.data_ptr()


def dwconv2d(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], stride: int, pad: int,
             scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None,
             relu: bool = False, out: Optional[torch.Tensor] = None, act_out: Optional[torch.Tensor] = None):
    """``F.conv2d(x, w, bias, stride, pad, groups=C)`` for a depthwise layer (``pleas_dwconv2d_fwd``): ``x`` [N, C, H, W], ``w``
    [C, 1, K, K], K odd up to 7, stride 1 or 2, pad <= K // 2; one fmaf chain per output in a fixed order.

    Without ``scale`` / ``act_out``: returns ``y`` (into ``out`` when given).  With ``scale`` and ``shift`` (fp32 [C]): also
    ``z = act(fma(y, scale, shift) (+ res))``, bit for bit ``bn_act(y, scale, shift, res, relu)``, and returns ``(y, z)``; with
    ``out=False`` ``y`` is not stored and ``z`` alone is returned (``act_out``: the tensor ``z`` goes to).  ``relu``: a bool or an
    ``ACT_*`` code."""
    name = "dwconv2d"
    relu = _act_code(name, relu)
    _need_gpu(x, w)
    if x.dim() != 4 or not x.is_contiguous() or x.data_ptr() % 16:
        raise PleasHipError("%s: a contiguous, 16-byte aligned [N, C, H, W] input expected, got %s" % (name, tuple(x.shape)))
    N, C, H, W = x.shape
    if w.dim() != 4 or w.shape[0] != C or w.shape[1] != 1 or w.shape[2] != w.shape[3]:
        raise PleasHipError("%s: a [C, 1, K, K] weight for %d channels expected, got %s" % (name, C, tuple(w.shape)))
    K = int(w.shape[2])
    if w.device != x.device or not w.is_contiguous() or w.data_ptr() % 16:
        raise PleasHipError("%s: the weight must be contiguous, 16-byte aligned and on the input's device" % name)
    stride, pad = int(stride), int(pad)
    if not dwconv_geometry_ok(K, stride, pad):
        raise PleasHipError("%s: K = %d, stride %d, pad %d is outside K odd in 1 .. %d, stride 1 or 2, pad <= K // 2"
                            % (name, K, stride, pad, DW_MAX_KERNEL))
    Ho, Wo = (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1
    if Ho <= 0 or Wo <= 0:
        raise PleasHipError("%s: a %d x %d kernel does not fit the padded %d x %d image" % (name, K, K, H + 2 * pad, W + 2 * pad))
    shape, dev = (N, C, Ho, Wo), x.device
    if (scale is None) != (shift is None):
        raise PleasHipError("%s: scale and shift come together" % name)
    image = scale is not None or act_out is not None
    if not image and (res is not None or relu or out is False):
        raise PleasHipError("%s: res / relu / out=False need scale and shift (or act_out)" % name)
    ptrs = (_dw_vector(name, "bias", bias, C, dev), _dw_vector(name, "scale", scale, C, dev), _dw_vector(name, "shift", shift, C, dev),
            _dw_image(name, "res", res, shape, dev))
    y = z = None
    if out is not False:
        y = out if out is not None else torch.empty(shape, dtype=torch.float32, device=dev)
        _dw_image(name, "out", y, shape, dev)
    if image:
        z = act_out if act_out is not None else torch.empty(shape, dtype=torch.float32, device=dev)
        _dw_image(name, "act_out", z, shape, dev)
    check(_lib.lib().pleas_dwconv2d_fwd(x.data_ptr(), w.data_ptr(), ptrs[0], y.data_ptr() if y is not None else None, ptrs[1], ptrs[2],
                                        ptrs[3], z.data_ptr() if z is not None else None, relu, N, C, H, W, K, stride, pad,
                                        _stream()), "pleas_dwconv2d_fwd")
    if not image:
        return y
    return z if y is None else (y, z)


class DwFwdBatch(_GroupedLaunch):
    """Forward + target + residual + loss of the depthwise layers of one update in ONE grouped launch (``pleas_dw_fwd_batch``):
    ``FwdBatch``'s contract per layer.  ``add`` per layer, ``flush(loss)`` once per update."""

    STRUCT, WS_BYTES, LAUNCH = _lib.DwLayer, "pleas_dw_fwd_batch_ws_bytes", "pleas_dw_fwd_batch"

    def add(self, ip, w, bias, o1, o2, row1, row2, n_merged: int, resid, dscale: float, loss_scale: float,
            stride: int = 1, pad: int = 0) -> None:
        for t in (ip, w, o1, o2, resid):
            if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
                raise PleasHipError("DwFwdBatch.add: contiguous fp32 tensors on the GPU expected")
        if ip.dim() != 4 or w.dim() != 4 or w.shape[0] != ip.shape[1] or w.shape[1] != 1 or w.shape[2] != w.shape[3]:
            raise PleasHipError("DwFwdBatch.add: ip [N, C, H, W] and w [C, 1, K, K] expected, got %s and %s" % (tuple(ip.shape), tuple(w.shape)))
        N, C, Hin, Win = ip.shape
        K = int(w.shape[2])
        want = (N, C, (Hin + 2 * pad - K) // stride + 1, (Win + 2 * pad - K) // stride + 1)
        if tuple(resid.shape) != want or o1.shape != o2.shape or o1.dim() != 4 or (o1.shape[0],) + tuple(o1.shape[2:]) != (N,) + want[2:]:
            raise PleasHipError("DwFwdBatch.add: resid must be %s and o1 / o2 [N, Csrc, Ho, Wo]" % (want,))
        for r in (row1, row2):
            if not r.is_cuda or r.dtype != torch.int32 or r.numel() != C or not r.is_contiguous():
                raise PleasHipError("DwFwdBatch.add: row maps must be contiguous int32 tensors of %d entries on the GPU" % C)
        if bias is not None and (not bias.is_cuda or bias.dtype != torch.float32 or bias.numel() != C or not bias.is_contiguous()):
            raise PleasHipError("DwFwdBatch.add: bias must be a contiguous fp32 tensor of %d elements on the GPU" % C)
        self._queue((ip, w, bias, o1, o2, row1, row2, resid),
                    (N, C, Hin, Win, K, int(stride), int(pad), o1.shape[1], int(n_merged), float(dscale), float(loss_scale)))

    def _fill(self, a, tensors, geo) -> None:
        a.ip, a.w, a.bias, a.o1, a.o2, a.row1, a.row2, a.resid = (t.data_ptr() if t is not None else None for t in tensors)
        a.N, a.C, a.Hin, a.Win, a.K, a.stride, a.pad, a.Csrc, a.n_merged, a.dscale, a.loss_scale = geo

    def _launch_args(self, loss: torch.Tensor) -> tuple:
        if loss.numel() != len(self._arr) or not loss.is_contiguous() or loss.dtype != torch.float32 or not loss.is_cuda:
            raise PleasHipError("DwFwdBatch: loss must hold one fp32 value per layer on the GPU")
        return (loss.data_ptr(),)

    def flush(self, loss: torch.Tensor) -> None:
        self._flush(loss)


class DwWgradBatch(_GroupedLaunch):
    """Weight gradients of the depthwise layers of one update in ONE grouped launch (``pleas_dw_wgrad_batch``): ``grad`` [C, 1, K, K]
    from the residual [N, C, Ho, Wo] and the merged input [N, C, H, W]; two stages, fixed order."""

    STRUCT, WS_BYTES, LAUNCH = _lib.DwWgradLayer, "pleas_dw_wgrad_batch_ws_bytes", "pleas_dw_wgrad_batch"

    def add(self, resid: torch.Tensor, ip: torch.Tensor, grad: torch.Tensor, stride: int = 1, pad: int = 0) -> None:
        for t in (resid, ip, grad):
            if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
                raise PleasHipError("DwWgradBatch.add: contiguous fp32 tensors on the GPU expected")
        if ip.dim() != 4 or grad.dim() != 4 or grad.shape[0] != ip.shape[1] or grad.shape[1] != 1 or grad.shape[2] != grad.shape[3]:
            raise PleasHipError("DwWgradBatch.add: ip [N, C, H, W] and grad [C, 1, K, K] expected, got %s and %s"
                                % (tuple(ip.shape), tuple(grad.shape)))
        N, C, Hin, Win = ip.shape
        K = int(grad.shape[2])
        want = (N, C, (Hin + 2 * pad - K) // stride + 1, (Win + 2 * pad - K) // stride + 1)
        if tuple(resid.shape) != want:
            raise PleasHipError("DwWgradBatch.add: resid must be %s, got %s" % (want, tuple(resid.shape)))
        self._queue((resid, ip, grad), (N, C, Hin, Win, K, int(stride), int(pad)))

    def _fill(self, a, tensors, geo) -> None:
        a.resid, a.ip, a.grad = (t.data_ptr() for t in tensors)
        a.N, a.C, a.Hin, a.Win, a.K, a.stride, a.pad = geo


# ---------------------------------------------------------------------------------------- depthwise closed form
# What ``solver="normal_eq"`` does with a depthwise layer the Adam fitter takes on its own kernels (``plan.dw``):
#   "refuse"  the fitter refuses the network, as every release so far (the default)
#   "hip"     csrc/dw_normal_eq.hip: per-channel normal equations by ``DwNormalEqBatch``, solved by ``dw_normal_eq_solve``
# ``PLEAS_DEPTHWISE_CLOSED_FORM`` in the environment sets the process's mode, ``depthwise_closed_form`` a block's.
DEPTHWISE_CLOSED_FORMS = ("refuse", "hip")


def _depthwise_closed_form_checked(mode) -> str:
    if mode not in DEPTHWISE_CLOSED_FORMS:
        raise ValueError("depthwise closed form %r is not one of %s" % (mode, DEPTHWISE_CLOSED_FORMS))
    return mode


DEPTHWISE_CLOSED_FORM = _depthwise_closed_form_checked(os.environ.get("PLEAS_DEPTHWISE_CLOSED_FORM", "refuse"))


@contextlib.contextmanager
def depthwise_closed_form(mode: str):
    """``DEPTHWISE_CLOSED_FORM = mode`` for the block, the previous mode again afterwards (also when the block raises).
    Process-wide, as ``depthwise_form``.  ``NormalEqFitter`` reads the mode when it is BUILT."""
    global DEPTHWISE_CLOSED_FORM
    before, DEPTHWISE_CLOSED_FORM = DEPTHWISE_CLOSED_FORM, _depthwise_closed_form_checked(mode)
    try:
        yield
    finally:
        DEPTHWISE_CLOSED_FORM = before


class DwNormalEqBatch(_GroupedLaunch):
    """Per-channel normal equations of the depthwise layers of one batch in ONE grouped launch (``pleas_dw_normal_eq_accum``):
    ``S[c] += sum_r v_r v_r^T`` with ``v_r`` = (the K*K taps of ``ip`` under output pixel r, 1, the merged target of (o1, o2, row1,
    row2, n_merged)); ``S`` fp64 [C, D, D], D = K*K + 2, lower triangle.  Two entries of one launch may not share an ``S``."""

    STRUCT, WS_BYTES, LAUNCH = _lib.DwNeqLayer, "pleas_dw_normal_eq_ws_bytes", "pleas_dw_normal_eq_accum"

    def add(self, ip, o1, o2, row1, row2, n_merged: int, S, stride: int = 1, pad: int = 0) -> None:
        for t in (ip, o1, o2):
            if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
                raise PleasHipError("DwNormalEqBatch.add: contiguous fp32 tensors on the GPU expected")
        if ip.dim() != 4 or not S.is_cuda or S.dtype != torch.float64 or not S.is_contiguous() or S.dim() != 3 or S.shape[0] != ip.shape[1] \
                or S.shape[1] != S.shape[2]:
            raise PleasHipError("DwNormalEqBatch.add: ip [N, C, H, W] and a contiguous fp64 S [C, D, D] on the GPU expected, got %s and %s"
                                % (tuple(ip.shape), tuple(S.shape)))
        N, C, Hin, Win = ip.shape
        K = math.isqrt(max(0, int(S.shape[1]) - 2))
        if K * K + 2 != S.shape[1]:
            raise PleasHipError("DwNormalEqBatch.add: S must be [C, K*K + 2, K*K + 2], got %s" % (tuple(S.shape),))
        want = (N, (Hin + 2 * pad - K) // stride + 1, (Win + 2 * pad - K) // stride + 1)
        if o1.shape != o2.shape or o1.dim() != 4 or (o1.shape[0],) + tuple(o1.shape[2:]) != want:
            raise PleasHipError("DwNormalEqBatch.add: o1 / o2 must be [N, Csrc, Ho, Wo] = [%d, Csrc, %d, %d]" % want)
        for r in (row1, row2):
            if not r.is_cuda or r.dtype != torch.int32 or r.numel() != C or not r.is_contiguous():
                raise PleasHipError("DwNormalEqBatch.add: row maps must be contiguous int32 tensors of %d entries on the GPU" % C)
        self._queue((ip, o1, o2, row1, row2, S), (N, C, Hin, Win, K, int(stride), int(pad), o1.shape[1], int(n_merged)))

    def _fill(self, a, tensors, geo) -> None:
        a.ip, a.o1, a.o2, a.row1, a.row2, a.S = (t.data_ptr() for t in tensors)
        a.N, a.C, a.Hin, a.Win, a.K, a.stride, a.pad, a.Csrc, a.n_merged = geo


def _dw_neq_solve_args(name: str, S: torch.Tensor, K: int, has_bias: bool, w: torch.Tensor, bias: Optional[torch.Tensor], cuda: bool):
    K = int(K)
    D = K * K + 2
    if S.dtype != torch.float64 or S.dim() != 3 or tuple(S.shape[1:]) != (D, D) or not S.is_contiguous() or S.is_cuda != cuda:
        raise PleasHipError("%s: a contiguous fp64 S [C, %d, %d] in %s memory expected, got %s"
                            % (name, D, D, "device" if cuda else "host", tuple(S.shape)))
    C = int(S.shape[0])
    if w.dtype != torch.float32 or w.numel() != C * K * K or not w.is_contiguous() or w.device != S.device:
        raise PleasHipError("%s: w must be a contiguous fp32 [C, 1, K, K] tensor beside S" % name)
    if has_bias and (bias is None or bias.dtype != torch.float32 or bias.numel() != C or not bias.is_contiguous() or bias.device != S.device):
        raise PleasHipError("%s: has_bias needs a contiguous fp32 bias of %d elements beside S" % (name, C))
    status = torch.zeros(C, dtype=torch.int32, device=S.device)
    return C, K, status


def dw_normal_eq_solve(S: torch.Tensor, K: int, has_bias: bool, ridge: float, w: torch.Tensor,
                       bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per channel ``(G_T + ridge * mean(diag G_T) I) x = h_T`` from ``S`` (``DwNormalEqBatch``) by fp64 Cholesky, ``x`` rounded once to
    fp32 into ``w[c]`` (and ``bias[c]``) in place (``pleas_dw_normal_eq_solve``).  Returns the int32 status per channel: 1 = a pivot
    was not positive, that channel's ``w`` and ``bias`` are untouched."""
    C, K, status = _dw_neq_solve_args("dw_normal_eq_solve", S, K, has_bias, w, bias, True)
    check(_lib.lib().pleas_dw_normal_eq_solve(S.data_ptr(), C, K, int(bool(has_bias)), float(ridge), w.data_ptr(),
                                              bias.data_ptr() if has_bias else None, status.data_ptr(), _stream()),
          "pleas_dw_normal_eq_solve")
    return status


def dw_normal_eq_solve_host(S: torch.Tensor, K: int, has_bias: bool, ridge: float, w: torch.Tensor,
                            bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``dw_normal_eq_solve`` on host tensors (``pleas_dw_normal_eq_solve_host``: the same routine, no GPU)."""
    C, K, status = _dw_neq_solve_args("dw_normal_eq_solve_host", S, K, has_bias, w, bias, False)
    check(_lib.lib().pleas_dw_normal_eq_solve_host(S.data_ptr(), C, K, int(bool(has_bias)), float(ridge), w.data_ptr(),
                                                   bias.data_ptr() if has_bias else None, status.data_ptr(), None),
          "pleas_dw_normal_eq_solve_host")
    return status


# ---------------------------------------------------------------------------------------- Linear
# Which kernel an nn.Linear the library runs itself goes through (the probe's head, the inference graph's classifier):
#   "conv"  ``pleas_conv2d_fwd`` with H = W = KH = KW = 1 on 4-D views, and ``channel_sum`` for the bias gradient: the calls and
#           the bits of every release so far (the default)
#   "gemm"  ``pleas_linear_fwd``, the split-K NT tile of csrc/linear.hip, and ``column_sum``
# Both are deterministic.  ``PLEAS_LINEAR`` in the environment sets the process's form, ``linear_form`` a block's.
LINEAR_FORMS = ("conv", "gemm")


def _linear_form_checked(mode) -> str:
    if mode not in LINEAR_FORMS:
        raise ValueError("linear form %r is not one of %s" % (mode, LINEAR_FORMS))
    return mode


LINEAR = _linear_form_checked(os.environ.get("PLEAS_LINEAR", "conv"))


@contextlib.contextmanager
def linear_form(mode: str):
    """``LINEAR = mode`` for the block, the previous form again afterwards (also when the block raises).  Process-wide, as
    ``arith``: not for blocks that run beside other threads' launches."""
    global LINEAR
    before, LINEAR = LINEAR, _linear_form_checked(mode)
    try:
        yield
    finally:
        LINEAR = before


def linear_plan_info(N: int, C: int, K: int) -> Tuple[int, int, int, int, int]:
    """``(sample tiles, class tiles, S, chunks per K range, chunks of the last range)`` of ``pleas_linear_fwd``; host only."""
    info = (ctypes.c_int * 5)()
    check(_lib.lib().pleas_linear_plan_info(N, C, K, info), "pleas_linear_plan_info")
    return tuple(info)


def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``F.linear(x, w, bias)`` for fp32 ``x`` [N, K] and contiguous ``w`` [C, K] on the GPU, into ``out`` [N, C] when given.
    The kernel is the one ``LINEAR`` names.  A non-contiguous ``x`` is copied first; under "conv" so is a ``x`` that is not
    16-byte aligned (what the two callers of ``conv2d`` did), under "gemm" it is read where it lies with 4-byte loads."""
    _need_gpu(x, w)
    if x.dim() != 2 or w.dim() != 2 or w.shape[1] != x.shape[1] or w.device != x.device or not w.is_contiguous():
        raise PleasHipError("linear: x [N, K] and a contiguous w [C, K] on one device expected, got %s and %s on %s / %s"
                            % (tuple(x.shape), tuple(w.shape), x.device, w.device))
    (N, K), C = x.shape, w.shape[0]
    if bias is not None and (bias.device != x.device or bias.dtype != torch.float32 or bias.numel() != C or not bias.is_contiguous()):
        raise PleasHipError("linear: bias must be a contiguous fp32 tensor of %d elements on the operands' device" % C)
    if out is None:
        out = torch.empty((N, C), dtype=torch.float32, device=x.device)
    elif out.device != x.device or out.dtype != torch.float32 or tuple(out.shape) != (N, C) or not out.is_contiguous():
        raise PleasHipError("linear: out must be a contiguous fp32 tensor of shape (%d, %d) on the operands' device" % (N, C))
    form = LINEAR
    if not x.is_contiguous() or (form == "conv" and x.data_ptr() % 16):
        x = x.clone(memory_format=torch.contiguous_format)
    if form == "conv":
        conv2d(x.view(N, K, 1, 1), w.view(C, K, 1, 1), bias, 1, 0, out=out.view(N, C, 1, 1))
        return out
    need = int(_lib.lib().pleas_linear_ws_bytes(N, C, K))
    ws = Workspace.get(x.device).reserve(need) if need else None
    check(_lib.lib().pleas_linear_fwd(x.data_ptr(), w.data_ptr(), bias.data_ptr() if bias is not None else None, out.data_ptr(),
                                      N, C, K, ws.data_ptr() if need else None, ws.numel() if need else 0, _stream()),
          "pleas_linear_fwd")
    return out


def column_sum(x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """``out[c] = sum over n of x[n][c]`` (``x`` [N, C] contiguous fp32, N, C >= 1): the bias gradient of a Linear from the
    gradient of its output, row-parallel (``pleas_column_sum``)."""
    _need_gpu(x, out)
    if x.dim() != 2 or not x.is_contiguous() or x.shape[0] < 1 or x.shape[1] < 1:
        raise PleasHipError("column_sum: x must be a contiguous, non-empty [N, C] tensor, got %s" % (tuple(x.shape),))
    if out.device != x.device or out.numel() != x.shape[1] or not out.is_contiguous():
        raise PleasHipError("column_sum: out must hold %d contiguous floats on x's device" % x.shape[1])
    check(_lib.lib().pleas_column_sum(x.data_ptr(), x.shape[0], x.shape[1], out.data_ptr(), _stream()), "pleas_column_sum")
    return out


IMAGE_LAYOUTS = {"nhwc": _lib.IMAGE_NHWC, "nchw": _lib.IMAGE_NCHW}


def image_table(mean=None, std=None, channels: int = 3) -> torch.Tensor:
    """The [channels, 256] fp32 table of ``image_batch``, built on the CPU with torch's own fp32 arithmetic:
    ``table[c][v] = ((v / 255) - mean[c]) / std[c]`` -- ``ToTensor`` then ``Normalize`` as the reference's drivers apply them, so a
    lookup reproduces their bits by construction.  ``mean=None`` / ``std=None``: that step is left out (both: the plain ``/ 255``
    of ``ToTensor``).  ``mean`` / ``std``: a number or one per channel.  Move the table to the GPU once (``.to(device)``)."""
    channels = int(channels)
    if not 1 <= channels <= 4:
        raise PleasHipError("image_table: channels must lie in 1 .. 4, got %d" % channels)
    table = (torch.arange(256, dtype=torch.float32) / 255).repeat(channels, 1)
    for name, v in (("mean", mean), ("std", std)):
        if v is None:
            continue
        v = torch.as_tensor(v, dtype=torch.float32).reshape(-1)
        if v.numel() not in (1, channels):
            raise PleasHipError("image_table: %s must hold one value or %d, got %d" % (name, channels, v.numel()))
        v = v.expand(channels).reshape(channels, 1)
        table = table.sub(v) if name == "mean" else table.div(v)
    return table.contiguous()


def image_batch(src_u8: torch.Tensor, table: torch.Tensor, out: Optional[torch.Tensor] = None, origin=None, flip=None,
                size: Optional[Tuple[int, int]] = None, layout: str = "nhwc") -> torch.Tensor:
    """uint8 images on the GPU to normalised fp32 [N, C, Ho, Wo] in one pass (``pleas_image_batch``):
    ``out[n, c, y, x] = table[c, src[n, y0 + y, x0 + xs, c]]`` with ``xs = Wo - 1 - x`` for a flipped sample, else ``x``.

    ``src_u8``: contiguous uint8 on the GPU, [N, H, W, C] (``layout="nhwc"``) or [N, C, H, W] (``"nchw"``), C in 1 .. 4, any
    alignment.  ``table``: ``image_table(...)`` on the same device.  ``size=(Ho, Wo)``: the window (default: the whole image).
    ``origin``: HOST integers [N, 2], ``(y0, x0)`` per sample (default ``(0, 0)``), checked HERE against ``[0, H - Ho]`` x
    ``[0, W - Wo]`` and then uploaded -- the kernel does not look again.  ``flip``: HOST flags [N].  ``out``: a contiguous fp32
    [N, C, Ho, Wo] tensor on the device, 16-byte aligned (allocated when not given)."""
    if not torch.is_tensor(src_u8) or src_u8.dtype != torch.uint8:
        raise PleasHipError("image_batch: src must be a uint8 tensor (got %s)" % getattr(src_u8, "dtype", type(src_u8)))
    if layout not in IMAGE_LAYOUTS:
        raise PleasHipError("image_batch: layout must be one of %r, got %r" % (tuple(IMAGE_LAYOUTS), layout))
    if src_u8.dim() != 4 or not src_u8.is_contiguous():
        raise PleasHipError("image_batch: src must be a contiguous 4-d tensor, got shape %s" % (tuple(src_u8.shape),))
    N, (H, W, C) = src_u8.shape[0], (src_u8.shape[1:] if layout == "nhwc" else (src_u8.shape[2], src_u8.shape[3], src_u8.shape[1]))
    if not 1 <= C <= 4:
        raise PleasHipError("image_batch: %d channels (layout %r); the kernel takes 1 .. 4" % (C, layout))
    if H < 1 or W < 1 or H >= 1 << 31 or W >= 1 << 31:
        raise PleasHipError("image_batch: empty or oversized images, shape %s" % (tuple(src_u8.shape),))
    Ho, Wo = (H, W) if size is None else (int(size[0]), int(size[1]))
    if not (1 <= Ho <= H and 1 <= Wo <= W):
        raise PleasHipError("image_batch: the window %s must be positive and fit inside the %d x %d image" % ((Ho, Wo), H, W))
    if origin is not None:
        if torch.is_tensor(origin) and origin.is_cuda:
            raise PleasHipError("image_batch: origins are checked on the host: pass a CPU tensor or a sequence")
        origin = torch.as_tensor(origin)
        if origin.dtype.is_floating_point or origin.dtype == torch.bool or tuple(origin.shape) != (N, 2):
            raise PleasHipError("image_batch: origin must hold integers of shape (%d, 2), got %s %s" % (N, origin.dtype, tuple(origin.shape)))
        origin = origin.to(torch.int64)
        if N and (int(origin.min()) < 0 or int(origin[:, 0].max()) > H - Ho or int(origin[:, 1].max()) > W - Wo):
            raise PleasHipError("image_batch: origin outside [0, %d] x [0, %d] (image %d x %d, window %d x %d)"
                                % (H - Ho, W - Wo, H, W, Ho, Wo))
    if flip is not None:
        if torch.is_tensor(flip) and flip.is_cuda:
            raise PleasHipError("image_batch: flip flags are host values: pass a CPU tensor or a sequence")
        flip = torch.as_tensor(flip)
        if tuple(flip.shape) != (N,):
            raise PleasHipError("image_batch: flip must hold %d flags, got shape %s" % (N, tuple(flip.shape)))
        flip = flip.ne(0).to(torch.uint8)
    if out is not None and (not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != (N, C, Ho, Wo) or not out.is_contiguous()
                            or out.data_ptr() % 16):
        raise PleasHipError("image_batch: out must be a contiguous, 16-byte aligned fp32 tensor of shape %s on the GPU"
                            % ((N, C, Ho, Wo),))
    if not src_u8.is_cuda:
        raise PleasHipError("HIP path needs tensors on the GPU (got device %s); no CPU fallback" % src_u8.device)
    _need_gpu(table)
    if table.device != src_u8.device or tuple(table.shape) != (C, 256) or not table.is_contiguous():
        raise PleasHipError("image_batch: table must be a contiguous fp32 [%d, 256] tensor on src's device" % C)
    if out is None:
        out = torch.empty((N, C, Ho, Wo), dtype=torch.float32, device=src_u8.device)
    elif out.device != src_u8.device:
        raise PleasHipError("image_batch: out must be on src's device")
    if N == 0:
        return out
    dev = src_u8.device
    origin_d = origin.to(torch.int32).contiguous().to(dev) if origin is not None else None
    flip_d = flip.contiguous().to(dev) if flip is not None else None
    check(_lib.lib().pleas_image_batch(src_u8.data_ptr(), out.data_ptr(), table.data_ptr(),
                                       origin_d.data_ptr() if origin_d is not None else None,
                                       flip_d.data_ptr() if flip_d is not None else None, N, C, H, W, Ho, Wo,
                                       IMAGE_LAYOUTS[layout], _stream()), "pleas_image_batch")
    return out


RESAMPLE_GEOM = 10      # int32 per sample: H, W, y0, x0, h, w, Hv, Wv, oy, ox (include/pleas_hip.h)


def _resample_geom(geom) -> torch.Tensor:
    if torch.is_tensor(geom) and geom.is_cuda:
        raise PleasHipError("image_resample_plan: the geometry is checked on the host: pass a CPU tensor or a sequence")
    geom = torch.as_tensor(geom)
    if geom.dtype.is_floating_point or geom.dtype == torch.bool or geom.dim() != 2 or geom.shape[1] != RESAMPLE_GEOM:
        raise PleasHipError("image_resample_plan: geom must hold integers of shape (N, %d), got %s %s"
                            % (RESAMPLE_GEOM, geom.dtype, tuple(geom.shape)))
    if geom.numel() and (int(geom.min()) < -(1 << 31) or int(geom.max()) >= 1 << 31):
        raise PleasHipError("image_resample_plan: geom does not fit int32")
    return geom.to(torch.int32).contiguous()


def image_resample_plan_bytes(geom, size: Tuple[int, int]) -> int:
    """Bytes of the plan of ``geom`` for outputs of ``size=(Ho, Wo)`` (``pleas_resample_plan_bytes``; refusals raise)."""
    geom = _resample_geom(geom)
    n = _lib.lib().pleas_resample_plan_bytes(geom.data_ptr(), geom.shape[0], int(size[0]), int(size[1]))
    if n == 0:
        raise PleasHipError("pleas_resample_plan_bytes: %s" % _lib.lib().pleas_last_error().decode())
    return n


def image_resample_plan(geom, src_offset, channels: int, size: Tuple[int, int], src_bytes: int,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The plan of ``image_resample`` for one ragged batch (``pleas_resample_plan``; host only): a uint8 tensor, pinned where a
    GPU is present, or the leading bytes of ``out`` (a contiguous uint8 HOST tensor on a 4-byte boundary, e.g. a staging buffer
    that also takes the images, so that one copy carries both).

    ``geom``: HOST integers [N, 10] per sample -- ``H, W`` (image), ``y0, x0, h, w`` (box), ``Hv, Wv`` (virtual output the box
    is resampled to), ``oy, ox`` (origin of the ``size=(Ho, Wo)`` window produced).  ``src_offset``: HOST integers [N], the byte
    offset of each packed uint8 ``[H, W, C]`` image in a buffer of ``src_bytes``.  Everything is validated by the library; a
    refusal raises ``PleasHipError``."""
    geom = _resample_geom(geom)
    n = geom.shape[0]
    if torch.is_tensor(src_offset) and src_offset.is_cuda:
        raise PleasHipError("image_resample_plan: offsets are checked on the host: pass a CPU tensor or a sequence")
    src_offset = torch.as_tensor(src_offset, dtype=torch.int64) if not torch.is_tensor(src_offset) and not len(src_offset) \
        else torch.as_tensor(src_offset)
    if src_offset.dtype.is_floating_point or src_offset.dtype == torch.bool or tuple(src_offset.shape) != (n,):
        raise PleasHipError("image_resample_plan: src_offset must hold %d integers, got %s %s" % (n, src_offset.dtype, tuple(src_offset.shape)))
    src_offset = src_offset.to(torch.int64).contiguous()
    nbytes = image_resample_plan_bytes(geom, size)
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8)
        if torch.cuda.is_available():
            out = out.pin_memory()
    elif (not torch.is_tensor(out) or out.dtype != torch.uint8 or out.is_cuda or not out.is_contiguous() or out.numel() < nbytes
          or out.data_ptr() % 4):
        raise PleasHipError("image_resample_plan: out must be a contiguous uint8 host tensor of at least %d bytes on a 4-byte boundary" % nbytes)
    plan = out.view(-1)[:nbytes]
    check(_lib.lib().pleas_resample_plan(geom.data_ptr(), src_offset.data_ptr(), n, int(channels), int(size[0]), int(size[1]),
                                         int(src_bytes), plan.data_ptr(), nbytes), "pleas_resample_plan")
    return plan


def image_resample_plan_info(plan: torch.Tensor) -> dict:
    """What a HOST plan says of itself: ``n, channels, size, src_bytes, ws_bytes, items`` (``pleas_resample_plan_info``)."""
    if not torch.is_tensor(plan) or plan.dtype != torch.uint8 or plan.is_cuda or not plan.is_contiguous():
        raise PleasHipError("image_resample: the host plan must be a contiguous uint8 CPU tensor (image_resample_plan's)")
    info = (ctypes.c_int64 * 8)()
    check(_lib.lib().pleas_resample_plan_info(plan.data_ptr(), plan.numel(), info), "pleas_resample_plan_info")
    return {"n": info[0], "channels": info[1], "size": (info[2], info[3]), "src_bytes": info[4], "ws_bytes": info[5],
            "items": (info[6], info[7])}


def _resample_flip(flip, n: int):
    if flip is None:
        return None
    flip = torch.as_tensor(flip)
    if tuple(flip.shape) != (n,):
        raise PleasHipError("image_resample: flip must hold %d flags, got shape %s" % (n, tuple(flip.shape)))
    return flip if flip.dtype == torch.uint8 and flip.is_contiguous() else flip.ne(0).to(torch.uint8).contiguous()


def image_resample_host(src_u8: torch.Tensor, plan: torch.Tensor, table: torch.Tensor, flip=None):
    """A plan executed on the CPU, item by item as the two kernels do (``pleas_image_resample_host``): returns ``(fp32 [N, C, Ho,
    Wo], uint8 [N, Ho, Wo, C])`` -- the resampled bytes through ``table``, and the bytes themselves, both after the flip.  The
    explicit host entry point of this path (what the GPU tests compare with); nothing here touches a device."""
    info = image_resample_plan_info(plan)
    n, c, (ho, wo) = info["n"], info["channels"], info["size"]
    if not torch.is_tensor(src_u8) or src_u8.dtype != torch.uint8 or src_u8.is_cuda or not src_u8.is_contiguous():
        raise PleasHipError("image_resample_host: src must be a contiguous uint8 CPU tensor")
    if src_u8.numel() < info["src_bytes"]:
        raise PleasHipError("image_resample_host: src holds %d bytes, the plan was built for %d" % (src_u8.numel(), info["src_bytes"]))
    if table.is_cuda or table.dtype != torch.float32 or tuple(table.shape) != (c, 256) or not table.is_contiguous():
        raise PleasHipError("image_resample_host: table must be a contiguous fp32 [%d, 256] CPU tensor" % c)
    flip = _resample_flip(flip, n)
    if flip is not None and flip.is_cuda:
        raise PleasHipError("image_resample_host: flip flags must be host values")
    f32, u8 = torch.empty((n, c, ho, wo), dtype=torch.float32), torch.empty((n, ho, wo, c), dtype=torch.uint8)
    check(_lib.lib().pleas_image_resample_host(src_u8.data_ptr(), plan.data_ptr(), plan.numel(), table.data_ptr(),
                                               flip.data_ptr() if flip is not None else None, f32.data_ptr(), u8.data_ptr()),
          "pleas_image_resample_host")
    return f32, u8


def image_resample(src_u8: torch.Tensor, plan_dev: torch.Tensor, plan: torch.Tensor, table: torch.Tensor, flip=None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Packed uint8 images of mixed sizes on the GPU to normalised fp32 [N, C, Ho, Wo]: PIL's 8-bit bilinear resampling (crop +
    resize, or resize + window), flip and table lookup in two launches (``pleas_image_resample``).

    ``src_u8``: the packed buffer the plan was built for, contiguous uint8 on the GPU, any alignment.  ``plan``: the HOST plan
    of ``image_resample_plan``; ``plan_dev``: its copy on src's device (uint8, 4-byte aligned) -- the kernels index with
    nothing else.  ``table``: ``image_table(...)`` on the device.  ``flip``: [N] flags, host values (uploaded) or a uint8 tensor
    already on the device.  ``out``: a contiguous, 16-byte aligned fp32 [N, C, Ho, Wo] tensor on the device (allocated when
    not given).  The scratch for the horizontally resampled rows comes from the stream's ``Workspace``."""
    if not torch.is_tensor(src_u8) or src_u8.dtype != torch.uint8:
        raise PleasHipError("image_resample: src must be a uint8 tensor (got %s)" % getattr(src_u8, "dtype", type(src_u8)))
    if not src_u8.is_contiguous():
        raise PleasHipError("image_resample: src must be contiguous (one packed buffer)")
    info = image_resample_plan_info(plan)
    n, c, (ho, wo) = info["n"], info["channels"], info["size"]
    if src_u8.numel() < info["src_bytes"]:
        raise PleasHipError("image_resample: src holds %d bytes, the plan was built for %d" % (src_u8.numel(), info["src_bytes"]))
    flip = _resample_flip(flip, n)
    if out is not None and (not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != (n, c, ho, wo) or not out.is_contiguous()
                            or out.data_ptr() % 16):
        raise PleasHipError("image_resample: out must be a contiguous, 16-byte aligned fp32 tensor of shape %s on the GPU"
                            % ((n, c, ho, wo),))
    if not src_u8.is_cuda:
        raise PleasHipError("HIP path needs tensors on the GPU (got device %s); no CPU fallback" % src_u8.device)
    dev = src_u8.device
    _need_gpu(table)
    if table.device != dev or tuple(table.shape) != (c, 256) or not table.is_contiguous():
        raise PleasHipError("image_resample: table must be a contiguous fp32 [%d, 256] tensor on src's device" % c)
    if (not torch.is_tensor(plan_dev) or plan_dev.dtype != torch.uint8 or plan_dev.device != dev or not plan_dev.is_contiguous()
            or plan_dev.numel() < plan.numel() or plan_dev.data_ptr() % 4):
        raise PleasHipError("image_resample: plan_dev must be the plan's %d bytes as a contiguous uint8 tensor on src's device, "
                            "4-byte aligned" % plan.numel())
    if out is None:
        out = torch.empty((n, c, ho, wo), dtype=torch.float32, device=dev)
    elif out.device != dev:
        raise PleasHipError("image_resample: out must be on src's device")
    if n == 0:
        return out
    if flip is not None and flip.device != dev:
        flip = flip.to(dev)
    ws = Workspace.get(dev).reserve(info["ws_bytes"])
    check(_lib.lib().pleas_image_resample(src_u8.data_ptr(), plan_dev.data_ptr(), plan.data_ptr(), plan.numel(), table.data_ptr(),
                                          flip.data_ptr() if flip is not None else None, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                          _stream()), "pleas_image_resample")
    return out


RESAMPLE_CHAIN_GEOM = 8      # int32 per sample: H, W, H1, W1, y0, x0, h, w (include/pleas_hip.h)


def _resample_chain_geom(geom) -> torch.Tensor:
    if torch.is_tensor(geom) and geom.is_cuda:
        raise PleasHipError("image_resample_chain_plan: the geometry is checked on the host: pass a CPU tensor or a sequence")
    geom = torch.as_tensor(geom)
    if geom.dtype.is_floating_point or geom.dtype == torch.bool or geom.dim() != 2 or geom.shape[1] != RESAMPLE_CHAIN_GEOM:
        raise PleasHipError("image_resample_chain_plan: geom must hold integers of shape (N, %d), got %s %s"
                            % (RESAMPLE_CHAIN_GEOM, geom.dtype, tuple(geom.shape)))
    if geom.numel() and (int(geom.min()) < -(1 << 31) or int(geom.max()) >= 1 << 31):
        raise PleasHipError("image_resample_chain_plan: geom does not fit int32")
    return geom.to(torch.int32).contiguous()


def image_resample_chain_plan_bytes(geom, size: Tuple[int, int]) -> int:
    """Bytes of the chain plan of ``geom`` for outputs of ``size=(Ho, Wo)`` (``pleas_resample_chain_plan_bytes``; refusals raise)."""
    geom = _resample_chain_geom(geom)
    n = _lib.lib().pleas_resample_chain_plan_bytes(geom.data_ptr(), geom.shape[0], int(size[0]), int(size[1]))
    if n == 0:
        raise PleasHipError("pleas_resample_chain_plan_bytes: %s" % _lib.lib().pleas_last_error().decode())
    return n


def image_resample_chain_plan(geom, src_offset, channels: int, size: Tuple[int, int], src_bytes: int,
                              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The plan of ``image_resample_chain`` for one ragged batch (``pleas_resample_chain_plan``; host only): a uint8 tensor,
    pinned where a GPU is present, or the leading bytes of ``out`` (as ``image_resample_plan``'s).

    ``geom``: HOST integers [N, 8] per sample -- ``H, W`` (image), ``H1, W1`` (its size after the first resize), ``y0, x0, h, w``
    (box inside ``H1 x W1``, resampled to ``size=(Ho, Wo)``).  ``src_offset``, ``src_bytes``: as ``image_resample_plan``'s.
    Everything is validated by the library; a refusal raises ``PleasHipError``."""
    geom = _resample_chain_geom(geom)
    n = geom.shape[0]
    if torch.is_tensor(src_offset) and src_offset.is_cuda:
        raise PleasHipError("image_resample_chain_plan: offsets are checked on the host: pass a CPU tensor or a sequence")
    src_offset = torch.as_tensor(src_offset, dtype=torch.int64) if not torch.is_tensor(src_offset) and not len(src_offset) \
        else torch.as_tensor(src_offset)
    if src_offset.dtype.is_floating_point or src_offset.dtype == torch.bool or tuple(src_offset.shape) != (n,):
        raise PleasHipError("image_resample_chain_plan: src_offset must hold %d integers, got %s %s"
                            % (n, src_offset.dtype, tuple(src_offset.shape)))
    src_offset = src_offset.to(torch.int64).contiguous()
    nbytes = image_resample_chain_plan_bytes(geom, size)
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8)
        if torch.cuda.is_available():
            out = out.pin_memory()
    elif (not torch.is_tensor(out) or out.dtype != torch.uint8 or out.is_cuda or not out.is_contiguous() or out.numel() < nbytes
          or out.data_ptr() % 4):
        raise PleasHipError("image_resample_chain_plan: out must be a contiguous uint8 host tensor of at least %d bytes on a 4-byte "
                            "boundary" % nbytes)
    plan = out.view(-1)[:nbytes]
    check(_lib.lib().pleas_resample_chain_plan(geom.data_ptr(), src_offset.data_ptr(), n, int(channels), int(size[0]), int(size[1]),
                                               int(src_bytes), plan.data_ptr(), nbytes), "pleas_resample_chain_plan")
    return plan


def image_resample_chain_plan_info(plan: torch.Tensor) -> dict:
    """What a HOST chain plan says of itself: ``n, channels, size, src_bytes, ws_bytes, mid_bytes, items`` (the item counts of the
    four launches; ``pleas_resample_chain_plan_info``)."""
    if not torch.is_tensor(plan) or plan.dtype != torch.uint8 or plan.is_cuda or not plan.is_contiguous():
        raise PleasHipError("image_resample_chain: the host plan must be a contiguous uint8 CPU tensor (image_resample_chain_plan's)")
    info = (ctypes.c_int64 * 11)()
    check(_lib.lib().pleas_resample_chain_plan_info(plan.data_ptr(), plan.numel(), info), "pleas_resample_chain_plan_info")
    return {"n": info[0], "channels": info[1], "size": (info[2], info[3]), "src_bytes": info[4], "ws_bytes": info[5],
            "mid_bytes": info[6], "items": tuple(info[7:11])}


def image_resample_chain_host(src_u8: torch.Tensor, plan: torch.Tensor, table: torch.Tensor, flip=None):
    """A chain plan executed on the CPU, launch by launch as the four kernels do (``pleas_image_resample_chain_host``): returns
    ``(fp32 [N, C, Ho, Wo], uint8 [N, Ho, Wo, C], uint8 [mid_bytes])`` -- the final bytes through ``table``, the final bytes
    (both after the flip), and the images between the two resizes, ``[h, w, C]`` per sample, end to end."""
    info = image_resample_chain_plan_info(plan)
    n, c, (ho, wo) = info["n"], info["channels"], info["size"]
    if not torch.is_tensor(src_u8) or src_u8.dtype != torch.uint8 or src_u8.is_cuda or not src_u8.is_contiguous():
        raise PleasHipError("image_resample_chain_host: src must be a contiguous uint8 CPU tensor")
    if src_u8.numel() < info["src_bytes"]:
        raise PleasHipError("image_resample_chain_host: src holds %d bytes, the plan was built for %d" % (src_u8.numel(), info["src_bytes"]))
    if table.is_cuda or table.dtype != torch.float32 or tuple(table.shape) != (c, 256) or not table.is_contiguous():
        raise PleasHipError("image_resample_chain_host: table must be a contiguous fp32 [%d, 256] CPU tensor" % c)
    flip = _resample_flip(flip, n)
    if flip is not None and flip.is_cuda:
        raise PleasHipError("image_resample_chain_host: flip flags must be host values")
    f32, u8 = torch.empty((n, c, ho, wo), dtype=torch.float32), torch.empty((n, ho, wo, c), dtype=torch.uint8)
    mid = torch.empty(info["mid_bytes"], dtype=torch.uint8)
    check(_lib.lib().pleas_image_resample_chain_host(src_u8.data_ptr(), plan.data_ptr(), plan.numel(), table.data_ptr(),
                                                     flip.data_ptr() if flip is not None else None, f32.data_ptr(), u8.data_ptr(),
                                                     mid.data_ptr()), "pleas_image_resample_chain_host")
    return f32, u8, mid


def image_resample_chain(src_u8: torch.Tensor, plan_dev: torch.Tensor, plan: torch.Tensor, table: torch.Tensor, flip=None,
                         out: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Packed uint8 images of mixed sizes on the GPU to normalised fp32 [N, C, Ho, Wo] through PIL's ``resize -> crop -> resize``
    chain, flip and table lookup in four launches (``pleas_image_resample_chain``).

    Arguments as ``image_resample``'s, with the plan of ``image_resample_chain_plan``.  The two scratches and the intermediate
    image come from the stream's ``Workspace``, or from ``scratch``: a contiguous uint8 tensor on src's device of at least the
    plan's ``ws_bytes`` (every byte read is written first, whatever it held)."""
    if not torch.is_tensor(src_u8) or src_u8.dtype != torch.uint8:
        raise PleasHipError("image_resample_chain: src must be a uint8 tensor (got %s)" % getattr(src_u8, "dtype", type(src_u8)))
    if not src_u8.is_contiguous():
        raise PleasHipError("image_resample_chain: src must be contiguous (one packed buffer)")
    info = image_resample_chain_plan_info(plan)
    n, c, (ho, wo) = info["n"], info["channels"], info["size"]
    if src_u8.numel() < info["src_bytes"]:
        raise PleasHipError("image_resample_chain: src holds %d bytes, the plan was built for %d" % (src_u8.numel(), info["src_bytes"]))
    flip = _resample_flip(flip, n)
    if out is not None and (not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != (n, c, ho, wo) or not out.is_contiguous()
                            or out.data_ptr() % 16):
        raise PleasHipError("image_resample_chain: out must be a contiguous, 16-byte aligned fp32 tensor of shape %s on the GPU"
                            % ((n, c, ho, wo),))
    if not src_u8.is_cuda:
        raise PleasHipError("HIP path needs tensors on the GPU (got device %s); no CPU fallback" % src_u8.device)
    dev = src_u8.device
    _need_gpu(table)
    if table.device != dev or tuple(table.shape) != (c, 256) or not table.is_contiguous():
        raise PleasHipError("image_resample_chain: table must be a contiguous fp32 [%d, 256] tensor on src's device" % c)
    if (not torch.is_tensor(plan_dev) or plan_dev.dtype != torch.uint8 or plan_dev.device != dev or not plan_dev.is_contiguous()
            or plan_dev.numel() < plan.numel() or plan_dev.data_ptr() % 4):
        raise PleasHipError("image_resample_chain: plan_dev must be the plan's %d bytes as a contiguous uint8 tensor on src's device, "
                            "4-byte aligned" % plan.numel())
    if scratch is not None and (not torch.is_tensor(scratch) or scratch.dtype != torch.uint8 or scratch.device != dev
                                or not scratch.is_contiguous() or scratch.numel() < info["ws_bytes"]):
        raise PleasHipError("image_resample_chain: scratch must be a contiguous uint8 tensor of at least %d bytes on src's device"
                            % info["ws_bytes"])
    if out is None:
        out = torch.empty((n, c, ho, wo), dtype=torch.float32, device=dev)
    elif out.device != dev:
        raise PleasHipError("image_resample_chain: out must be on src's device")
    if n == 0:
        return out
    if flip is not None and flip.device != dev:
        flip = flip.to(dev)
    ws = scratch if scratch is not None else Workspace.get(dev).reserve(info["ws_bytes"])
    check(_lib.lib().pleas_image_resample_chain(src_u8.data_ptr(), plan_dev.data_ptr(), plan.data_ptr(), plan.numel(), table.data_ptr(),
                                                flip.data_ptr() if flip is not None else None, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                _stream()), "pleas_image_resample_chain")
    return out


def conv2d_bn_act(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], stride: int, pad: int, kpos_major: bool,
                  scale: torch.Tensor, shift: torch.Tensor, res: Optional[torch.Tensor], relu: bool):
    """``y = conv2d(x, w, bias)`` and ``z = bn_act(y, scale, shift, res, relu)`` from ONE launch (``pleas_conv2d_bn_act_fwd``):
    the activated image is written from the registers that hold y, bit for bit what ``bn_act`` makes of y.  Returns ``(y, z)``.
    ``relu``: a bool or an ``ACT_*`` code."""
    relu = _act_code("conv2d_bn_act", relu)
    operands, geometry, out_shape = _conv_call("conv2d_bn_act", x, w, bias, stride, pad, kpos_major, scale, shift)
    image = _image_operands("conv2d_bn_act", x, scale, shift, res, out_shape)
    y = torch.empty(out_shape, dtype=torch.float32, device=x.device)
    z = torch.empty_like(y)
    check(_lib.lib().pleas_conv2d_bn_act_fwd(*operands, y.data_ptr(), *image, z.data_ptr(), relu, *geometry, _stream()),
          "pleas_conv2d_bn_act_fwd")
    return y, z


# per-call limits of the convolution kernels (fwd_describe, csrc/conv_fwd.hip): fewer than 2^30 output elements and fewer than
# 2^31 output pixels over the batch
CONV_MAX_OUTPUT, CONV_MAX_PIXELS = 1 << 30, 1 << 31


def conv2d_sample_split(N: int, per_sample_out: int, pixels: int, limit: int = CONV_MAX_OUTPUT, align: int = 1) -> List[Tuple[int, int]]:
    """``[(first sample, samples)]`` of the FEWEST calls that each stay under the per-call limits (``samples * per_sample_out
    < limit``, ``samples * pixels < 2^31``), sizes as equal as possible (they differ by at most ``align``, larger ones first).
    ``align``: every call but the last starts and ends on a multiple of it (the sample count that keeps slices 16-byte
    aligned).  Host arithmetic only.  One sample that does not fit is refused."""
    if N <= 0:
        return []
    most = min((limit - 1) // per_sample_out, (CONV_MAX_PIXELS - 1) // pixels) // align * align
    if most <= 0:
        raise PleasHipError("conv2d_act: one sample (%d output elements, %d pixels) exceeds the per-call limit" % (per_sample_out, pixels))
    groups = -(-N // align)
    calls = -(-groups // (most // align))
    base, extra = divmod(groups, calls)
    parts, at = [], 0
    for i in range(calls):
        n = min((base + (1 if i < extra else 0)) * align, N - at)
        parts.append((at, n))
        at += n
    return parts


def conv2d_act(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], stride: int, pad: int, kpos_major: bool,
               scale: torch.Tensor, shift: torch.Tensor, res: Optional[torch.Tensor], relu: bool,
               _limit: int = CONV_MAX_OUTPUT) -> torch.Tensor:
    """``z = bn_act(conv2d(x, w, bias), scale, shift, res, relu)`` with z as the ONLY output (``pleas_conv2d_act_fwd``): bit for
    bit the ``z`` of ``conv2d_bn_act``, the convolution's own output is never written.  For forwards nobody hooks (evaluation).
    A batch whose output crosses the per-call limit of the kernels is split along the sample axis (``conv2d_sample_split``)
    into calls that write one ``z``.  ``_limit``: the output-element limit, for tests.  ``relu``: a bool or an ``ACT_*`` code."""
    relu = _act_code("conv2d_act", relu)
    (_, wp, bp), geometry, out_shape = _conv_call("conv2d_act", x, w, bias, stride, pad, kpos_major, scale, shift)
    sp, tp, _ = _image_operands("conv2d_act", x, scale, shift, res, out_shape)
    (N, Cin, H, W), (_, Cout, Ho, Wo) = geometry[:4], out_shape
    z = torch.empty(out_shape, dtype=torch.float32, device=x.device)
    if N == 0 or Ho <= 0 or Wo <= 0:
        return z
    per_out, per_in = Cout * Ho * Wo, Cin * H * W
    if N * per_out < _limit and N * Ho * Wo < CONV_MAX_PIXELS:
        parts = [(0, N)]
    else:
        # slices of x, z and the identity must start 16-byte aligned: whole groups of `align` samples
        align = max(4 // math.gcd(4, per_out), 4 // math.gcd(4, per_in))
        parts = conv2d_sample_split(N, per_out, Ho * Wo, _limit, align)
    fn, st = _lib.lib().pleas_conv2d_act_fwd, _stream()
    for at, n in parts:
        check(fn(x[at:at + n].data_ptr(), wp, bp, sp, tp, res[at:at + n].data_ptr() if res is not None else None,
                 z[at:at + n].data_ptr(), relu, n, *geometry[1:], st), "pleas_conv2d_act_fwd")
    return z


CONV_BN_STATS_TILE = 128      # output pixels of a work item of the convolution kernels (fTN, csrc/conv_fwd.hip)


def conv2d_bn_stats_takes(N: int, Cout: int, Ho: int, Wo: int, batches: int) -> str:
    """What ``pleas_conv2d_bn_stats_fwd`` makes of an ``[N, Cout, Ho, Wo]`` output in ``batches`` batches, from host arithmetic:
    ``"fused"``; ``"straddle"`` -- batches of fewer than 128 pixels share the forward, a tile would touch more than two of them:
    fold after ``conv2d``; ``"limits"`` -- over the per-call limits of the convolution kernels, or nothing to normalise."""
    if N <= 0 or Ho <= 0 or Wo <= 0 or batches < 1 or N % batches or N * Ho * Wo >= CONV_MAX_PIXELS or N * Ho * Wo * Cout >= CONV_MAX_OUTPUT:
        return "limits"
    per_batch = N // batches * Ho * Wo
    if per_batch <= 1:
        return "limits"
    return "straddle" if batches > 1 and per_batch < CONV_BN_STATS_TILE else "fused"


class ConvBnStats(_PerModuleFold):
    """``conv2d`` + ``BnTrainFold`` as ONE call of ``pleas_conv2d_bn_stats_fwd`` for one train-mode BatchNorm2d called forward after
    forward (graph callable of the BN-reset pass): the convolution's work items leave the sums of their tile's outputs, so ``y`` is
    not read back for its statistics.  Workspace, the ``[2][batches][C]`` outputs and the module's addresses are looked up once per
    input shape; ``bn.momentum`` is read per call.  The returned ``(scale, shift)`` are views of a buffer that the NEXT call
    overwrites (as ``BnTrainFold``'s); ``y`` is a fresh tensor."""

    def _prepare(self, x: torch.Tensor, w: torch.Tensor, stride: int, pad: int, kpos_major: bool, batches: int) -> None:
        bn = self.bn
        _, geometry, (N, Cout, Ho, Wo) = _conv_call("conv2d_bn_stats", x, w, None, stride, pad, kpos_major)
        if N % batches:
            raise PleasHipError("conv2d_bn_stats: %d samples do not split into %d batches" % (N, batches))
        if N // batches * max(Ho, 0) * max(Wo, 0) <= 1:
            raise ValueError("Expected more than 1 value per channel when training, got input size %s" % ((N // batches, Cout, Ho, Wo),))
        g, b, rm, rv, nbt = _bn_pointers("conv2d_bn_stats", bn, x.device, Cout)
        need = int(_lib.lib().pleas_conv2d_bn_stats_ws_bytes(N, Cout, Ho, Wo, batches))
        self._ws = torch.empty(need // 8, dtype=torch.float64, device=x.device)
        self._out = torch.empty(2, batches, Cout, dtype=torch.float32, device=x.device)
        self._tensors = self._addresses()
        self._geo = geometry + (batches,)
        self._tail = (g, b) + self._tensors[-2:] + (rm, rv, nbt, self._out[0].data_ptr(), self._out[1].data_ptr(), self._ws.data_ptr(), need)
        self._y_shape = (N, Cout, Ho, Wo)
        self._shape = (tuple(x.shape), tuple(w.shape), x.device, stride, pad, kpos_major, batches)

    def __call__(self, x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], stride: int, pad: int,
                 kpos_major: bool = False, batches: int = 1) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``(y, scale, shift)``: ``y = conv2d(x, w, bias)``; ``x`` holds ``batches`` batches back to back along dim 0, each folded
        on its own samples, in order -- ``scale`` / ``shift`` are ``[C]`` for one batch, ``[batches, C]`` for several."""
        _need_gpu(x, w)
        if self._shape != (tuple(x.shape), tuple(w.shape), x.device, stride, pad, kpos_major, batches) or self._tensors != self._addresses():
            self._prepare(x, w, stride, pad, kpos_major, batches)
        y = torch.empty(self._y_shape, dtype=torch.float32, device=x.device)
        rc = _lib.lib().pleas_conv2d_bn_stats_fwd(x.data_ptr(), w.data_ptr(), bias.data_ptr() if bias is not None else None,
                                                  y.data_ptr(), *self._geo, *self._tail, _stream())
        check(rc, "pleas_conv2d_bn_stats_fwd")
        return (y, self._out[0, 0], self._out[1, 0]) if batches == 1 else (y, self._out[0], self._out[1])


def conv2d_bn_stats(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], stride: int, pad: int, kpos_major: bool,
                    bn: "torch.nn.BatchNorm2d", batches: int = 1) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``y = conv2d(x, w, bias)`` and train-mode ``bn`` on ``y`` as ``bn_train_fold`` returns it -- ``(y, scale, shift)``, ``bn``'s
    running statistics and counter moved on -- from ONE call (``pleas_conv2d_bn_stats_fwd``): ``y`` bit for bit ``conv2d``'s, its
    statistics taken in the convolution's epilogue.  One-off form of ``ConvBnStats``."""
    y, scale, shift = ConvBnStats(bn)(x, w, bias, stride, pad, kpos_major, batches)
    return y, scale.clone(), shift.clone()


def channel_map(index, channels: int, device) -> torch.Tensor:
    """A channel map for ``pool_gather``: ``index`` (any integer sequence / tensor) as a contiguous int32 tensor on ``device``,
    its entries checked against ``[0, channels)`` on the HOST, once -- ``pool_gather`` takes it without looking again."""
    idx = torch.as_tensor(index).detach().to("cpu", torch.int64).reshape(-1)
    if idx.numel() == 0 or int(idx.min()) < 0 or int(idx.max()) >= channels:
        raise PleasHipError("channel_map: entries must lie in [0, %d) and the map must not be empty" % channels)
    src = idx.to(torch.int32).to(device).contiguous()
    src._pleas_channels = channels
    return src


def pool_gather(x: torch.Tensor, src: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``y[n, k] = mean over the pixels of x[n, src[k]]`` for ``x`` [N, C, ...] (``pleas_pool_gather``): ``AdaptiveAvgPool2d((1, 1))``
    + ``flatten(1)`` and, with ``src`` (int32 device vector; entries may repeat or reorder), the gather of
    ``permute_final_features`` in the same pass.  Fixed summation order: the same bits run after run.  A map not made by
    ``channel_map`` is range-checked here (one read-back); an entry outside ``[0, C)`` is refused."""
    _need_gpu(x)
    if x.dim() < 2:
        raise PleasHipError("pool_gather needs an fp32 [N, C, ...] tensor")
    x = x.contiguous()
    N, C = x.shape[0], x.shape[1]
    HW = math.prod(x.shape[2:])
    K = C
    if src is not None:
        if not src.is_cuda or src.device != x.device or src.dtype != torch.int32 or src.dim() != 1 or not src.is_contiguous() or src.numel() == 0:
            raise PleasHipError("pool_gather: the channel map must be a non-empty contiguous int32 vector on x's device")
        if getattr(src, "_pleas_channels", None) != C:
            lo, hi = (int(v) for v in torch.aminmax(src))
            if lo < 0 or hi >= C:
                raise PleasHipError("pool_gather: channel map entries must lie in [0, %d), got [%d, %d]" % (C, lo, hi))
        K = src.numel()
    y = torch.empty((N, K), dtype=torch.float32, device=x.device)
    if N == 0:
        return y
    if HW == 0:
        raise PleasHipError("pool_gather: empty images")
    check(_lib.lib().pleas_pool_gather(x.data_ptr(), src.data_ptr() if src is not None else None, y.data_ptr(), N, C, HW, K,
                                       _stream()), "pleas_pool_gather")
    return y


def top1_count(logits: torch.Tensor, labels: torch.Tensor, hits: torch.Tensor, pred: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``hits += number of rows n with argmax(logits[n]) == labels[n]`` on the device, no synchronisation
    (``pleas_top1_count``): the first maximal index wins, a NaN counts as maximal (``torch.argmax``).  ``logits`` [N, C] fp32,
    ``labels`` / ``pred`` int64 [N], ``hits`` a one-element int64 device tensor the caller zeroes once and reads once;
    ``pred`` (optional) receives the predictions.  Returns ``hits``."""
    _need_gpu(logits)
    if logits.dim() != 2 or not logits.is_contiguous() or logits.shape[1] < 1:
        raise PleasHipError("top1_count: logits must be a contiguous [N, C] tensor with C >= 1")
    N, C = logits.shape
    for name, t, n in (("labels", labels, N), ("hits", hits, 1)) + ((("pred", pred, N),) if pred is not None else ()):
        if t.device != logits.device or t.dtype != torch.int64 or t.numel() != n or not t.is_contiguous():
            raise PleasHipError("top1_count: %s must be a contiguous int64 tensor of %d element(s) on the logits' device" % (name, n))
    if N:
        check(_lib.lib().pleas_top1_count(logits.data_ptr(), labels.data_ptr(), N, C, hits.data_ptr(),
                                          pred.data_ptr() if pred is not None else None, _stream()), "pleas_top1_count")
    return hits


def softmax_xent(logits: torch.Tensor, labels: torch.Tensor, scale: Optional[float] = None, dlogits: Optional[torch.Tensor] = None,
                 row_loss: Optional[torch.Tensor] = None, loss: Optional[torch.Tensor] = None,
                 counts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Softmax cross-entropy of ``logits`` [N, C] fp32 against ``labels`` int64 [N] from one pass, no synchronisation
    (``pleas_softmax_xent``): ``row_loss[n] = logsumexp(logits[n]) - logits[n, labels[n]]`` (allocated when not given, returned);
    ``dlogits`` (optional, [N, C]) ``= scale * (softmax(logits) - onehot(labels))``; ``loss`` (optional, fp32 [2]):
    ``loss[0] = scale * row_loss.sum()`` in a fixed order and ``loss[1] += loss[0]``; ``counts`` (optional, int64 [2]):
    ``counts[0] +=`` rows whose top-1 (``top1_count``'s rule) is their label, ``counts[1] +=`` rows whose label lies outside
    ``[0, C)`` -- such a row has loss 0, a zero ``dlogits`` row and no hit, and the caller raises when it reads ``counts`` back.
    ``scale`` defaults to ``1 / N`` (``F.cross_entropy``'s ``reduction="mean"``)."""
    _need_gpu(logits)
    if logits.dim() != 2 or not logits.is_contiguous() or logits.shape[1] < 1:
        raise PleasHipError("softmax_xent: logits must be a contiguous [N, C] tensor with C >= 1")
    N, C = logits.shape
    if N * C >= 1 << 30:
        raise PleasHipError("softmax_xent: N * C = %d is not below 2^30" % (N * C))
    if row_loss is None:
        row_loss = torch.empty(N, dtype=torch.float32, device=logits.device)
    for name, t, dtype, shape in (("labels", labels, torch.int64, (N,)), ("dlogits", dlogits, torch.float32, (N, C)),
                                  ("row_loss", row_loss, torch.float32, (N,)), ("loss", loss, torch.float32, (2,)),
                                  ("counts", counts, torch.int64, (2,))):
        if t is not None and (t.device != logits.device or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous()):
            raise PleasHipError("softmax_xent: %s must be a contiguous %s tensor of shape %s on the logits' device" % (name, dtype, shape))
    outs = [t for t in (dlogits, row_loss, loss) if t is not None]
    for i, t in enumerate(outs):            # outputs overlap neither the logits nor each other
        for o in [logits] + outs[:i]:
            if t.numel() and o.numel() and t.data_ptr() < o.data_ptr() + o.numel() * 4 and o.data_ptr() < t.data_ptr() + t.numel() * 4:
                raise PleasHipError("softmax_xent: dlogits / row_loss / loss must not overlap the logits or each other")
    if N:
        check(_lib.lib().pleas_softmax_xent(logits.data_ptr(), labels.data_ptr(), N, C, 1.0 / N if scale is None else float(scale),
                                            dlogits.data_ptr() if dlogits is not None else None, row_loss.data_ptr(),
                                            loss.data_ptr() if loss is not None else None,
                                            counts.data_ptr() if counts is not None else None, _stream()), "pleas_softmax_xent")
    return row_loss


class WgradBatch(_GroupedLaunch):
    """Weight gradients of all merged layers of one update in ONE grouped launch (``pleas_wgrad_batch``).
    ``add`` per layer (operands must stay unmodified until ``flush``), ``flush`` once per update."""

    STRUCT, WS_BYTES, LAUNCH = _lib.WgradLayer, "pleas_wgrad_batch_ws_bytes", "pleas_wgrad_batch"
    ACCUMULATE, KPOS_MAJOR = 1, 2

    def add(self, resid: torch.Tensor, ip: torch.Tensor, grad: torch.Tensor, kernel=(1, 1), stride: int = 1,
            pad: int = 0, flags: int = 0) -> None:
        if not (resid.is_contiguous() and ip.is_contiguous() and grad.is_contiguous()):
            raise PleasHipError("WgradBatch.add: contiguous tensors expected")
        N, Cout, Cin = resid.shape[0], resid.shape[1], ip.shape[1]
        Hin, Win = (ip.shape[2], ip.shape[3]) if ip.dim() == 4 else (1, 1)
        self._queue((resid, ip, grad), (N, Cout, Cin, Hin, Win, kernel[0], kernel[1], stride, pad, flags))

    def _fill(self, a, tensors, geo) -> None:
        a.resid, a.ip, a.grad = (t.data_ptr() for t in tensors)
        a.N, a.Cout, a.Cin, a.Hin, a.Win, a.KH, a.KW, a.stride, a.pad, a.flags = geo

    @staticmethod
    def plan_info(geometries) -> List[dict]:
        """Host-side facts about the grouped launch of a layer list (``pleas_wgrad_plan_info``; no GPU work, no tensors):
        per ``(N, Cout, Cin, Hin, Win, KH, KW, stride, pad, flags)`` the tile form ``variant`` the plan builder picks under the
        current ``pleas_arith``, the slabs ``S`` of the pixel axis, the tile counts, the work items, and whether the epilogue
        takes the staged 16-byte row path (for 16-byte aligned destinations)."""
        geometries = list(geometries)
        n = len(geometries)
        if n == 0:
            return []
        arr = (_lib.WgradLayer * n)()
        for a, geo in zip(arr, geometries):
            a.N, a.Cout, a.Cin, a.Hin, a.Win, a.KH, a.KW, a.stride, a.pad, a.flags = (int(v) for v in geo)
        info = (ctypes.c_int * (6 * n))()
        check(_lib.lib().pleas_wgrad_plan_info(arr, n, info), "pleas_wgrad_plan_info")
        return [{"variant": info[6 * i], "S": info[6 * i + 1], "tiles_cout": info[6 * i + 2], "tiles_cin": info[6 * i + 3],
                 "items": info[6 * i + 4], "rows": bool(info[6 * i + 5])} for i in range(n)]

class NormalEqBatch(_GroupedLaunch):
    """A_l += U_l^T U_l for all layers of one batch in ONE grouped launch (``pleas_normal_eq_accum``)."""

    STRUCT, WS_BYTES, LAUNCH = _lib.NeqLayer, "pleas_normal_eq_ws_bytes", "pleas_normal_eq_accum"

    def __init__(self, device: torch.device):
        super().__init__(device)
        self._seen: dict = {}      # A's address -> (A, geometry): every matrix this object has accumulated into

    def add(self, ip: torch.Tensor, A: torch.Tensor, kernel=(1, 1), stride: int = 1, pad: int = 0) -> None:
        if not (ip.is_contiguous() and A.is_contiguous()):
            raise PleasHipError("NormalEqBatch.add: contiguous tensors expected")
        N, Cin = ip.shape[0], ip.shape[1]
        Hin, Win = (ip.shape[2], ip.shape[3]) if ip.dim() == 4 else (1, 1)
        K = kernel[0] * kernel[1] * Cin
        if tuple(A.shape) != (K, K):
            raise PleasHipError("NormalEqBatch.add: A must be (%d, %d)" % (K, K))
        geo = (N, Cin, Hin, Win, kernel[0], kernel[1], stride, pad)
        self._queue((ip, A), geo)
        self._seen[A.data_ptr()] = (A, geo)

    def _fill(self, a, tensors, geo) -> None:
        ip, A = tensors
        a.ip, a.A = (ip.data_ptr() if ip is not None else 0), A.data_ptr()
        a.N, a.Cin, a.Hin, a.Win, a.KH, a.KW, a.stride, a.pad = geo

    def _layer_array(self, pairs):
        arr = (_lib.NeqLayer * len(pairs))()
        for a, (A, geo) in zip(arr, pairs):
            self._fill(a, (None, A), geo)
        return arr

    def seen(self) -> dict:
        """``{address of A: (A, geometry)}`` of every matrix this object has accumulated into."""
        return dict(self._seen)

    def finalize(self, pairs=None) -> None:
        """Fill the blocks ``flush`` leaves to the end (``pleas_normal_eq_finalize``: stride-1 k x k layers contract one
        block per lag class only).  Once, after the last batch -- and after the all-reduce of a multi-GPU run.
        ``pairs``: the ``(A, geometry)`` list to finalize when it is not this object's own -- a data-parallel rank that
        accumulated no batch still receives the all-reduced matrices and must complete ALL of them."""
        pairs = list(self._seen.values()) if pairs is None else list(pairs)
        if pairs:
            check(_lib.lib().pleas_normal_eq_finalize(self._layer_array(pairs), len(pairs), _stream()),
                  "pleas_normal_eq_finalize")

    def plan_info(self) -> dict:
        """Host-side facts about the grouped launch of the matrices seen so far (no GPU work)."""
        pairs = list(self._seen.values())
        info = (ctypes.c_double * 4)()
        if pairs:
            check(_lib.lib().pleas_normal_eq_plan_info(self._layer_array(pairs), len(pairs), info), "pleas_normal_eq_plan_info")
        return {"flops": info[0], "flops_executed": info[1], "items": int(info[2]), "blocks_to_finalize": int(info[3])}

    @staticmethod
    def layer_info(geometries) -> List[dict]:
        """Host-side facts per layer of a list (``pleas_normal_eq_layer_info``; no GPU work, no tensors): per
        ``(N, Cin, Hin, Win, KH, KW, stride, pad)`` the tile form ``variant`` (0-3 direct, 6-7 shifted loader, 8-11 lag classes),
        the slabs ``S`` of the pixel axis, the tiles per side of a block, the block tiles contracted and the blocks left to
        ``finalize``."""
        geometries = list(geometries)
        n = len(geometries)
        arr = (_lib.NeqLayer * max(n, 1))()
        for a, geo in zip(arr, geometries):
            a.N, a.Cin, a.Hin, a.Win, a.KH, a.KW, a.stride, a.pad = (int(v) for v in geo)
        info = (ctypes.c_int * (5 * max(n, 1)))()
        check(_lib.lib().pleas_normal_eq_layer_info(arr if n else None, n, info), "pleas_normal_eq_layer_info")
        return [{"variant": info[5 * i], "S": info[5 * i + 1], "tiles": info[5 * i + 2], "block_tiles": info[5 * i + 3],
                 "blocks_to_finalize": info[5 * i + 4]} for i in range(n)]


def cholesky_solve_batched(As: Sequence[torch.Tensor], Bts: Sequence[torch.Tensor], ridge: float = 0.0) -> torch.Tensor:
    """In place: every row of ``Bts[p]`` (N_p x K_p) becomes the solution of ``x (A_p + ridge*mean(diag) I) = row``.
    ``As[p]`` (K_p x K_p, lower triangle read) is overwritten by its Cholesky factor.  Returns the device info vector."""
    k = len(As)
    if k == 0:
        return torch.zeros(0, dtype=torch.int32)
    _need_gpu(*As, *Bts)
    for a, b in zip(As, Bts):
        if a.dim() != 2 or a.shape[0] != a.shape[1] or b.dim() != 2 or b.shape[1] != a.shape[0] or not a.is_contiguous() \
                or not b.is_contiguous():
            raise PleasHipError("cholesky_solve_batched: A must be (K, K), Bt (N, K), both contiguous")
    info = torch.zeros(k, dtype=torch.int32, device=As[0].device)
    rc = _lib.lib().pleas_cholesky_solve_batched(
        (ctypes.c_void_p * k)(*[a.data_ptr() for a in As]), (ctypes.c_void_p * k)(*[b.data_ptr() for b in Bts]),
        (ctypes.c_int * k)(*[a.shape[0] for a in As]), (ctypes.c_int * k)(*[b.shape[0] for b in Bts]), k, float(ridge),
        info.data_ptr(), _stream())
    check(rc, "pleas_cholesky_solve_batched")
    return info


# ---------------------------------------------------------------------------------------- arithmetic of the contractions
@contextlib.contextmanager
def arith(mode: int):
    """``pleas_arith(mode)`` for the block (``ARITH_FP32``, ``ARITH_SPLIT_BF16``: six of the nine bf16 products of every fp32
    product, ``ARITH_SPLIT_BF16_EXACT``: all nine), the previous arithmetic again afterwards.  Process-wide, as the switch
    itself: not for blocks that run beside other threads' launches.  Nothing in the package turns a split mode on."""
    if mode not in (ARITH_FP32, ARITH_SPLIT_BF16, ARITH_SPLIT_BF16_EXACT):
        raise PleasHipError("arith: unknown mode %r" % (mode,))
    lib = _lib.lib()
    before = lib.pleas_arith_get()
    lib.pleas_arith(mode)
    try:
        yield
    finally:
        lib.pleas_arith(before)


# ---------------------------------------------------------------------------------------- live kernel timing
def profile_enable(on: bool, skip: Sequence[str] = ()) -> None:
    """``skip``: kernel names left unrecorded (the two events per launch are not free for kernels that run
    hundreds of times per step, e.g. ``bn_act`` / ``merge_blocks``)."""
    mask = 0xFFFFFFFF
    for name in skip:
        mask &= ~(1 << _lib.PROF_KERNELS.index(name))
    _lib.lib().pleas_prof_select(mask)
    _lib.lib().pleas_prof_enable(int(bool(on)))


def profile_reset() -> None:
    _lib.lib().pleas_prof_reset()


def profile_collect() -> dict:
    """{kernel name: (launches, total_ms, algorithmic flops, algorithmic bytes)} since the last reset."""
    out = {}
    for kid, name in enumerate(_lib.PROF_KERNELS):
        n, ms, fl, by = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        check(_lib.lib().pleas_prof_collect(kid, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)),
              "pleas_prof_collect")
        if n.value:
            out[name] = (int(n.value), float(ms.value), float(fl.value), float(by.value))
    return out
