#!/usr/bin/env python3
"""Times the depthwise closed form (csrc/dw_normal_eq.hip) against the stock-operator formulation of the same commit, in one process.
A GPU is required.

1. Accumulate, per MobileNet-family shape (k = 3, pad 1) at N = 16 and N = 128: ``DwNormalEqBatch`` on the layer alone against
   ``F.unfold`` on ``[N*C, 1, H, W]`` + ``bmm`` in fp32 and in fp64 (the target handed to the stock legs ready-made).  All warmed,
   device events, 5 windows per leg ALTERNATING, the median over the windows of a window's time per call.  Algorithmic bytes
   ``4 N C (Hin Win + 2 Ho Wo)`` over that time and its share of the 8 TB/s peak; MACs ``N C Ho Wo D (D + 1) / 2`` over that time.
   Then the nine shapes of a batch size in ONE grouped launch against the sum of the nine alone.
2. K = 5 and K = 7 on one shape each (not optimised: one matrix instruction per 16 x 16 tile of the padded system).
3. A closed-form job of the MobileNet-shaped stack of tools/dwconv_bench.py (batch 16, 224 x 224, ratio 0): ``NormalEqFitter.step`` per
   batch under ``depthwise_closed_form("hip")`` against one Adam update of ``PleasFitter`` under ``depthwise_form("hip")``, windows
   alternating, and the solve on its own.

Prints one JSON line and writes it to ``--out`` (default profiles/dw_normal_eq_bench.json).
Run under a time limit:  timeout -k 10 900 python tools/dw_normal_eq_bench.py
"""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from dwconv_bench import PEAK_BYTES_PER_S, SHAPES, WINDOWS, Stack, alternate  # noqa: E402


def _layer(N, C, H, stride, K=3):
    from pleas_merging_amd import hip_ops

    g = torch.Generator().manual_seed(C + H + K)
    pad = K // 2
    Ho = (H + 2 * pad - K) // stride + 1
    x = torch.randn(N, C, H, H, generator=g).cuda()
    o1, o2 = torch.randn(N, C, Ho, Ho, generator=g).cuda(), torch.randn(N, C, Ho, Ho, generator=g).cuda()
    rows = torch.arange(C, dtype=torch.int32, device="cuda")
    S = torch.zeros(C, K * K + 2, K * K + 2, dtype=torch.float64, device="cuda")
    tgt = hip_ops.merge_blocks(o1, o2, 1, rows, rows, C)
    return dict(x=x, o1=o1, o2=o2, rows=rows, S=S, tgt=tgt, geo=(N, C, H, stride, K, pad, Ho))


def _own(batch, layers):
    def run():
        for d in layers:
            N, C, H, stride, K, pad, Ho = d["geo"]
            batch.add(d["x"], d["o1"], d["o2"], d["rows"], d["rows"], C, d["S"], stride, pad)
        batch.flush()
    return run


def _stock(d, dtype):
    N, C, H, stride, K, pad, Ho = d["geo"]

    def run():
        x, t = d["x"].to(dtype), d["tgt"].to(dtype)
        U = F.unfold(x.view(N * C, 1, H, H), K, padding=pad, stride=stride)                   # N*C, K*K, L
        V = torch.cat([U, torch.ones(N * C, 1, U.shape[-1], dtype=dtype, device="cuda"), t.view(N * C, 1, -1)], 1)
        return torch.bmm(V, V.transpose(1, 2)).view(N, C, K * K + 2, K * K + 2).sum(0)
    return run


def _row(d, t):
    N, C, H, stride, K, pad, Ho = d["geo"]
    D = K * K + 2
    nbytes, macs = 4.0 * N * C * (H * H + 2 * Ho * Ho), N * C * Ho * Ho * D * (D + 1) / 2.0
    return {"N": N, "C": C, "H": H, "stride": stride, "K": K, "own_us": round(t["own"] * 1e6, 2),
            "stock_fp32_us": round(t["stock_fp32"] * 1e6, 2), "stock_fp64_us": round(t["stock_fp64"] * 1e6, 2),
            "own_TBps": round(nbytes / t["own"] / 1e12, 3), "own_share_of_peak": round(nbytes / t["own"] / PEAK_BYTES_PER_S, 3),
            "own_TMACps": round(macs / t["own"] / 1e12, 3), "own_wins_fp32": bool(t["own"] <= t["stock_fp32"]),
            "own_wins_fp64": bool(t["own"] <= t["stock_fp64"])}


def accumulate_table(batches, calls):
    from pleas_merging_amd import hip_ops

    rows, grouped = [], []
    for N in batches:
        layers = [_layer(N, C, H, stride) for C, H, stride in SHAPES]
        alone = 0.0
        for d in layers:
            legs = {"own": _own(hip_ops.DwNormalEqBatch(torch.device("cuda")), [d]), "stock_fp32": _stock(d, torch.float32),
                    "stock_fp64": _stock(d, torch.float64)}
            t = {k: statistics.median(v) for k, v in alternate(legs, calls).items()}
            rows.append(_row(d, t))
            alone += t["own"]
        t = statistics.median(alternate({"own": _own(hip_ops.DwNormalEqBatch(torch.device("cuda")), layers)}, calls)["own"])
        grouped.append({"N": N, "layers": len(layers), "grouped_us": round(t * 1e6, 2), "sum_of_alone_us": round(alone * 1e6, 2)})
        del layers
        torch.cuda.empty_cache()
    return rows, grouped


def large_kernels(calls):
    from pleas_merging_amd import hip_ops

    rows = []
    for K in (5, 7):
        d = _layer(16, 192, 28, 1, K)
        legs = {"own": _own(hip_ops.DwNormalEqBatch(torch.device("cuda")), [d]), "stock_fp32": _stock(d, torch.float32),
                "stock_fp64": _stock(d, torch.float64)}
        rows.append(dict(_row(d, {k: statistics.median(v) for k, v in alternate(legs, calls).items()}), optimised=False))
    return rows


def stack_job(batch, updates):
    from pleas_merging_amd import hip_ops
    from pleas_merging_amd.core.compiler import get_permutation_spec
    from pleas_merging_amd.core.utils import make_identity_perm
    from pleas_merging_amd.methods import partial_merge
    from pleas_merging_amd.methods.normal_eq import NormalEqFitter
    from pleas_merging_amd.methods.pleas_merging import PleasFitter

    g = torch.Generator().manual_seed(0)
    models = []
    for seed in (0, 1):
        torch.manual_seed(seed)
        m = Stack().train()
        with torch.no_grad():
            m(torch.randn(4, 3, 224, 224, generator=g))
        models.append(m.eval().cuda())
    spec = get_permutation_spec(models[0], ((1, 3, 224, 224),))
    perm = make_identity_perm(spec)
    costs = {k: (torch.eye(grp.size) + 0.01 * torch.rand(grp.size, grp.size, generator=g)).cuda() for k, grp in spec.items()}
    merged = partial_merge(spec, models[0], models[1], perm, costs, 0.0).cuda()
    xs = [torch.randn(batch, 3, 224, 224, generator=g).cuda() for _ in range(4)]
    with hip_ops.depthwise_form("hip"), hip_ops.depthwise_closed_form("hip"):
        fits = {"adam": PleasFitter(models[0], models[1], copy.deepcopy(merged), spec, perm, costs, 0.0, 10 ** 6, num_classes=1000),
                "normal_eq": NormalEqFitter(models[0], models[1], copy.deepcopy(merged), spec, perm, costs, 0.0, 10 ** 6, num_classes=1000)}
    turn = {k: 0 for k in fits}

    def step(name):
        def run():
            fits[name].step(xs[turn[name] % len(xs)])
            turn[name] += 1
        return run

    per_window = alternate({name: step(name) for name in fits}, updates)
    med = {k: statistics.median(v) for k, v in per_window.items()}
    neq = fits["normal_eq"]
    info = neq.solve()                      # warm
    torch.cuda.synchronize()
    solves = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        neq.solve()
        b.record()
        torch.cuda.synchronize()
        solves.append(a.elapsed_time(b))
    dw = [i for i, p in enumerate(neq.plans) if p.dw]
    # channels whose taps never saw a non-zero input (dead units of the randomly initialised stack): what a layer without bias flags
    all_zero = sum(int((neq.S[i][:, :9, :9].diagonal(dim1=1, dim2=2).sum(1) == 0).sum()) for i in dw)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in dw:
        hip_ops.dw_normal_eq_solve(neq.S[i], 3, neq.plans[i].b is not None, neq.ridge, neq.plans[i].w, neq.plans[i].b)
    b.record()
    torch.cuda.synchronize()
    per_batch, solve = med["normal_eq"] * 1e3, statistics.median(solves)
    return {"batch": batch, "steps_per_window": updates, "windows": WINDOWS, "depthwise_layers": len(dw),
            "step_ms_windows": {k: [round(s * 1e3, 3) for s in v] for k, v in per_window.items()},
            "adam_update_ms_median": round(med["adam"] * 1e3, 3), "normal_eq_batch_ms_median": round(per_batch, 3),
            "solve_ms_median_of_3": round(solve, 3), "depthwise_solves_ms": round(a.elapsed_time(b), 3),
            "dw_singular_channels": info.get("dw_singular_channels"), "dw_all_zero_channels": all_zero,
            "job_of_401_batches_ms": {"adam": round(401 * med["adam"] * 1e3, 1), "normal_eq": round(401 * per_batch + solve, 1)},
            "fast_updates_adam": fits["adam"].fast_updates}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10, help="launches per window")
    ap.add_argument("--updates", type=int, default=20, help="fitter steps per window")
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dw_normal_eq_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dw_normal_eq_bench: a GPU is required")
    rows, grouped = accumulate_table(args.batches, args.calls)
    result = {"tool": "dw_normal_eq_bench", "device": torch.cuda.get_device_name(0), "kernel": 3, "pad": 1,
              "peak_TBps": PEAK_BYTES_PER_S / 1e12, "calls_per_window": args.calls, "windows": WINDOWS, "accumulate": rows,
              "grouped": grouped, "large_kernels": large_kernels(args.calls), "stack_job": stack_job(16, args.updates)}
    result["shapes_lost_to_stock_fp32"] = ["N%d C%d H%d s%d" % (r["N"], r["C"], r["H"], r["stride"]) for r in rows if not r["own_wins_fp32"]]
    result["shapes_lost_to_stock_fp64"] = ["N%d C%d H%d s%d" % (r["N"], r["C"], r["H"], r["stride"]) for r in rows if not r["own_wins_fp64"]]
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
