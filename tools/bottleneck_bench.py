#!/usr/bin/env python3
"""Times the batched bottleneck assignment on 71 cdist-structured matrices with ResNet-101's group sizes
(tests/golden/spec_resnet101.json) and prints one JSON line:

  * pleas_bottleneck_batched as one call (HIP events), and split into its LAP (the library's per-kernel HIP-event timing
    of pleas_lsap_batched, pleas_prof_*) and the rest: the t* kernel, the masking kernel and the launches;
  * pleas_lsap_batched alone on the same matrices;
  * scipy_solve_minimax_assignment, the reference's host solver (with its device-to-host copies).

Run on the GPU box under a time limit:  timeout -k 10 300 python tools/bottleneck_bench.py [--reps 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def matrices(seed=7):
    spec = json.load(open(os.path.join(ROOT, "tests", "golden", "spec_resnet101.json")))["spec"]
    g = torch.Generator().manual_seed(seed)
    mats = []
    for row in spec:
        n = row["size"]
        x = torch.randn(n, 64, generator=g)
        y = x[torch.randperm(n, generator=g)] + 0.5 * torch.randn(n, 64, generator=g)
        mats.append((-torch.cdist(x, y)).float().contiguous())
    return mats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    from pleas.core.solvers import scipy_solve_minimax_assignment
    from pleas_merging_amd import hip_ops

    mats = [m.cuda() for m in matrices()]
    hip_ops.solve_bottleneck_batched(mats)          # warm-up: library load, code objects
    hip_ops.solve_lsa_batched(mats)
    torch.cuda.synchronize()

    def timed(fn):
        best = float("inf")
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            best = min(best, a.elapsed_time(b))
        return best

    whole = timed(lambda: hip_ops.solve_bottleneck_batched(mats, deferred=[]))
    lsap = timed(lambda: hip_ops.solve_lsa_batched(mats))
    hip_ops.profile_enable(True)
    hip_ops.profile_reset()
    hip_ops.solve_bottleneck_batched(mats)
    prof = hip_ops.profile_collect()
    hip_ops.profile_enable(False)
    res = {"tool": "bottleneck_bench", "groups": len(mats), "sizes": sorted({m.shape[0] for m in mats}),
           "batched_ms": round(whole, 2), "lap_in_batched_ms": round(prof.get("lsap", (0, 0.0))[1], 2),
           "lsap_alone_ms": round(lsap, 2)}
    res["t_kernel_and_mask_ms"] = round(whole - res["lap_in_batched_ms"], 2)
    res["batched_over_lsap"] = round(whole / lsap, 3)
    if not args.no_scipy:
        t0 = time.perf_counter()
        for m in mats:
            scipy_solve_minimax_assignment(m)
        res["scipy_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        res["speedup_vs_scipy"] = round(res["scipy_ms"] / whole, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
