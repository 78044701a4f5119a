#!/usr/bin/env python3
"""Times the depthwise kernels (csrc/dwconv.hip) against the vendor's path of the same commit, in one process.  A GPU is required.

1. Forward, per MobileNet-family shape (k = 3, pad 1) at N = 16 and N = 128: ``hip_ops.dwconv2d`` against
   ``F.conv2d(groups=C)``.  Both warmed, device events, 5 windows per leg ALTERNATING, the median over the windows of a window's
   time per call.  Algorithmic bytes ``4 (N C (Hin Win + Ho Wo) + C K K)`` over that time, and its share of the 8 TB/s peak.
2. One PLeaS update of a MobileNet-shaped stack (those depthwise layers alternating with 1 x 1 layers, batch 16, ratio 0) under
   ``depthwise_form("hip")`` and under ``"vendor"``: two fitters, windows of ``--updates`` updates alternating, per form the median
   over its windows of a window's time per update, the vendor path's spread between its windows, and ``fast_updates``.

Prints one JSON line and writes it to ``--out`` (default profiles/dwconv_bench.json).
Run under a time limit:  timeout -k 10 600 python tools/dwconv_bench.py
"""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch import nn  # noqa: E402

SHAPES = [(32, 112, 1), (96, 112, 2), (144, 56, 1), (144, 56, 2), (192, 28, 1), (192, 28, 2), (384, 14, 1), (576, 14, 2), (960, 7, 1)]
PEAK_BYTES_PER_S = 8e12
WINDOWS = 5


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / calls


def alternate(legs, calls, warm=3):
    """``{name: [seconds per call of each window]}``: the legs' windows alternate."""
    for fn in legs.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in legs}
    for _ in range(WINDOWS):
        for name, fn in legs.items():
            out[name].append(window(fn, calls))
    return out


def forward_table(batches, calls):
    from pleas_merging_amd import hip_ops

    rows = []
    for N in batches:
        for C, H, stride in SHAPES:
            g = torch.Generator().manual_seed(C + H)
            x = torch.randn(N, C, H, H, generator=g).cuda()
            w = torch.randn(C, 1, 3, 3, generator=g).cuda()
            Ho = (H + 2 - 3) // stride + 1
            out = torch.empty(N, C, Ho, Ho, device="cuda")
            legs = {"hip": lambda: hip_ops.dwconv2d(x, w, None, stride, 1, out=out),
                    "vendor": lambda: F.conv2d(x, w, None, stride, 1, 1, C)}
            t = {k: statistics.median(v) for k, v in alternate(legs, calls).items()}
            nbytes = 4.0 * (N * C * (H * H + Ho * Ho) + C * 9)
            rows.append({"N": N, "C": C, "H": H, "stride": stride, "hip_us": round(t["hip"] * 1e6, 2), "vendor_us": round(t["vendor"] * 1e6, 2),
                         "hip_TBps": round(nbytes / t["hip"] / 1e12, 3), "hip_share_of_peak": round(nbytes / t["hip"] / PEAK_BYTES_PER_S, 3),
                         "vendor_TBps": round(nbytes / t["vendor"] / 1e12, 3), "hip_wins": bool(t["hip"] <= t["vendor"])})
            del x, w, out
    return rows


class Stack(nn.Module):
    """3 x 3 stride-2 stem, then per entry of SHAPES a depthwise 3 x 3 (+ BN + ReLU) and a 1 x 1 to the next entry's width
    (+ BN + ReLU), pool, fc: MobileNet's layer pattern on the benchmark's shapes."""

    def __init__(self, classes=1000):
        super().__init__()
        self.stem = nn.Conv2d(3, SHAPES[0][0], 3, stride=2, padding=1, bias=False)
        self.stem_bn = nn.BatchNorm2d(SHAPES[0][0])
        widths = [c for c, _, _ in SHAPES[1:]] + [320]
        self.blocks = nn.ModuleList()
        for (c, _, stride), nxt in zip(SHAPES, widths):
            self.blocks.append(nn.Sequential(nn.Conv2d(c, c, 3, stride=stride, padding=1, groups=c, bias=False), nn.BatchNorm2d(c), nn.ReLU(),
                                             nn.Conv2d(c, nxt, 1, bias=False), nn.BatchNorm2d(nxt), nn.ReLU()))
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(320, classes)

    def forward(self, x):
        x = torch.relu(self.stem_bn(self.stem(x)))
        for block in self.blocks:
            x = block(x)
        return self.fc(torch.flatten(self.avgpool(x), 1))


def stack_update(batch, updates):
    from pleas_merging_amd import hip_ops
    from pleas_merging_amd.core.compiler import get_permutation_spec
    from pleas_merging_amd.core.utils import make_identity_perm
    from pleas_merging_amd.methods import partial_merge
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
    fits, turn = {}, {"hip": 0, "vendor": 0}
    for form in ("hip", "vendor"):
        with hip_ops.depthwise_form(form):
            fits[form] = PleasFitter(models[0], models[1], copy.deepcopy(merged), spec, perm, costs, 0.0, 10 ** 6, num_classes=1000)

    def step(form):
        def run():
            fits[form].step(xs[turn[form] % len(xs)])
            turn[form] += 1
        return run

    per_window = alternate({form: step(form) for form in fits}, updates)
    med = {k: statistics.median(v) for k, v in per_window.items()}
    spread = max(per_window["vendor"]) - min(per_window["vendor"])
    depthwise = sum(1 for p in fits["hip"].plans if p.dw)
    return {"batch": batch, "updates_per_window": updates, "windows": WINDOWS, "depthwise_layers": depthwise,
            "vendor_layers": {k: len(f.vendor_layers) for k, f in fits.items()},
            "update_ms_windows": {k: [round(s * 1e3, 3) for s in v] for k, v in per_window.items()},
            "update_ms_median": {k: round(s * 1e3, 3) for k, s in med.items()}, "vendor_spread_ms": round(spread * 1e3, 3),
            "hip_not_slower_than_vendor_plus_spread": bool(med["hip"] <= med["vendor"] + spread),
            "fast_updates": {k: f.fast_updates for k, f in fits.items()}, "updates_run": dict(turn)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="forward calls per window")
    ap.add_argument("--updates", type=int, default=30, help="updates per window")
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dwconv_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dwconv_bench: a GPU is required")
    result = {"tool": "dwconv_bench", "device": torch.cuda.get_device_name(0), "kernel": 3, "pad": 1, "peak_TBps": PEAK_BYTES_PER_S / 1e12,
              "calls_per_window": args.calls, "windows": WINDOWS, "forward": forward_table(args.batches, args.calls),
              "stack_update": stack_update(16, args.updates)}
    lost = [r for r in result["forward"] if not r["hip_wins"]]
    result["forward_shapes_lost_to_vendor"] = ["N%d C%d H%d s%d" % (r["N"], r["C"], r["H"], r["stride"]) for r in lost]
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
