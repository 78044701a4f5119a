#!/usr/bin/env python3
"""Times ReLU6 in the fused epilogues against the same chains with the activation left as a separate pass, in one process.  A GPU
is required.

(a) Fused against unfused, at N = 16 and N = 128: ONE fused call carrying ``ACT_RELU6`` against the same call with ``ACT_NONE``
    followed by ``F.relu6`` (in place, the vendor's elementwise kernel) -- what a graph that does not recognise the activation runs.
    ``bn_act`` on the three activation shapes below; ``conv2d_bn_act`` for the 1 x 1 layers 96 -> 24 at 56 x 56 and 320 -> 1280 at
    7 x 7; ``dwconv2d`` (3 x 3, pad 1) for 144 channels at 56 x 56 with stride 1 and 2 and 960 channels at 7 x 7.
(b) A whole evaluation forward of ``mobilenet_v2()`` at 16 x 3 x 224 x 224: the ``InferenceBackbone`` under
    ``depthwise_form("hip")`` against the module forward on the vendor's kernels (``torch.no_grad``, eval mode).

Both legs warmed, device events around windows of calls, 5 windows per leg ALTERNATING, the median over the windows of a window's
time per call.  A window's time holds the enqueue as well as the kernels: the two are NOT separated, so at small shapes the figures
compare launch counts (one against two) as much as memory passes.  Not measured: kernel times alone (no profiler run), the twin /
source / BN-reset forwards, other batch sizes, a trained checkpoint's activation statistics.

Prints one JSON line and writes it to ``--out`` (default profiles/relu6_bench.json).
Run under a time limit:  timeout -k 10 600 python tools/relu6_bench.py
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

BN_SHAPES = [(24, 56), (144, 56), (1280, 7)]                    # (C, H): bn_act on [N, C, H, H]
PW_SHAPES = [(96, 24, 56), (320, 1280, 7)]                      # (Cin, Cout, H): 1 x 1 convolutions
DW_SHAPES = [(144, 56, 1), (144, 56, 2), (960, 7, 1)]           # (C, H, stride): depthwise 3 x 3, pad 1
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


def _row(kind, N, shape, legs, calls):
    t = {k: statistics.median(v) for k, v in alternate(legs, calls).items()}
    return {"op": kind, "N": N, "shape": shape, "fused_us": round(t["fused"] * 1e6, 2), "unfused_us": round(t["unfused"] * 1e6, 2),
            "fused_over_unfused": round(t["fused"] / t["unfused"], 3), "fused_wins": bool(t["fused"] <= t["unfused"])}


def fused_table(batches, calls):
    from pleas_merging_amd import hip_ops

    six, none = hip_ops.ACT_RELU6, hip_ops.ACT_NONE
    rows = []
    for N in batches:
        for C, H in BN_SHAPES:
            g = torch.Generator().manual_seed(C + H)
            x, s, t = (6 * torch.randn(N, C, H, H, generator=g)).cuda(), torch.randn(C, generator=g).cuda(), torch.randn(C, generator=g).cuda()
            rows.append(_row("bn_act", N, "C%d %dx%d" % (C, H, H),
                             {"fused": lambda: hip_ops.bn_act(x, s, t, None, six),
                              "unfused": lambda: F.relu6(hip_ops.bn_act(x, s, t, None, none), inplace=True)}, calls))
        for Cin, Cout, H in PW_SHAPES:
            g = torch.Generator().manual_seed(Cin + Cout)
            x, w = torch.randn(N, Cin, H, H, generator=g).cuda(), (torch.randn(Cout, Cin, 1, 1, generator=g) / Cin ** 0.5).cuda()
            s, t = torch.randn(Cout, generator=g).cuda(), torch.randn(Cout, generator=g).cuda()
            rows.append(_row("conv2d_bn_act", N, "1x1 %d->%d %dx%d" % (Cin, Cout, H, H),
                             {"fused": lambda: hip_ops.conv2d_bn_act(x, w, None, 1, 0, False, s, t, None, six),
                              "unfused": lambda: F.relu6(hip_ops.conv2d_bn_act(x, w, None, 1, 0, False, s, t, None, none)[1], inplace=True)}, calls))
        for C, H, stride in DW_SHAPES:
            g = torch.Generator().manual_seed(C + H + stride)
            x, w = torch.randn(N, C, H, H, generator=g).cuda(), torch.randn(C, 1, 3, 3, generator=g).cuda()
            s, t = torch.randn(C, generator=g).cuda(), torch.randn(C, generator=g).cuda()
            rows.append(_row("dwconv2d", N, "C%d %dx%d s%d" % (C, H, H, stride),
                             {"fused": lambda: hip_ops.dwconv2d(x, w, None, stride, 1, s, t, None, six),
                              "unfused": lambda: F.relu6(hip_ops.dwconv2d(x, w, None, stride, 1, s, t, None, none)[1], inplace=True)}, calls))
    return rows


def whole_forward(batch, calls):
    from pleas_merging_amd import hip_ops
    from pleas_merging_amd.methods import source_forward as sf
    from pleas_merging_amd.mobilenet import mobilenet_v2

    torch.manual_seed(0)
    g = torch.Generator().manual_seed(0)
    net = mobilenet_v2().train()
    with torch.no_grad():
        net(torch.randn(4, 3, 224, 224, generator=g))          # BatchNorm statistics of the random weights
    net = net.eval().cuda()
    x = torch.randn(batch, 3, 224, 224, generator=g).cuda()
    with hip_ops.depthwise_form("hip"):
        graph = sf.InferenceBackbone(net)
        nodes = list(graph.graph.graph.nodes)
        fused = [n for n in nodes if n.op == "call_function" and isinstance(n.target, sf.HipConvAct)]

        def modules():
            with torch.no_grad():
                return net(x)

        got, want = graph(x), modules()
        rel = float((got - want).norm() / want.norm())
        per_window = alternate({"hip_graph": lambda: graph(x), "modules": modules}, calls)
    med = {k: statistics.median(v) for k, v in per_window.items()}
    return {"batch": batch, "calls_per_window": calls, "graph_calls": sum(1 for n in nodes if n.op in ("call_function", "call_module")),
            "conv_chains_fused": len(fused), "of_them_relu6": sum(1 for n in fused if n.args[4] == hip_ops.ACT_RELU6),
            "logits_rel_fro_from_modules": rel,
            "forward_ms_windows": {k: [round(s * 1e3, 3) for s in v] for k, v in per_window.items()},
            "forward_ms_median": {k: round(s * 1e3, 3) for k, s in med.items()},
            "hip_graph_over_modules": round(med["hip_graph"] / med["modules"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="calls per window of the fused / unfused pairs")
    ap.add_argument("--forwards", type=int, default=10, help="forwards per window of the whole model")
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relu6_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("relu6_bench: a GPU is required")
    result = {"tool": "relu6_bench", "device": torch.cuda.get_device_name(0), "calls_per_window": args.calls, "windows": WINDOWS,
              "timing": "device events around a window of calls: enqueue and kernel time are not separated",
              "fused_vs_unfused": fused_table(args.batches, args.calls), "mobilenet_v2_forward": whole_forward(16, args.forwards)}
    lost = [r for r in result["fused_vs_unfused"] if not r["fused_wins"]]
    result["fused_slower_than_unfused"] = ["%s N%d %s" % (r["op"], r["N"], r["shape"]) for r in lost]
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
