#!/usr/bin/env python3
"""Times the BN-statistics reset that every driver runs after ``train`` (``reset_bn_stats``) on a merged ResNet-101 (ratio 0.5:
widths 1.5x): 101 device-resident batches of 16 at 224 x 224, three legs alternating inside one process --

  ``vendor``    ``fused=False``: the model's own modules (the reference's loop)
  ``modules``   ``fused=True, backbone="modules"``: HIP BatchNorm folds, vendor convolutions
  ``hip``       ``fused=True, backbone="hip"``: the library's own convolutions, batch statistics from their epilogues

Per leg: one warm-up call, then ``--repeats`` (>= 5) timed calls, HIP events around the call and a synchronise.  Every call
starts from the same merged model (``reset_bn_stats`` resets the running statistics itself).  Also reports whether two ``hip``
calls left ``torch.equal`` state dicts, and whether two ``modules`` calls did.  Prints one JSON line and, with ``--out``, writes
it to a file.

Run on the GPU box under a time limit:  timeout -k 10 900 python tools/bn_reset_bench.py --out profiles/bn_reset_bench.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def build(arch, batch, n_distinct, size, seed=0):
    from pleas_merging_amd import resnet as zoo
    from pleas_merging_amd.core.compiler import get_permutation_spec
    from pleas_merging_amd.core.utils import make_identity_perm
    from pleas_merging_amd.methods import partial_merge

    g = torch.Generator().manual_seed(seed)
    calib = [torch.randn(8, 3, size, size, generator=g) for _ in range(2)]
    models = []
    for s in (0, 1):
        torch.manual_seed(s)
        m = zoo.MODELS[arch](num_classes=1000)
        zoo.calibrate_bn(m, calib)
        models.append(m.eval())
    spec = get_permutation_spec(models[0], ((1, 3, size, size),))
    perm = make_identity_perm(spec)
    costs = {k: (torch.eye(grp.size) + 0.01 * torch.rand(grp.size, grp.size, generator=g)).cuda() for k, grp in spec.items()}
    merged = partial_merge(spec, models[0].cuda(), models[1].cuda(), perm, costs, 0.5).cuda()
    xs = [torch.randn(batch, 3, size, size, generator=g).cuda() for _ in range(n_distinct)]
    return merged, xs


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3, out


def same_state(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="resnet101")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--batches", type=int, default=101)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--distinct", type=int, default=8, help="distinct device-resident batches the 101 cycle through")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 2:
        ap.error("--repeats: at least two calls per leg (the repeatability report compares two)")
    from pleas_merging_amd.methods import reset_bn_stats

    merged, xs = build(args.arch, args.batch, args.distinct, args.size)
    data = [(xs[i % len(xs)], None) for i in range(args.batches)]
    legs = {"vendor": dict(fused=False), "modules": dict(fused=True, backbone="modules"), "hip": dict(fused=True, backbone="hip")}

    def call(kw):
        reset_bn_stats(merged, data, args.batches, **kw)
        return {k: v.clone() for k, v in merged.state_dict().items() if "running_" in k or k.endswith("num_batches_tracked")}

    for kw in legs.values():
        timed(lambda: call(kw))
    seconds, states = {name: [] for name in legs}, {name: [] for name in legs}
    for _ in range(args.repeats):                  # legs alternate: vendor, modules, hip, vendor, ...
        for name, kw in legs.items():
            s, state = timed(lambda: call(kw))
            seconds[name].append(s)
            states[name] = (states[name] + [state])[-2:]
    result = {"tool": "bn_reset_bench", "arch": args.arch, "merge_ratio": 0.5, "input": "%dx%d" % (args.size, args.size),
              "batch": args.batch, "batches": args.batches, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
              "seconds_per_call": {k: [round(s, 4) for s in v] for k, v in seconds.items()},
              "median_seconds": {k: round(statistics.median(v), 4) for k, v in seconds.items()},
              "min_max_seconds": {k: [round(min(v), 4), round(max(v), 4)] for k, v in seconds.items()},
              "two_runs_equal": {k: same_state(*states[k]) for k in ("hip", "modules")},
              "note": "every call includes building its runner (fx trace); batches are device-resident"}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
