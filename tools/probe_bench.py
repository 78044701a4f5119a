#!/usr/bin/env python3
"""Times the linear probe's head and a whole probe (``train_eval_linear_probe``) at ResNet-50's 2048 features, 200 classes,
batches of 64 and 256, everything device-resident.

1. The head alone: one training step on a fixed feature batch -- ``head="hip"`` (``HipProbeHead.step``: own Linear forward,
   ``softmax_xent``, one grouped weight gradient, ``channel_sum``, ``masked_adam``), once per form of ``hip_ops.linear`` (leg
   ``hip``: "conv", the default; leg ``hip_gemm``: ``linear_form("gemm")``), against the autograd step of the default path
   (Linear, cross entropy, backward, Adam, the scheduler, argmax / compare / sum), the latter with and without the
   ``float(loss)`` read-back that path does every step.  ``--warmup`` steps, then ``--repeats`` windows of ``--steps`` steps per
   leg, the legs alternating; HIP events around a window and a synchronise.
2. A whole ``--epochs``-epoch probe on a ResNet-50 under ``backbone="hip"`` over ``--batches`` batches per epoch (and 2 test
   batches): the heads (``hip`` again under both forms), with and without ``cache_features`` (``--probe-legs`` picks legs by
   name, e.g. the three ``*/cache`` ones); one warm-up call (1 epoch) per leg, then ``--repeats`` timed calls.

``--profile-steps N`` instead runs N ``head="hip"`` steps per batch size and form, untimed: run it under
``rocprofv3 --kernel-trace --stats -- python tools/probe_bench.py --profile-steps 100`` to read each kernel's share of a step
(the two forms' forward and bias-gradient kernels have names of their own, the other kernels run 2 N times).

Prints one JSON line and, with ``--out``, writes it to a file.
Run on the GPU box under a time limit:  timeout -k 10 900 python tools/probe_bench.py --out profiles/probe_bench.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from torch import nn  # noqa: E402

D, C = 2048, 200


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3


def head_legs(batch, lr=1e-3):
    """name -> ``run(steps)`` of the four head legs on one fixed batch; every leg owns its head and optimiser state."""
    from pleas_merging_amd import hip_ops
    from pleas_merging_amd.methods.linear_probe import HipProbeHead

    g = torch.Generator().manual_seed(batch)
    feats = torch.randn(batch, D, generator=g).cuda()
    labels = torch.randint(0, C, (batch,), generator=g).cuda()

    def hip_head(form):
        torch.manual_seed(0)
        hip = HipProbeHead(nn.Linear(D, C).cuda())
        state = {"t": 0}

        def run(steps):
            with hip_ops.linear_form(form):
                for _ in range(steps):
                    state["t"] += 1
                    hip.step(feats, labels, lr, state["t"])
            hip.epoch_readback()                   # what an epoch ends with
        return run

    def autograd(readback):
        torch.manual_seed(0)
        fc = nn.Linear(D, C).cuda()
        opt = torch.optim.Adam(fc.parameters(), lr=lr)
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 1 << 30, eta_min=lr / 10)
        loss_fn = nn.CrossEntropyLoss()

        def run(steps):
            hit = torch.zeros((), dtype=torch.long, device="cuda")
            total = 0.0
            for _ in range(steps):
                logits = fc(feats)
                loss = loss_fn(logits, labels)
                opt.zero_grad()
                loss.backward()
                opt.step()
                sched.step()
                hit += (logits.argmax(1) == labels).sum()
                if readback:
                    total += float(loss)
            float(hit)
        return run

    return {"hip": hip_head("conv"), "hip_gemm": hip_head("gemm"), "autograd": autograd(True),
            "autograd_no_readback": autograd(False)}


def backbone_and_data(batch, n_train, seed=0):
    from pleas_merging_amd import resnet as zoo

    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    model = zoo.MODELS["resnet50"](num_classes=1000)
    zoo.calibrate_bn(model, [torch.randn(8, 3, 224, 224, generator=g) for _ in range(2)])
    model.fc = nn.Identity()
    model = model.cuda().eval()
    make = lambda: (torch.randn(batch, 3, 224, 224, generator=g).cuda(), torch.randint(0, C, (batch,), generator=g).cuda())
    distinct = [make() for _ in range(4)]
    return model, [distinct[i % 4] for i in range(n_train)], distinct[:2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-sizes", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--skip-probe", action="store_true")
    ap.add_argument("--probe-legs", nargs="+", default=None, help="whole-probe legs to time, e.g. hip/cache hip_gemm/cache")
    ap.add_argument("--profile-steps", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pleas_merging_amd import hip_ops
    from pleas_merging_amd.methods import train_eval_linear_probe

    if args.profile_steps:
        for batch in args.batch_sizes:
            legs = head_legs(batch)
            legs["hip"](args.profile_steps)
            legs["hip_gemm"](args.profile_steps)
        torch.cuda.synchronize()
        print(json.dumps({"profile_steps": args.profile_steps, "batch_sizes": args.batch_sizes}))
        return
    result = {"tool": "probe_bench", "features": D, "classes": C, "device": torch.cuda.get_device_name(0),
              "head_step": {"steps_timed": args.steps, "steps_warmup": args.warmup, "microseconds_per_step": {}},
              "probe": {"arch": "resnet50", "backbone": "hip", "input": "224x224", "epochs": args.epochs,
                        "train_batches": args.batches, "test_batches": 2, "seconds_per_call": {}}}
    for batch in args.batch_sizes:
        legs = head_legs(batch)
        for run in legs.values():
            timed(lambda: run(args.warmup))
        seconds = {name: [] for name in legs}
        for _ in range(args.repeats):              # legs alternate
            for name, run in legs.items():
                seconds[name].append(timed(lambda: run(args.steps)))
        result["head_step"]["microseconds_per_step"][str(batch)] = {k: [round(1e6 * s / args.steps, 1) for s in v]
                                                                    for k, v in seconds.items()}
    for batch in ([] if args.skip_probe else args.batch_sizes):
        model, train, test = backbone_and_data(batch, args.batches)
        legs = {"%s/%s" % (head, "cache" if cache else "no_cache"): (head, cache)
                for head in ("autograd", "hip", "hip_gemm") for cache in (False, True)}
        if args.probe_legs:
            legs = {name: legs[name] for name in args.probe_legs}

        def probe(head, cache, epochs):
            with hip_ops.linear_form("gemm" if head == "hip_gemm" else "conv"):
                return train_eval_linear_probe(model, train, test, C, None, "bench", epochs=epochs, backbone="hip",
                                               head=head.split("_")[0], cache_features=cache)
        for head, cache in legs.values():
            timed(lambda: probe(head, cache, 1))
        seconds = {name: [] for name in legs}
        for _ in range(args.repeats):
            for name, (head, cache) in legs.items():
                seconds[name].append(timed(lambda: probe(head, cache, args.epochs)))
        result["probe"]["seconds_per_call"][str(batch)] = {k: [round(s, 4) for s in v] for k, v in seconds.items()}
        del model, train, test
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
