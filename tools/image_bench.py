#!/usr/bin/env python3
"""Times the step in front of the first convolution for uint8 image batches of 224 x 224 x 3 (16 and 128 images), legs
alternating inside one process --

  ``kernel``        ``hip_ops.image_batch`` into a preallocated output: whole images, rows on 16-byte boundaries
  ``kernel_shifted``  the same call on a src moved by one byte: no row on a 16-byte boundary (what a crop with odd x0 gives)
  ``kernel_aug``    random 192 x 192 crops and flips: the mix a training loader produces (origins uploaded per call)
  ``stock``         what a caller can do today with stock operators on the same GPU:
                    ``permute / float / div / sub / div / contiguous`` on the device-resident uint8 batch
  ``h2d_u8`` / ``h2d_fp32``   the pinned host-to-device copy of the batch as uint8, and of the host-normalised fp32 batch

Per leg: a warm-up, then ``--repeats`` (>= 5) windows of ``--calls`` calls enqueued back to back, HIP events around the window
and a synchronise; the figure is the window over the calls, so it holds launch gaps when a call is shorter than its enqueue
(16 images: said in the output).  ``roof`` is the kernel's algorithmic traffic, 5 bytes per output element, over the time, as a
fraction of 8 TB/s.  The kernel must be ``torch.equal`` to the chain computed on the CPU or the tool fails; whether the stock
device chain is, is reported.  Prints one JSON line
and, with ``--out``, writes it.  ``--profile-legs N``: N calls of ``kernel`` and ``stock`` per batch size and nothing else, for
a ``rocprofv3 --kernel-trace --stats`` pass.

Run on the GPU box under a time limit:  timeout -k 10 300 python tools/image_bench.py --out profiles/image_batch_bench.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
HBM_PEAK = 8.0e12


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls          # microseconds per call


def legs_for(n, size, ops):
    g = torch.Generator().manual_seed(n)
    host_u8 = torch.randint(0, 256, (n, size, size, 3), dtype=torch.uint8, generator=g).pin_memory()
    mean, std = torch.tensor(MEAN).view(1, 3, 1, 1), torch.tensor(STD).view(1, 3, 1, 1)
    host_fp32 = host_u8.permute(0, 3, 1, 2).float().div(255).sub(mean).div(std).contiguous().pin_memory()
    u8 = host_u8.cuda()
    shifted = torch.empty(u8.numel() + 16, dtype=torch.uint8, device="cuda")[1:1 + u8.numel()].view(u8.shape)
    shifted.copy_(u8)
    table = ops.image_table(MEAN, STD, 3).cuda()
    mean_d, std_d = mean.cuda(), std.cuda()
    out = torch.empty(n, 3, size, size, device="cuda")
    crop = size - 32
    out_aug = torch.empty(n, 3, crop, crop, device="cuda")
    origin = torch.randint(0, size - crop + 1, (n, 2), generator=g)
    flip = torch.randint(0, 2, (n,), generator=g)
    sink_u8, sink_fp32 = torch.empty_like(u8), torch.empty_like(out)

    def stock():
        return u8.permute(0, 3, 1, 2).float().div(255).sub(mean_d).div(std_d).contiguous()

    legs = {
        "kernel": lambda: ops.image_batch(u8, table, out=out),
        "kernel_shifted": lambda: ops.image_batch(shifted, table, out=out),
        "kernel_aug": lambda: ops.image_batch(u8, table, out=out_aug, origin=origin, flip=flip, size=(crop, crop)),
        "stock": stock,
        "h2d_u8": lambda: sink_u8.copy_(host_u8, non_blocking=True),
        "h2d_fp32": lambda: sink_fp32.copy_(host_fp32, non_blocking=True),
    }
    want = host_fp32.cuda()          # the chain as the drivers run it, on the CPU
    same = all(torch.equal(legs[k](), want) for k in ("kernel", "kernel_shifted"))
    return legs, same, bool(torch.equal(stock(), want)), out.numel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--profile-legs", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats: medians of at least 5 windows")
    if not torch.cuda.is_available():
        sys.exit("image_bench: no GPU; nothing is measured on the host")
    from pleas_merging_amd import hip_ops as ops

    result = {"tool": "image_bench", "input": "%dx%dx3 uint8 nhwc" % (args.size, args.size), "device": torch.cuda.get_device_name(0),
              "repeats": args.repeats, "calls_per_window": args.calls, "hbm_peak_tb_s": HBM_PEAK / 1e12, "batch": {}}
    for n in args.batches:
        legs, same, stock_same, elements = legs_for(n, args.size, ops)
        if not same:
            sys.exit("image_bench: the kernel and the CPU chain differ at batch %d" % n)
        if args.profile_legs:
            for name in ("kernel", "stock"):
                for _ in range(args.profile_legs):
                    legs[name]()
            torch.cuda.synchronize()
            continue
        for fn in legs.values():
            window(fn, 10)
        us = {name: [] for name in legs}
        for _ in range(args.repeats):                  # legs alternate
            for name, fn in legs.items():
                us[name].append(window(fn, args.calls if not name.startswith("h2d") else max(10, args.calls // 10)))
        med = {k: statistics.median(v) for k, v in us.items()}
        result["batch"][str(n)] = {
            "median_us": {k: round(v, 2) for k, v in med.items()},
            "min_max_us": {k: [round(min(v), 2), round(max(v), 2)] for k, v in us.items()},
            "kernel_equals_cpu_chain_bits": same,
            "stock_equals_cpu_chain_bits": stock_same,
            "stock_over_kernel": round(med["stock"] / med["kernel"], 2),
            "stock_over_kernel_shifted": round(med["stock"] / med["kernel_shifted"], 2),
            "kernel_shifted_over_kernel": round(med["kernel_shifted"] / med["kernel"], 2),
            "kernel_algorithmic_bytes": 5 * elements,
            "kernel_tb_s": round(5 * elements / (med["kernel"] * 1e-6) / 1e12, 3),
            "kernel_roof_fraction": round(5 * elements / (med["kernel"] * 1e-6) / HBM_PEAK, 3),
            "kernel_shifted_roof_fraction": round(5 * elements / (med["kernel_shifted"] * 1e-6) / HBM_PEAK, 3),
            "caller_today_us": {"u8_h2d_plus_stock": round(med["h2d_u8"] + med["stock"], 2), "fp32_h2d": round(med["h2d_fp32"], 2)},
            "with_kernel_us": round(med["h2d_u8"] + med["kernel"], 2),
        }
    if args.profile_legs:
        return
    result["note"] = ("per call = window of back-to-back calls / calls (Python wrapper included): a call shorter than its enqueue "
                      "is measured at the enqueue rate; copies and conversions are timed apart, not overlapped")
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
