#!/usr/bin/env python3
"""Times the resampling of ragged uint8 batches (16 and 128 images, sides drawn around 375 x 500, 3 channels, output 224 x 224)
for the two chains of the drivers' loaders, legs alternating inside one process --

  ``kernels_train`` / ``kernels_eval``   ``hip_ops.image_resample`` into a preallocated output: the two launches, on a packed
                    batch and a plan already on the device.  train: ``RandomResizedCrop(224)`` boxes drawn by ``DeviceImages``;
                    eval: ``Resize(256)`` + ``CenterCrop(224)``
  ``stock_train`` / ``stock_eval``       the device chain a caller can write with stock operators, per image: slice the box,
                    ``permute / float``, ``F.interpolate(mode="bilinear", antialias=True)``, crop the window, then one
                    ``stack / div / sub / div`` for the batch (its result is NOT the PIL chain's: reported as a level count)
  ``h2d``           the pinned host-to-device copy of the packed batch with its plan and flags, as ``DeviceImages`` sends it
  ``plan_host``     building the plan on the host (host clock), and, where PIL imports, ``pil_per_image``: the per-image CPU
                    time of the PIL chain the path replaces (host clock, one thread)

Per device leg: a warm-up, then ``--repeats`` (>= 5) windows of calls enqueued back to back, HIP events around the window and a
synchronise; the figure is the window over the calls, so it holds launch gaps when a call is shorter than its enqueue.
``roof``: the algorithmic traffic -- the boxes' source rows under the window (h * Ho / Hv of them) read once and the fp32 output
written once -- over the time, as a fraction of 8 TB/s; ``traffic_with_rows`` adds the uint8 intermediate written and read once.
The kernels must be ``torch.equal`` to the host executor or the tool fails.  Prints one JSON line and, with ``--out``, writes it.

Run on the GPU box under a time limit:  timeout -k 10 300 python tools/resample_bench.py --out profiles/image_resample_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
HBM_PEAK = 8.0e12
SIZE = (224, 224)


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls          # microseconds per call


def pil_chain_us(images, geom):
    """Per-image host time of the PIL chain (decoded image in hand: crop, resize, crop), or None without PIL."""
    try:
        from PIL import Image
    except ImportError:
        return None
    pil = [Image.frombytes("RGB", (im.shape[1], im.shape[0]), im.numpy().tobytes()) for im in images]
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        for img, g in zip(pil, geom.tolist()):
            H, W, y0, x0, h, w, Hv, Wv, oy, ox = g
            img.crop((x0, y0, x0 + w, y0 + h)).resize((Wv, Hv), Image.BILINEAR).crop((ox, oy, ox + SIZE[1], oy + SIZE[0]))
        dt = (time.perf_counter() - t0) * 1e6 / len(pil)
        best = dt if best is None else min(best, dt)
    return best


def legs_for(n, ops, DeviceImages):
    g = torch.Generator().manual_seed(n)
    hs = torch.randint(300, 451, (n,), generator=g).tolist()
    ws = torch.randint(400, 601, (n,), generator=g).tolist()
    images = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g) for h, w in zip(hs, ws)]
    sizes = [im.numel() for im in images]
    offsets = [sum(sizes[:i]) for i in range(n)]
    src_bytes = sum(sizes)
    host_src = torch.cat([im.reshape(-1) for im in images])
    src = host_src.cuda()
    table = ops.image_table(MEAN, STD, 3)
    table_d = table.cuda()
    mean_d, std_d = torch.tensor(MEAN).view(1, 3, 1, 1).cuda(), torch.tensor(STD).view(1, 3, 1, 1).cuda()
    dev_images = [im.cuda() for im in images]
    draws = {"train": DeviceImages([], MEAN, STD, "cuda", resized_crop=SIZE, flip=True, seed=0),
             "eval": DeviceImages([], MEAN, STD, "cuda", resize=256, crop=SIZE, seed=None)}
    legs, facts = {}, {}
    for name, wrapper in draws.items():
        geom, flip = wrapper.ragged_augmentation(0, 0, list(zip(hs, ws)))
        t0 = time.perf_counter()
        plan = ops.image_resample_plan(geom, offsets, 3, SIZE, src_bytes)
        plan_us = (time.perf_counter() - t0) * 1e6
        info = ops.image_resample_plan_info(plan)
        plan_d = plan.cuda()
        flip_d = flip.cuda() if flip is not None else None
        out = torch.empty(n, 3, *SIZE, device="cuda")
        want, _ = ops.image_resample_host(host_src, plan, table, flip=flip)
        got = ops.image_resample(src, plan_d, plan, table_d, flip=flip_d, out=out)
        if not torch.equal(got.cpu(), want):
            sys.exit("resample_bench: the kernels and the host executor differ at batch %d (%s)" % (n, name))
        boxes = geom.tolist()

        def stock(boxes=boxes, flip=flip):
            planes = []
            for i, (im, b) in enumerate(zip(dev_images, boxes)):
                H, W, y0, x0, h, w, Hv, Wv, oy, ox = b
                x = im[y0:y0 + h, x0:x0 + w].permute(2, 0, 1).unsqueeze(0).float()
                x = F.interpolate(x, size=(Hv, Wv), mode="bilinear", antialias=True, align_corners=False)
                x = x[:, :, oy:oy + SIZE[0], ox:ox + SIZE[1]]
                planes.append(x.flip(3) if flip is not None and flip[i] else x)
            return torch.cat(planes).div(255).sub(mean_d).div(std_d)

        own = lambda plan_d=plan_d, plan=plan, flip_d=flip_d, out=out: ops.image_resample(src, plan_d, plan, table_d, flip=flip_d, out=out)
        legs["kernels_" + name], legs["stock_" + name] = own, stock
        # what the stock chain makes of the same boxes, in 8-bit levels of the un-normalised value
        diff = (stock() - got).mul(std_d).mul(255).abs()
        # source rows under the window: all of the box for a resized crop, its share Ho / Hv for resize + window
        box_bytes = sum(3 * b[5] * -(-b[4] * SIZE[0] // b[6]) for b in boxes)
        dst_bytes = out.numel() * 4
        facts[name] = {"plan_bytes": plan.numel(), "plan_host_us": round(plan_us, 1), "ws_bytes": info["ws_bytes"], "items": list(info["items"]),
                       "algorithmic_bytes": box_bytes + dst_bytes, "traffic_with_rows": box_bytes + dst_bytes + 2 * info["ws_bytes"],
                       "stock_max_level_diff": round(float(diff.max()), 3),
                       "stock_share_of_pixels_off_by_half_a_level": round(float((diff > 0.5).float().mean()), 4),
                       "pil_per_image_us": pil_chain_us(images, geom)}
        if facts[name]["pil_per_image_us"] is not None:
            facts[name]["pil_per_image_us"] = round(facts[name]["pil_per_image_us"], 1)
        if name == "train":                                  # the staging buffer DeviceImages would send: plan | flags | images
            total = (plan.numel() + 15) // 16 * 16 + (n + 15) // 16 * 16 + src_bytes
            staged = torch.empty(total, dtype=torch.uint8).pin_memory()
            sink = torch.empty(total, dtype=torch.uint8, device="cuda")
            legs["h2d"] = lambda staged=staged, sink=sink: sink.copy_(staged, non_blocking=True)
            facts["h2d_bytes"] = total
    facts["src_bytes"] = src_bytes
    return legs, facts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats: medians of at least 5 windows")
    if not torch.cuda.is_available():
        sys.exit("resample_bench: no GPU; nothing is measured on the host")
    from pleas_merging_amd import hip_ops as ops
    from pleas_merging_amd.methods import DeviceImages

    result = {"tool": "resample_bench", "input": "uint8 hwc, sides U(300..450) x U(400..600), 3 channels -> 224 x 224",
              "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "calls_per_window": args.calls,
              "hbm_peak_tb_s": HBM_PEAK / 1e12, "batch": {}}
    for n in args.batches:
        legs, facts = legs_for(n, ops, DeviceImages)
        calls = {name: args.calls if name.startswith("kernels") else max(5, args.calls // 10) for name in legs}
        for name, fn in legs.items():
            window(fn, 3)
        us = {name: [] for name in legs}
        for _ in range(args.repeats):                  # legs alternate
            for name, fn in legs.items():
                us[name].append(window(fn, calls[name]))
        med = {k: statistics.median(v) for k, v in us.items()}
        row = {"median_us": {k: round(v, 2) for k, v in med.items()},
               "min_max_us": {k: [round(min(v), 2), round(max(v), 2)] for k, v in us.items()},
               "kernels_equal_host_executor_bits": True}
        for name in ("train", "eval"):
            f = facts[name]
            k = med["kernels_" + name]
            f["stock_over_kernels"] = round(med["stock_" + name] / k, 2)
            f["kernels_tb_s"] = round(f["algorithmic_bytes"] / (k * 1e-6) / 1e12, 3)
            f["kernels_roof_fraction"] = round(f["algorithmic_bytes"] / (k * 1e-6) / HBM_PEAK, 3)
            f["kernels_roof_fraction_with_rows"] = round(f["traffic_with_rows"] / (k * 1e-6) / HBM_PEAK, 3)
            f["with_kernels_us"] = round(med["h2d"] + k, 2)
            row[name] = f
        row["src_bytes"], row["h2d_bytes"] = facts["src_bytes"], facts["h2d_bytes"]
        row["h2d_gb_s"] = round(facts["h2d_bytes"] / (med["h2d"] * 1e-6) / 1e9, 1)
        result["batch"][str(n)] = row
    result["note"] = ("per call = window of back-to-back calls / calls (Python wrapper included): a call shorter than its enqueue is "
                      "measured at the enqueue rate; copies and conversions are timed apart, not overlapped; host figures are host clocks")
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
