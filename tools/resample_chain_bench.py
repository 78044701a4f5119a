#!/usr/bin/env python3
"""Times the train transform of most of the reference's datasets, ``Resize(256)`` -> ``RandomResizedCrop(224)`` (-> flip, table),
on ragged uint8 batches (16 and 128 images, sides U(300..450) x U(400..600), 3 channels), legs alternating inside one process --

  ``chain``         (a) ``hip_ops.image_resample_chain`` into a preallocated output: the four launches, on a packed batch and a
                    chain plan already on the device; boxes drawn by ``DeviceImages(pre_resize=256, resized_crop=(224, 224))``
  ``single_crop`` / ``single_window``   (b) the two single-stage paths on the same images: ``hip_ops.image_resample`` for
                    ``RandomResizedCrop(224)`` boxes on the images themselves, and for ``Resize(256)`` + the centre 224 x 224 window
  ``stock``         (c) the device chain a caller can write with stock operators, per image: ``F.interpolate(bilinear,
                    antialias=True)`` to ``(H1, W1)``, slice the box, interpolate to 224 x 224, flip; then one normalise
  ``pil_per_image`` (d) PIL's chain per image on one host thread (host clock; None where PIL does not import)
  ``h2d``           (e) the pinned host-to-device copy of the packed batch with its chain plan and flags, as ``DeviceImages`` sends it

Per device leg: a warm-up, then ``--repeats`` (>= 5) windows of calls enqueued back to back, HIP events around the window and a
synchronise; the figure is the window over the calls, so it holds launch gaps when a call is shorter than its enqueue.
``algorithmic_bytes``: the source bytes under the first stage's taps (rows the boxes' vertical pass reads x columns their
horizontal pass reads), both scratches and the intermediate written and read once, the fp32 output written once; over the time,
as a fraction of 8 TB/s.  The kernels must be ``torch.equal`` to the host executor or the tool fails.  Prints one JSON line and,
with ``--out``, writes it.

Run on the GPU box under a time limit:
    timeout -k 10 400 python tools/resample_chain_bench.py --out profiles/image_resample_chain_bench.json
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
PRE = 256


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls          # microseconds per call


def taps_span(n_in, n_out, first, count):
    """Inputs ``[lo, hi)`` that outputs ``first .. first + count`` of a PIL bilinear pass from ``n_in`` to ``n_out`` read."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    lo = max(0, int((first + 0.5) * scale - fs + 0.5))
    hi = min(n_in, int((first + count - 0.5) * scale + fs + 0.5))
    return lo, hi


def pil_chain_us(images, geom):
    try:
        from PIL import Image
    except ImportError:
        return None
    pil = [Image.frombytes("RGB", (im.shape[1], im.shape[0]), im.numpy().tobytes()) for im in images]
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        for img, (H, W, H1, W1, y0, x0, h, w) in zip(pil, geom.tolist()):
            img.resize((W1, H1), Image.BILINEAR).crop((x0, y0, x0 + w, y0 + h)).resize((SIZE[1], SIZE[0]), Image.BILINEAR)
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
    dev_images = [im.permute(2, 0, 1).unsqueeze(0).float().cuda() for im in images]
    out = torch.empty(n, 3, *SIZE, device="cuda")
    legs, facts = {}, {"src_bytes": src_bytes}

    # (a) the chain
    geom, flip = DeviceImages([], MEAN, STD, "cuda", pre_resize=PRE, resized_crop=SIZE, flip=True, seed=0).chain_augmentation(
        0, 0, list(zip(hs, ws)))
    t0 = time.perf_counter()
    plan = ops.image_resample_chain_plan(geom, offsets, 3, SIZE, src_bytes)
    facts["plan_host_us"] = round((time.perf_counter() - t0) * 1e6, 1)
    info = ops.image_resample_chain_plan_info(plan)
    plan_d, flip_d = plan.cuda(), flip.cuda()
    want = ops.image_resample_chain_host(host_src, plan, table, flip=flip)[0]
    got = ops.image_resample_chain(src, plan_d, plan, table_d, flip=flip_d, out=out)
    if not torch.equal(got.cpu(), want):
        sys.exit("resample_chain_bench: the kernels and the host executor differ at batch %d" % n)
    legs["chain"] = lambda: ops.image_resample_chain(src, plan_d, plan, table_d, flip=flip_d, out=out)
    read = 0
    for H, W, H1, W1, y0, x0, h, w in geom.tolist():
        (rlo, rhi), (clo, chi) = taps_span(H, H1, y0, h), taps_span(W, W1, x0, w)
        read += 3 * (rhi - rlo) * (chi - clo)
    facts.update(plan_bytes=plan.numel(), ws_bytes=info["ws_bytes"], mid_bytes=info["mid_bytes"], items=list(info["items"]),
                 source_bytes_read=read, algorithmic_bytes=read + 2 * info["ws_bytes"] + out.numel() * 4,
                 box_area_over_window_area=round(sum(r[6] * r[7] for r in geom.tolist()) / (n * SIZE[0] * SIZE[1]), 3))

    # (b) the two single-stage paths on the same images
    singles = {"single_crop": DeviceImages([], MEAN, STD, "cuda", resized_crop=SIZE, flip=True, seed=0),
               "single_window": DeviceImages([], MEAN, STD, "cuda", resize=PRE, crop=SIZE, seed=None)}
    for name, wrapper in singles.items():
        g10, f10 = wrapper.ragged_augmentation(0, 0, list(zip(hs, ws)))
        p10 = ops.image_resample_plan(g10, offsets, 3, SIZE, src_bytes)
        p10_d, f10_d, out10 = p10.cuda(), (f10.cuda() if f10 is not None else None), torch.empty_like(out)
        legs[name] = lambda p10_d=p10_d, p10=p10, f10_d=f10_d, out10=out10: ops.image_resample(src, p10_d, p10, table_d, flip=f10_d, out=out10)

    # (c) the stock device chain on the chain's own boxes
    boxes, flags = geom.tolist(), flip.tolist()

    def stock():
        planes = []
        for im, (H, W, H1, W1, y0, x0, h, w), fl in zip(dev_images, boxes, flags):
            x = F.interpolate(im, size=(H1, W1), mode="bilinear", antialias=True, align_corners=False)
            x = F.interpolate(x[:, :, y0:y0 + h, x0:x0 + w], size=SIZE, mode="bilinear", antialias=True, align_corners=False)
            planes.append(x.flip(3) if fl else x)
        return torch.cat(planes).div(255).sub(mean_d).div(std_d)

    legs["stock"] = stock
    diff = (stock() - got).mul(std_d).mul(255).abs()
    facts["stock_max_level_diff"] = round(float(diff.max()), 3)
    facts["stock_share_of_pixels_off_by_half_a_level"] = round(float((diff > 0.5).float().mean()), 4)

    # (d) PIL on one host thread, (e) the staging buffer DeviceImages would send: plan | flags | images
    pil = pil_chain_us(images, geom)
    facts["pil_per_image_us"] = None if pil is None else round(pil, 1)
    total = (plan.numel() + 15) // 16 * 16 + (n + 15) // 16 * 16 + src_bytes
    staged, sink = torch.empty(total, dtype=torch.uint8).pin_memory(), torch.empty(total, dtype=torch.uint8, device="cuda")
    legs["h2d"] = lambda: sink.copy_(staged, non_blocking=True)
    facts["h2d_bytes"] = total
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
        sys.exit("resample_chain_bench: no GPU; nothing is measured on the host")
    from pleas_merging_amd import hip_ops as ops
    from pleas_merging_amd.methods import DeviceImages

    result = {"tool": "resample_chain_bench",
              "input": "uint8 hwc, sides U(300..450) x U(400..600), 3 channels -> Resize(256) -> RandomResizedCrop(224)",
              "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "calls_per_window": args.calls,
              "hbm_peak_tb_s": HBM_PEAK / 1e12, "batch": {}}
    for n in args.batches:
        legs, facts = legs_for(n, ops, DeviceImages)
        calls = {name: max(5, args.calls // 10) if name in ("stock", "h2d") else args.calls for name in legs}
        for name, fn in legs.items():
            window(fn, 3)
        us = {name: [] for name in legs}
        for _ in range(args.repeats):                  # legs alternate
            for name, fn in legs.items():
                us[name].append(window(fn, calls[name]))
        med = {k: statistics.median(v) for k, v in us.items()}
        a, b = med["chain"], med["single_crop"] + med["single_window"]
        row = dict(facts, median_us={k: round(v, 2) for k, v in med.items()},
                   min_max_us={k: [round(min(v), 2), round(max(v), 2)] for k, v in us.items()},
                   kernels_equal_host_executor_bits=True, chain_over_sum_of_singles=round(a / b, 3),
                   stock_over_chain=round(med["stock"] / a, 2), chain_below_stock=bool(a < med["stock"]),
                   chain_tb_s=round(facts["algorithmic_bytes"] / (a * 1e-6) / 1e12, 3),
                   chain_roof_fraction=round(facts["algorithmic_bytes"] / (a * 1e-6) / HBM_PEAK, 3),
                   h2d_gb_s=round(facts["h2d_bytes"] / (med["h2d"] * 1e-6) / 1e9, 1), h2d_over_chain=round(med["h2d"] / a, 2))
        if facts["pil_per_image_us"] is not None:
            row["pil_batch_us"] = round(n * facts["pil_per_image_us"], 1)
            row["chain_below_pil_batch"] = bool(a < row["pil_batch_us"])
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
