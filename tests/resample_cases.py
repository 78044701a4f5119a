"""The geometries of the resampling tests (``pleas_image_resample``), their seeded inputs and the two PIL chains the library
must equal bit for bit (plain data + small helpers, shared by tests/golden/make_golden_resample.py, tests/test_resample_host.py
and tests/test_hip_resample.py).

A case is ``(name, H, W, Ho, Wo, box, resize)``: ``box = (y0, x0, h, w)`` or None = the whole image; ``resize = s`` or None.
  resize is None   resized crop:     img.crop(box).resize((Wo, Ho), BILINEAR)
  resize = s       resize + window:  img.resize(Resize(s)'s size, BILINEAR).crop(centre Ho x Wo window)
Chosen to cover: one tap (1 x 1), two to three taps (upscaling), many taps (300 -> 5), clamped edges, an unchanged axis, a box
with odd origin, a window.  Each runs on random bytes and on a smooth ramp, for 1, 3 and 4 channels.
"""
import zlib

import numpy as np

CASES = [
    ("down", 37, 53, 16, 24, None, None),
    ("up", 20, 31, 32, 32, None, None),
    ("near", 9, 7, 8, 8, None, None),
    ("pixel", 1, 1, 4, 4, None, None),
    ("tiny", 2, 3, 7, 5, None, None),
    ("mixed", 300, 17, 5, 40, None, None),
    ("axis", 64, 64, 64, 32, None, None),
    ("box", 120, 90, 48, 32, (20, 10, 75, 60), None),
    ("eval_tall", 50, 37, 20, 20, None, 24),
    ("eval_wide", 31, 64, 20, 20, None, 24),
]
CHANNELS = (1, 3, 4)
FILLS = ("random", "ramp")
PIL_MODES = {1: "L", 3: "RGB", 4: "CMYK"}      # plain 8-bit bands ("RGBA" would be premultiplied by Image.resize)


def key(case, channels, fill):
    return "%s/c%d/%s" % (case[0], channels, fill)


def resized_size(height, width, s):
    """torchvision's ``Resize(s)``: the shorter side becomes ``s``, the longer one ``int(s * long / short)``."""
    return (int(s * height / width), s) if width <= height else (s, int(s * width / height))


def geom_row(case):
    """The int32 descriptor ``H, W, y0, x0, h, w, Hv, Wv, oy, ox`` of a case (include/pleas_hip.h)."""
    _, H, W, Ho, Wo, box, resize = case
    y0, x0, h, w = box if box is not None else (0, 0, H, W)
    if resize is None:
        return [H, W, y0, x0, h, w, Ho, Wo, 0, 0]
    Hv, Wv = resized_size(H, W, resize)
    return [H, W, y0, x0, h, w, Hv, Wv, int(round((Hv - Ho) / 2.0)), int(round((Wv - Wo) / 2.0))]


def source(case, channels, fill):
    """The uint8 ``[H, W, C]`` input of a case: a frozen stream (``RandomState``) seeded by the case's key, or a ramp."""
    _, H, W = case[:3]
    if fill == "random":
        seed = zlib.crc32(key(case, channels, fill).encode()) & 0x7fffffff
        return np.random.RandomState(seed).randint(0, 256, (H, W, channels)).astype(np.uint8)
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(channels), indexing="ij")
    return np.clip(255.0 * (x + y) / max(H + W - 2, 1) + 10 * c, 0, 255).astype(np.uint8)


def pil_chain(src, geom, Ho, Wo):
    """The PIL chain of a descriptor on a uint8 ``[H, W, C]`` array: crop the box, resize to the virtual size, crop the window."""
    from PIL import Image

    H, W, y0, x0, h, w, Hv, Wv, oy, ox = [int(v) for v in geom]
    C = src.shape[2]
    img = Image.frombytes(PIL_MODES[C], (W, H), np.ascontiguousarray(src).tobytes())
    out = img.crop((x0, y0, x0 + w, y0 + h)).resize((Wv, Hv), Image.BILINEAR).crop((ox, oy, ox + Wo, oy + Ho))
    return np.frombuffer(out.tobytes(), dtype=np.uint8).reshape(Ho, Wo, C).copy()
