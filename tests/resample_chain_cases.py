"""The geometries of the chain resampling tests (``pleas_image_resample_chain``), their seeded inputs and the PIL chain the
library must equal bit for bit (plain data + small helpers, shared by tests/golden/make_golden_resample_chain.py,
tests/test_resample_chain_host.py and tests/test_hip_resample_chain.py).

A case is ``(name, H, W, s, box, Ho, Wo)``: ``Resize(s)`` takes the ``H x W`` image to ``H1 x W1`` (shorter side ``s``), ``box =
(y0, x0, h, w)`` inside ``H1 x W1`` or None = all of it, resampled to ``Ho x Wo``:
    img.resize((W1, H1), BILINEAR).crop((x0, y0, x0 + w, y0 + h)).resize((Wo, Ho), BILINEAR)
The smallest shapes at which a stage can go wrong:
  dd    down, then down; a box with odd origin          ud    up, then down
  du    many taps, then up; a tall image                id    a first stage that leaves the size unchanged
  px    one tap                                         one   a 1 x 1 box in the last row and column
  edge  a box touching the bottom-right corner
Each runs on random bytes and on a smooth ramp, for 1, 3 and 4 channels.  A batch has ONE output size, so the fixture also holds
every case's output at ``BATCH_SIZE``: that is what a ragged batch of all the cases is compared with.
"""
import zlib

import numpy as np

CASES = [
    ("dd", 37, 53, 24, (3, 5, 17, 22), 16, 16),
    ("ud", 9, 7, 20, None, 8, 8),
    ("du", 300, 17, 8, (60, 1, 30, 6), 12, 10),
    ("id", 24, 40, 24, (2, 3, 20, 30), 16, 16),
    ("px", 1, 1, 4, None, 4, 4),
    ("one", 20, 31, 12, (11, 17, 1, 1), 5, 5),
    ("edge", 50, 37, 24, (20, 10, 12, 14), 7, 9),
]
FIRST_SIZES = {"dd": (24, 34), "ud": (25, 20), "du": (141, 8), "id": (24, 40), "px": (4, 4), "one": (12, 18), "edge": (32, 24)}
BATCH_SIZE = (16, 16)
CHANNELS = (1, 3, 4)
FILLS = ("random", "ramp")
PIL_MODES = {1: "L", 3: "RGB", 4: "CMYK"}      # plain 8-bit bands ("RGBA" would be premultiplied by Image.resize)


def key(case, channels, fill):
    return "%s/c%d/%s" % (case[0], channels, fill)


def resized_size(height, width, s):
    """torchvision's ``Resize(s)``: the shorter side becomes ``s``, the longer one ``int(s * long / short)``."""
    return (int(s * height / width), s) if width <= height else (s, int(s * width / height))


def geom_row(case):
    """The int32 descriptor ``H, W, H1, W1, y0, x0, h, w`` of a case (include/pleas_hip.h)."""
    name, H, W, s, box, _, _ = case
    H1, W1 = resized_size(H, W, s)
    assert (H1, W1) == FIRST_SIZES[name]
    y0, x0, h, w = box if box is not None else (0, 0, H1, W1)
    return [H, W, H1, W1, y0, x0, h, w]


def source(case, channels, fill):
    """The uint8 ``[H, W, C]`` input of a case: a frozen stream (``RandomState``) seeded by the case's key, or a ramp."""
    _, H, W = case[:3]
    if fill == "random":
        seed = zlib.crc32(("chain/" + key(case, channels, fill)).encode()) & 0x7fffffff
        return np.random.RandomState(seed).randint(0, 256, (H, W, channels)).astype(np.uint8)
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(channels), indexing="ij")
    return np.clip(255.0 * (x + y) / max(H + W - 2, 1) + 10 * c, 0, 255).astype(np.uint8)


def pil_chain(src, geom, Ho, Wo):
    """PIL's chain of a descriptor on a uint8 ``[H, W, C]`` array: ``(intermediate [h, w, C], final [Ho, Wo, C])``."""
    from PIL import Image

    H, W, H1, W1, y0, x0, h, w = [int(v) for v in geom]
    C = src.shape[2]
    img = Image.frombytes(PIL_MODES[C], (W, H), np.ascontiguousarray(src).tobytes())
    mid = img.resize((W1, H1), Image.BILINEAR).crop((x0, y0, x0 + w, y0 + h))
    out = mid.resize((Wo, Ho), Image.BILINEAR)
    return (np.frombuffer(mid.tobytes(), dtype=np.uint8).reshape(h, w, C).copy(),
            np.frombuffer(out.tobytes(), dtype=np.uint8).reshape(Ho, Wo, C).copy())
