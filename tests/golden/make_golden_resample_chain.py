#!/usr/bin/env python3
"""Writes tests/golden/resample_chain_pil.npz: what PIL makes of the chains of tests/resample_chain_cases.py
(``resize -> crop -> resize``, all BILINEAR), for 1, 3 and 4 channels, on random bytes and on a ramp.  Uses PIL and numpy only.
Per case the file holds the expected final ``[Ho, Wo, C]`` bytes (``want``), the expected image between the two resizes ``[h, w,
C]`` (``mid``), the final bytes at the common size of a batch of all the cases (``want_batch``), the descriptor and the CRC-32
of the input, which the tests regenerate from its seed (``resample_chain_cases.source``) and check against that CRC.

Two identities are asserted on the way, with PIL alone: the chain equals "window of the first resize, then whole-image resize of
that window", and a first stage that leaves the size unchanged (case ``id``) equals the single-stage resized crop.

    python tests/golden/make_golden_resample_chain.py
"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import PIL  # noqa: E402
from PIL import Image  # noqa: E402
import resample_chain_cases as cc  # noqa: E402


def _image(a):
    return Image.frombytes(cc.PIL_MODES[a.shape[2]], (a.shape[1], a.shape[0]), np.ascontiguousarray(a).tobytes())


def _array(img, channels):
    return np.frombuffer(img.tobytes(), dtype=np.uint8).reshape(img.size[1], img.size[0], channels).copy()


def main():
    out = {"pil_version": np.array(PIL.__version__)}
    for case in cc.CASES:
        geom = cc.geom_row(case)
        H, W, H1, W1, y0, x0, h, w = geom
        Ho, Wo = case[5:7]
        for channels in cc.CHANNELS:
            for fill in cc.FILLS:
                src = cc.source(case, channels, fill)
                k = cc.key(case, channels, fill)
                mid, want = cc.pil_chain(src, geom, Ho, Wo)
                first = _array(_image(src).resize((W1, H1), Image.BILINEAR), channels)
                assert np.array_equal(mid, first[y0:y0 + h, x0:x0 + w])
                assert np.array_equal(want, _array(_image(mid).resize((Wo, Ho), Image.BILINEAR), channels))
                if (H1, W1) == (H, W):
                    single = _image(src).crop((x0, y0, x0 + w, y0 + h)).resize((Wo, Ho), Image.BILINEAR)
                    assert np.array_equal(want, _array(single, channels))
                out[k + "/want"] = want
                out[k + "/mid"] = mid
                out[k + "/want_batch"] = cc.pil_chain(src, geom, *cc.BATCH_SIZE)[1]
                out[k + "/geom"] = np.array(geom, dtype=np.int32)
                out[k + "/src_crc"] = np.array(zlib.crc32(src.tobytes()), dtype=np.uint32)
    path = os.path.join(HERE, "resample_chain_pil.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(cc.CASES) * len(cc.CHANNELS) * len(cc.FILLS), "cases")


if __name__ == "__main__":
    main()
