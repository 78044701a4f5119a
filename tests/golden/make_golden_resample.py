#!/usr/bin/env python3
"""Writes tests/golden/resample_pil.npz: what PIL's ``Image.resize(..., BILINEAR)`` makes of the cases of
tests/resample_cases.py (crop + resize, and resize + centre window), for 1, 3 and 4 channels, on random bytes and on a ramp.
Uses PIL and numpy only.  Per case the file holds the expected ``[Ho, Wo, C]`` bytes, the descriptor and the CRC-32 of the
input, which the tests regenerate from its seed (``resample_cases.source``) and check against that CRC.

    python tests/golden/make_golden_resample.py
"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import PIL  # noqa: E402
import resample_cases as rc  # noqa: E402


def main():
    out = {"pil_version": np.array(PIL.__version__)}
    for case in rc.CASES:
        geom = rc.geom_row(case)
        for channels in rc.CHANNELS:
            for fill in rc.FILLS:
                src = rc.source(case, channels, fill)
                k = rc.key(case, channels, fill)
                out[k + "/want"] = rc.pil_chain(src, geom, case[3], case[4])
                out[k + "/geom"] = np.array(geom, dtype=np.int32)
                out[k + "/src_crc"] = np.array(zlib.crc32(src.tobytes()), dtype=np.uint32)
    path = os.path.join(HERE, "resample_pil.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(rc.CASES) * len(rc.CHANNELS) * len(rc.FILLS), "cases")


if __name__ == "__main__":
    main()
