"""The geometries of the tile-form tests of the convolution forward (csrc/conv_fwd.hip) and the weight gradient
(csrc/conv.hip), and the host-only queries that say which form the library picks for one (plain data + small helpers; no
GPU, no tensors).  Shared by tests/test_hip_kernels.py, test_hip_determinism.py, test_hip_split_bf16.py (the tables they
always ran on), tests/test_tile_coverage.py (the ledger: every reachable form has a case) and tests/test_hip_tile_forms.py
(every case on the GPU).

Forward forms (fwd_describe): 0 / 1 = general tile with 128 / 64 rows and 16-byte weight loads, 2 / 3 = the same with scalar
weight loads (Cin * k * k % 4 != 0), 4 / 5 / 6 = 128-row flat-shift tile for 1 x 1 layers with HW % 4 == 0 / 1 x 1 with
HW % 4 != 0 / k x k, 7 / 8 / 9 = the same with 64 rows.  Weight-gradient `variant` bits: pleas_hip.h, pleas_wgrad_plan_info.

A comment after a case says what the case is FOR; the form it takes today is what the ledger prints."""
import contextlib
import ctypes

F_TN = 128          # pixels per forward tile (fTN)
W_BK = 32           # pixels per weight-gradient chunk (kBK)

# ------------------------------------------------------------------------------------------------ forward
FWD_CASES = [
    # N, Cout, Cin, H, W, k, stride, pad, bias
    (4, 256, 64, 14, 14, 1, 1, 0, False),
    (4, 64, 256, 14, 14, 1, 1, 0, False),     # TM = 64
    (3, 96, 80, 7, 7, 1, 1, 0, False),        # ragged pixels / channels
    (4, 128, 128, 14, 14, 3, 1, 1, False),    # 3x3 with padding
    (2, 40, 24, 9, 11, 3, 1, 1, False),       # non-square image
    (4, 128, 64, 28, 28, 3, 2, 1, False),     # stride 2
    (3, 72, 96, 10, 7, 3, 1, 1, False),       # kernel-position-major with ragged rows / pixels, non-square image
    (2, 64, 32, 12, 12, 5, 1, 2, False),      # 5x5 taps
    (2, 64, 3, 32, 32, 7, 2, 3, False),       # stem geometry: Kd = 147 (scalar weight loads)
    (16, 70, 300, 1, 1, 1, 1, 0, True),       # linear layer with bias
    # flat-shift tile forms (stride 1, "same" padding, Cin % 32 == 0): one LDS image per channel block, taps = shifts
    (5, 200, 96, 14, 14, 1, 1, 0, False),     # 1x1, 16-B pixel loads, ragged last pixel tile (980 pixels) and channel tile
    (3, 136, 64, 7, 7, 1, 1, 0, False),       # 1x1, HW = 49: scalar pixel loads, tiles straddle samples
    (16, 40, 64, 1, 1, 1, 1, 0, True),        # linear layer on the flat path (HW = 1), TM = 64, bias
    (5, 136, 64, 14, 14, 3, 1, 1, False),     # 3x3: tiles straddle samples and rows, every border case
    (2, 64, 32, 56, 56, 3, 1, 1, False),      # 3x3 at W = 56: widest halo (242 data columns), TM = 64
    (3, 130, 96, 7, 7, 3, 1, 1, False),       # 3x3 at 7x7: halo 8, three samples per tile
    (2, 72, 32, 9, 11, 5, 1, 2, False),       # 5x5 "same", non-square image
    (3, 96, 64, 28, 28, 3, 1, 1, True),       # 3x3 at W = 28 with bias
]

# the plain convolution's geometries (test_hip_determinism.py), in ITS column order
GEOMETRIES = [
    # (N, Cin, H, W, Cout, k, stride, pad, bias)
    (4, 64, 56, 56, 64, 3, 1, 1, False),       # flat-shift k x k form, kernel-position-major weights
    (3, 128, 28, 28, 96, 3, 1, 1, True),       # Cout not a multiple of the tile, bias
    (2, 128, 56, 56, 128, 3, 2, 1, False),     # strided 3 x 3: general form
    (2, 3, 224, 224, 64, 7, 2, 3, False),      # the stem: K = 147, scalar weight loads
    (5, 512, 7, 7, 512, 3, 1, 1, False),       # 7 x 7 images (HW % 4 != 0)
    (2, 32, 17, 23, 40, 5, 1, 2, True),        # H != W, 5 x 5
    (2, 48, 15, 15, 24, 3, 1, 0, False),       # "valid" padding, Cin % 32 != 0
    (3, 256, 14, 14, 1024, 1, 1, 0, False),    # 1 x 1 (mode "all")
    (2, 256, 56, 56, 512, 1, 2, 0, False),     # strided 1 x 1 (mode "all")
]
# the two more of test_conv2d_bn_act_equals_the_two_launches_it_replaces
GEOMETRIES_BN_EXTRA = [
    (2, 64, 56, 56, 256, 1, 1, 0, False),      # short-K 1 x 1, 128-row tiles
    (3, 2048, 7, 7, 512, 1, 1, 0, False),      # 1 x 1 on 7 x 7 images
]

# Cases added for the ledger (tests/test_tile_coverage.py): small tensors, one purpose each.  FWD_CASES order.
FWD_NEW_CASES = [
    # general 128-row tile with scalar weight loads (Cout > 64, Cin * k * k odd / not a multiple of 4): unreached before
    (3, 130, 15, 9, 7, 3, 1, 1, True),        # Kd = 135: ragged channel + pixel tiles, tiles straddle samples, bias, H != W
    (2, 200, 33, 5, 6, 1, 2, 0, False),       # Kd = 33, strided 1 x 1, HWo = 9
    (2, 72, 3, 12, 10, 5, 1, 3, True),        # Kd = 75, pad > k / 2: output larger than the input
    # general 64-row tile, scalar weight loads: bias, H != W, pad beyond "same"
    (3, 40, 5, 7, 9, 3, 2, 2, True),          # Kd = 45
    # general tiles with 16-byte weight loads: what the hand-picked cases left out (bias; 128 rows with H != W)
    (3, 136, 24, 9, 11, 3, 1, 0, True),       # 128 rows, "valid" padding, ragged everything
    (5, 48, 64, 10, 7, 3, 2, 1, True),        # 64 rows, stride 2; kernel-position-major in the general tile
    (2, 24, 16, 3, 4, 5, 1, 3, True),         # image smaller than the kernel, pad 3: 64 rows
    (2, 200, 64, 4, 5, 7, 1, 3, False),       # 7 x 7 "same" (49 taps: no flat form), 128 rows, kernel-position-major too
    # flat 1 x 1 forms
    (3, 56, 64, 6, 10, 1, 1, 0, True),        # 64 rows, HW = 60 (16-byte pixel loads): ragged everything, bias
    (5, 64, 256, 14, 14, 1, 1, 0, False),     # 256 -> 64 (the layer1 conv1 shape of a bottleneck ResNet), whole channel tile
    (3, 40, 32, 7, 7, 1, 1, 0, True),         # 64 rows, HW = 49: scalar pixel loads off HW = 1, tiles straddle samples, bias
    (5, 56, 96, 5, 3, 1, 1, 0, False),        # 64 rows, HW = 15
    (3, 200, 32, 5, 5, 1, 1, 0, True),        # 128 rows, HW = 25, bias
    (4, 130, 64, 6, 6, 1, 1, 0, True),        # 128 rows, HW = 36, bias
    # flat k x k forms: bias and H != W on both tile heights
    (3, 136, 32, 6, 10, 3, 1, 1, True),       # 128 rows
    (3, 40, 64, 5, 9, 5, 1, 2, True),         # 64 rows, 5 x 5
]

FWD_TABLE = (FWD_CASES + [(N, Cout, Cin, H, W, k, s, p, b) for (N, Cin, H, W, Cout, k, s, p, b) in GEOMETRIES + GEOMETRIES_BN_EXTRA]
             + FWD_NEW_CASES)

# ------------------------------------------------------------------------------------------------ weight gradient
WGRAD_CASES = [
    # N, Cout, Cin, H, W, k, stride, pad
    (4, 256, 64, 14, 14, 1, 1, 0),     # 1x1: direct loader, TN = 64
    (4, 64, 256, 14, 14, 1, 1, 0),     # TM = 64
    (3, 96, 80, 7, 7, 1, 1, 0),        # HW = 49: scalar loads, ragged tiles
    (4, 128, 128, 14, 14, 3, 1, 1),    # 3x3 "same" at HW % 4 == 0: shifted through aligned 16-byte loads, padding
    (2, 40, 24, 9, 11, 3, 1, 1),       # ragged everything, non-square image
    (4, 128, 64, 28, 28, 3, 2, 1),     # 3x3 stride 2
    (4, 256, 128, 28, 28, 1, 2, 0),    # 1x1 stride 2 (downsample)
    (2, 64, 64, 56, 56, 3, 1, 1),      # long pixel axis -> split into slabs + reduce
    (16, 64, 32, 1, 1, 1, 1, 0),       # linear-like (HW = 1)
    # fewer than 16 input channels: rows of the tile are (channel, tap) pairs ("virtual channels")
    (4, 64, 3, 224, 224, 7, 2, 3),     # the ResNet stem (K = 147, slabs + reduce)
    (2, 8, 3, 9, 11, 3, 1, 1),         # tiny, ragged, one tile
    (2, 20, 5, 12, 12, 5, 2, 2),       # 5x5 stride 2: 125 virtual channels, HWo = 36
    (3, 70, 15, 7, 7, 3, 1, 1),        # 135 virtual channels: TN = 128, HW = 49 (scalar residual loads)
    # images with HW % 4 != 0 on stride-1 same-size layers (one pixel per load; a padded-pixel 16-byte form was built and measured
    # in round 5: no gain on these short-K layers, profiles/r05_padk_ab.txt -- the cases stay)
    (4, 96, 64, 7, 7, 3, 1, 1),        # 3x3 at 7 x 7 (layer4)
    (16, 512, 512, 7, 7, 3, 1, 1),     # the same at ResNet size: 128 x 128 tiles, 25 chunks
    (16, 2048, 512, 7, 7, 1, 1, 0),    # 1x1 at 7 x 7, batch 16 (layer4 conv3)
    (2, 20, 32, 5, 5, 5, 1, 2),        # 5x5 "same" on a 5 x 5 image (HW = 25)
    (1, 33, 17, 3, 3, 1, 1, 0),        # one sample, HW = 9: the last row's run is clamped at the tensor's end
]

# Cases added for the ledger, picked by a greedy cover of the (variant, slabs, staged rows) combinations the grid reaches under
# either arithmetic, smallest tensors first: output channels 24 / 72 and input channels 3 / 20 / 65 make every channel tile
# ragged, N in the tens to hundreds on a tiny image makes the pixel axis long enough for slabs in a small tensor.  Which
# combination a case takes is what the ledger prints.
WGRAD_NEW_CASES = [
    # 1 x 1, stride 1
    (3, 72, 3, 2, 3, 1, 1, 0),
    (3, 24, 3, 6, 10, 1, 1, 0),
    (3, 72, 3, 6, 10, 1, 1, 0),
    (617, 24, 3, 2, 3, 1, 1, 0),
    (62, 24, 3, 6, 10, 1, 1, 0),
    (617, 72, 3, 2, 3, 1, 1, 0),
    (62, 72, 3, 6, 10, 1, 1, 0),
    (3, 24, 3, 2, 3, 1, 1, 0),
    (3, 72, 20, 2, 3, 1, 1, 0),
    (3, 24, 20, 6, 10, 1, 1, 0),
    (185, 24, 20, 2, 3, 1, 1, 1),
    (106, 24, 20, 3, 5, 1, 1, 1),
    (617, 24, 20, 2, 3, 1, 1, 0),
    (62, 24, 20, 6, 10, 1, 1, 0),
    (185, 72, 20, 2, 3, 1, 1, 1),
    (106, 72, 20, 3, 5, 1, 1, 1),
    (617, 72, 20, 2, 3, 1, 1, 0),
    (62, 72, 20, 6, 10, 1, 1, 0),
    (3, 24, 20, 2, 3, 1, 1, 0),
    (3, 72, 20, 6, 10, 1, 1, 0),
    (3, 24, 65, 2, 3, 1, 1, 0),
    (3, 72, 65, 2, 3, 1, 1, 0),
    (3, 24, 65, 2, 3, 1, 1, 1),
    (3, 72, 65, 2, 3, 1, 1, 1),
    (3, 24, 65, 6, 10, 1, 1, 0),
    (3, 72, 65, 6, 10, 1, 1, 0),
    (185, 24, 65, 2, 3, 1, 1, 1),
    (106, 24, 65, 3, 5, 1, 1, 1),
    (617, 24, 65, 2, 3, 1, 1, 0),
    (62, 24, 65, 6, 10, 1, 1, 0),
    (185, 72, 65, 2, 3, 1, 1, 1),
    (106, 72, 65, 3, 5, 1, 1, 1),
    (617, 72, 65, 2, 3, 1, 1, 0),
    (62, 72, 65, 6, 10, 1, 1, 0),
    # 1 x 1, stride 2
    (3, 24, 20, 2, 3, 1, 2, 0),
    (3, 72, 20, 2, 3, 1, 2, 0),
    (3, 72, 20, 3, 5, 1, 2, 1),
    (3, 24, 65, 2, 3, 1, 2, 0),
    (3, 72, 65, 2, 3, 1, 2, 0),
    # 3 x 3, stride 1
    (3, 24, 3, 6, 10, 3, 1, 1),
    (3, 72, 3, 6, 10, 3, 1, 1),
    (106, 24, 3, 3, 5, 3, 1, 2),
    (62, 24, 3, 6, 10, 3, 1, 1),
    (185, 72, 3, 2, 3, 3, 1, 2),
    (106, 72, 3, 3, 5, 3, 1, 2),
    (3, 24, 20, 6, 10, 3, 1, 1),
    (3, 72, 20, 6, 10, 3, 1, 1),
    (62, 72, 20, 6, 10, 3, 1, 1),
    (62, 24, 20, 6, 10, 3, 1, 1),
    (3, 24, 65, 6, 10, 3, 1, 1),
    (62, 24, 65, 6, 10, 3, 1, 1),
    (62, 72, 65, 6, 10, 3, 1, 1),
    (3, 72, 65, 6, 10, 3, 1, 1),
    # 3 x 3, stride 2
    (3, 72, 3, 2, 3, 3, 2, 1),
    (3, 24, 3, 2, 3, 3, 2, 1),
    (3, 24, 20, 3, 5, 3, 2, 2),
    # 5 x 5, stride 1
    (62, 72, 3, 6, 10, 5, 1, 2),
    (185, 24, 3, 2, 3, 5, 1, 3),
    (106, 24, 3, 3, 5, 5, 1, 3),
    (106, 72, 3, 3, 5, 5, 1, 3),
    # 5 x 5, stride 2
    (3, 24, 3, 2, 3, 5, 2, 2),
    (3, 72, 3, 8, 12, 5, 2, 0),
    (3, 72, 3, 2, 3, 5, 2, 2),
    (3, 24, 3, 3, 5, 5, 2, 3),
]

WGRAD_TABLE = WGRAD_CASES + WGRAD_NEW_CASES


# ------------------------------------------------------------------------------------------------ the library's answers
@contextlib.contextmanager
def arith(mode):
    """``pleas_arith(mode)`` for the block; the exact arithmetic again afterwards."""
    from pleas_merging_amd import _lib

    lib = _lib.lib()
    assert lib.pleas_arith_get() == 0
    lib.pleas_arith(mode)
    try:
        yield
    finally:
        lib.pleas_arith(0)


def out_hw(H, W, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def kpos_legal(case):
    """Kernel-position-major weights: a k x k layer with whole 32-channel blocks."""
    return case[5] > 1 and case[2] % 32 == 0


def fwd_layouts(case):
    """The weight layouts a forward test runs a case in: standard, and kernel-position-major where legal."""
    return (False, True) if kpos_legal(case) else (False,)


FWD_ENTRY_POINTS = ("fwd_batch", "conv2d", "conv2d_bn_act")


def fwd_runs(entry):
    """(case, kernel-position-major) pairs that the GPU tests of one forward entry point run (tests/test_hip_tile_forms.py takes
    its list from here, tests/test_tile_coverage.py its ledger): the whole table, both weight layouts where legal."""
    if entry not in FWD_ENTRY_POINTS:
        raise KeyError(entry)
    return [(c, kp) for c in FWD_TABLE for kp in fwd_layouts(c)]


def wgrad_runs():
    """(case, destination layout flag) pairs that the GPU test of the weight gradient runs (each overwriting and accumulating)."""
    return [(c, fl) for c in WGRAD_TABLE for fl in wgrad_layouts(c)]


def fwd_layer(case, kpos):
    from pleas_merging_amd import _lib

    N, Cout, Cin, H, W, k, stride, pad = case[:8]
    a = _lib.FwdLayer()
    a.N, a.Cout, a.Cin, a.Hin, a.Win, a.KH, a.KW, a.stride, a.pad = N, Cout, Cin, H, W, k, k, stride, pad
    a.Csrc, a.n_merged, a.flags = Cout, Cout, 1 if kpos else 0
    return a


def fwd_units(cases_kpos, form_ms=None, max_units=24):
    """``pleas_fwd_plan_units`` of a layer list: [(form, first item, items, lane)] in launch order."""
    from pleas_merging_amd import _lib

    n = len(cases_kpos)
    arr = (_lib.FwdLayer * n)(*[fwd_layer(c, kp) for c, kp in cases_kpos])
    units = (ctypes.c_int * (4 * max_units))()
    ms = None if form_ms is None else (ctypes.c_double * 10)(*form_ms)
    got = _lib.lib().pleas_fwd_plan_units(arr, n, ms, units, max_units)
    if got <= 0 or got > max_units:
        raise RuntimeError("pleas_fwd_plan_units: %d (%s)" % (got, _lib.lib().pleas_last_error().decode()))
    return [tuple(units[4 * i:4 * i + 4]) for i in range(got)]


def fwd_form(case, kpos):
    """The tile form the library gives this layer (one-layer plan: one unit)."""
    units = fwd_units([(case, kpos)])
    assert len(units) == 1, units
    return units[0][0]


def fwd_tile_rows(form):
    return 128 if form in (0, 2, 4, 5, 6) else 64


def fwd_traits(case, kpos, form):
    """What of a tile form's edges a case exercises."""
    N, Cout, Cin, H, W, k, stride, pad, bias = case
    Ho, Wo = out_hw(H, W, k, stride, pad)
    t = set()
    if Cout % fwd_tile_rows(form):
        t.add("ragged_cout")
    if (N * Ho * Wo) % F_TN:
        t.add("ragged_pixels")
    if N > 1 and (Ho * Wo) % F_TN:        # some tile holds the last pixels of one sample and the first of the next
        t.add("straddles_samples")
    if bias:
        t.add("bias")
    if k > 1 and H != W:
        t.add("h_ne_w")
    return t


WG_ACC, WG_KPOS = 1, 2


def wgrad_geo(case, flags=0):
    N, Cout, Cin, H, W, k, stride, pad = case[:8]
    return (N, Cout, Cin, H, W, k, k, stride, pad, flags)


def wgrad_layouts(case):
    """Destination layouts a weight-gradient test runs a case in: standard, and kernel-position-major for k x k layers."""
    return (0, WG_KPOS) if case[5] > 1 else (0,)


def wgrad_key(info):
    """The ledger's key of a planned layer: (variant, slabs + reduce, staged 16-byte row epilogue)."""
    return (info["variant"], info["S"] > 1, info["rows"])


def wgrad_traits(case, info):
    N, Cout, Cin, H, W, k, stride, pad = case[:8]
    v = info["variant"]
    cin = Cin * k * k if v & 32 else Cin       # virtual channels: the tile's columns are (channel, tap) pairs
    t = set()
    if Cout % (64 if v & 1 else 128):
        t.add("ragged_cout")
    if cin % (64 if v & 2 else 128):
        t.add("ragged_cin")
    return t


def variant_name(v):
    s = "%dx%d" % (64 if v & 1 else 128, 64 if v & 2 else 128)
    s += " Xscalar" if v & 4 else " X16B"
    s += " Yvirtual" if v & 32 else (" Yshift16B" if v & 16 else (" Yshift" if v & 8 else " Ydirect"))
    return s + (" split" if v & 64 else "")


# ------------------------------------------------------------------------------------------------ the grid of the ledger
GRID = dict(Cout=(8, 64, 65, 200), Cin=(3, 15, 16, 32, 33, 64, 65, 130), HW=(1, 4, 7, 8, 14), k=(1, 3, 5, 7), stride=(1, 2),
            N=(2, 40))       # pad: 0, k // 2, k // 2 + 1;  N = 40 at 14 x 14: 7840 pixels, three slabs


def grid_geometries():
    """(Cout, Cin, H, W, k, stride, pad) of the sweep that says which forms a caller's geometry can reach."""
    for Cout in GRID["Cout"]:
        for Cin in GRID["Cin"]:
            for H in GRID["HW"]:
                for W in GRID["HW"]:
                    for k in GRID["k"]:
                        for stride in GRID["stride"]:
                            for pad in sorted({0, k // 2, k // 2 + 1}):
                                if H + 2 * pad >= k and W + 2 * pad >= k:
                                    yield (Cout, Cin, H, W, k, stride, pad)


def reachable_fwd():
    """{(form, kernel-position-major)} over the grid (the form does not depend on N or on the arithmetic's LDS sizes, but it is
    asked under the current one)."""
    seen = set()
    for (Cout, Cin, H, W, k, stride, pad) in grid_geometries():
        case = (2, Cout, Cin, H, W, k, stride, pad, False)
        for kp in fwd_layouts(case):
            seen.add((fwd_form(case, kp), kp))
    return seen


def wgrad_infos(geos, chunk=512):
    from pleas_merging_amd import hip_ops

    out = []
    for i in range(0, len(geos), chunk):
        out += hip_ops.WgradBatch.plan_info(geos[i:i + chunk])
    return out


def reachable_wgrad():
    """{(variant, S > 1, rows path)} over the grid, both destination layouts, under the current arithmetic."""
    geos = []
    for (Cout, Cin, H, W, k, stride, pad) in grid_geometries():
        for N in GRID["N"]:
            case = (N, Cout, Cin, H, W, k, stride, pad)
            geos += [wgrad_geo(case, fl) for fl in wgrad_layouts(case)]
    return {wgrad_key(i) for i in wgrad_infos(geos)}


# ------------------------------------------------------------------------------------------------ the random draw
RANDOM_SEED = 0          # chosen below the generator; tests/test_tile_coverage.py holds what its draw must reach
RANDOM_CASES = 30


def random_cases(seed=None, n=RANDOM_CASES):
    """General geometries of the property test: stride 1-3, pad 0..k, images down to smaller than the kernel (with padding),
    channel counts of every residue.  (N, Cout, Cin, H, W, k, stride, pad, bias); python's own generator, so that the draw
    is the same wherever it is made."""
    import random

    rng = random.Random(RANDOM_SEED if seed is None else seed)
    out = []
    while len(out) < n:
        k = rng.choice((1, 1, 2, 3, 3, 3, 5, 7))
        stride, pad = rng.randint(1, 3), rng.randint(0, k)
        H, W = rng.randint(1, 20), rng.randint(1, 20)
        if H + 2 * pad < k or W + 2 * pad < k:
            continue
        Cin = rng.choice((rng.randint(1, 15), rng.randint(16, 140), 4 * rng.randint(1, 35), 32 * rng.randint(1, 4)))
        Cout = rng.choice((rng.randint(1, 64), rng.randint(65, 200)))
        out.append((rng.randint(1, 6), Cout, Cin, H, W, k, stride, pad, rng.random() < 0.5))
    return out


# ------------------------------------------------------------------------------------------------ the schedule test's list
# One mixed-form grouped forward whose calibration launch makes the scheduler cut forms into slices: a flat 1 x 1 form with
# 392 short items (the filler: most items, cut into one slice per lane) and a flat 3 x 3 form with 196 longer ones (more than
# 64 items and more than 0.7 of a lane's fair share: equal slices) dominate two small forms.  The eight-launch test of
# tests/test_hip_tile_forms.py; SCHEDULE_MS are the durations per form its calibration launch measured on an MI355X.
SCHEDULE_CASES = [
    (16, 512, 256, 28, 28, 1, 1, 0, False),   # flat 1 x 1, 128 rows: 392 items
    (16, 256, 128, 28, 28, 3, 1, 1, True),    # flat 3 x 3 (kernel-position-major), 128 rows: 196 items
    (6, 136, 64, 7, 7, 1, 1, 0, False),       # flat 1 x 1 with scalar pixel loads
    (2, 64, 3, 32, 32, 7, 2, 3, True),        # stem-like: scalar weight loads, 64 rows
]
SCHEDULE_MS = (0.0, 0.0, 0.0, 0.0904, 0.1278, 0.0959, 0.1224, 0.0, 0.0, 0.0)      # exact arithmetic; split: 0.0611, 0.0816, 0.0752, 0.0858


def schedule_list():
    return [(c, kpos_legal(c)) for c in SCHEDULE_CASES]
