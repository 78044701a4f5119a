"""The geometries of the variant tests of the matching contraction (csrc/gram.hip) and of the normal equations
(csrc/normal_eq.hip), and the host-only queries that say which variant the library picks for one (plain data + small helpers;
no GPU, no tensors).  Shared by tests/test_contraction_coverage.py (the ledger: every reachable variant has a case with every
edge a tile can go wrong at) and tests/test_hip_contraction_forms.py (every case on the GPU, element by element).

Gram variants (build_batch_plan): 0 / 1 = 128-row tile with 16-byte / 4-byte loads, 2 / 3 = the same with 64 rows, 4 / 5 = 128 /
64 rows over the K axis padded to four pixels per group (HW % 4 != 0, HW >= 4).  Normal-equation variants (build_neq_plan):
bit 0 = 64-wide tiles, bit 1 = 4-byte loads, bits 2-3 = 0 direct (1 x 1, stride 1, no padding) / 1 shifted loader / 2 lag
classes (stride-1 "same" k x k): the values 0-3, 6-7, 8-11.

Every operand stays under 4 MB, every A under 8 MB; a size is the workload's only where the size is the point (W = 14 lag
shifts, HW = 49).  A comment after a case says what the case is FOR; the variant it takes today is what the ledger prints."""
import test_hip_kernels as hk

BK = 32                    # k per chunk (kBK)
ITEM_CHUNKS = 112          # chunks per slab under the default tuning: S > 1 above 3584 k

# ------------------------------------------------------------------------------------------------ matching contraction
GRAM_VARIANTS = (0, 1, 2, 3, 4, 5)
GRAM_CASES = [
    # (B, C, H, W), a derived node (eval-mode BatchNorm image) hangs on it
    # 128-row tile, 16-byte loads
    ((8, 72, 24, 24), True),       # K = 4608: two slabs, the source of a derived node: row sums over both
    ((3, 130, 6, 6), False),       # 2 x 2 tiles, ragged; HW = 36: chunks straddle samples, K = 108 ends inside a chunk
    ((3, 70, 2, 6), True),         # HW = 12 < 32: the division path of load_chunk; K = 36
    ((2, 96, 14, 14), False),      # of GRAM_SHAPES
    # 128-row tile, 4-byte loads: HW < 4 only
    ((1300, 70, 3, 1), True),      # K = 3900: two slabs, source of a derived node
    ((5, 130, 1, 1), False),       # 2 x 2 tiles at K = 5
    ((7, 70, 2, 1), True),         # HW = 2
    ((16, 300), False),            # of GRAM_SHAPES: flatten-like
    # 64-row tile, 16-byte loads
    ((8, 40, 24, 24), True),       # K = 4608: two slabs, source of a derived node
    ((3, 40, 6, 6), False),        # HW = 36
    ((3, 40, 2, 6), True),         # HW = 12
    ((4, 8, 6, 6), False),         # of GRAM_SHAPES: tiny C
    # 64-row tile, 4-byte loads
    ((1300, 40, 3, 1), True),      # K = 3900: two slabs
    ((5, 40, 1, 1), False),
    ((7, 24, 1, 2), True),
    # padded K axis, 128 rows
    ((6, 130, 25, 25), True),      # HWp = 628, B * HWp = 3768: two slabs, 2 x 2 tiles, source of a derived node
    ((3, 70, 1, 5), False),        # HW = 5, 6, 7: barely more than one group of four
    ((3, 70, 2, 3), True),
    ((3, 70, 1, 7), False),
    ((2, 70, 3, 3), False),        # HW = 9
    ((3, 70, 7, 7), True),         # HW = 49: the 7 x 7 maps, a sample ends inside a chunk
    ((5, 130, 9, 9), False),       # of GRAM_SHAPES: HW = 81
    # padded K axis, 64 rows
    ((6, 40, 25, 25), True),       # two slabs
    ((3, 40, 1, 5), True),
    ((3, 40, 2, 3), False),
    ((3, 40, 1, 7), False),
    ((2, 40, 3, 3), True),
    ((3, 20, 7, 7), False),        # of GRAM_SHAPES
]
assert all((s, 1) in hk.GRAM_SHAPES for s in [(2, 96, 14, 14), (16, 300), (4, 8, 6, 6), (5, 130, 9, 9), (3, 20, 7, 7)])
GRAM_LAUNCH = 8                    # cases per grouped launch
GRAM_TRAITS = ("ragged_c", "multi_tile", "slabs", "k_tail", "straddles_samples", "short_image", "source_sums", "source_sums_slabs")
PAD_HW = (5, 6, 7, 9, 49)          # the padded forms' image sizes
# (variant, trait) a variant cannot have, by name
GRAM_CANNOT = {(v, "multi_tile"): "a 64-row tile is chosen for C <= 64: one tile per side" for v in (2, 3, 5)}

# the single-node entry (pleas_gram_accum): (shape, one float off a 16-byte boundary)
GRAM_SINGLE_CASES = [
    ((3, 130, 6, 6), False),       # tile 128, 16-byte loads
    ((3, 130, 6, 6), True),        # the same shape from a view one float off: 4-byte loads at HW % 4 == 0
    ((3, 70, 7, 7), False),        # tile 128, 4-byte loads (HW = 49)
    ((3, 40, 6, 6), False),        # tile 64, 16-byte loads
    ((3, 40, 6, 6), True),         # tile 64, 4-byte loads at HW % 4 == 0
    ((7, 24, 1, 2), False),        # tile 64, 4-byte loads
    ((2, 40, 40, 40), False),      # K = 3200 through 50 split-K slabs
]


def bchw(shape):
    """(B, C, HW) of a shape contracted along axis 1."""
    hw = 1
    for s in shape[2:]:
        hw *= s
    return shape[0], shape[1], hw


def gram_launches():
    """The grouped launches of the table: lists of case indices, a stride through the table so that a launch mixes variants."""
    n = -(-len(GRAM_CASES) // GRAM_LAUNCH)
    return [list(range(i, len(GRAM_CASES), n)) for i in range(n)]


def gram_nodes(indices):
    """(nodes, group_C) of one launch: every case a contracted node, its derived node right behind the list of contracted
    ones; one group per channel count.  A node is (case index, B, C, HW, group, source)."""
    group_C, nodes = [], []
    for i in indices:
        B, C, HW = bchw(GRAM_CASES[i][0])
        if C not in group_C:
            group_C.append(C)
        nodes.append((i, B, C, HW, group_C.index(C), None))
    for pos, i in enumerate(indices):
        if GRAM_CASES[i][1]:
            _, B, C, HW, g, _ = nodes[pos]
            nodes.append((i, B, C, HW, g, pos))
    return nodes, group_C


def gram_infos(nodes, group_C):
    from pleas_merging_amd import hip_ops

    return hip_ops.GramBatch.plan_info([n[1:] for n in nodes], group_C)


def gram_traits(shape, derived, info):
    B, C, HW = bchw(shape)
    tile = 128 if info["variant"] in (0, 1, 4) else 64
    t = set()
    if C % tile:
        t.add("ragged_c")
    if tile == 128 and C > 128:
        t.add("multi_tile")
    if info["S"] > 1:
        t.add("slabs")
    if B * HW % BK:
        t.add("k_tail")
    if B > 1 and HW % BK:
        t.add("straddles_samples")
    if HW < BK:
        t.add("short_image")
    if derived:
        t.add("source_sums")
        if info["S"] > 1:
            t.add("source_sums_slabs")
    if info["variant"] >= 4:
        t.add("hw_%d" % HW)
    return t


GRAM_GRID = dict(C=(8, 40, 63, 64, 65, 72, 127, 128, 129, 200), HW=(1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 36, 49, 81, 196, 625),
                 B=(1, 7, 64, 1300))


def reachable_gram():
    """{(variant, S > 1)} over the grid, asked of the library."""
    from pleas_merging_amd import hip_ops

    geos = [(B, C, HW) for C in GRAM_GRID["C"] for HW in GRAM_GRID["HW"] for B in GRAM_GRID["B"] if B * C * HW * 4 < (256 << 20)]
    return {(i["variant"], i["S"] > 1) for i in hip_ops.GramBatch.plan_info(geos)}


# ------------------------------------------------------------------------------------------------ normal equations
NEQ_VARIANTS = (0, 1, 2, 3, 6, 7, 8, 9, 10, 11)
NEQ_CASES = [
    # N, Cin, H, W, KH, KW, stride, pad
    # direct (1 x 1, stride 1, no padding), 128-wide tiles, 16-byte loads
    (1, 130, 60, 60, 1, 1, 1, 0),      # 3600 pixels: two slabs; 2 x 2 block tiles, ragged, Cin % 4 != 0
    (3, 72, 6, 6, 1, 1, 1, 0),         # HWo = 36: chunks straddle samples, 108 pixels end inside a chunk
    (4, 200, 14, 14, 1, 1, 1, 0),      # of test_hip_kernels.NEQ_CASES
    # direct, 64-wide tiles, 16-byte loads
    (1, 40, 60, 60, 1, 1, 1, 0),       # two slabs
    (3, 30, 6, 6, 1, 1, 1, 0),         # Cin % 4 != 0: the scalar epilogue
    (4, 64, 14, 14, 1, 1, 1, 0),       # of NEQ_CASES: a full tile
    # direct, 128-wide tiles, 4-byte loads
    (1, 130, 61, 59, 1, 1, 1, 0),      # 3599 pixels: two slabs, 2 x 2 block tiles
    (3, 70, 7, 7, 1, 1, 1, 0),         # HW = 49
    # direct, 64-wide tiles, 4-byte loads
    (1, 40, 61, 59, 1, 1, 1, 0),       # two slabs
    (3, 30, 7, 7, 1, 1, 1, 0),
    (3, 40, 7, 7, 1, 1, 1, 0),         # of NEQ_CASES
    # shifted loader, 128-wide tiles
    (1, 66, 62, 62, 3, 3, 1, 0),       # 3 x 3 stride 1 pad 0 ("valid"), 3600 output pixels: two slabs
    (2, 130, 12, 12, 3, 3, 2, 1),      # of NEQ_CASES: 2 x 2 block tiles
    (3, 70, 9, 9, 1, 1, 2, 0),         # 1 x 1 stride 2: a ResNet's downsample convolution
    (2, 70, 9, 7, 3, 3, 2, 1),         # odd image: the last output column's right tap is the padding column
    (2, 70, 6, 7, 1, 3, 1, 1),         # KH != KW
    # shifted loader, 64-wide tiles
    (1, 24, 62, 62, 3, 3, 1, 0),       # two slabs
    (2, 24, 9, 9, 3, 3, 2, 1),         # of NEQ_CASES
    (3, 30, 9, 9, 1, 1, 2, 0),         # 1 x 1 stride 2
    (2, 3, 20, 20, 7, 7, 2, 3),        # the stem: 7 x 7 stride 2 pad 3, Cin = 3
    (2, 24, 6, 7, 1, 3, 1, 1),         # KH != KW
    (2, 30, 7, 7, 3, 3, 1, 0),         # 3 x 3 stride 1 pad 0, Cin % 4 != 0
    # lag classes, 128-wide tiles, 16-byte loads
    (1, 72, 60, 60, 3, 3, 1, 1),       # 3600 pixels: two slabs
    (3, 130, 6, 10, 3, 3, 1, 1),       # 2 x 2 block tiles, ragged, H != W, Cin % 4 != 0
    (2, 70, 2, 2, 3, 3, 1, 1),         # image smaller than the kernel
    (2, 72, 14, 14, 3, 3, 1, 1),       # W = 14: lag shifts 0..3 of the 16-byte runs
    # lag classes, 64-wide tiles, 16-byte loads
    (1, 24, 60, 60, 3, 3, 1, 1),       # two slabs
    (4, 48, 10, 10, 3, 3, 1, 1),       # of NEQ_CASES
    (3, 30, 6, 10, 3, 3, 1, 1),        # H != W, Cin % 4 != 0
    (2, 20, 2, 2, 3, 3, 1, 1),         # image smaller than the kernel
    (5, 24, 8, 8, 5, 5, 1, 2),         # of NEQ_CASES: 5 x 5
    # lag classes, 128-wide tiles, 4-byte loads
    (3, 72, 35, 35, 3, 3, 1, 1),       # 3675 pixels: two slabs
    (3, 130, 5, 7, 3, 3, 1, 1),        # 2 x 2 block tiles, H != W
    (2, 70, 2, 3, 3, 3, 1, 1),         # image smaller than the kernel
    # lag classes, 64-wide tiles, 4-byte loads
    (3, 24, 35, 35, 3, 3, 1, 1),       # two slabs
    (3, 30, 5, 7, 3, 3, 1, 1),         # H != W, Cin % 4 != 0
    (2, 20, 2, 3, 3, 3, 1, 1),         # of NEQ_CASES: image smaller than the kernel
    (3, 24, 7, 7, 5, 5, 1, 2),         # 5 x 5 at HW = 49
]
_old = [c[:4] + (c[4], c[4]) + c[5:] for c in hk.NEQ_CASES]
assert sum(c in _old for c in NEQ_CASES) == 8
NEQ_LAUNCH = 8
NEQ_TRAITS = ("ragged_cin", "multi_tile", "slabs", "k_tail", "straddles_samples", "cin_mod4")
NEQ_LAG_TRAITS = ("h_ne_w", "small_image", "k5")
NEQ_SHIFT_TRAITS = ("k1_s2_p0", "k3_s1_p0", "kh_ne_kw")          # + "stem" where Cin = 3 can be: 64-wide tiles
NEQ_CANNOT = {(v, "multi_tile"): "64-wide tiles are chosen for Cin <= 64: one tile per side" for v in (1, 3, 7, 9, 11)}
NEQ_CANNOT.update({(v, "k5"): "5 x 5 at Cin > 64 has K >= 1625: A over the 8 MB this table allows" for v in (8, 10)})
NEQ_CANNOT[(6, "stem")] = "Cin = 3 takes 64-wide tiles"


def neq_out(case):
    N, Cin, H, W, KH, KW, stride, pad = case
    return (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1


def neq_launches():
    n = -(-len(NEQ_CASES) // NEQ_LAUNCH)
    return [list(range(i, len(NEQ_CASES), n)) for i in range(n)]


def neq_infos(cases):
    from pleas_merging_amd import hip_ops

    return hip_ops.NormalEqBatch.layer_info(cases)


def neq_traits(case, info):
    N, Cin, H, W, KH, KW, stride, pad = case
    Ho, Wo = neq_out(case)
    T = 64 if info["variant"] & 1 else 128
    t = set()
    if Cin % T:
        t.add("ragged_cin")
    if T == 128 and Cin > 128:
        t.add("multi_tile")
    if info["S"] > 1:
        t.add("slabs")
    if N * Ho * Wo % BK:
        t.add("k_tail")
    if N > 1 and Ho * Wo % BK:
        t.add("straddles_samples")
    if Cin % 4:
        t.add("cin_mod4")
    if H != W:
        t.add("h_ne_w")
    if H < KH or W < KW:
        t.add("small_image")
    if (KH, KW) == (5, 5):
        t.add("k5")
    if (KH, KW, stride, pad) == (1, 1, 2, 0):
        t.add("k1_s2_p0")
    if (KH, KW, stride, pad) == (3, 3, 1, 0):
        t.add("k3_s1_p0")
    if (KH, KW, stride, pad, Cin) == (7, 7, 2, 3, 3):
        t.add("stem")
    if KH != KW:
        t.add("kh_ne_kw")
    return t


NEQ_GRID = dict(Cin=(3, 24, 63, 64, 65, 72, 128, 129), HW=((1, 1), (2, 3), (6, 6), (7, 7), (9, 7), (14, 14), (35, 35), (62, 62)),
                N=(1, 3, 8), k=(1, 3, 5, 7), stride=(1, 2))


def reachable_neq():
    """{(variant, S > 1)} over the grid: stride 1 and 2, pad equal and not equal to (k - 1) / 2, k in 1, 3, 5, 7."""
    geos = []
    for Cin in NEQ_GRID["Cin"]:
        for H, W in NEQ_GRID["HW"]:
            for N in NEQ_GRID["N"]:
                for k in NEQ_GRID["k"]:
                    for stride in NEQ_GRID["stride"]:
                        for pad in sorted({(k - 1) // 2, 0, (k - 1) // 2 + 1}):
                            if H + 2 * pad >= k and W + 2 * pad >= k:
                                geos.append((N, Cin, H, W, k, k, stride, pad))
    return {(i["variant"], i["S"] > 1) for i in neq_infos(geos)}
