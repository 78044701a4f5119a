"""Case tables of the streaming kernels (csrc/elementwise.hip, csrc/bn_train.hip, target_residual / loss_final in csrc/conv.hip):
one table per kernel, shared by the coverage ledger (tests/test_stream_coverage.py, no GPU) and the GPU file
(tests/test_hip_stream_paths.py).

Which path a case takes -- floats per load ``vec``, kernel ``form``, workgroups, sweeps of the grid-stride loop -- is ASKED of
the built library (``hip_ops.stream_plan_info``, the function the launchers themselves compute their grid with), never
re-derived here.  A case is a dict; ``off`` names the operands that are a contiguous view one float past an aligned
allocation.  ``traits(kernel, case)`` turns a case and the library's answer into the set of trait names the ledger counts.

General traits, per path: ``one_sweep`` / ``wrapped`` (sweeps >= 2 and a ragged last sweep: the work is neither a multiple of
what one pass of the grid covers nor of what one workgroup covers), ``vec`` / ``scalar_by_size`` (inner % 4 != 0) /
``scalar_by_alignment`` (inner % 4 == 0, an operand one float off).  channel_sum and bn_train_fold have no grid-stride loop:
their ``wrapped`` is a thread's inner loop that runs more than once with a ragged last trip."""
import math

MAX_TENSOR_BYTES = 64 << 20
MAX_WRAPPED = 3


def case(**kw):
    kw.setdefault("off", ())
    return kw


# ------------------------------------------------------------------------------------------------ merge_blocks
# shape: the sources; axis: the row axis; rows: rows of the output; merged: n_merged_rows; cols: output columns (axis + 1 is
# merged too) or None; absent: which map entries are -1 -- "r1" / "r2": rows absent in source 1 / 2 only, "cross": an absent row
# of one source crossed with an absent column of the same and of the other source
MERGE_BLOCKS = [
    case(shape=(12, 10, 3, 3), axis=0, rows=14, merged=5, cols=11, absent=("r1", "r2", "cross")),      # the old test's weight
    case(shape=(12, 10, 2, 2), axis=0, rows=14, merged=5, cols=11, absent=("r1", "r2", "cross")),      # 2 x 2 kernel: 16-byte
    case(shape=(3, 9, 6, 8), axis=1, rows=11, merged=4, cols=7, absent=("r1", "r2", "cross")),         # activation, two axes
    case(shape=(3, 9, 6, 5), axis=1, rows=11, merged=4, cols=7, absent=("r1", "r2", "cross")),
    case(shape=(2, 6, 8), axis=1, rows=7, merged=0, cols=None, absent=("r1", "r2")),
    case(shape=(2, 6, 8), axis=1, rows=7, merged=7, cols=None, absent=()),
    case(shape=(2, 6, 5), axis=1, rows=7, merged=0, cols=None, absent=("r1", "r2")),
    case(shape=(2, 6, 5), axis=1, rows=7, merged=7, cols=None, absent=()),
    case(shape=(4, 16, 8), axis=1, rows=20, merged=6, cols=None, absent=("r1", "r2"), off=("w1",)),
    case(shape=(4, 16, 8), axis=1, rows=20, merged=6, cols=None, absent=("r1", "r2"), off=("w2",)),
    case(shape=(4, 6, 5, 4), axis=1, rows=8, merged=3, cols=6, absent=("r1", "r2", "cross"), off=("out",)),
    case(shape=(5, 100, 3204), axis=1, rows=131, merged=40, cols=None, absent=("r1", "r2")),           # wrapped, 16-byte
    case(shape=(3, 50, 3499), axis=1, rows=50, merged=20, cols=None, absent=("r1", "r2")),             # wrapped, scalar
]


def merge_geo(c):
    shape, a = c["shape"], c["axis"]
    outer, rows_src = math.prod(shape[:a]), shape[a]
    if c["cols"] is None:
        return outer, c["rows"], 1, math.prod(shape[a + 1:]), rows_src, 1, 0
    return outer, c["rows"], c["cols"], math.prod(shape[a + 2:]), rows_src, shape[a + 1], 1


def _merge(c):
    g = merge_geo(c)
    t = {"colmaps"} if c["cols"] is not None else set()
    if c["cols"] is not None and g[0] > 1:
        t.add("outer_colmaps")
    t |= {"absent_" + a for a in c["absent"]}
    if c["merged"] == 0:
        t.add("merged_none")
    if c["merged"] == c["rows"]:
        t.add("merged_all")
    out_shape = c["shape"][:c["axis"]] + (c["rows"],) + ((c["cols"],) if c["cols"] is not None else ()) \
        + c["shape"][c["axis"] + (1 if c["cols"] is None else 2):]
    return g, g[3], g[0] * g[1] * g[2] * g[3], t, [c["shape"], out_shape]


# ------------------------------------------------------------------------------------------------ bn_act (three entry points)
# entry: "bn_act" (pleas_bn_act), "tracked" (pleas_bn_act_tracked), "batches" (pleas_bn_act_tracked_batches);
# combos: (res, relu, y_bn, y_sum) tuples to launch; plant: the operand that gets NaN and +-inf
BN_COMBOS_TRACKED = [(0, 0, 0, 0), (0, 1, 1, 0), (1, 0, 1, 0), (1, 1, 1, 1), (0, 1, 0, 0), (1, 0, 0, 0), (1, 1, 0, 1)]   # keep_bn or not
BN_COMBOS_PLAIN = [(0, 0, 0, 0), (0, 1, 0, 0), (1, 0, 0, 0), (1, 1, 0, 0)]
BN_COMBOS = sorted(set(BN_COMBOS_TRACKED + BN_COMBOS_PLAIN))
FULL = [(1, 1, 1, 1)]
BN_ACT = [
    case(entry="bn_act", shape=(6, 5, 4, 4), batches=1, combos=BN_COMBOS_PLAIN),
    case(entry="bn_act", shape=(6, 7, 3, 3), batches=1, combos=BN_COMBOS_PLAIN),
    case(entry="tracked", shape=(6, 5, 4, 4), batches=1, combos=BN_COMBOS),
    case(entry="tracked", shape=(6, 7, 3, 3), batches=1, combos=BN_COMBOS),
    case(entry="batches", shape=(6, 5, 4, 4), batches=2, combos=BN_COMBOS),       # 60 pieces a batch: the boundary is inside a workgroup
    case(entry="batches", shape=(6, 5, 4, 4), batches=3, combos=FULL),
    case(entry="batches", shape=(6, 7, 3, 3), batches=2, combos=BN_COMBOS),
    case(entry="batches", shape=(6, 7, 3, 3), batches=3, combos=FULL),
    case(entry="tracked", shape=(3, 16, 8, 8), batches=1, combos=FULL, off=("x",)),
    case(entry="tracked", shape=(3, 16, 8, 8), batches=1, combos=FULL, off=("res",)),
    case(entry="tracked", shape=(3, 16, 8, 8), batches=1, combos=FULL, off=("y_bn",)),
    case(entry="batches", shape=(4, 16, 8, 8), batches=2, combos=FULL, off=("y_sum",)),
    case(entry="bn_act", shape=(3, 16, 8, 8), batches=1, combos=[(1, 1, 0, 0)], off=("y",)),
    case(entry="tracked", shape=(2, 5, 4, 4), batches=1, combos=BN_COMBOS, plant="x"),
    case(entry="tracked", shape=(2, 5, 4, 4), batches=1, combos=[c for c in BN_COMBOS if c[0]], plant="res"),
    case(entry="bn_act", shape=(2, 7, 3, 3), batches=1, combos=BN_COMBOS_PLAIN, plant="x"),
    case(entry="bn_act", shape=(2, 7, 3, 3), batches=1, combos=[(1, 0, 0, 0), (1, 1, 0, 0)], plant="res"),
    case(entry="batches", shape=(6, 37, 98, 98), batches=3, combos=FULL),         # wrapped, 16-byte: sweep 2 starts inside batch 3
    case(entry="batches", shape=(4, 13, 101, 101), batches=2, combos=FULL),       # wrapped, scalar
]


def bn_act_geo(c):
    n, C = c["shape"][:2]
    return n, C, math.prod(c["shape"][2:]), (n // c["batches"] if c["batches"] > 1 else 0)


def _bn_act(c):
    g = bn_act_geo(c)
    t = {"combo_%d%d%d%d" % k for k in c["combos"]} | {"batches_%d" % c["batches"], "entry_" + c["entry"]}
    if c.get("plant"):
        t.add("plant_" + c["plant"])
    return g, g[2], g[0] * g[1] * g[2], t, [c["shape"]]


# ------------------------------------------------------------------------------------------------ bn_act_maxpool
BN_ACT_MAXPOOL = [
    case(shape=(2, 5, 8, 8), k=3, stride=2, pad=1, relu=True, scale=True),        # stem, W = 8: q is 0 everywhere
    case(shape=(2, 3, 9, 16), k=3, stride=2, pad=1, relu=True, scale=True),       # stem, H odd, W = 16
    case(shape=(1, 4, 1, 8), k=3, stride=2, pad=1, relu=False, scale=True),
    case(shape=(1, 4, 2, 16), k=3, stride=2, pad=1, relu=True, scale=True),
    case(shape=(3, 4, 6, 24), k=3, stride=2, pad=1, relu=False, scale=False),     # plain pooling through the stem form
    case(shape=(2, 5, 7, 16), k=3, stride=2, pad=1, relu=True, scale=True, plant="x"),
    case(shape=(2, 5, 7, 16), k=3, stride=2, pad=1, relu=False, scale=True, plant="x"),
    case(shape=(9, 57, 130, 128), k=3, stride=2, pad=1, relu=True, scale=True),   # wrapped, stem: a 34 MB input
    case(shape=(2, 7, 9, 11), k=3, stride=2, pad=1, relu=True, scale=True),       # general: W % 8 != 0
    case(shape=(3, 16, 16, 16), k=3, stride=2, pad=1, relu=True, scale=True, off=("x",)),      # the stem's geometry, x one float off
    case(shape=(3, 16, 16, 16), k=3, stride=2, pad=1, relu=True, scale=True, off=("y",)),
    case(shape=(2, 3, 7, 7), k=2, stride=2, pad=0, relu=False, scale=True),
    case(shape=(2, 3, 6, 9), k=3, stride=1, pad=1, relu=True, scale=False),
    case(shape=(1, 4, 1, 9), k=3, stride=2, pad=1, relu=True, scale=True),
    case(shape=(1, 4, 2, 9), k=3, stride=2, pad=1, relu=False, scale=True),
    case(shape=(2, 5, 7, 9), k=3, stride=2, pad=1, relu=True, scale=True, plant="x"),
    case(shape=(2, 5, 7, 9), k=3, stride=2, pad=1, relu=False, scale=True, plant="x"),
    case(shape=(3, 11, 253, 251), k=3, stride=2, pad=1, relu=True, scale=True),   # wrapped, general
]


def pool_out(c):
    N, C, H, W = c["shape"]
    return N, C, (H + 2 * c["pad"] - c["k"]) // c["stride"] + 1, (W + 2 * c["pad"] - c["k"]) // c["stride"] + 1


def _maxpool(c):
    N, C, H, W = c["shape"]
    g = (N, C, H, W, c["k"], c["k"], c["stride"], c["pad"])
    t = {"relu" if c["relu"] else "no_relu", "scale" if c["scale"] else "no_scale"}
    stem_geo = (c["k"], c["stride"], c["pad"]) == (3, 2, 1) and W % 8 == 0
    if stem_geo:
        t |= {"W_%d" % W} if W in (8, 16) and not c["off"] else set()
        t |= {"stem_geometry_%s_off" % o for o in c["off"]}
    else:
        t.add("W_not_8")
    if stem_geo or W % 8:
        t |= {"H_odd"} if H % 2 and H > 1 else set()
    t |= {"H_%d" % H} if H in (1, 2) else set()
    if c.get("plant"):
        t.add("plant_" + c["plant"])
    return g, 4, math.prod(pool_out(c)), t, [c["shape"], pool_out(c)]      # inner: the predicate has no size half of this kind


# ------------------------------------------------------------------------------------------------ masked_adam
# mask: None, "01" (0 / 1 entries); view: p, g and the mask are views at an odd offset of larger buffers, m and v dense;
# steps: the step numbers run in turn (gradients span 1e-6 .. 1 from step to step)
BIG_STEP = 100000          # 1 - 0.999^step rounds to 1 in fp32 from step 17329 on
MASKED_ADAM = [
    case(n=1000, mask="01", view=False, steps=tuple(range(1, 12))),               # the project's criterion: 11 steps
    case(n=1000, mask=None, view=False, steps=tuple(range(1, 12))),
    case(n=1001, mask="01", view=True, steps=(1, 2, 3)),
    case(n=777, mask=None, view=True, steps=(1,)),
    case(n=513, mask="01", view=False, steps=(BIG_STEP,)),
    case(n=524621, mask="01", view=False, steps=(7,)),                            # wrapped
]


def _adam(c):
    t = {"mask_none" if c["mask"] is None else "mask_01"}
    if c["view"]:
        t.add("views")
    if 1 in c["steps"]:
        t.add("step_1")
    if max(c["steps"]) >= 17329:
        t.add("step_big")
    if len(c["steps"]) >= 11:
        t.add("grad_span")
    return (c["n"],), 1, c["n"], t, [(c["n"],)]


# ------------------------------------------------------------------------------------------------ sqerr
SQERR = [
    case(n=1, diff=True, accumulate=False),
    case(n=37, diff=False, accumulate=True),
    case(n=1000, diff=True, accumulate=True),
    case(n=100003, diff=False, accumulate=False),
    case(n=266465, diff=True, accumulate=True),                                   # wrapped: 1024 workgroups, two sweeps
]


def _sqerr(c):
    t = {"diff" if c["diff"] else "no_diff", "accumulate" if c["accumulate"] else "overwrite"}
    if c["n"] == 1:
        t.add("n_1")
    if c["n"] < 64:
        t.add("n_lt_64")
    return (c["n"],), 1, c["n"], t, [(c["n"],)]


# ------------------------------------------------------------------------------------------------ target_residual
# N, C (rows of the merged output), Csrc (channels of each source output), HW; inplace: resid is out
TARGET_RESIDUAL = [
    case(N=3, C=9, Csrc=8, HW=25, inplace=True),
    case(N=2, C=6, Csrc=5, HW=16, inplace=False),                                 # one partial
    case(N=2, C=6, Csrc=5, HW=16, inplace=True),
    case(N=1, C=3, Csrc=3, HW=7, inplace=False),                                  # one partial, scalar
    case(N=4, C=33, Csrc=24, HW=512, inplace=True),                               # 66 partials
    case(N=3, C=23, Csrc=20, HW=255, inplace=False),                              # 69 partials, scalar
    case(N=2, C=6, Csrc=5, HW=16, inplace=True, off=("out",)),
    case(N=2, C=6, Csrc=5, HW=16, inplace=False, off=("o1",)),
    case(N=2, C=6, Csrc=5, HW=16, inplace=False, off=("o2",)),
    case(N=2, C=6, Csrc=5, HW=16, inplace=False, off=("resid",)),
    case(N=5, C=131, Csrc=100, HW=3204, inplace=True),                            # wrapped, 16-byte: every partial is written
    case(N=3, C=50, Csrc=40, HW=3499, inplace=False),                             # wrapped, scalar
]


def _target(c):
    t = {"inplace" if c["inplace"] else "separate"}
    if c["Csrc"] != c["C"]:
        t.add("csrc_ne_c")
    return (c["N"], c["C"], c["Csrc"], c["HW"]), c["HW"], c["N"] * c["C"] * c["HW"], t, [(c["N"], max(c["C"], c["Csrc"]), c["HW"])]


# ------------------------------------------------------------------------------------------------ channel_sum
CHANNEL_SUM = [
    case(shape=(4, 1, 6)), case(shape=(4, 1, 8)), case(shape=(1, 5, 8)), case(shape=(1, 5, 9)), case(shape=(7, 3)),
    case(shape=(3, 4, 4, 4)), case(shape=(3, 4, 4, 4), off=("x",)),
    case(shape=(2, 3, 5200)),                                                     # 1300 16-byte pieces: six trips, the last ragged
    case(shape=(2, 3, 1031)),                                                     # five trips, scalar
]


def _chansum(c):
    N, C = c["shape"][:2]
    HW = math.prod(c["shape"][2:])
    t = set()
    if C == 1:
        t.add("C_1")
    if N == 1:
        t.add("N_1")
    if len(c["shape"]) == 2:
        t.add("HW_1")
    return (N, C, HW), HW, HW, t, [c["shape"]]


# ------------------------------------------------------------------------------------------------ pool_gather
# K: entries of the channel map, None: no map
POOL_GATHER = [
    case(N=5, C=7, HW=1, K=None), case(N=5, C=7, HW=1, K=4), case(N=5, C=7, HW=1, K=12),
    case(N=3, C=6, HW=49, K=None), case(N=3, C=6, HW=49, K=9),
    case(N=3, C=6, HW=16, K=None), case(N=3, C=6, HW=16, K=4), case(N=3, C=6, HW=16, K=11),
    case(N=2, C=5, HW=196, K=None), case(N=2, C=5, HW=196, K=3, off=("x",)), case(N=2, C=5, HW=197, K=8),
    case(N=2, C=3, HW=1024, K=5),
    case(N=4194309, C=1, HW=1, K=None),                                           # wrapped, scalar: evaluation.py's shape
    case(N=838861, C=2, HW=4, K=5),                                               # wrapped, 16-byte: 4 194 305 rows
]


def _pool_gather(c):
    K = c["K"] if c["K"] is not None else c["C"]
    t = {"map" if c["K"] is not None else "no_map"}
    if c["K"] is not None:
        t |= {"K_lt_C"} if K < c["C"] else ({"K_gt_C"} if K > c["C"] else set())
    HW = c["HW"]
    t |= {"HW_1"} if HW == 1 else set()
    t |= {"HW_lt_64"} if 1 < HW < 64 and HW % 4 else set()
    t |= {"HW4_lt_64"} if HW % 4 == 0 and HW // 4 < 64 else set()
    t |= {"HW_196"} if HW == 196 else set()
    t |= {"lane_loop"} if HW // (4 if HW % 4 == 0 and not c["off"] else 1) > 64 else set()
    return (c["N"], c["C"], HW, K, int(c["K"] is not None)), HW, c["N"] * K, t, [(c["N"], c["C"], HW), (c["N"], K)]


# ------------------------------------------------------------------------------------------------ top1_count
# labels: "right" (every label is the argmax), "wrong" (none is), "mixed"; rows with ties at both ends and a NaN before and
# after the maximum are planted in every case with C >= 3 (stream_ref.top1_inputs)
TOP1_COUNT = [
    case(N=9, C=1, labels="right", pred=True), case(N=37, C=37, labels="mixed", pred=True),
    case(N=37, C=64, labels="wrong", pred=False), case(N=37, C=65, labels="right", pred=True),
    case(N=21, C=1000, labels="mixed", pred=False),
    case(N=8195, C=10, labels="mixed", pred=True),                                # wrapped: 2048 workgroups of four rows, then three
]


def _top1(c):
    C = c["C"]
    t = {"labels_" + c["labels"], "pred" if c["pred"] else "no_pred"}
    t |= {"C_1"} if C == 1 else set()
    t |= {"C_lt_64"} if 1 < C < 64 else set()
    t |= {"C_%d" % C} if C in (64, 65) else set()
    t |= {"ties", "nan"} if C >= 3 else set()
    return (c["N"], C), 1, c["N"], t, [(c["N"], C)]


# ------------------------------------------------------------------------------------------------ bn_train_fold(_batches)
# shape: all batches back to back along dim 0; momentum None: the cumulative average, from `counter` batches already seen
BN_TRAIN_FOLD = [
    case(shape=(6, 5, 4, 4), batches=1, affine=True, track=True, momentum=0.1),
    case(shape=(6, 5, 3, 3), batches=1, affine=False, track=True, momentum=None),
    case(shape=(6, 5, 4, 4), batches=1, affine=False, track=False, momentum=0.1),
    case(shape=(6, 5, 3, 3), batches=1, affine=True, track=False, momentum=0.1),
    case(shape=(6, 5, 4, 4), batches=2, affine=True, track=True, momentum=None, counter=3),
    case(shape=(6, 5, 3, 3), batches=3, affine=True, track=True, momentum=None, counter=3),
    case(shape=(6, 5, 4, 4), batches=1, affine=True, track=True, momentum=None),
    case(shape=(6, 5, 3, 3), batches=1, affine=True, track=True, momentum=0.1),
    case(shape=(3, 1024, 2, 2), batches=1, affine=True, track=True, momentum=0.1),         # S = 1
    case(shape=(3, 1030, 1, 3), batches=1, affine=True, track=True, momentum=0.1),
    case(shape=(7, 300, 2, 2), batches=1, affine=True, track=True, momentum=0.1),          # S = 4, seven samples
    case(shape=(7, 300, 3, 3), batches=1, affine=True, track=True, momentum=0.1),
    case(shape=(6, 600, 2, 2), batches=2, affine=True, track=True, momentum=0.1),          # 1200 (batch, channel) pairs
    case(shape=(9, 400, 1, 3), batches=3, affine=True, track=True, momentum=None),
    case(shape=(6, 5, 4, 4), batches=1, affine=True, track=True, momentum=0.1, off=("x",)),
    case(shape=(8, 6, 8, 8), batches=1, affine=True, track=True, momentum=0.1, mean=1e3),
    case(shape=(8, 6, 7, 9), batches=2, affine=True, track=True, momentum=0.1, mean=1e3),
    case(shape=(3, 8, 36, 36), batches=1, affine=True, track=True, momentum=0.1),          # 324 pieces a slab: two trips
    case(shape=(3, 8, 17, 17), batches=1, affine=True, track=True, momentum=0.1),
    case(shape=(300, 4, 2, 2), batches=1, affine=True, track=True, momentum=0.1),          # S = 256 < N
    case(shape=(300, 4, 1, 3), batches=1, affine=True, track=True, momentum=0.1),
]


def bn_train_geo(c):
    return c["shape"][0] // c["batches"], c["batches"], c["shape"][1], math.prod(c["shape"][2:])


def _bn_train(c):
    g = bn_train_geo(c)
    t = {"affine" if c["affine"] else "no_affine", "track" if c["track"] else "no_track", "batches_%d" % min(c["batches"], 2)}
    if c["track"]:
        t.add("momentum_0.1" if c["momentum"] is not None else ("momentum_none_seen" if c.get("counter") else "momentum_none"))
    if c["batches"] >= 2 and c["batches"] * g[2] > 1024:
        t.add("pairs_gt_1024")
    if c.get("mean"):
        t.add("large_mean")
    return g, g[3], g[3], t, [c["shape"]]


# ------------------------------------------------------------------------------------------------ the ledger's view
KERNELS = {
    "merge_blocks": (MERGE_BLOCKS, _merge), "bn_act": (BN_ACT, _bn_act), "bn_act_maxpool": (BN_ACT_MAXPOOL, _maxpool),
    "masked_adam": (MASKED_ADAM, _adam), "sqerr": (SQERR, _sqerr), "target_residual": (TARGET_RESIDUAL, _target),
    "channel_sum": (CHANNEL_SUM, _chansum), "pool_gather": (POOL_GATHER, _pool_gather), "top1_count": (TOP1_COUNT, _top1),
    "bn_train_fold": (BN_TRAIN_FOLD, _bn_train),
}
# the operands of each launch's 16-byte predicate: each must be the misaligned one at least once across its table
PREDICATE_OPERANDS = {
    "merge_blocks": ("w1", "w2", "out"), "bn_act": ("x", "res", "y_bn", "y_sum", "y"), "bn_act_maxpool": ("x", "y"),
    "target_residual": ("out", "o1", "o2", "resid"), "channel_sum": ("x",), "pool_gather": ("x",), "bn_train_fold": ("x",),
    "masked_adam": (), "sqerr": (), "top1_count": (),
}
WIDTH_TRAITS = ("vec", "scalar_by_size", "scalar_by_alignment")
PER_KERNEL_TRAITS = {
    "merge_blocks": ("colmaps", "outer_colmaps", "absent_r1", "absent_r2", "absent_cross", "merged_none", "merged_all"),
    "bn_act": tuple("combo_%d%d%d%d" % k for k in BN_COMBOS) + ("batches_1", "batches_2", "batches_3", "boundary_in_workgroup",
                                                                 "batches_wrapped", "plant_x", "plant_res", "entry_bn_act",
                                                                 "entry_tracked", "entry_batches"),
    "bn_act_maxpool": ("W_8", "W_16", "H_odd", "H_1", "H_2", "W_not_8", "stem_geometry_x_off", "stem_geometry_y_off", "no_scale",
                       "scale", "relu", "no_relu", "plant_x"),
    "masked_adam": ("mask_none", "mask_01", "views", "step_1", "step_big", "grad_span"),
    "sqerr": ("diff", "no_diff", "accumulate", "overwrite", "n_1", "n_lt_64"),
    "target_residual": ("inplace", "separate", "partials_1", "partials_ge_65", "partials_max", "csrc_ne_c"),
    "channel_sum": ("C_1", "N_1", "HW_1"),
    "pool_gather": ("map", "no_map", "K_lt_C", "K_gt_C", "HW_1", "HW_lt_64", "HW4_lt_64", "HW_196", "lane_loop"),
    "top1_count": ("C_1", "C_lt_64", "C_64", "C_65", "ties", "nan", "labels_right", "labels_wrong", "labels_mixed", "pred", "no_pred"),
    "bn_train_fold": ("affine", "no_affine", "track", "no_track", "momentum_0.1", "momentum_none", "momentum_none_seen", "S_1",
                      "S_gt_1_ragged", "N_gt_S", "batches_1", "batches_2", "pairs_gt_1024", "large_mean"),
}
# (kernel, path, trait) -> why no case can have it.  A path is (form, vec).
SCALAR, VEC, STEM = ("", 1), ("", 4), ("stem", 4)
GENERAL = ("general", 1)
CANNOT = {}
for _k in ("masked_adam", "sqerr", "top1_count"):
    for _t in WIDTH_TRAITS:
        CANNOT[(_k, SCALAR, _t)] = "the kernel has one width and no 16-byte predicate: nothing selects a path"
for _k in ("merge_blocks", "bn_act", "target_residual", "channel_sum", "pool_gather", "bn_train_fold"):
    CANNOT[(_k, VEC, "scalar_by_size")] = CANNOT[(_k, VEC, "scalar_by_alignment")] = "a scalar trait on the 16-byte path"
    CANNOT[(_k, SCALAR, "vec")] = "the 16-byte trait on the scalar path"
for _t in WIDTH_TRAITS:
    CANNOT[("bn_act_maxpool", STEM, _t)] = CANNOT[("bn_act_maxpool", GENERAL, _t)] = \
        "the two pooling kernels are told apart by form; the general one is scalar at every size, the stem one never is"
for _t in ("W_not_8", "stem_geometry_x_off", "stem_geometry_y_off"):
    CANNOT[("bn_act_maxpool", STEM, _t)] = "the stem form needs W % 8 == 0 and 16-byte aligned x and y"
for _t in ("W_8", "W_16"):
    CANNOT[("bn_act_maxpool", GENERAL, _t)] = "W = 8 / 16 at 3 x 3 / 2 / 1 is the stem form unless misaligned (stem_geometry_*_off)"
CANNOT[("channel_sum", VEC, "HW_1")] = CANNOT[("pool_gather", VEC, "HW_1")] = "HW = 1 is not a multiple of 4"
CANNOT[("pool_gather", VEC, "HW_lt_64")] = "counted on HW % 4 != 0 (HW4_lt_64 is its 16-byte twin)"


def seed(kernel, i):
    """The seed of case i of a table (masked_adam: stream_ref.ADAM_SEED + i, what its measured constant was taken on)."""
    return 500 + i if kernel == "masked_adam" else 1000 * (list(KERNELS).index(kernel) + 1) + i


def reachable(kernel):
    """The paths the query returns over a small grid: every case's geometry and its neighbour one float longer, aligned or not."""
    from pleas_merging_amd import hip_ops

    inner_at = {"merge_blocks": 3, "bn_act": 2, "bn_act_maxpool": 3, "target_residual": 3, "channel_sum": 2, "pool_gather": 2,
                "bn_train_fold": 3}
    seen = set()
    for c in KERNELS[kernel][0]:
        geo = list(KERNELS[kernel][1](c)[0])
        for bump in (0, 1):
            if bump and kernel not in inner_at:
                continue
            g = list(geo)
            if bump:
                g[inner_at[kernel]] += 1
            for aligned in (True, False):
                seen.add(path(hip_ops.stream_plan_info(kernel, *g, aligned=aligned)))
    return seen


def plan(kernel, c):
    """(info, geo) of a case from the library: ``aligned`` is False when any operand of the case is one float off."""
    from pleas_merging_amd import hip_ops

    geo = KERNELS[kernel][1](c)[0]
    return hip_ops.stream_plan_info(kernel, *geo, aligned=not c["off"]), geo


def path(info):
    return (info.get("form", ""), info["vec"])


def tensors(kernel, c):
    """Shapes of the case's large tensors (for the size cap)."""
    return KERNELS[kernel][1](c)[4]


def traits(kernel, c):
    info, geo = plan(kernel, c)
    _, inner, total, t, _ = KERNELS[kernel][1](c)
    t = set(t)
    per_block = info["threads"] // (64 if kernel in ("pool_gather", "top1_count") else 1)
    if kernel in ("channel_sum", "bn_train_fold"):
        work, per_block = inner // info["vec"], info["threads"]           # one slab against one workgroup's threads
        ragged = work % per_block != 0
    else:
        work = total if per_block != info["threads"] else total // info["vec"]      # a wave per row: the rows are the work
        ragged = work % per_block != 0 and work % (per_block * info["blocks"]) != 0
    if info["sweeps"] == 1:
        t.add("one_sweep")
    elif info["sweeps"] >= 2 and ragged:
        t.add("wrapped")
    if kernel in PREDICATE_OPERANDS and PREDICATE_OPERANDS[kernel] and kernel != "bn_act_maxpool":
        if info["vec"] == 4:
            t.add("vec")
        elif inner % 4:
            t.add("scalar_by_size")
        elif c["off"]:
            t.add("scalar_by_alignment")
    if kernel == "bn_act" and c["batches"] > 1:
        per_batch = total // info["vec"] // c["batches"]
        if per_batch % info["threads"]:
            t.add("boundary_in_workgroup")
        if "wrapped" in t:
            t.add("batches_wrapped")
    if kernel == "target_residual":
        from pleas_merging_amd import hip_ops

        n = info["blocks"]
        t |= {"partials_1"} if n == 1 else set()
        t |= {"partials_ge_65"} if n >= 65 else set()
        t |= {"partials_max"} if n == hip_ops.target_residual_max_partials() else set()
    if kernel == "bn_train_fold":
        n, S = geo[0], info["S"]
        t |= {"S_1"} if S == 1 else set()
        t |= {"S_gt_1_ragged"} if S > 1 and n % S else set()
        t |= {"N_gt_S"} if n > S > 1 else set()
    return t, info
