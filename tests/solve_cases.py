"""Size tables of the batched SPD solve tests (tests/test_hip_solve.py): plain data, (K, N) per problem -- K unknowns,
N right-hand-side rows.  The solve's panel width is 64 and one launch group holds 96 problems."""
import random

# Batches in which a problem in its last, narrow panel (K % 64 != 0) has more rows below that panel than the problem with
# the largest K has left at the same step: the forward sweep's row grid used to be sized by the latter.
MIXED_LAST_PANEL = {
    "128x1+65x100": [(128, 1), (65, 100)],
    "192x8+130x150": [(192, 8), (130, 150)],
    "256x100+65x321": [(256, 100), (65, 321)],
    "320x3+70x300+129x200": [(320, 3), (70, 300), (129, 200)],
}


def _draw(seed, count, kmax, nmax):
    rng = random.Random(seed)
    return [(rng.randint(1, kmax), rng.randint(0, nmax)) for _ in range(count)]


BATCHES = dict(MIXED_LAST_PANEL)
BATCHES.update({
    # problems without right-hand sides (factor only) next to others, first, last and in between
    "no_rhs": [(70, 0), (33, 5), (129, 0), (64, 64), (1, 0), (200, 1), (65, 0)],
    # every K around the panel width and around two panels, the widest rows on the narrowest last panels
    "panel_edges": [(1, 3), (63, 10), (64, 10), (65, 130), (127, 70), (128, 5), (129, 257), (1, 1)],
    # 3 * 3 * 128 + 1 columns: nineteen panels, the last one column wide, beside a short problem with many rows
    "k1153": [(1153, 5), (65, 200), (640, 3)],
    # more problems than one launch group holds
    "draw120": _draw(20250, 120, 400, 400),
})

# moderately ill-conditioned family (cond about 1e4)
ILL_BATCH = [(1, 3), (64, 7), (65, 100), (130, 17), (200, 256), (513, 40)]

RIDGE_BATCH = [(1, 2), (65, 100), (130, 17), (70, 0), (200, 64), (96, 4)]

# info: (index in the batch, K, m) -- A[m][m] = -1; the other problems of the batch are healthy
INFO_COUNT = 101
INFO_BAD = [(0, 80, 0), (3, 80, 5), (50, 80, 63), (95, 80, 64), (96, 80, 69), (100, 80, 79), (98, 1, 0)]
INFO_HEALTHY = [(5, 2), (64, 3), (65, 9), (130, 4), (33, 0), (1, 1), (70, 40)]     # cycled over the other indices
