#!/usr/bin/env python3
"""Generate tests/golden/minimax_small.npz by RUNNING THE REFERENCE's ``scipy_solve_minimax_assignment``
(pleas/core/solvers.py:88-115).

Run only where a checkout of the reference is available (it never travels):
``python tests/golden/make_golden_minimax.py <reference checkout>``
The reference is imported unmodified, with the same stubs as make_golden.py.

Cases (inputs + expected outputs only):
  * the 210 matrices of lap_small.npz, on A ("lap_<i>_pos") and on -A ("lap_<i>_neg"): matrices are read from there;
  * seeded larger cases "seed_<n>_<kind>": A = np.random.default_rng(seed) ... (see seeded_matrix), stored by seed.
Per case: t (the reference's bottleneck value min_i A[i, p(i)], a zero as +0, fp32) and perm (its permutation, int64).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

SEEDED = [(300, "normal", 11), (300, "int", 12), (1000, "normal", 13), (1000, "int", 14), (2048, "normal", 15),
          (2048, "int", 16)]


def seeded_matrix(n, kind, seed):
    """The larger cases, rebuilt from their seed by the tests (fp32)."""
    rng = np.random.default_rng(seed)
    if kind == "normal":
        return rng.standard_normal((n, n)).astype(np.float32)
    return rng.integers(-20, 20, (n, n)).astype(np.float32)       # integer-tied


def main(ref_root):
    tv = types.ModuleType("torchvision")
    tv.ops = types.ModuleType("torchvision.ops")
    tv.ops.stochastic_depth = lambda *a, **k: a[0]
    sys.modules["torchvision"], sys.modules["torchvision.ops"] = tv, tv.ops
    gp = types.ModuleType("gurobipy")
    gp.GRB, gp.Model = object(), object
    sys.modules["gurobipy"] = gp
    sys.modules["torchmetrics"] = types.ModuleType("torchmetrics")
    sys.path.insert(0, ref_root)
    from pleas.core.solvers import scipy_solve_minimax_assignment as ref  # noqa: E402

    def solve(A):
        p = ref(torch.from_numpy(A)).numpy().astype(np.int64)
        t = np.float32(A[np.arange(A.shape[0]), p].min()) + np.float32(0)
        return t, p

    lap = np.load(os.path.join(HERE, "lap_small.npz"))
    out = {}
    names = []
    for i in range(int(lap["n_cases"])):
        A = lap["cost_%d" % i].astype(np.float32)
        for sign, tag in ((1, "pos"), (-1, "neg")):
            name = "lap_%d_%s" % (i, tag)
            out[name + "/t"], out[name + "/perm"] = solve(A if sign > 0 else -A)
            names.append(name)
    for n, kind, seed in SEEDED:
        name = "seed_%d_%s" % (n, kind)
        out[name + "/t"], out[name + "/perm"] = solve(seeded_matrix(n, kind, seed))
        out[name + "/seed"] = np.int64(seed)
        names.append(name)
    out["names"] = np.array(names)
    out["versions"] = np.array("torch %s numpy %s" % (torch.__version__, np.__version__))
    np.savez_compressed(os.path.join(HERE, "minimax_small.npz"), **out)
    print("wrote", len(names), "cases")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_minimax.py <reference checkout>")
    main(sys.argv[1])
