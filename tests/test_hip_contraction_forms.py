"""Every variant of the matching contraction (csrc/gram.hip) and of the normal equations (csrc/normal_eq.hip) against fp64, element
by element, over the case tables of tests/contraction_cases.py (tests/test_contraction_coverage.py holds, without a GPU, that
the tables reach every variant a geometry can reach, with every edge, and that the references and bounds used here are sound).

The cases run in grouped launches of mixed variants, about eight per launch, as a real batch does; every launch runs twice, the
second time through the cached plan on fresh copies of the operands, and the two results must be ``torch.equal``.  Every output
is followed by a guard band that must stay intact; Gram matrices under overwrite are pre-filled with NaN; accumulated Gram
matrices and every A start from a random base that the reference adds; the strict upper block tiles of A hold a sentinel.

Bounds (tests/contraction_ref.py; u = 2^-24, gamma_n = n u / (1 - n u), Higham section 3.1 -- derived, none measured):
Gram inner product gamma_(K+S+nodes+1) * sum |x||y| + u |base|; negative distance min(sqrt(E), E / |want|) + 2u |want| per node
with E = gamma_(K+S+3) * (Nx + Ny + 2 sum |x||y|); derived nodes the same term by term; normal equations
gamma_(reps (Ktot+S+1)) * sum |u_i||u_j| + u |base| over the lower block tiles, copied blocks as contracted ones.

Arithmetics (``pleas_arith``; the matching contraction only, the normal equations have one): variants 0 and 2 run the split
kernels, every other variant the exact tile under every mode.  Mode 2 (nine products, each exact) is held to min(gamma, the
six-product constant).  Mode 1 (six products) has no derivable constant: the exact kernels' worst ratio |got - want| /
sum |x||y| over this table was measured on the MI355X -- never on the split kernels -- and the six-product kernels are allowed
4 x that, the margin of FWD_SPLIT_BOUND (tests/test_hip_tile_forms.py) for the same reason.  Measured: 8.618e-07 (grouped
launch, inner product, overwrite: long correlated sums, K = 3900 and 4608, added chunk by chunk) / 3.805e-07 (single-node
entry, split-K over up to 50 slabs); the larger is taken.  The tests print both again on every run."""
import pytest
import torch

import contraction_cases as cc
import contraction_ref as cr
import tile_cases as tc
from test_hip_tile_forms import Guarded, U, _elementwise, gamma  # noqa: F401  (gamma through contraction_ref.gamma_n)

pytestmark = pytest.mark.gpu

GRAM_EXACT_RATIO = 8.618e-07
GRAM_SPLIT_BOUND = 4 * GRAM_EXACT_RATIO
SPLIT_VARIANTS = (0, 2)            # gram_batch_body: the 16-byte-loadable variants have split-bf16 twins
UPPER = 123.5                      # what the strict upper block tiles of A hold


@pytest.fixture(scope="module")
def ops():
    from pleas_merging_amd import hip_ops

    return hip_ops


@pytest.fixture(params=[0, 1, 2], ids=["fp32", "split_bf16", "split_bf16_exact"])
def mode(request):
    with tc.arith(request.param):
        yield request.param


@pytest.fixture(scope="module", autouse=True)
def _references_released():
    yield
    _GRAM_REF.clear()
    _NEQ_REF.clear()
    torch.cuda.empty_cache()


_GRAM_REF, _NEQ_REF = {}, {}


def gram_ref(i):
    """Operands, affine image and fp64 facts of Gram case i (computed once, left unchanged)."""
    if i not in _GRAM_REF:
        shape, derived = cc.GRAM_CASES[i]
        x, y = cr.gram_operands(shape, 1000 + i, "cuda")
        aff = cr.gram_affine(shape[1], 2000 + i, "cuda") if derived else None
        _GRAM_REF[i] = dict(x=x, y=y, aff=aff, ref=cr.gram_node_ref(x, y), dref=cr.gram_node_ref(x, y, aff) if derived else None)
    return _GRAM_REF[i]


def _product_bound(mode, variant):
    if mode == 0 or variant not in SPLIT_VARIANTS:
        return None
    return (GRAM_SPLIT_BOUND, mode == 2)


# ------------------------------------------------------------------------------------------------ pleas_gram_batch
def _gram_launch(ops, indices, cdist, accumulate, mode, fails, worst):
    nodes, group_C = cc.gram_nodes(indices)
    infos = cc.gram_infos(nodes, group_C)
    mats = [Guarded((C, C)) for C in group_C]
    g = torch.Generator().manual_seed(sum(indices))
    # the base passes through one rounding per node of its group, the bound grants it one (u |base|) and the products one more
    # than they need: a base well below sum |x||y| keeps the bound a theorem instead of a likelihood
    bases = [(0.1 * torch.randn(C, C, generator=g)).cuda() for C in group_C]
    batch = ops.GramBatch([m.t for m in mats], ops.EPI_NEG_CDIST if cdist else ops.EPI_INNER)
    results = []
    for call in range(2):      # the second call: the cached plan, every operand at a new address
        for m, b in zip(mats, bases):
            if accumulate:
                m.t.copy_(b)
            else:
                m.poison()
        for i, B, C, HW, group, src in nodes:
            r = gram_ref(i)
            if src is None:
                x, y = (r["x"], r["y"]) if call == 0 else (r["x"].clone(), r["y"].clone())
                assert x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0
                batch.add(x, y, 1, group)
            else:
                batch.add_derived(src, *r["aff"], group)      # the plan holds these addresses: they stay
        batch.flush(accumulate=accumulate)
        torch.cuda.synchronize()
        results.append([m.t.clone() for m in mats])
    for gi, C in enumerate(group_C):
        members = [(n, info) for n, info in zip(nodes, infos) if n[4] == gi]
        refs, slabs, pbs, names = [], [], [], []
        for (i, B, _, HW, _, src), info in members:
            own = info if src is None else infos[src]
            refs.append(gram_ref(i)["ref" if src is None else "dref"])
            slabs.append(own["S"])
            pbs.append(_product_bound(mode, own["variant"]))
            names.append("%r%s v%d S=%d" % (cc.GRAM_CASES[i][0], " derived" if src is not None else "", own["variant"], own["S"]))
        tag = ("cdist" if cdist else "inner", "acc" if accumulate else "ovw", "C=%d" % C, names)
        want, bound = cr.gram_group_ref(refs, slabs, cdist, bases[gi] if accumulate else None, pbs)
        ok, err = _elementwise(results[0][gi], want, bound)
        if not ok:
            fails.append((tag, "element-wise bound missed at %d elements: worst |err| / bound %.3e" % (int((~(err <= bound)).sum()),
                                                                                                      float((err / bound).max()))))
        if not torch.equal(results[0][gi], results[1][gi]):
            fails.append((tag, "the second call (cached plan, moved operands) differs from the first"))
        if not mats[gi].intact():
            fails.append((tag, "guard band written"))
        if not cdist and not accumulate and all(pb is None for pb in pbs):
            worst[0] = max(worst[0], float((err / sum(r["T"] for r in refs).clamp_min(1e-300)).max()))
        worst[1] += len(members)


def test_gram_batch_every_variant(ops, mode):
    fails, worst = [], [0.0, 0]
    launches = cc.gram_launches()
    for cdist in (False, True):
        for accumulate in (False, True):
            for indices in launches:
                _gram_launch(ops, indices, cdist, accumulate, mode, fails, worst)
    print("gram_batch, pleas_arith(%d), %d nodes in %d launches: worst ratio |got - want| / sum|x||y| of the exact kernels %.3e "
          "(GRAM_EXACT_RATIO %.3e, six-product bound %.3e)" % (mode, worst[1], 4 * len(launches), worst[0], GRAM_EXACT_RATIO,
                                                               GRAM_SPLIT_BOUND))
    assert not fails, "\n".join(repr(f) for f in fails)


# ------------------------------------------------------------------------------------------------ pleas_gram_accum
def _one_float_off(t):
    """A contiguous copy of ``t`` that starts one float behind a 16-byte boundary."""
    arena = torch.zeros(t.numel() + 8, device=t.device)
    view = arena[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def test_gram_single_node_entry_every_tile_and_load(ops, mode):
    fails, worst = [], 0.0
    for n, (shape, off) in enumerate(cc.GRAM_SINGLE_CASES):
        B, C, HW = cc.bchw(shape)
        x, y = cr.gram_operands(shape, 3000 + n, "cuda")
        ref = cr.gram_node_ref(x, y)
        if off:
            x, y = _one_float_off(x), _one_float_off(y)
        info = ops.gram_plan_info(B, C, HW, aligned=not off)
        assert info["vec"] == (1 if off or HW % 4 else 4)
        pb = [(GRAM_SPLIT_BOUND, mode == 2)] if mode and info["vec"] == 4 else None
        base = torch.randn(C, C, generator=torch.Generator().manual_seed(n)).cuda()
        for cdist in (False, True):
            for accumulate in (False, True):
                tag = (shape, "one float off" if off else "aligned", "cdist" if cdist else "inner", "acc" if accumulate else "ovw", info)
                out = Guarded((C, C))
                if accumulate:
                    out.t.copy_(base)
                ops.gram_accum(x, y, 1, out.t, ops.EPI_NEG_CDIST if cdist else ops.EPI_INNER, accumulate=accumulate)
                # the single-node entry adds its epilogue's value to the base in one step: one group of one node
                want, bound = cr.gram_group_ref([ref], [info["S"]], cdist, base if accumulate else None, pb)
                ok, err = _elementwise(out.t, want, bound)
                if not ok:
                    fails.append((tag, "element-wise bound missed: worst |err| / bound %.3e" % float((err / bound).max())))
                if not out.intact():
                    fails.append((tag, "guard band written"))
                if pb is None and not cdist and not accumulate:
                    worst = max(worst, float((err / ref["T"]).max()))
    print("gram_accum, pleas_arith(%d): worst ratio |got - want| / sum|x||y| of the exact kernels %.3e" % (mode, worst))
    assert not fails, "\n".join(repr(f) for f in fails)


# ------------------------------------------------------------------------------------------------ pleas_normal_eq_accum
def neq_ref(i):
    if i not in _NEQ_REF:
        case = cc.NEQ_CASES[i]
        g = torch.Generator().manual_seed(4000 + i)
        ip = torch.randn(case[:4], generator=g).cuda()
        # the base: what an earlier batch left in A.  A lag-form layer's copied blocks are only defined by their class's
        # contracted block, so the base has to be a matrix of the same structure; and it is rounded once per batch while the
        # bound grants it one u |base|, so it comes from 0.7 x the same input: 0.49 of every element's own sum |u_i||u_j| at
        # most, which the products' gamma covers
        want, Sabs = cr.neq_ref(ip, case)
        _NEQ_REF[i] = dict(ip=ip, base=(0.49 * want).float(), want=want, Sabs=Sabs, lower=cr.neq_lower_tiles(case, "cuda"))
    return _NEQ_REF[i]


def _neq_check(tag, what, A, r, info, rows, reps, fails):
    lower = r["lower"]
    want = r["base"].double() + reps * r["want"]
    bound = cr.neq_bound(r["Sabs"], rows, info["S"], reps, r["base"])
    ok, err = _elementwise(A.t[lower], want[lower], bound[lower])
    if not ok:
        bad = (~(err <= bound[lower])).nonzero()[:, 0]
        where = lower.nonzero()[bad[0]].tolist()
        fails.append((tag, what, "element-wise bound missed at %d elements, first (%d, %d): worst |err| / bound %.3e" % (
            bad.numel(), where[0], where[1], float((err / bound[lower]).max()))))
    if not bool((A.t[~lower] == UPPER).all()):
        fails.append((tag, what, "strict upper block tiles written"))
    if not A.intact():
        fails.append((tag, what, "guard band written"))


def _neq_launch(ops, indices, fails):
    cases = [cc.NEQ_CASES[i] for i in indices]
    infos = cc.neq_infos(cases)
    batch = ops.NormalEqBatch(torch.device("cuda"))
    first, second = [], []
    for held, call in ((first, 0), (second, 1)):
        for i, case in zip(indices, cases):
            r = neq_ref(i)
            K = case[1] * case[4] * case[5]
            A = Guarded((K, K))
            A.t.copy_(torch.where(r["lower"], r["base"], torch.full_like(r["base"], UPPER)))
            ip = r["ip"] if call == 0 else r["ip"].clone()
            batch.add(ip, A.t, case[4:6], case[6], case[7])
            held.append((A, ip))
        batch.flush()
    torch.cuda.synchronize()
    pairs = lambda held: [(A.t, tuple(case)) for case, (A, _) in zip(cases, held)]
    tags = [(case, "variant %d" % info["variant"], "S=%d" % info["S"]) for case, info in zip(cases, infos)]
    rows = [case[0] * cc.neq_out(case)[0] * cc.neq_out(case)[1] for case in cases]
    for tag, (A1, _), (A2, _) in zip(tags, first, second):
        if not torch.equal(A1.t, A2.t):
            fails.append((tag, "the second call (cached plan, moved operands) differs from the first"))
    batch.finalize(pairs(first))
    batch.finalize(pairs(first))      # idempotent
    for i, tag, info, n, (A1, _) in zip(indices, tags, infos, rows, first):
        _neq_check(tag, "one batch, finalized twice", A1, neq_ref(i), info, n, 1, fails)
    # a second batch into the matrices of the second call, finalized once after both
    for case, (A2, ip) in zip(cases, second):
        batch.add(ip, A2.t, case[4:6], case[6], case[7])
    batch.flush()
    batch.finalize(pairs(second))
    torch.cuda.synchronize()
    for i, tag, info, n, (A2, _) in zip(indices, tags, infos, rows, second):
        _neq_check(tag, "two batches, finalized once", A2, neq_ref(i), info, n, 2, fails)
    return len(cases)


@pytest.mark.parametrize("launch", range(len(cc.neq_launches())))
def test_normal_eq_every_variant(ops, launch):
    fails = []
    n = _neq_launch(ops, cc.neq_launches()[launch], fails)
    print("normal_eq_accum, launch %d: %d layers, each accumulated once, again from moved operands, and twice" % (launch, n))
    assert not fails, "\n".join(repr(f) for f in fails)


# ------------------------------------------------------------------------------------------------ refusals: errors, not faults
def test_grouped_launches_refuse_a_misaligned_operand_and_a_derived_source(ops):
    x, y = cr.gram_operands((3, 40, 6, 6), 5, "cuda")
    acc = torch.zeros(40, 40, device="cuda")
    batch = ops.GramBatch([acc], ops.EPI_INNER)
    batch.add(_one_float_off(x), _one_float_off(y), 1, 0)
    with pytest.raises(ops.PleasHipError, match="16-byte aligned"):
        batch.flush()
    assert not acc.any()
    ip = _one_float_off(torch.randn(3, 40, 6, 6, device="cuda"))
    A = torch.zeros(40, 40, device="cuda")
    neq = ops.NormalEqBatch(torch.device("cuda"))
    neq.add(ip, A, (1, 1), 1, 0)
    with pytest.raises(ops.PleasHipError, match="16-byte alignment"):
        neq.flush()
    assert not A.any()
    batch = ops.GramBatch([acc], ops.EPI_INNER)
    src = batch.add(x, y, 1, 0)
    aff = cr.gram_affine(40, 6, "cuda")
    derived = batch.add_derived(src, *aff, 0)
    with pytest.raises(ops.PleasHipError, match="source must be a contracted node"):
        batch.add_derived(derived, *aff, 0)
    # and the library's own answer to such a list, whatever the wrapper lets through
    from pleas_merging_amd import _lib

    import ctypes

    arr = (_lib.GramNode * 3)()
    for a in arr:
        a.x, a.y, a.B, a.C, a.HW, a.group = x.data_ptr(), y.data_ptr(), 3, 40, 36, 0
    for a, s in ((arr[1], 0), (arr[2], 1)):
        a.derived, a.source = 1, s
        a.scale_x, a.shift_x, a.scale_y, a.shift_y = (v.data_ptr() for v in aff)
    lib, ws = _lib.lib(), torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    accs, gc = (ctypes.c_void_p * 1)(acc.data_ptr()), (ctypes.c_int * 1)(40)
    assert lib.pleas_gram_batch_ws_bytes(arr, 3, gc, 1) == 0
    assert lib.pleas_gram_batch(arr, 3, accs, gc, 1, ops.EPI_INNER, 0, ws.data_ptr(), ws.numel(), 1, ops._stream()) == -22
    assert b"derived node needs a contracted source node" in lib.pleas_last_error()
    torch.cuda.synchronize()
    assert not acc.any()
