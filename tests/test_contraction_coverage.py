"""The coverage ledger of the matching contraction (csrc/gram.hip) and the normal equations (csrc/normal_eq.hip), no GPU: every
(variant, slabs) a caller's geometry can reach has a case in tests/contraction_cases.py, and every variant has a case at every
edge a tile goes wrong at.

Which variant a geometry gets is decided by ``build_batch_plan`` / ``make_plan`` and ``build_neq_plan``; both sides of the
comparison are ASKED of the built library through its host-only queries (``GramBatch.plan_info``, ``gram_plan_info``,
``NormalEqBatch.layer_info``), never re-derived here.  A threshold that moves a case off its variant fails here, on a machine
without a GPU, and the printed ledger (``pytest -s``) shows which.

The last two tests hold the harness itself before anything runs on a GPU: plain fp32 on the CPU, in whatever order torch sums,
must lie inside the per-element bounds of tests/contraction_ref.py around the fp64 reference."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import contraction_cases as cc
import contraction_ref as cr

# A reachable combination may only be left out if no tensor under 256 MB reaches it: by name, with the reason; at most two.
EXCLUSIONS = {}          # {(kernel, key): reason}


def _gram_ledger():
    ledger, mixed = {}, 0
    for indices in cc.gram_launches():
        nodes, group_C = cc.gram_nodes(indices)
        infos = cc.gram_infos(nodes, group_C)
        for (i, B, C, HW, g, src), info in zip(nodes, infos):
            if src is None:
                shape, derived = cc.GRAM_CASES[i]
                assert info["sums"] == derived, (shape, info)
                ledger.setdefault((info["variant"], info["S"] > 1), []).append((shape, cc.gram_traits(shape, derived, info)))
            else:
                assert info["S"] == 0, info
        for g in range(len(group_C)):
            mixed += len({info["variant"] for n, info in zip(nodes, infos) if n[4] == g and n[5] is None}) > 1
    return ledger, mixed


def test_gram_table_reaches_every_reachable_variant_with_every_trait():
    reach = cc.reachable_gram()
    assert {v for v, _ in reach} == set(cc.GRAM_VARIANTS), "the grid itself no longer reaches all six variants: %r" % sorted(reach)
    ledger, mixed = _gram_ledger()
    print("\npleas_gram_batch: (variant, slabs) -> cases")
    for key in sorted(set(ledger) | reach):
        print("  variant %d %-4s: %s" % (key[0], "S>1" if key[1] else "S=1", [c for c, _ in ledger.get(key, [])] or "NO CASE"))
    missing = [k for k in sorted(reach) if k not in ledger and ("gram", k) not in EXCLUSIONS]
    assert not missing, "reachable (variant, S > 1) without a case: %r" % missing
    for v in cc.GRAM_VARIANTS:
        have = set().union(*[t for k, rows in ledger.items() if k[0] == v for _, t in rows])
        want = {t for t in cc.GRAM_TRAITS if (v, t) not in cc.GRAM_CANNOT}
        if v >= 4:
            want |= {"hw_%d" % hw for hw in cc.PAD_HW}
        assert want <= have, "variant %d has no case with %r" % (v, sorted(want - have))
    for (v, t), why in sorted(cc.GRAM_CANNOT.items()):
        print("  variant %d cannot have %s: %s" % (v, t, why))
    assert mixed >= 2, "no launch holds a group with nodes of different variants"
    assert len(EXCLUSIONS) <= 2


def test_gram_single_node_table_reaches_both_tiles_and_both_loads():
    from pleas_merging_amd import hip_ops

    seen = set()
    print("\npleas_gram_accum: (tile, floats per load) -> cases")
    for shape, off in cc.GRAM_SINGLE_CASES:
        B, C, HW = cc.bchw(shape)
        info = hip_ops.gram_plan_info(B, C, HW, aligned=not off)
        print("  %r%s: %r" % (shape, " one float off" if off else "", info))
        seen.add((info["tile"], info["vec"], off and HW % 4 == 0, info["S"] > 1))
        assert info["S"] >= 1 and info["S"] * info["chunks_per_slab"] >= -(-B * HW // cc.BK)
    assert {(t, v) for t, v, _, _ in seen} == {(64, 4), (64, 1), (128, 4), (128, 1)}
    assert {(64, 1, True), (128, 1, True)} <= {s[:3] for s in seen}, "no misaligned view at HW % 4 == 0"
    assert any(s[3] for s in seen)


def _neq_ledger():
    ledger = {}
    for indices in cc.neq_launches():
        cases = [cc.NEQ_CASES[i] for i in indices]
        for case, info in zip(cases, cc.neq_infos(cases)):
            ledger.setdefault((info["variant"], info["S"] > 1), []).append((case, cc.neq_traits(case, info)))
    return ledger


def test_neq_table_reaches_every_reachable_variant_with_every_trait():
    reach = cc.reachable_neq()
    assert {v for v, _ in reach} == set(cc.NEQ_VARIANTS), "the grid itself no longer reaches all ten variants: %r" % sorted(reach)
    ledger = _neq_ledger()
    print("\npleas_normal_eq_accum: (variant, slabs) -> cases")
    for key in sorted(set(ledger) | reach):
        print("  variant %2d %-4s: %s" % (key[0], "S>1" if key[1] else "S=1", [c for c, _ in ledger.get(key, [])] or "NO CASE"))
    missing = [k for k in sorted(reach) if k not in ledger and ("neq", k) not in EXCLUSIONS]
    assert not missing, "reachable (variant, S > 1) without a case: %r" % missing
    for v in cc.NEQ_VARIANTS:
        have = set().union(*[t for k, rows in ledger.items() if k[0] == v for _, t in rows])
        want = set(cc.NEQ_TRAITS)
        if v >= 8:
            want |= set(cc.NEQ_LAG_TRAITS)
        elif v >= 4:
            want |= set(cc.NEQ_SHIFT_TRAITS) | {"stem"}
        want = {t for t in want if (v, t) not in cc.NEQ_CANNOT}
        assert want <= have, "variant %d has no case with %r" % (v, sorted(want - have))
    for (v, t), why in sorted(cc.NEQ_CANNOT.items()):
        print("  variant %d cannot have %s: %s" % (v, t, why))
    assert len(EXCLUSIONS) <= 2


def test_tables_stay_small():
    for shape, _ in cc.GRAM_CASES:
        B, C, HW = cc.bchw(shape)
        assert 4 * B * C * HW < 4e6, shape
    for case in cc.NEQ_CASES:
        N, Cin, H, W, KH, KW, stride, pad = case
        assert 4 * N * Cin * H * W < 4e6 and 4 * (KH * KW * Cin) ** 2 < 8e6, case


def test_queries_answer_entry_by_entry_and_refuse_what_the_launch_refuses():
    """The queries run the launches' own plan builders: a node's or layer's answer does not depend on its neighbours, an empty
    list or NULL is -22, and a geometry the launch refuses is refused with the launch's message."""
    from pleas_merging_amd import _lib, hip_ops

    geos = [cc.bchw(s) for s, _ in cc.GRAM_CASES]
    together = hip_ops.GramBatch.plan_info(geos)
    assert together == [hip_ops.GramBatch.plan_info([g])[0] for g in geos]
    assert together == hip_ops.GramBatch.plan_info(geos[::-1])[::-1]
    for (B, C, HW), info in zip(geos, together):
        assert info["S"] >= 1 and info["S"] * info["chunks_per_slab"] * cc.BK >= B * info["HWp"] and not info["sums"]
        assert info["tiles"] == -(-C // (128 if info["variant"] in (0, 1, 4) else 64))
    # a derived node: no slabs of its own, its source writes row sums -- and is the only node that does
    got = hip_ops.GramBatch.plan_info([(8, 72, 576, 0, None), (8, 72, 576, 0, None), (8, 72, 576, 0, 1)], [72])
    assert [i["sums"] for i in got] == [False, True, False] and [i["S"] for i in got] == [2, 2, 0]
    lib = _lib.lib()
    with pytest.raises(_lib.PleasHipError, match="derived node needs a contracted source node"):
        hip_ops.GramBatch.plan_info([(2, 8, 4, 0, None), (2, 8, 4, 0, 0), (2, 8, 4, 0, 1)], [8])
    with pytest.raises(_lib.PleasHipError, match="node shape"):
        hip_ops.GramBatch.plan_info([(0, 8, 4)])
    with pytest.raises(_lib.PleasHipError, match="fewer than 2\\^30 elements"):
        hip_ops.GramBatch.plan_info([(1 << 10, 1 << 10, 1 << 10)])
    with pytest.raises(_lib.PleasHipError):
        hip_ops.GramBatch.plan_info([])
    one = (ctypes.c_int * 6)()
    assert lib.pleas_gram_batch_plan_info(None, 0, None, 0, one) == -22 and lib.pleas_gram_batch_plan_info(None, 3, None, 1, one) == -22
    assert lib.pleas_gram_plan_info(2, 8, 4, 1, None) == -22
    with pytest.raises(_lib.PleasHipError, match="must be positive"):
        hip_ops.gram_plan_info(2, 0, 4)
    with pytest.raises(_lib.PleasHipError, match="B\\*C\\*HW must be < 2\\^30"):
        hip_ops.gram_plan_info(1 << 10, 1 << 10, 1 << 10)

    layers = hip_ops.NormalEqBatch.layer_info(cc.NEQ_CASES)
    assert layers == [hip_ops.NormalEqBatch.layer_info([c])[0] for c in cc.NEQ_CASES]
    assert layers == hip_ops.NormalEqBatch.layer_info(cc.NEQ_CASES[::-1])[::-1]
    for case, info in zip(cc.NEQ_CASES, layers):
        R, lag = case[4] * case[5], info["variant"] >= 8
        assert info["S"] >= 1 and info["tiles"] == -(-case[1] // (64 if info["variant"] & 1 else 128))
        assert (info["blocks_to_finalize"] > 0) == lag
        if not lag:       # every lower block tile is contracted
            assert info["block_tiles"] == (R * info["tiles"]) * (R * info["tiles"] + 1) // 2
    assert [i["blocks_to_finalize"] for c, i in zip(cc.NEQ_CASES, layers) if c[4:] == (3, 3, 1, 1) and min(c[2:4]) >= 3][0] == 16
    with pytest.raises(_lib.PleasHipError, match="empty output"):
        hip_ops.NormalEqBatch.layer_info([(4, 64, 2, 2, 7, 7, 1, 0)])
    with pytest.raises(_lib.PleasHipError, match="layer geometry"):
        hip_ops.NormalEqBatch.layer_info([(4, 64, 8, 8, 3, 3, 0, 1)])
    with pytest.raises(_lib.PleasHipError):
        hip_ops.NormalEqBatch.layer_info([])
    assert lib.pleas_normal_eq_layer_info(None, 0, one) == -22 and lib.pleas_normal_eq_layer_info(None, 2, one) == -22


# ------------------------------------------------------------------------------------------------ the harness on the CPU
def _smallest(cases, size, count=5):
    return sorted(cases, key=size)[:count]


def test_plain_fp32_gram_on_the_cpu_lies_inside_the_bounds():
    small = _smallest(cc.GRAM_CASES, lambda c: cc.bchw(c[0])[0] * cc.bchw(c[0])[1] ** 2 * cc.bchw(c[0])[2])
    small.append(((3, 70, 7, 7), True))
    for n, (shape, _) in enumerate(small):
        x, y = cr.gram_operands(shape, 100 + n)
        B, C, HW = cc.bchw(shape)
        xf, yf = x.reshape(B, C, HW), y.reshape(B, C, HW)
        G = torch.einsum("bip,bjp->ij", xf, yf)
        nx, ny = (xf * xf).sum((0, 2)), (yf * yf).sum((0, 2))
        ref = cr.gram_node_ref(x, y)
        base = torch.randn(C, C, generator=torch.Generator().manual_seed(n))
        for cdist, got in ((False, G), (True, -(nx[:, None] + ny[None, :] - 2 * G).clamp_min(0).sqrt())):
            want, bound = cr.gram_group_ref([ref], [1], cdist)
            assert ((got.double() - want).abs() <= bound).all(), (shape, cdist)
            assert (bound < 0.05 * (want.abs() + 1)).all()                  # and the bound is no blank cheque
            want, bound = cr.gram_group_ref([ref], [1], cdist, base)
            assert (((base + got).double() - want).abs() <= bound).all(), (shape, cdist, "accumulate")
        # the derived image from the fp32 sums, combined in fp64 as the reduce pass does
        aff = cr.gram_affine(C, 200 + n)
        ax, bx, ay, by = (v.double() for v in aff)
        sx, sy = xf.sum((0, 2)).double(), yf.sum((0, 2)).double()
        K = B * HW
        inner = (ax[:, None] * ay[None, :] * G.double() + (ax * sx)[:, None] * by[None, :] + bx[:, None] * (ay * sy)[None, :]
                 + K * bx[:, None] * by[None, :])
        n1 = ax * ax * nx.double() + 2 * ax * bx * sx + K * bx * bx
        n2 = ay * ay * ny.double() + 2 * ay * by * sy + K * by * by
        dref = cr.gram_node_ref(x, y, aff)
        for cdist, got in ((False, inner.float()), (True, -(n1[:, None] + n2[None, :] - 2 * inner).float().clamp_min(0).sqrt())):
            want, bound = cr.gram_group_ref([dref], [1], cdist)
            assert ((got.double() - want).abs() <= bound).all(), (shape, cdist, "derived")
            both, bound2 = cr.gram_group_ref([ref, dref], [1, 1], cdist)
            assert torch.allclose(both, want + cr.gram_group_ref([ref], [1], cdist)[0], rtol=1e-12, atol=0) and (bound2 >= bound).all()


def test_plain_fp32_normal_equations_on_the_cpu_lie_inside_the_bound():
    """Also the index mapping: ``F.unfold`` orders its columns (ci, r); A is kernel-position-major, k = r * Cin + ci."""
    small = _smallest(cc.NEQ_CASES, lambda c: c[0] * c[2] * c[3] * (c[1] * c[4] * c[5]) ** 2)
    small += [(2, 24, 6, 7, 1, 3, 1, 1), (2, 3, 20, 20, 7, 7, 2, 3)]
    for n, case in enumerate(small):
        N, Cin, H, W, KH, KW, stride, pad = case
        ip = torch.randn(N, Cin, H, W, generator=torch.Generator().manual_seed(300 + n))
        cols = F.unfold(ip, (KH, KW), 1, pad, stride)
        Uf = cols.view(N, Cin, KH * KW, -1).permute(0, 3, 2, 1).reshape(-1, KH * KW * Cin)
        got = Uf.t() @ Uf
        want, Sabs = cr.neq_ref(ip, case)
        Ho, Wo = cc.neq_out(case)
        assert Uf.shape[0] == N * Ho * Wo
        bound = cr.neq_bound(Sabs, N * Ho * Wo, 1, 1)
        assert ((got.double() - want).abs() <= bound).all(), case
        assert (bound <= 0.01 * (want.abs().max() + 1)).all()
        # the mapping, from the definition: column (r, ci) of U at output pixel (oh, ow) is ip[ci, oh s + kh - pad, ow s + kw - pad]
        padded = F.pad(ip.double(), (pad, pad, pad, pad))
        Um = cr.neq_unfold(ip, case).view(N, Ho, Wo, KH * KW, Cin)
        for r in {0, KH * KW // 2, KH * KW - 1}:
            kh, kw = divmod(r, KW)
            view = padded[:, :, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride]
            assert torch.equal(Um[:, :, :, r, :], view.permute(0, 2, 3, 1)), (case, r)
        lower = cr.neq_lower_tiles(case)
        assert lower.diagonal().all() and lower[-1].all() and not lower[0, -1] or KH * KW * Cin <= 64
