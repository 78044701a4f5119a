"""The coverage ledger of the streaming kernels (csrc/elementwise.hip, csrc/bn_train.hip, target_residual in csrc/conv.hip), no
GPU: every path a geometry can take -- floats per load, kernel form -- has a case in tests/stream_cases.py with every trait a
streaming kernel goes wrong at: the second sweep of its grid-stride loop with a ragged end, the scalar path by size and by
alignment, and the kernel's own edges.

Which path a case takes and how many sweeps it runs is ASKED of the built library (``hip_ops.stream_plan_info``: the function
the launchers compute their grids with), never re-derived here.  A cap or a predicate that moves a case off its path fails here,
on a machine without a GPU, and the printed ledger (``pytest -s``) shows which.

The last tests hold the harness itself before anything runs on a GPU: plain fp32 torch on the CPU lies inside every bound of
tests/stream_ref.py around the fp64 reference, and no bound is a blank cheque."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import stream_cases as sc
import stream_ref as sr

# A reachable (path, trait) may only be left out if no tensor under 64 MB reaches it: by name, with the reason; at most two.
EXCLUSIONS = {}          # {(kernel, path, trait): reason}


@pytest.mark.parametrize("kernel", list(sc.KERNELS))
def test_table_reaches_every_path_with_every_trait(kernel):
    table = sc.KERNELS[kernel][0]
    ledger, off_seen = {}, set()
    for c in table:
        t, info = sc.traits(kernel, c)
        ledger.setdefault(sc.path(info), []).append((c, t, info))
        off_seen |= set(c["off"])
    reach = sc.reachable(kernel)
    print("\n%s: (form, floats per load) -> cases" % kernel)
    for key in sorted(set(ledger) | reach):
        rows = ledger.get(key, [])
        print("  %-8s vec %d: %s" % (key[0] or "-", key[1], "%d cases" % len(rows) if rows else "NO CASE"))
        for c, t, info in rows:
            print("      %s\n        blocks %d sweeps %d%s: %s" % ({k: v for k, v in c.items() if k != "combos"}, info["blocks"], info["sweeps"],
                                                                 " S %d" % info["S"] if "S" in info else "", " ".join(sorted(t))))
    assert reach == set(ledger), "paths the query returns / paths with a case: %r / %r" % (sorted(reach), sorted(ledger))
    general = ("one_sweep", "wrapped") + sc.WIDTH_TRAITS
    for key, rows in sorted(ledger.items()):
        have = set().union(*[t for _, t, _ in rows])
        want = {t for t in general + sc.PER_KERNEL_TRAITS[kernel]
                if (kernel, key, t) not in sc.CANNOT and (kernel, key, t) not in EXCLUSIONS}
        assert want <= have, "%s %r has no case with %r" % (kernel, key, sorted(want - have))
    for (k, key, t), why in sorted(sc.CANNOT.items()):
        if k == kernel:
            assert key in ledger or key in (sc.SCALAR, sc.VEC, sc.STEM, sc.GENERAL)
            print("  %s vec %d cannot have %s: %s" % (key[0] or "-", key[1], t, why))
    missing = set(sc.PREDICATE_OPERANDS[kernel]) - off_seen
    assert not missing, "%s: never the misaligned operand: %r" % (kernel, sorted(missing))
    assert len(EXCLUSIONS) <= 2


def test_tables_stay_small():
    for kernel, (table, _) in sc.KERNELS.items():
        wrapped = 0
        for c in table:
            for shape in sc.tensors(kernel, c):
                assert 4 * math.prod(shape) <= sc.MAX_TENSOR_BYTES, (kernel, c, shape)
            wrapped += "wrapped" in sc.traits(kernel, c)[0] and kernel not in ("channel_sum", "bn_train_fold")
        assert wrapped <= sc.MAX_WRAPPED, (kernel, wrapped)


def test_query_answers_case_by_case_and_refuses_what_the_launch_refuses():
    """The query runs the launches' own plan functions: an answer does not depend on neighbouring calls, NULL is -22, and a
    geometry the launch refuses is refused with the launch's message."""
    from pleas_merging_amd import _lib, hip_ops

    jobs = [(k, c) for k, (table, _) in sc.KERNELS.items() for c in table]
    first = [sc.plan(k, c)[0] for k, c in jobs]
    assert first == [sc.plan(k, c)[0] for k, c in jobs[::-1]][::-1]
    for (k, c), info in zip(jobs, first):
        assert info["threads"] == 256 and info["vec"] in (1, 4) and info["blocks"] >= 1 and info["sweeps"] >= 1, (k, c, info)
    # the caps the sweeps come from
    assert hip_ops.stream_plan_info("masked_adam", 2048 * 256)["sweeps"] == 1 and hip_ops.stream_plan_info("masked_adam", 2048 * 256 + 1)["sweeps"] == 2
    assert hip_ops.stream_plan_info("sqerr", 1024 * 256 + 1) == {"vec": 1, "blocks": 1024, "threads": 256, "sweeps": 2}
    assert hip_ops.stream_plan_info("top1_count", 8193, 5)["sweeps"] == 2 and hip_ops.stream_plan_info("pool_gather", 1 << 22, 1, 1, 1, 0)["sweeps"] == 1
    assert hip_ops.stream_plan_info("target_residual", 1, 1, 1, 4 * 2048 * 256)["blocks"] == hip_ops.target_residual_max_partials()
    assert hip_ops.stream_plan_info("bn_train_fold", 7, 2, 300, 9)["S"] == 4 and hip_ops.stream_plan_info("bn_train_fold", 7, 2, 1024, 9)["S"] == 1
    # nothing to do: no workgroups, as the launch enqueues nothing
    assert hip_ops.stream_plan_info("bn_act", 0, 4, 9, 0)["blocks"] == 0 and hip_ops.stream_plan_info("masked_adam", 0)["sweeps"] == 0
    refused = [("merge_blocks", (1, 2, 3, 0, 2, 3, 1), "negative size"), ("merge_blocks", (1, 2, 3, 4, 2, 5, 0), "cols_out != cols_src"),
               ("bn_act", (6, 4, 9, 4), "whole batches"), ("bn_act", (1 << 20, 1 << 12, 1, 0), "tensor too large"),
               ("bn_act_maxpool", (1, 1, 8, 8, 3, 3, 2, 2), "pooling window"), ("bn_act_maxpool", (1, 1, 1, 1, 4, 4, 1, 1), "larger than the padded input"),
               ("masked_adam", (-1,), "n < 0"), ("sqerr", (-1,), "n < 0"), ("target_residual", (0, 5, 5, 25), "target_residual: shape"),
               ("target_residual", (1 << 10, 1 << 10, 4, 1 << 12), "more than 2\\^32 elements"), ("channel_sum", (0, 3, 4), "channel_sum: empty tensor"),
               ("pool_gather", (2, 3, 4, 5, 0), "K != C without a channel map"), ("top1_count", (3, 0), "top1_count: empty rows"),
               ("bn_train_fold", (0, 1, 4, 9), "empty batch"), ("bn_train_fold", (4, 1, 70000, 9), "tensor too large")]
    for kernel, geo, message in refused:
        with pytest.raises(_lib.PleasHipError, match=message):
            hip_ops.stream_plan_info(kernel, *geo)
    with pytest.raises(_lib.PleasHipError, match="unknown kernel"):
        hip_ops.stream_plan_info("softmax", 3)
    with pytest.raises(_lib.PleasHipError, match="wrong geometry length"):
        hip_ops.stream_plan_info("sqerr", 3, 4)
    lib = _lib.lib()
    one, geo = (ctypes.c_int * 6)(), (ctypes.c_int64 * 1)(5)
    assert lib.pleas_stream_plan_info(4, geo, 1, 1, None) == -22 and lib.pleas_stream_plan_info(4, None, 1, 1, one) == -22
    assert lib.pleas_stream_plan_info(10, geo, 1, 1, one) == -22 and lib.pleas_stream_plan_info(-1, geo, 1, 1, one) == -22
    # the launches themselves, refused before anything touches a device: the same words
    for call, message in ((lambda: lib.pleas_target_residual(8, 8, 8, 8, 8, 0, 0, 5, 5, 25, 1.0, 8, 8, ctypes.byref(ctypes.c_int()), None), "target_residual: shape"),
                          (lambda: lib.pleas_channel_sum(8, 0, 3, 4, 8, None), "channel_sum: empty tensor"),
                          (lambda: lib.pleas_bn_act(8, 8, 8, None, 8, 1 << 20, 1 << 12, 1, 1, None), "tensor too large"),
                          (lambda: lib.pleas_masked_adam(8, 8, None, 8, 8, -1, 1e-3, 0.9, 0.999, 1e-8, 1, None), "n < 0")):
        assert call() == -22 and message in lib.pleas_last_error().decode()


# ------------------------------------------------------------------------------------------------ the harness on the CPU
def _smallest(kernel, count=5):
    table = sc.KERNELS[kernel][0]
    order = sorted(range(len(table)), key=lambda i: sum(math.prod(s) for s in sc.tensors(kernel, table[i])))
    return [(i, table[i]) for i in order[:count]]


def _no_blank_cheque_map(bound, want):
    fin = torch.isfinite(want)
    assert (bound[fin] < 1e-4 * (want[fin].abs() + 1)).all()


def test_merge_reference_is_the_definition_and_never_reads_a_planted_row():
    for i, c in _smallest("merge_blocks", 8):
        w1, w2, r1, r2, c1, c2 = sr.merge_inputs(c, sc.seed("merge_blocks", i))
        a = c["axis"]
        want = sr.merge_ref(w1, w2, r1, r2, c1, c2, c["merged"], a)
        assert not torch.isnan(want).any() and torch.isnan(w1).any() and torch.isnan(w2).any(), c
        outer = math.prod(c["shape"][:a])
        cols = c["cols"] if c["cols"] is not None else 1
        v1, v2 = (w.reshape(outer, c["shape"][a], -1 if c["cols"] is None else c["shape"][a + 1], *([] if c["cols"] is None else [-1])) for w in (w1, w2))
        got = want.reshape(outer, c["rows"], cols, -1)
        for o in range(outer):
            for r in range(c["rows"]):
                for j in range(cols):
                    j1, j2 = (int(c1[j]), int(c2[j])) if c["cols"] is not None else (0, 0)
                    e = torch.zeros(got.shape[3])
                    if r1[r] >= 0 and j1 >= 0:
                        e = e + (v1[o, r1[r], j1] if c["cols"] is not None else v1[o, r1[r]])
                    if r2[r] >= 0 and j2 >= 0:
                        e = e + (v2[o, r2[r], j2] if c["cols"] is not None else v2[o, r2[r]])
                    assert torch.equal(got[o, r, j], e * (0.5 if r < c["merged"] else 1.0)), (c, o, r, j)


def test_plain_fp32_affine_maps_on_the_cpu_lie_inside_the_bounds():
    for i, c in _smallest("bn_act"):
        x, res, scale, shift = sr.bn_act_inputs(c, sc.seed("bn_act", i))
        n = x.shape[0] // c["batches"]
        a = scale.repeat_interleave(n, 0).view(x.shape[0], -1, 1, 1)
        b = shift.repeat_interleave(n, 0).view(x.shape[0], -1, 1, 1)
        bn32 = x * a + b
        bn, sm, act, bound_bn, bound_sum = sr.bn_chain_ref(x, scale, shift, res, True)
        assert not sr.finite_close(bn32, bn, bound_bn).any() and not sr.finite_close(bn32 + res, sm, bound_sum).any(), c
        assert not sr.finite_close(torch.relu(bn32 + res), act, bound_sum).any(), c
        _no_blank_cheque_map(bound_bn, bn)
        _no_blank_cheque_map(bound_sum, sm)
    for i, c in _smallest("bn_act_maxpool"):
        x, scale, shift = sr.pool_inputs(c, sc.seed("bn_act_maxpool", i))
        want, bound = sr.pool_ref(x, scale, shift, c)
        act = x * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1) if c["scale"] else x
        got = F.max_pool2d(torch.relu(act) if c["relu"] else act, c["k"], c["stride"], c["pad"])
        assert got.shape == want.shape == sc.pool_out(c) and not sr.finite_close(got, want, bound).any(), c
        assert torch.equal(torch.isnan(got), torch.isnan(want))
        _no_blank_cheque_map(bound, want)


def test_torch_adam_in_fp32_lies_inside_the_measured_bound():
    for i, c in enumerate(sc.MASKED_ADAM):
        p64, lr_sum, pt, _ = sr.adam_ref(c, sr.ADAM_SEED + i)
        bound = sr.adam_bound(p64, lr_sum)
        ratio = float(((pt.double() - p64).abs() / (p64.abs() + lr_sum)).max())
        assert ratio <= sr.ADAM_FP32_VS_FP64, (c, ratio)          # the stored constant is the measured maximum
        assert ((pt.double() - p64).abs() <= bound).all() and (bound < 1e-4 * (p64.abs() + 1)).all()
        assert sr.ADAM_FACTOR == 4


def test_plain_fp32_sums_on_the_cpu_lie_inside_the_bounds():
    for i, c in _smallest("sqerr"):
        a, b, base = sr.sqerr_inputs(c, sc.seed("sqerr", i))
        base = base if c["accumulate"] else 0.0
        scale = 1.0 / c["n"]
        want, bound = sr.sqerr_ref(a, b, scale, base, sc.plan("sqerr", c)[0]["sweeps"])
        got = float(torch.tensor(base) + ((a - b) ** 2).sum() * scale)
        total = float(((a.double() - b.double()) ** 2).sum())
        assert abs(got - want) <= bound and bound < 1e-3 * (scale * total + abs(base)) + 2 * sr.TINY, (c, got, want, bound)
    for i, c in _smallest("target_residual"):
        info = sc.plan("target_residual", c)[0]
        assert info["sweeps"] == 1
        out, o1, o2, r1, r2, merged = sr.target_inputs(c, sc.seed("target_residual", i))
        t32 = sr.merge_ref(o1, o2, r1, r2, None, None, merged, 1)
        d32 = out - t32
        assert not torch.isnan(d32).any()
        d64 = out.double() - sr.merge_ref(o1.double(), o2.double(), r1, r2, None, None, merged, 1)
        want, bound = sr.target_partials_ref(d64, info["vec"], info["blocks"], 1)
        got = torch.stack([blk.sum() for blk in (d32 * d32).flatten().split(256 * info["vec"])])
        assert got.numel() == info["blocks"] and ((got.double() - want).abs() <= bound).all(), c
        assert (bound < 1e-3 * want + 2 * sr.TINY).all()
    for i, c in _smallest("channel_sum"):
        info = sc.plan("channel_sum", c)[0]
        x = torch.randn(c["shape"], generator=sr.gen(sc.seed("channel_sum", i))) + 0.25
        want, bound = sr.channel_sum_ref(x, info["vec"], info["sweeps"])
        got = x.reshape(x.shape[0], x.shape[1], -1).sum((0, 2))
        assert ((got.double() - want).abs() <= bound).all(), c
        assert (bound < 1e-3 * x.double().abs().reshape(x.shape[0], x.shape[1], -1).sum((0, 2)) + 2 * sr.TINY).all()
    for i, c in _smallest("pool_gather"):
        x, src = sr.pool_gather_inputs(c, sc.seed("pool_gather", i))
        want, bound = sr.pool_gather_ref(x, src, sc.plan("pool_gather", c)[0]["vec"])
        got = (x if src is None else x[:, src.long()]).mean(2)
        assert got.shape == want.shape and ((got.double() - want).abs() <= bound).all(), c
        assert (bound < 1e-3 * (x if src is None else x[:, src.long()]).double().abs().sum(2) + 2 * sr.TINY).all()


def test_top1_inputs_follow_argmax_rules():
    """The first maximal index, a NaN is maximal: the rule restated as a loop, on the planted rows."""
    for i, c in enumerate(sc.TOP1_COUNT[:5]):
        x, labels, arg = sr.top1_inputs(c, sc.seed("top1_count", i))
        for n in range(min(c["N"], 8)):
            row = x[n].tolist()
            nans = [j for j, v in enumerate(row) if v != v]
            want = nans[0] if nans else row.index(max(row))
            assert int(arg[n]) == want, (c, n)
        hits = int((arg == labels).sum())
        assert {"right": hits == c["N"], "wrong": hits == 0, "mixed": 0 < hits < c["N"]}[c["labels"]], (c, hits)


def test_single_pass_fp64_statistics_on_the_cpu_lie_inside_the_fold_bounds():
    """bn_train_fold's stand-in on the CPU is its own algorithm, not an fp32 BatchNorm (the kernel sums in fp64, so its bound has
    no fp32 summation term): sum x and sum x^2 in fp64 in torch's order, var = E[x^2] - mean^2, the fold in fp64, ONE rounding
    to fp32; running statistics rounded after every batch.  Against the two-pass module chain in fp64 -- at a mean of 1e3 too."""
    table = sc.BN_TRAIN_FOLD
    picks = _smallest("bn_train_fold") + [(i, c) for i, c in enumerate(table) if c.get("mean") or c["batches"] > 1]
    for i, c in picks:
        x, bn = sr.bn_train_inputs(c, sc.seed("bn_train_fold", i))
        ref = sr.bn_train_ref(x, bn, c["batches"])
        C = x.shape[1]
        rm = bn.running_mean.clone().double() if c["track"] else None
        rv = bn.running_var.clone().double() if c["track"] else None
        seen = int(bn.num_batches_tracked) if c["track"] else 0
        for bt, xb in enumerate(x.double().chunk(c["batches"])):
            cnt = xb.numel() // C
            mean = xb.sum((0, 2, 3)) / cnt
            var = ((xb * xb).sum((0, 2, 3)) / cnt - mean * mean).clamp_min(0)
            g = bn.weight.double() if c["affine"] else torch.ones(C, dtype=torch.float64)
            b = bn.bias.double() if c["affine"] else torch.zeros(C, dtype=torch.float64)
            sc64 = g / torch.sqrt(var + bn.eps)
            scale, shift = sc64.float(), (b - mean * sc64).float()
            assert ((scale.double() - ref["scale"][bt]).abs() <= ref["bound_scale"][bt]).all(), (c, bt)
            assert ((shift.double() - ref["shift"][bt]).abs() <= ref["bound_shift"][bt]).all(), (c, bt)
            assert (ref["bound_scale"][bt] < 1e-4 * (ref["scale"][bt].abs() + 1)).all()
            assert (ref["bound_shift"][bt] < 1e-4 * (ref["shift"][bt].abs() + 1)).all()
            if c["track"]:
                f = c["momentum"] if c["momentum"] is not None else 1.0 / (seen + bt + 1)
                rm = ((1 - f) * rm + f * mean).float().double()
                rv = ((1 - f) * rv + f * var * cnt / (cnt - 1)).float().double()
        if c["track"]:
            assert ((rm - ref["running_mean"]).abs() <= ref["bound_rm"]).all() and ((rv - ref["running_var"]).abs() <= ref["bound_rv"]).all(), c
            assert (ref["bound_rm"] < 1e-4 * (ref["running_mean"].abs() + 1)).all() and (ref["bound_rv"] < 1e-4 * (ref["running_var"].abs() + 1)).all()
            assert ref["counter"] == seen + c["batches"]
