"""The ``ws`` / ``ws_fresh`` protocol of the five grouped launches (``pleas_gram_batch``, ``pleas_merge_batch``,
``pleas_fwd_batch``, ``pleas_wgrad_batch``, ``pleas_normal_eq_accum``) as ``hip_ops`` drives it: one object used again on the same
list, on a list that needs more workspace (the library answers ``PLEAS_ENOMEM`` once, the object sizes its workspace again and
launches once more), on the first list again, through ``table()`` / ``relaunch`` with rewritten pointers, and next to a second
object of its class on the same stream.

Every comparison is ``torch.equal`` against a FRESH object of the same class on the same operands: the kernels are deterministic
by design, no tolerance is involved.  Outputs are filled with NaN before each launch; the normal equations accumulate
(``A += U^T U``), so their matrices start from zero instead.  The calls that reach the library are counted per symbol through a
proxy around ``hip_ops._lib.lib``.

Shapes are the smallest that take every branch: list A is two entries, list B is A plus one strictly larger entry (for the
convolution launches a layer whose pixel axis is cut into two K ranges, so that its plan carries slabs behind the tables).
"""
import collections

import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from pleas_merging_amd import hip_ops

    return hip_ops


class CountingLib:
    """``_lib.lib()`` with every call counted by symbol name."""

    def __init__(self, real):
        self._real = real
        self.calls = collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def counted(*args):
            self.calls[name] += 1
            return fn(*args)

        return counted


@pytest.fixture
def counted(ops, monkeypatch):
    proxy = CountingLib(ops._lib.lib())
    monkeypatch.setattr(ops._lib, "lib", lambda: proxy)
    return proxy


def _randn(g, *shape):
    return torch.randn(*shape, generator=g).cuda()


def _maps(c):
    return torch.arange(c, dtype=torch.int32, device="cuda"), torch.arange(c - 1, -1, -1, dtype=torch.int32, device="cuda")


# (N, Cout, Cin, H, W, k, pad, kernel-position-major); the third: N * H * W = 4096 pixels = 128 chunks of 32 -> two K ranges
LAYERS_A = [(2, 32, 32, 4, 4, 1, 0, False), (2, 32, 32, 4, 4, 3, 1, True)]
LAYERS_B = LAYERS_A + [(4, 32, 32, 32, 32, 1, 0, False)]


class Gram:
    ws_bytes, launch = "pleas_gram_batch_ws_bytes", "pleas_gram_batch"
    A = [(2, 32, 4, 4), (2, 32, 4, 4)]
    B = A + [(2, 32, 8, 8)]
    pointers = None

    def __init__(self, ops):
        self.ops = ops
        self.mat = torch.zeros(32, 32, device="cuda")
        self.obj = ops.GramBatch([self.mat], ops.EPI_NEG_CDIST)

    @staticmethod
    def operands(entries, seed):
        g = torch.Generator().manual_seed(seed)
        return [(_randn(g, *s), _randn(g, *s)) for s in entries]

    def add(self, data):
        for x, y in data:
            self.obj.add(x, y, 1, 0)

    def outputs(self, data):
        return [self.mat]

    def flush(self, data):
        self.obj.flush(accumulate=False)


class Merge:
    ws_bytes, launch = "pleas_merge_batch_ws_bytes", "pleas_merge_batch"
    A = [(2, 8, 4, 4), (2, 8, 4, 4)]
    B = A + [(4, 16, 8, 8)]
    pointers = ("w1", "w2")

    def __init__(self, ops):
        self.ops = ops
        self.obj = ops.MergeBatch(torch.device("cuda"))

    @staticmethod
    def operands(entries, seed):
        g = torch.Generator().manual_seed(seed)
        return [(_randn(g, *s), _randn(g, *s)) + _maps(s[1]) + (torch.empty(s, device="cuda"),) for s in entries]

    def add(self, data):
        for w1, w2, r1, r2, out in data:
            self.obj.add(w1, w2, 1, r1, r2, w1.shape[1], out=out)

    def outputs(self, data):
        return [d[4] for d in data]

    def flush(self, data):
        self.obj.flush()

    def relaunch(self, data):
        self.obj.relaunch()


class Fwd:
    ws_bytes, launch = "pleas_fwd_batch_ws_bytes", "pleas_fwd_batch"
    A, B = LAYERS_A, LAYERS_B
    pointers = ("ip", "o1")

    def __init__(self, ops):
        self.ops = ops
        self.obj = ops.FwdBatch(torch.device("cuda"))

    @staticmethod
    def operands(entries, seed):
        g = torch.Generator().manual_seed(seed)
        data = []
        for N, Cout, Cin, H, W, k, pad, kpos in entries:
            w = _randn(g, Cout, k, k, Cin) if kpos else _randn(g, Cout, Cin, k, k)
            data.append(dict(ip=_randn(g, N, Cin, H, W), w=w / (Cin * k * k) ** 0.5, bias=None if kpos else _randn(g, Cout),
                             o1=_randn(g, N, Cout, H, W), o2=_randn(g, N, Cout, H, W), maps=_maps(Cout),
                             resid=torch.empty(N, Cout, H, W, device="cuda"), geo=((k, k), 1, pad), kpos=kpos))
        data[0]["loss"] = torch.empty(len(entries), device="cuda")
        return data

    def add(self, data):
        for d in data:
            n = d["resid"].numel()
            self.obj.add(d["ip"], d["w"], d["bias"], d["o1"], d["o2"], *d["maps"], d["w"].shape[0], d["resid"], 2.0 / n, 1.0 / n,
                         *d["geo"], flags=self.ops.FwdBatch.KPOS_MAJOR if d["kpos"] else 0)

    def outputs(self, data):
        return [d["resid"] for d in data] + [data[0]["loss"]]

    def flush(self, data):
        self.obj.flush(data[0]["loss"])

    def relaunch(self, data):
        self.obj.relaunch(data[0]["loss"])


class Wgrad:
    ws_bytes, launch = "pleas_wgrad_batch_ws_bytes", "pleas_wgrad_batch"
    A, B = LAYERS_A, LAYERS_B
    pointers = ("resid", "ip")

    def __init__(self, ops):
        self.ops = ops
        self.obj = ops.WgradBatch(torch.device("cuda"))

    @staticmethod
    def operands(entries, seed):
        g = torch.Generator().manual_seed(seed)
        return [dict(resid=_randn(g, N, Cout, H, W), ip=_randn(g, N, Cin, H, W),
                     grad=torch.empty((Cout, k, k, Cin) if kpos else (Cout, Cin, k, k), device="cuda"), geo=((k, k), 1, pad), kpos=kpos)
                for N, Cout, Cin, H, W, k, pad, kpos in entries]

    def add(self, data):
        for d in data:
            self.obj.add(d["resid"], d["ip"], d["grad"], *d["geo"], flags=self.ops.WgradBatch.KPOS_MAJOR if d["kpos"] else 0)

    def outputs(self, data):
        return [d["grad"] for d in data]

    def flush(self, data):
        self.obj.flush()

    def relaunch(self, data):
        self.obj.relaunch()


class NormalEq:
    ws_bytes, launch = "pleas_normal_eq_ws_bytes", "pleas_normal_eq_accum"
    A, B = LAYERS_A, LAYERS_B
    pointers = None
    fill = 0.0          # A += U^T U: the matrices cannot start from NaN

    def __init__(self, ops):
        self.ops = ops
        self.obj = ops.NormalEqBatch(torch.device("cuda"))

    @staticmethod
    def operands(entries, seed):
        g = torch.Generator().manual_seed(seed)
        return [dict(ip=_randn(g, N, Cin, H, W), A=torch.empty(k * k * Cin, k * k * Cin, device="cuda"), geo=((k, k), 1, pad))
                for N, Cout, Cin, H, W, k, pad, kpos in entries]

    def add(self, data):
        for d in data:
            self.obj.add(d["ip"], d["A"], *d["geo"])

    def outputs(self, data):
        return [d["A"] for d in data]

    def flush(self, data):
        self.obj.flush()


KINDS = [Gram, Merge, Fwd, Wgrad, NormalEq]
REPLAYED = [Merge, Fwd, Wgrad]


def run(driver, data, how="flush"):
    """One launch of ``driver``'s object on ``data`` into poisoned outputs; returns copies of the outputs."""
    outs = driver.outputs(data)
    for o in outs:
        o.fill_(getattr(driver, "fill", NAN))
    if how == "flush":
        driver.add(data)
        driver.flush(data)
    else:
        driver.relaunch(data)
    return [o.clone() for o in outs]


_CASES = {}


def case(ops, kind, which, seed):
    """Operands of list ``which`` ("A" / "B") of ``kind`` drawn from ``seed``, and what a fresh object makes of them (computed once
    per module and left unchanged)."""
    key = (kind, which, seed)
    if key not in _CASES:
        data = kind.operands(getattr(kind, which), seed)
        want = run(kind(ops), data)
        assert all(bool(torch.isfinite(w).all()) for w in want), (kind.__name__, which)
        _CASES[key] = (data, want)
    return _CASES[key]


@pytest.fixture(scope="module", autouse=True)
def _cases_released():
    yield
    _CASES.clear()
    torch.cuda.empty_cache()


def same(got, want):
    return len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: k.__name__)
def test_one_object_over_repeat_regrow_and_return(ops, counted, kind):
    """A, A with new values, B (one ENOMEM answer, one new workspace, one more launch), A again: a fresh object's outputs each
    time; ``*_ws_bytes`` once per workspace, the launch once per flush plus once for the regrow."""
    steps = [case(ops, kind, "A", 1), case(ops, kind, "A", 2), case(ops, kind, "B", 3), case(ops, kind, "A", 4)]
    counted.calls.clear()           # the fresh objects behind the references are not what is counted
    driver = kind(ops)
    for n, (data, want) in enumerate(steps):
        assert same(run(driver, data), want), (kind.__name__, "step %d" % n)
    assert counted.calls[kind.ws_bytes] == 2, dict(counted.calls)
    assert counted.calls[kind.launch] == len(steps) + 1, dict(counted.calls)


@pytest.mark.parametrize("kind", REPLAYED, ids=lambda k: k.__name__)
def test_relaunch_needs_a_flush_and_follows_rewritten_pointers(ops, counted, kind):
    first, _ = case(ops, kind, "A", 1)
    other, want_other = case(ops, kind, "A", 2)
    driver = kind(ops)
    with pytest.raises(ops.PleasHipError):      # nothing flushed yet
        driver.relaunch(first)
    pending = kind(ops)
    pending.add(first)
    with pytest.raises(ops.PleasHipError):      # entries pending
        pending.relaunch(first)
    run(driver, first)
    counted.calls.clear()
    table = driver.obj.table()
    assert len(table) == len(first)
    # `other`'s inputs, outputs still `first`'s: rewrite the pointer columns that differ between the two operand sets
    if kind is Merge:
        table["w1"][:] = [d[0].data_ptr() for d in other]
        table["w2"][:] = [d[1].data_ptr() for d in other]
    elif kind is Fwd:
        for col in ("ip", "w", "o1", "o2"):
            table[col][:] = [d[col].data_ptr() for d in other]
        table["bias"][:] = [d["bias"].data_ptr() if d["bias"] is not None else 0 for d in other]
    else:
        for col in ("resid", "ip"):
            table[col][:] = [d[col].data_ptr() for d in other]
    assert same(run(driver, first, how="relaunch"), want_other)
    assert counted.calls[kind.launch] == 1 and counted.calls[kind.ws_bytes] == 0, dict(counted.calls)


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: k.__name__)
def test_two_objects_alternate_on_one_stream(ops, kind):
    """Each object has its own workspace and finds its own plan again: outputs as in its solo run, turn after turn."""
    (data1, want1), (data2, want2) = case(ops, kind, "A", 1), case(ops, kind, "B", 3)
    one, two = kind(ops), kind(ops)
    for turn in range(3):
        assert same(run(one, data1), want1), (kind.__name__, "first object, turn %d" % turn)
        assert same(run(two, data2), want2), (kind.__name__, "second object, turn %d" % turn)
