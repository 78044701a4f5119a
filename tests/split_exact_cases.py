"""Operands on which only an arithmetic with EXACT fp32 products reproduces the true result bit for bit: the cases of
tests/test_hip_split_exact.py (GPU) and their preconditions (tests/test_arith_exact_host.py, CPU).  Plain torch on the CPU.

Along the contraction axis entries come in adjacent pairs (2j, 2j + 1).  With v = h1 + h2 + h3 the three-plane bf16 split of
the contraction kernels (csrc/common.hpp: each plane the round-to-nearest-even bf16 of what the previous ones left):

* x[2j] is a random-sign integer in [2^17, 2^18), x[2j + 1] = -(h1 + h2) of x[2j], whose planes are (-h1, -h2, 0);
* both meet the same multiplier w, a random-sign integer in [2^8, 2^9): w3 = 0 and w2 in {-1, 0, 1}.

Every dot product is then sum x3 * w: a small integer, every partial sum exactly representable.  Nine bf16 products per fp32
product give exactly that; six leave out x3 * w2; an fmaf chain rounds the 27-bit products."""
import torch
import torch.nn.functional as F


def planes(v):
    """(h1, h2, h3) of fp32 `v`, as floats: the split of csrc/common.hpp (split3_pair), round-to-nearest-even through torch.bfloat16."""
    v = v.float()
    h1 = v.bfloat16().float()
    r1 = v - h1
    h2 = r1.bfloat16().float()
    h3 = (r1 - h2).bfloat16().float()
    return h1, h2, h3


def _signed_ints(shape, lo, hi, g):
    return (torch.randint(lo, hi, shape, generator=g) * (2 * torch.randint(0, 2, shape, generator=g) - 1)).float()


def paired(rows, K, g):
    """[rows][K] with the pairs along the last axis.  An entry whose partner's planes are not (-h1, -h2, 0) -- a round-to-even tie
    of h1 + h2 -- is drawn again until every entry holds."""
    assert K % 2 == 0
    even = _signed_ints((rows, K // 2), 1 << 17, 1 << 18, g)
    while True:
        h1, h2, _ = planes(even)
        odd = -(h1 + h2)
        o1, o2, o3 = planes(odd)
        bad = ~((o1 == -h1) & (o2 == -h2) & (o3 == 0))
        if not bool(bad.any()):
            break
        even[bad] = _signed_ints((int(bad.sum()),), 1 << 17, 1 << 18, g)
    return torch.stack([even, odd], -1).reshape(rows, K)


def multipliers(rows, K, g):
    """[rows][K], both entries of a pair equal."""
    return _signed_ints((rows, K // 2), 1 << 8, 1 << 9, g).repeat_interleave(2, dim=1)


def _conv_case(N, Cin, H, W, Cout, k, seed):
    g = torch.Generator().manual_seed(seed)
    x = paired(N * H * W, Cin, g).reshape(N, H, W, Cin).permute(0, 3, 1, 2).contiguous()             # pairs along channels
    w = multipliers(Cout * k * k, Cin, g).reshape(Cout, k, k, Cin).permute(0, 3, 1, 2).contiguous()
    op = lambda a, b: F.conv2d(a.double(), b.double(), None, 1, k // 2)
    return dict(kind="conv2d", name="conv2d %dx%d Cin %d Cout %d" % (k, k, Cin, Cout), geo=(N, Cin, H, W, Cout, k), x=x, w=w, op=op)


def _wgrad_case(N, Cout, Cin, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    P = N * H * W                                                                                     # pairs along pixels
    resid = paired(Cout, P, g).reshape(Cout, N, H, W).permute(1, 0, 2, 3).contiguous()
    ip = multipliers(Cin, P, g).reshape(Cin, N, H, W).permute(1, 0, 2, 3).contiguous()
    op = lambda a, b: torch.einsum("nohw,nihw->oi", a.double(), b.double())[:, :, None, None]
    return dict(kind="wgrad", name="wgrad 1x1 Cout %d Cin %d" % (Cout, Cin), geo=(N, Cout, Cin, H, W), x=resid, w=ip, op=op)


def _gram_case(N, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    P = N * H * W
    x = paired(C, P, g).reshape(C, N, H, W).permute(1, 0, 2, 3).contiguous()
    y = multipliers(C, P, g).reshape(C, N, H, W).permute(1, 0, 2, 3).contiguous()
    op = lambda a, b: torch.einsum("nihw,njhw->ij", a.double(), b.double())
    return dict(kind="gram", name="gram C %d" % C, geo=(N, C, H, W), x=x, w=y, op=op)


_CASES = None


def cases():
    """The cases, built once: 1 x 1 convolutions with Cin 32 / 64 and 3 x 3 with Cin 32 (three 8 x 8 images: two pixel tiles,
    the second ragged), each with Cout 48 / 136 (64- / 128-row tiles, ragged); the weight gradient of a 1 x 1 layer and the
    matching contraction over N * HW = 128 pixels.  `want` = op(x, w) in fp64."""
    global _CASES
    if _CASES is None:
        out = []
        for k, Cin in ((1, 32), (1, 64), (3, 32)):
            for Cout in (48, 136):
                out.append(_conv_case(3, Cin, 8, 8, Cout, k, 1000 + 100 * k + Cin + Cout))
        out.append(_wgrad_case(2, 136, 48, 8, 8, 2001))
        out.append(_wgrad_case(2, 48, 136, 8, 8, 2002))
        out.append(_gram_case(2, 64, 8, 8, 3001))
        out.append(_gram_case(2, 132, 8, 8, 3002))
        for c in out:
            c["want"] = c["op"](c["x"], c["w"])
        _CASES = out
    return _CASES
