"""fp64 references and derived per-element bounds of the matching contraction and the normal equations, on whatever device the
operands live (tests/test_contraction_coverage.py checks them against plain fp32 on the CPU before anything runs on a GPU;
tests/test_hip_contraction_forms.py holds the kernels to them).

u = 2^-24, gamma_n = n u / (1 - n u): any fp32 summation order of n terms satisfies |got - want| <= gamma_n * sum |terms|
(Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).  Nothing here is measured.

* Gram, inner product: gamma_n * sum |x||y| + u |base|, n = K + S + nodes_in_group + 1 (slab adds and group adds are summands).
* Gram, negative distance: E = gamma_(K+S+3) * (Nx_i + Ny_j + 2 sum |x||y|) bounds the squared distance's error; then
  |got - want| <= min(sqrt(E), E / |want|) + 2u |want| per node, because |sqrt(max(a, 0)) - sqrt(b)| <= min(sqrt|a - b|,
  |a - b| / sqrt(b)); summed over the nodes of a group.
* Derived nodes (x' = ax x + bx, y' = ay y + by per channel): the same rules term by term on
  ax ay G + ax by Sx + bx ay Sy + K bx by and on the norms ax^2 Nx + 2 ax bx Sx + K bx^2: every fp32 sum carries gamma times its
  absolute-value sum, the fp64 combination adds nothing worth counting.  The reference is fp64 on the transformed tensors.
* Normal equations: gamma_n * sum |u_i||u_j| + u |base|, n = reps * (Ktot + S + 1), over the lower block tiles."""
import torch
import torch.nn.functional as F

from test_hip_tile_forms import U, gamma


def gamma_n(n):
    """gamma_n proper (test_hip_tile_forms.gamma counts two more summands than it is given)."""
    return gamma(n - 2)


# ------------------------------------------------------------------------------------------------ matching contraction
def gram_operands(shape, seed, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    y = 0.7 * x + 0.5 * torch.randn(shape, generator=g)
    return x.to(device), y.to(device)


def gram_affine(C, seed, device="cpu"):
    """(scale_x, shift_x, scale_y, shift_y) of a derived node: scales of either sign away from zero."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(2):
        s = (0.5 + torch.rand(C, generator=g)) * (1 - 2 * (torch.rand(C, generator=g) < 0.3).float())
        out += [s.to(device), (0.5 * torch.randn(C, generator=g)).to(device)]
    return tuple(out)


def _rows(t):
    """[B][C][...] -> fp64 [C][B * HW]: a channel's whole K axis in one row."""
    return t.reshape(t.shape[0], t.shape[1], -1).double().permute(1, 0, 2).reshape(t.shape[1], -1)


def gram_node_ref(x, y, affine=None):
    """fp64 facts of one node along axis 1: G = <x_i, y_j>, the squared norms Nx / Ny, and the absolute-value sums its bounds
    need: T (of the inner product's terms), Ax / Ay (of the norms' terms).  With ``affine`` the node is the derived image."""
    xd, yd = _rows(x), _rows(y)
    K = xd.shape[1]
    ein = lambda a, b: a @ b.t()
    if affine is None:
        Nx, Ny = (xd * xd).sum(1), (yd * yd).sum(1)
        return dict(K=K, G=ein(xd, yd), T=ein(xd.abs(), yd.abs()), Nx=Nx, Ny=Ny, Ax=Nx, Ay=Ny)
    ax, bx, ay, by = (v.double() for v in affine)
    xt, yt = ax[:, None] * xd + bx[:, None], ay[:, None] * yd + by[:, None]
    sxa, sya = xd.abs().sum(1), yd.abs().sum(1)
    T = (ax.abs()[:, None] * ay.abs()[None, :] * ein(xd.abs(), yd.abs()) + (ax.abs() * sxa)[:, None] * by.abs()[None, :]
         + bx.abs()[:, None] * (ay.abs() * sya)[None, :] + K * bx.abs()[:, None] * by.abs()[None, :])
    Ax = ax * ax * (xd * xd).sum(1) + 2 * (ax * bx).abs() * sxa + K * bx * bx
    Ay = ay * ay * (yd * yd).sum(1) + 2 * (ay * by).abs() * sya + K * by * by
    return dict(K=K, G=ein(xt, yt), T=T, Nx=(xt * xt).sum(1), Ny=(yt * yt).sum(1), Ax=Ax, Ay=Ay)


def gram_group_ref(refs, slabs, cdist, base=None, product_bound=None):
    """(want, bound) of a group matrix: ``refs`` its nodes' gram_node_ref, ``slabs`` the S each went through (a derived node:
    its source's), ``base`` what the matrix held under accumulate.  ``product_bound[i]``: a constant that replaces gamma on
    node i's products (the six-product arithmetic) or, as ``(constant, True)``, caps it (the nine-product one); None: the exact
    arithmetic's gamma alone."""
    nodes = len(refs)
    want = torch.zeros_like(refs[0]["G"])
    bound = torch.zeros_like(want)
    for i, (r, S) in enumerate(zip(refs, slabs)):
        pb = None if product_bound is None else product_bound[i]
        coef = lambda g: g if pb is None else (min(g, pb[0]) if pb[1] else pb[0])
        if not cdist:
            want += r["G"]
            bound += coef(gamma_n(r["K"] + S + nodes + 1)) * r["T"]
            continue
        gam = gamma_n(r["K"] + S + 3)
        E = gam * (r["Ax"][:, None] + r["Ay"][None, :]) + 2 * coef(gam) * r["T"]
        w = -(r["Nx"][:, None] + r["Ny"][None, :] - 2 * r["G"]).clamp_min(0).sqrt()
        want += w
        bound += torch.minimum(E.sqrt(), E / w.abs()) + 2 * U * w.abs()       # E / 0 = inf: the square root stands
    if base is not None:
        want += base.double()
        bound += U * base.double().abs()
    return want, bound


# ------------------------------------------------------------------------------------------------ normal equations
def neq_unfold(ip, case):
    """U = im2col(ip) in fp64: rows = (sample, output pixel), columns kernel-position-major k = r * Cin + ci."""
    N, Cin, H, W, KH, KW, stride, pad = case
    cols = F.unfold(ip.double(), (KH, KW), 1, pad, stride)                                # N, (ci, r), L
    return cols.view(N, Cin, KH * KW, -1).permute(0, 3, 2, 1).reshape(-1, KH * KW * Cin)


def neq_ref(ip, case):
    """(U^T U, |U|^T |U|) in fp64."""
    Um = neq_unfold(ip, case)
    return Um.t() @ Um, Um.abs().t() @ Um.abs()


def neq_lower_tiles(case, device="cpu"):
    """Mask of the lower block tiles of A (64 / 128 wide inside every kernel-position block): what the kernels write."""
    N, Cin, H, W, KH, KW, stride, pad = case
    T = 128 if Cin > 64 else 64
    tiles = -(-Cin // T)
    idx = torch.arange(KH * KW * Cin, device=device)
    blk = (idx // Cin) * tiles + (idx % Cin) // T
    return blk[:, None] >= blk[None, :]


def neq_bound(Sabs, rows, S, reps, base=None):
    b = gamma_n(reps * (rows + S + 1)) * reps * Sabs
    return b if base is None else b + U * base.double().abs()
