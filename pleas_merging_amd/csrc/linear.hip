// An nn.Linear's forward and its bias gradient on gfx950 (MI355X).
//
//   y[n][c]  = bias[c] + sum_k x[n][k] * w[c][k]         pleas_linear_fwd   (fp32 MFMA, exact-fp32 products)
//   out[c]   = sum_n x[n][c]                             pleas_column_sum
//
// Replaces: the `fc(feats)` of the linear probe's step and of the merged model's classifier (pleas/methods/pleas_merging.py:499-570,
// :469-496) where the library ran them through pleas_conv2d_fwd with H = W = KH = KW = 1: a convolution tile on one pixel per
// sample, a handful of workgroups walking K = 2048 each.
//
// Both operands are K-contiguous: the NT contraction of nt_tile.hpp with samples on the A axis (whose accumulator rows are
// spread over registers) and classes on the B axis (lane-contiguous), so a wave's stores to y are 128-byte runs along c.  One
// tile form: 64 x 64 outputs, K chunk 32, 256 threads.  The head's shapes give 4 to 16 such tiles, so K is cut into S ranges of
// whole chunks; a work item (sample tile, class tile, K range) writes its partial tile to slab s of the caller's workspace
// [S][N][C], and a second grid adds the slabs in slab order, then the bias.  S == 1: the tile writes y itself.  No atomics:
// the same call gives the same bits.
//
// Arithmetic: exact fp32 MFMA under every pleas_arith mode -- the switch does not reach this file (launch-latency-sized work:
// 0.05 to 0.2 GFLOP; a split image would buy nothing).
#include "nt_tile.hpp"

namespace pleas {

constexpr int kLinTile = 64;
constexpr int kLinTargetBlocks = 512;      // split K: about two workgroups per CU (256 CUs) ...
constexpr int kLinMinChunks = 2;           // ... of at least two chunks each (gram.hip's rule)

struct LinPlan {
    int tiles_n, tiles_c, nchunks, cps, S, last;      // cps: chunks per range; last: chunks of range S - 1
    size_t ws_bytes;
};

// a pure function of (N, C, K): no range is empty, the ranges tile [0, nchunks)
static LinPlan lin_plan(int64_t N, int C, int K) {
    LinPlan p;
    p.tiles_n = (int)ceil_div(N, kLinTile);
    p.tiles_c = (int)ceil_div(C, kLinTile);
    p.nchunks = (int)ceil_div(K, kBK);
    const int64_t tiles = std::max<int64_t>((int64_t)p.tiles_n * p.tiles_c, 1);
    int64_t S = std::max<int64_t>(kLinTargetBlocks / tiles, 1);
    S = std::min<int64_t>(S, std::max(p.nchunks / kLinMinChunks, 1));
    p.cps = (int)ceil_div(p.nchunks, S);
    p.S = p.cps ? (int)ceil_div(p.nchunks, p.cps) : 1;
    p.last = p.nchunks - (p.S - 1) * p.cps;
    p.ws_bytes = p.S > 1 ? (size_t)p.S * (size_t)N * (size_t)C * sizeof(float) : 0;
    return p;
}

struct LinGeom {
    const float* x;        // [N][K]
    const float* w;        // [C][K]
    const float* bias;     // [C] or null
    float* out;            // S == 1: y [N][C];  else the slabs [S][N][C]
    int N, C, K;
    int tiles_c, tiles_n, cps, nchunks, S;
};

// One work item: output tile (tm, tn) over K chunks [c_begin, c_end).  VEC = 4: 16-byte loads (K % 4 == 0, both bases 16-byte
// aligned: a thread's four k lie inside K together or not at all); VEC = 1: 4-byte loads.
template <int VEC>
__device__ __forceinline__ void lin_tile(const LinGeom& g, float* smem, const int tm, const int tn, const int split, const int c_begin,
                                         const int c_end) {
    constexpr int TILE = kLinTile;
    constexpr int LANES_PER_ROW = kBK / VEC;         // 8 (16-B loads) or 32 (4-B loads)
    constexpr int ROWS_PER_PASS = kThreads / LANES_PER_ROW;
    constexpr int PASSES = TILE / ROWS_PER_PASS;
    float* As = smem;                         // [2][TILE][kLds]  x rows (samples)
    float* Bs = smem + 2 * TILE * kLds;       // [2][TILE][kLds]  w rows (classes)

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int i0 = tm * TILE, j0 = tn * TILE;
    const int srow = tid / LANES_PER_ROW, scol = (tid % LANES_PER_ROW) * VEC;

    f32x16 acc[1][1];
    nt_zero(acc);

    // loads are UNCONDITIONAL from clamped (always valid) addresses and masked when written to LDS; byte offsets
    // in 32 bits (the entry point refuses operands of 2^30 elements or more)
    unsigned rows_ok_a = 0, rows_ok_b = 0;
    uint32_t row_off_a[PASSES], row_off_b[PASSES];
#pragma unroll
    for (int q = 0; q < PASSES; ++q) {
        const int gi = i0 + srow + q * ROWS_PER_PASS, gj = j0 + srow + q * ROWS_PER_PASS;
        if (gi < g.N) rows_ok_a |= 1u << q;
        if (gj < g.C) rows_ok_b |= 1u << q;
        row_off_a[q] = 4u * ((uint32_t)min(gi, g.N - 1) * (uint32_t)g.K);
        row_off_b[q] = 4u * ((uint32_t)min(gj, g.C - 1) * (uint32_t)g.K);
    }
    const bool interior = i0 + TILE <= g.N && j0 + TILE <= g.C;      // every row of both operand tiles exists
    bool staged_kin = false, staged_full = false;
    float ra[PASSES][VEC], rb[PASSES][VEC];
    const char* xb = reinterpret_cast<const char*>(g.x);
    const char* wb = reinterpret_cast<const char*>(g.w);
    auto load_chunk = [&](int c) {
        const int k = c * kBK + scol;
        staged_kin = k < g.K;
        staged_full = (c + 1) * kBK <= g.K;
        const uint32_t koff = 4u * (uint32_t)(staged_kin ? k : 0);
#pragma unroll
        for (int q = 0; q < PASSES; ++q) {
            if constexpr (VEC == 4) {
                const f32x4 va = *(const __attribute__((address_space(1))) f32x4*)(xb + (row_off_a[q] + koff));
                const f32x4 vb = *(const __attribute__((address_space(1))) f32x4*)(wb + (row_off_b[q] + koff));
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    ra[q][e] = va[e];
                    rb[q][e] = vb[e];
                }
            } else {
                ra[q][0] = *(const __attribute__((address_space(1))) float*)(xb + (row_off_a[q] + koff));
                rb[q][0] = *(const __attribute__((address_space(1))) float*)(wb + (row_off_b[q] + koff));
            }
        }
    };
    auto store_chunk = [&](int buf) {
        float* a = As + buf * TILE * kLds;
        float* b = Bs + buf * TILE * kLds;
#pragma unroll
        for (int q = 0; q < PASSES; ++q) {
            const int row = srow + q * ROWS_PER_PASS;
            if (!(interior && staged_full)) {      // block-uniform: a tile inside the matrix on a chunk inside K needs no masking
                const bool oka = staged_kin && ((rows_ok_a >> q) & 1u);
                const bool okb = staged_kin && ((rows_ok_b >> q) & 1u);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    ra[q][e] = oka ? ra[q][e] : 0.f;
                    rb[q][e] = okb ? rb[q][e] : 0.f;
                }
            }
            if constexpr (VEC == 4) {
                *reinterpret_cast<f32x4*>(a + row * kLds + scol) = f32x4{ra[q][0], ra[q][1], ra[q][2], ra[q][3]};
                *reinterpret_cast<f32x4*>(b + row * kLds + scol) = f32x4{rb[q][0], rb[q][1], rb[q][2], rb[q][3]};
            } else {
                a[row * kLds + scol] = ra[q][0];
                b[row * kLds + scol] = rb[q][0];
            }
        }
    };
    nt_pipeline<0>(c_begin, c_end, load_chunk, store_chunk, [&](int buf) { nt_mma_fp32<TILE, TILE>(As, Bs, buf, acc); });

    // ---- the tile -> y (+ bias) when K is not split, else -> slab `split`.  For a fixed r lanes 0 .. 31 hold 32 consecutive
    // classes of one sample: 128-byte runs along c.  Rows and columns outside [N] x [C] are not stored.
    const bool direct = g.S == 1;
    gfloat* o = PLEAS_GLOBAL_W(g.out) + (direct ? (size_t)0 : (size_t)split * (size_t)g.N * (size_t)g.C);
    const int j = j0 + wn * (TILE / 2) + (lane & 31);
    if (j < g.C) {
        const float bj = direct && g.bias ? PLEAS_GLOBAL(g.bias)[j] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = i0 + wm * (TILE / 2) + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (i < g.N) o[(size_t)i * g.C + j] = acc[0][0][r] + bj;
        }
    }
}

// grid = class tiles x sample tiles x S (class tile fastest: the items of one sample tile and K range share their x rows)
template <int VEC>
__global__ __launch_bounds__(kThreads) void linear_fwd_tile_kernel(const LinGeom g) {
    __shared__ __attribute__((aligned(16))) float smem[4 * kLinTile * kLds];
    int bid = blockIdx.x;
    const int tn = bid % g.tiles_c;
    bid /= g.tiles_c;
    const int tm = bid % g.tiles_n;
    const int split = bid / g.tiles_n;
    const int c_begin = split * g.cps;
    lin_tile<VEC>(g, smem, tm, tn, split, c_begin, min(c_begin + g.cps, g.nchunks));
}

// y[idx] = ((slab 0 + slab 1) + ... + slab S-1) + bias: one thread per element, slab order
__global__ __launch_bounds__(256) void linear_fwd_reduce_kernel(const float* __restrict__ slabs, const float* __restrict__ bias,
                                                                float* __restrict__ y, uint32_t total, int C, int S) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= total) return;
    const float* p = slabs + idx;
    float v = p[0];
    int s = 1;
    for (; s + 3 < S; s += 4) {      // four loads in flight, added in slab order
        const float v0 = p[(size_t)s * total], v1 = p[(size_t)(s + 1) * total], v2 = p[(size_t)(s + 2) * total],
                    v3 = p[(size_t)(s + 3) * total];
        v = (((v + v0) + v1) + v2) + v3;
    }
    for (; s < S; ++s) v += p[(size_t)s * total];
    if (bias) v += bias[idx % (uint32_t)C];
    y[idx] = v;
}

// Row-parallel column sums.  A workgroup owns 32 columns: thread (stripe, col) = (tid / 32, tid % 32) adds rows stripe, stripe + 32,
// ... of its column in increasing n (a wave reads two 128-byte runs per step), then the first 32 threads add the 32 stripes of
// their column in stripe order.  Fixed order, no atomics.
constexpr int kColSumCols = 32, kColSumStripes = 32;
__global__ __launch_bounds__(kColSumCols * kColSumStripes) void column_sum_kernel(const float* __restrict__ x, uint32_t N, uint32_t C,
                                                                                 float* __restrict__ out) {
    __shared__ float part[kColSumStripes][kColSumCols + 1];
    const uint32_t col = threadIdx.x % kColSumCols, stripe = threadIdx.x / kColSumCols;
    const uint32_t c = blockIdx.x * kColSumCols + col;
    const uint32_t cc = min(c, C - 1);      // clamped: loads stay unconditional, the column past C is not stored
    float s = 0.f;
    uint32_t n = stripe;
    for (; n + 3 * kColSumStripes < N; n += 4 * kColSumStripes) {      // four loads in flight, added in increasing n
        const float v0 = x[n * C + cc], v1 = x[(n + kColSumStripes) * C + cc], v2 = x[(n + 2 * kColSumStripes) * C + cc],
                    v3 = x[(n + 3 * kColSumStripes) * C + cc];
        s = (((s + v0) + v1) + v2) + v3;
    }
    for (; n < N; n += kColSumStripes) s += x[n * C + cc];
    part[stripe][col] = s;
    __syncthreads();
    if (stripe == 0 && c < C) {
        float t = part[0][col];
#pragma unroll
        for (int q = 1; q < kColSumStripes; ++q) t += part[q][col];
        out[c] = t;
    }
}

static int lin_check_sizes(const char* what, int64_t N, int C, int K) {
    if (N < 0 || C < 0 || K < 0) return bad_arg(what);
    if (N >= (1ll << 30) || N * (int64_t)K >= (1ll << 30) || (int64_t)C * K >= (1ll << 30) || N * (int64_t)C >= (1ll << 30))
        return bad_arg("linear: x, w and y must each hold fewer than 2^30 elements");
    return PLEAS_OK;
}

}  // namespace pleas

using namespace pleas;

extern "C" size_t pleas_linear_ws_bytes(int64_t N, int C, int K) {
    if (lin_check_sizes("linear_ws_bytes: negative size", N, C, K) != PLEAS_OK) return 0;
    return lin_plan(N, C, K).ws_bytes;
}

extern "C" int pleas_linear_plan_info(int64_t N, int C, int K, int* info) {
    if (!info) return bad_arg("linear_plan_info: null pointer");
    if (const int rc = lin_check_sizes("linear_plan_info: negative size", N, C, K); rc != PLEAS_OK) return rc;
    const LinPlan p = lin_plan(N, C, K);
    info[0] = p.tiles_n;
    info[1] = p.tiles_c;
    info[2] = p.S;
    info[3] = p.cps;
    info[4] = p.last;
    return PLEAS_OK;
}

extern "C" int pleas_linear_fwd(const float* x, const float* w, const float* bias, float* y, int64_t N, int C, int K, void* ws,
                                size_t ws_bytes, void* stream_) {
    if (const int rc = lin_check_sizes("linear_fwd: negative size", N, C, K); rc != PLEAS_OK) return rc;
    if (N == 0 || C == 0) return PLEAS_OK;      // nothing to write
    if (!y || (K > 0 && (!x || !w))) return bad_arg("linear_fwd: null tensor pointer");
    const LinPlan p = lin_plan(N, C, K);
    if (p.S > 1 && (!ws || ws_bytes < p.ws_bytes)) return workspace_too_small("linear_fwd", p.ws_bytes);
    hipStream_t stream = (hipStream_t)stream_;
    LinGeom g;
    g.x = x;
    g.w = w;
    g.bias = bias;
    g.out = p.S > 1 ? (float*)ws : y;
    g.N = (int)N;
    g.C = C;
    g.K = K;
    g.tiles_c = p.tiles_c;
    g.tiles_n = p.tiles_n;
    g.cps = p.cps;
    g.nchunks = p.nchunks;
    g.S = p.S;
    const dim3 grid((unsigned)((int64_t)p.tiles_c * p.tiles_n * p.S));
    if (K % 4 == 0 && (((uintptr_t)x | (uintptr_t)w) & 15) == 0)
        hipLaunchKernelGGL(linear_fwd_tile_kernel<4>, grid, dim3(kThreads), 0, stream, g);
    else
        hipLaunchKernelGGL(linear_fwd_tile_kernel<1>, grid, dim3(kThreads), 0, stream, g);
    PLEAS_LAUNCH_CHECK("linear_fwd_tile_kernel");
    if (p.S > 1) {
        const uint32_t total = (uint32_t)(N * C);
        hipLaunchKernelGGL(linear_fwd_reduce_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, stream, (const float*)ws, bias,
                           y, total, C, p.S);
        PLEAS_LAUNCH_CHECK("linear_fwd_reduce_kernel");
    }
    return PLEAS_OK;
}

extern "C" int pleas_column_sum(const float* x, int64_t N, int C, float* out, void* stream_) {
    if (!x || !out) return bad_arg("column_sum: null pointer");
    if (N <= 0 || C <= 0) return bad_arg("column_sum: empty tensor");
    if (N >= (1ll << 30) || N * (int64_t)C >= (1ll << 30)) return bad_arg("column_sum: N * C must stay below 2^30");
    hipLaunchKernelGGL(column_sum_kernel, dim3((unsigned)ceil_div(C, kColSumCols)), dim3(kColSumCols * kColSumStripes), 0,
                       (hipStream_t)stream_, x, (uint32_t)N, (uint32_t)C, out);
    PLEAS_LAUNCH_CHECK("column_sum_kernel");
    return PLEAS_OK;
}
