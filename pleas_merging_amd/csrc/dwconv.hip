// Depthwise convolutions (groups == channels) on gfx950 (MI355X): the plain / source-chain / inference forward, and the two
// grouped launches of the PLeaS fit of such layers.
//
//   y[n][c][oy][ox] = sum_{ky,kx} x[n][c][oy*s+ky-p][ox*s+kx-p] * w[c][0][ky][kx] (+ bias[c])      pleas_dwconv2d_fwd
//   z               = act(fma(y, scale[c], shift[c]) (+ res))                                       (same call, optional)
//   resid, loss     = dscale * (out - tgt),  loss_scale * sum (out - tgt)^2                         pleas_dw_fwd_batch
//   grad[c][ky][kx] = sum_{n,oy,ox} resid[n][c][oy][ox] * ip[n][c][oy*s+ky-p][ox*s+kx-p]            pleas_dw_wgrad_batch
//
// A depthwise layer has no contraction over channels: K*K multiply-adds per output, no MFMA, bound by HBM.  fp32 tensors, plain FMA,
// the same code under every pleas_arith mode (the switch does not reach this file).  No atomics; every output element is written
// once.  The fit's forward alone accumulates in fp64 (v_fma_f64, at K*K per 8 bytes of traffic still far from the ALU roof): its
// loss over M outputs is held to M * 2^-24 of the fp64 sum, and on a layer with ONE output that leaves no room for the roundings
// of an fp32 chain (measured: 1.4 * 2^-24 on a 3 x 3 layer with a single output pixel).
//
// Form.  A thread owns one output COLUMN ox of a strip of kDwRows = 4 output rows of one (n, c) plane: it walks the
// (kDwRows - 1) * s + K input rows of the strip once, K 4-byte loads per row, and every loaded row feeds the up to K / s output rows
// it lies under from registers.  Lanes run along ox first, then along the strips and planes (narrow maps still fill a wave), so a
// wave's loads and stores are contiguous 4-byte runs along a row whatever the row's width and alignment: rows of odd width need no
// special case.  The channel's K*K weights sit in registers (loads of one address per plane).  K (1, 3, 5, 7) and the stride (1, 2)
// are template parameters; the grouped kernels branch on them per workgroup.
//
// Summation orders (the same bits run after run, grouped or alone):
//   forward      per output: taps ky outer, kx inner, ascending, ONE fmaf chain from 0; taps outside the image are multiplied by 0
//                (the chain's value is unchanged); the bias is added last.  z is computed from that y exactly as pleas_bn_act does:
//                fmaf(y, scale, shift), then + res (or + 0), then max(., 0).
//   fwd_batch    out: the forward's chain and order in fp64 (fp32 operands: every product is exact there), as is all that follows:
//                d = out - (o1' + o2') * coef, resid = (float)(dscale * d) -- the only fp32 rounding of a residual --, and the squares:
//                per thread over its rows ascending, per wave by a
//                shuffle tree (offsets 32 .. 1), the workgroup's waves in wave order, the layer's workgroups by 64 stripes
//                (stripe t: partials t, t + 64, ... ascending) and the same shuffle tree; loss = (float)(loss_scale * sum).
//   wgrad_batch  stage one, per (channel, slab of kDwSlabOutputs / Wo rows of the N * Ho output rows): thread t adds the slab's
//                outputs t, t + 256, ... ascending into K*K fmaf chains, then the shuffle tree, then the 4 waves in wave order;
//                stage two adds the slabs of a (channel, tap) in slab order.  The slab split depends on the geometry alone.
#include <mutex>

#include "common.hpp"

namespace pleas {

constexpr int kDwThreads = 256;
constexpr int kDwRows = 4;                 // output rows of a strip
constexpr int kDwSlabOutputs = 2048;       // weight gradient: about this many outputs of a channel per slab
constexpr int kDwPtrBatch = 16;            // layers whose addresses ride in one launch of the pointer kernel
constexpr int kDwMaxPtrs = 8;

struct DwItem {          // one workgroup of a grouped launch
    int layer, local;
};

struct DwPtrs {
    const void* p[kDwMaxPtrs];
};
struct DwPtrBatch {
    int base, count;
    DwPtrs l[kDwPtrBatch];
};
__global__ void dw_set_ptrs_kernel(DwPtrs* table, const DwPtrBatch b) {
    const int t = threadIdx.x;
    if (t < b.count * kDwMaxPtrs) table[b.base + t / kDwMaxPtrs].p[t % kDwMaxPtrs] = b.l[t / kDwMaxPtrs].p[t % kDwMaxPtrs];
}

__device__ __forceinline__ float dw_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double dw_fma(double a, double b, double c) { return fma(a, b, c); }

// The strip's kDwRows chains: acc[r] = output (oy0 + r, ox) of the plane at xp, taps in (ky, kx) order.  Rows / columns outside the
// image contribute 0 * w; the address of such a tap is never formed into a load.
// T = float: fmaf chains (the forward); T = double: the same chains in fp64, where every fp32 product is exact (the fit's forward).
template <int K, int S, typename T>
__device__ __forceinline__ void dw_strip(const float* __restrict__ xp, const float* __restrict__ wc, const int Hin, const int Win,
                                         const int oy0, const int ox, const int pad, T (&acc)[kDwRows]) {
    T w[K * K];
#pragma unroll
    for (int t = 0; t < K * K; ++t) w[t] = (T)wc[t];
#pragma unroll
    for (int r = 0; r < kDwRows; ++r) acc[r] = (T)0;
    constexpr int IR = (kDwRows - 1) * S + K;
    const int iy0 = oy0 * S - pad, ix0 = ox * S - pad;
#pragma unroll
    for (int i = 0; i < IR; ++i) {
        const int iy = iy0 + i;
        const bool row_in = iy >= 0 && iy < Hin;
        T v[K];
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
            const int ix = ix0 + kx;
            v[kx] = (T)((row_in && ix >= 0 && ix < Win) ? xp[(size_t)iy * Win + ix] : 0.f);
        }
#pragma unroll
        for (int r = 0; r < kDwRows; ++r) {
            const int ky = i - r * S;       // compile-time after unrolling
            if (ky >= 0 && ky < K) {
#pragma unroll
                for (int kx = 0; kx < K; ++kx) acc[r] = dw_fma(v[kx], w[ky * K + kx], acc[r]);
            }
        }
    }
}

__device__ __forceinline__ void dw_strip_any(const int K, const int S, const float* xp, const float* wc, const int Hin, const int Win,
                                             const int oy0, const int ox, const int pad, double (&acc)[kDwRows]) {
    switch (K * 2 + S) {       // uniform per workgroup
        case 1 * 2 + 1: dw_strip<1, 1, double>(xp, wc, Hin, Win, oy0, ox, pad, acc); break;
        case 1 * 2 + 2: dw_strip<1, 2, double>(xp, wc, Hin, Win, oy0, ox, pad, acc); break;
        case 3 * 2 + 1: dw_strip<3, 1, double>(xp, wc, Hin, Win, oy0, ox, pad, acc); break;
        case 3 * 2 + 2: dw_strip<3, 2, double>(xp, wc, Hin, Win, oy0, ox, pad, acc); break;
        case 5 * 2 + 1: dw_strip<5, 1, double>(xp, wc, Hin, Win, oy0, ox, pad, acc); break;
        case 5 * 2 + 2: dw_strip<5, 2, double>(xp, wc, Hin, Win, oy0, ox, pad, acc); break;
        case 7 * 2 + 1: dw_strip<7, 1, double>(xp, wc, Hin, Win, oy0, ox, pad, acc); break;
        default: dw_strip<7, 2, double>(xp, wc, Hin, Win, oy0, ox, pad, acc); break;
    }
}

// ---------------------------------------------------------------------------------------------------------------- forward
struct DwFwdArgs {
    const float* x;
    const float* w;
    const float* bias;
    float* y;
    const float* scale;
    const float* shift;
    const float* res;
    float* z;
    int relu, C, Hin, Win, Ho, Wo, pad;
    uint32_t strips, items;      // strips per plane; items = planes * strips * Wo
};

template <int K, int S>
__global__ __launch_bounds__(kDwThreads) void dw_fwd_kernel(const DwFwdArgs a) {
    const uint32_t idx = blockIdx.x * (uint32_t)kDwThreads + threadIdx.x;
    if (idx >= a.items) return;
    const uint32_t ox = idx % (uint32_t)a.Wo, t = idx / (uint32_t)a.Wo;
    const uint32_t strip = t % a.strips, plane = t / a.strips;
    const int c = (int)(plane % (uint32_t)a.C), oy0 = (int)strip * kDwRows;
    float acc[kDwRows];
    dw_strip<K, S, float>(a.x + (size_t)plane * a.Hin * a.Win, a.w + (size_t)c * (K * K), a.Hin, a.Win, oy0, (int)ox, a.pad, acc);
    const float b = a.bias ? a.bias[c] : 0.f;
    const float sc = a.scale ? a.scale[c] : 0.f, sh = a.scale ? a.shift[c] : 0.f;
#pragma unroll
    for (int r = 0; r < kDwRows; ++r) {
        const int oy = oy0 + r;
        if (oy >= a.Ho) break;
        const size_t at = ((size_t)plane * a.Ho + oy) * a.Wo + ox;
        const float y = a.bias ? acc[r] + b : acc[r];
        if (a.y) a.y[at] = y;
        if (a.z) {
            const float bn = a.scale ? fmaf(y, sc, sh) : y;
            const float sm = bn + (a.res ? a.res[at] : 0.f);
            a.z[at] = a.relu == PLEAS_ACT_RELU6 ? relu6_keep_nan(sm) : a.relu ? fmaxf(sm, 0.f) : sm;
        }
    }
}

// geometry checks shared by every entry point; Ho / Wo out
static int dw_check_geometry(const char* who, int64_t N, int C, int Hin, int Win, int K, int stride, int pad, int& Ho, int& Wo) {
    char msg[160];
    auto fail = [&](const char* what) {
        std::snprintf(msg, sizeof(msg), "%s: %s", who, what);
        return bad_arg(msg);
    };
    if (N < 0 || C <= 0 || Hin <= 0 || Win <= 0) return fail("sizes must be positive");
    if (K < 1 || K > 7 || K % 2 == 0) return fail("the kernel must be odd and at most 7 x 7");
    if (stride != 1 && stride != 2) return fail("the stride must be 1 or 2");
    if (pad < 0 || pad > K / 2) return fail("the padding must lie in 0 .. K / 2");
    Ho = (Hin + 2 * pad - K) / stride + 1;
    Wo = (Win + 2 * pad - K) / stride + 1;
    if (Hin + 2 * pad < K || Win + 2 * pad < K || Ho <= 0 || Wo <= 0) return fail("the kernel does not fit the padded image");
    const int64_t lim = 1ll << 30;
    if (N >= lim || N * C >= lim || N * C * (int64_t)Hin * Win >= lim || N * C * (int64_t)Ho * Wo >= lim)
        return fail("the input and the output must each hold fewer than 2^30 elements");
    return PLEAS_OK;
}

static bool dw_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// --------------------------------------------------------------------------------------------------- grouped forward (the fit)
struct DwFwdGeo {
    int N, C, Hin, Win, Ho, Wo, K, stride, pad, Csrc, n_merged;
    uint32_t strips, items, first_block, nblocks;
    float dscale, loss_scale;
};
enum { kIp = 0, kW, kBias, kO1, kO2, kRow1, kRow2, kResid };

// fixed-order sum over a wave (the value of lane 0 counts), then over the workgroup's waves in wave order (thread 0 returns it)
__device__ __forceinline__ double dw_block_sum(double v, double* smem) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) smem[wave] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int q = 0; q < kDwThreads / 64; ++q) s += smem[q];
    return s;
}

__global__ __launch_bounds__(kDwThreads) void dw_fwd_batch_kernel(const DwFwdGeo* __restrict__ geo, const DwPtrs* __restrict__ ptrs,
                                                                  const DwItem* __restrict__ items, double* __restrict__ parts) {
    __shared__ double smem[kDwThreads / 64];
    const DwItem it = items[blockIdx.x];
    const DwFwdGeo g = geo[it.layer];
    const DwPtrs P = ptrs[it.layer];
    const uint32_t idx = (uint32_t)it.local * kDwThreads + threadIdx.x;
    double sq = 0.0;
    if (idx < g.items) {
        const uint32_t ox = idx % (uint32_t)g.Wo, t = idx / (uint32_t)g.Wo;
        const uint32_t strip = t % g.strips, plane = t / g.strips;
        const uint32_t n = plane / (uint32_t)g.C;
        const int c = (int)(plane % (uint32_t)g.C), oy0 = (int)strip * kDwRows;
        double acc[kDwRows];
        dw_strip_any(g.K, g.stride, (const float*)P.p[kIp] + (size_t)plane * g.Hin * g.Win, (const float*)P.p[kW] + (size_t)c * (g.K * g.K),
                     g.Hin, g.Win, oy0, (int)ox, g.pad, acc);
        const float* bias = (const float*)P.p[kBias];
        const double b = bias ? (double)bias[c] : 0.0;
        const int r1 = ((const int32_t*)P.p[kRow1])[c], r2 = ((const int32_t*)P.p[kRow2])[c];
        const double coef = c < g.n_merged ? 0.5 : 1.0;
        const float* o1 = (const float*)P.p[kO1];
        const float* o2 = (const float*)P.p[kO2];
        float* resid = (float*)P.p[kResid];
#pragma unroll
        for (int r = 0; r < kDwRows; ++r) {
            const int oy = oy0 + r;
            if (oy >= g.Ho) break;
            const size_t px = (size_t)oy * g.Wo + ox, hw = (size_t)g.Ho * g.Wo;
            const double out = acc[r] + b;
            const double ta = r1 >= 0 ? (double)o1[((size_t)n * g.Csrc + r1) * hw + px] : 0.0;
            const double tb = r2 >= 0 ? (double)o2[((size_t)n * g.Csrc + r2) * hw + px] : 0.0;
            const double d = out - (ta + tb) * coef;
            sq = fma(d, d, sq);
            resid[(size_t)plane * hw + px] = (float)((double)g.dscale * d);
        }
    }
    const double s = dw_block_sum(sq, smem);
    if (threadIdx.x == 0) parts[blockIdx.x] = s;
}

__global__ __launch_bounds__(64) void dw_loss_kernel(const DwFwdGeo* __restrict__ geo, const double* __restrict__ parts,
                                                     float* __restrict__ loss) {
    const DwFwdGeo g = geo[blockIdx.x];
    double v = 0.0;
    for (uint32_t i = threadIdx.x; i < g.nblocks; i += 64) v += parts[g.first_block + i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (threadIdx.x == 0) loss[blockIdx.x] = (float)((double)g.loss_scale * v);
}

struct DwFwdPlan {
    std::vector<int64_t> key;
    size_t total = 0;
    bool uploaded = false;
    std::vector<DwFwdGeo> geo;
    std::vector<DwItem> items;
    size_t off_geo = 0, off_ptrs = 0, off_items = 0, off_parts = 0;
};

static int dw_fwd_build(DwFwdPlan& p, const pleas_dw_layer* layers, int n) {
    p.geo.clear();
    p.items.clear();
    uint64_t blocks = 0;
    for (int i = 0; i < n; ++i) {
        const pleas_dw_layer& l = layers[i];
        DwFwdGeo g{};
        if (const int rc = dw_check_geometry("dw_fwd_batch", l.N, l.C, l.Hin, l.Win, l.K, l.stride, l.pad, g.Ho, g.Wo); rc != PLEAS_OK)
            return rc;
        if (l.N <= 0) return bad_arg("dw_fwd_batch: a layer without samples");
        if (l.Csrc <= 0 || l.n_merged < 0 || l.n_merged > l.C) return bad_arg("dw_fwd_batch: Csrc / n_merged out of range");
        if ((int64_t)l.N * l.Csrc * g.Ho * g.Wo >= (1ll << 30)) return bad_arg("dw_fwd_batch: a source output of 2^30 elements or more");
        g.N = l.N; g.C = l.C; g.Hin = l.Hin; g.Win = l.Win; g.K = l.K; g.stride = l.stride; g.pad = l.pad;
        g.Csrc = l.Csrc; g.n_merged = l.n_merged; g.dscale = l.dscale; g.loss_scale = l.loss_scale;
        g.strips = (uint32_t)ceil_div(g.Ho, kDwRows);
        g.items = (uint32_t)((int64_t)l.N * l.C * g.strips * g.Wo);
        g.first_block = (uint32_t)blocks;
        g.nblocks = (uint32_t)ceil_div(g.items, kDwThreads);
        for (uint32_t b = 0; b < g.nblocks; ++b) p.items.push_back(DwItem{i, (int)b});
        blocks += g.nblocks;
        if (blocks >= (1ull << 30)) return bad_arg("dw_fwd_batch: too many workgroups");
        p.geo.push_back(g);
    }
    size_t off = 0;
    p.off_geo = off;   off += align256(p.geo.size() * sizeof(DwFwdGeo));
    p.off_ptrs = off;  off += align256((size_t)n * sizeof(DwPtrs));
    p.off_items = off; off += align256(p.items.size() * sizeof(DwItem));
    p.off_parts = off; off += align256(p.items.size() * sizeof(double));
    p.total = off;
    return PLEAS_OK;
}

static int dw_fwd_check_list(const pleas_dw_layer* layers, int n, bool pointers) {
    if (!layers || n <= 0) return bad_arg("dw_fwd_batch: empty layer list");
    if (!pointers) return PLEAS_OK;
    for (int i = 0; i < n; ++i) {
        const pleas_dw_layer& l = layers[i];
        if (!l.ip || !l.w || !l.o1 || !l.o2 || !l.row1 || !l.row2 || !l.resid) return bad_arg("dw_fwd_batch: null pointer");
        if (!dw_aligned16(l.ip) || !dw_aligned16(l.w) || !dw_aligned16(l.o1) || !dw_aligned16(l.o2) || !dw_aligned16(l.resid))
            return bad_arg("dw_fwd_batch: ip, w, o1, o2 and resid must be 16-byte aligned");
    }
    return PLEAS_OK;
}

static std::mutex g_dw_mu;
static PlanCache<DwFwdPlan, 1> g_dw_fwd_plans;

// ------------------------------------------------------------------------------------------------ grouped weight gradient
struct DwWgGeo {
    int N, C, Hin, Win, Ho, Wo, K, stride, pad;
    uint32_t rows, rows_per_slab, nslab, part_off;      // rows = N * Ho; part_off: the layer's partials [C][nslab][K*K], in floats
};
enum { kWgResid = 0, kWgIp, kWgGrad };

template <int K>
__device__ __forceinline__ void dw_wgrad_slab(const DwWgGeo& g, const float* __restrict__ resid, const float* __restrict__ ip, const int c,
                                              const uint32_t slab, float* __restrict__ part, float (*smem)[49]) {
    float acc[K * K];
#pragma unroll
    for (int t = 0; t < K * K; ++t) acc[t] = 0.f;
    const uint32_t row0 = slab * g.rows_per_slab;
    const uint32_t nrows = min(g.rows_per_slab, g.rows - row0);
    const uint32_t count = nrows * (uint32_t)g.Wo;
    for (uint32_t e = threadIdx.x; e < count; e += kDwThreads) {
        const uint32_t row = row0 + e / (uint32_t)g.Wo, ox = e % (uint32_t)g.Wo;
        const uint32_t n = row / (uint32_t)g.Ho, oy = row % (uint32_t)g.Ho;
        const size_t plane = (size_t)n * g.C + c;
        const float r = resid[(plane * g.Ho + oy) * g.Wo + ox];
        const float* xp = ip + plane * g.Hin * g.Win;
        const int iy0 = (int)oy * g.stride - g.pad, ix0 = (int)ox * g.stride - g.pad;
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
            const int iy = iy0 + ky;
            const bool row_in = iy >= 0 && iy < g.Hin;
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                const int ix = ix0 + kx;
                const float v = (row_in && ix >= 0 && ix < g.Win) ? xp[(size_t)iy * g.Win + ix] : 0.f;
                acc[ky * K + kx] = fmaf(r, v, acc[ky * K + kx]);
            }
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int t = 0; t < K * K; ++t) {
        float v = acc[t];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) smem[wave][t] = v;
    }
    __syncthreads();
    if (threadIdx.x < K * K) {
        float s = smem[0][threadIdx.x];
        for (int q = 1; q < kDwThreads / 64; ++q) s += smem[q][threadIdx.x];
        part[g.part_off + ((size_t)c * g.nslab + slab) * (K * K) + threadIdx.x] = s;
    }
}

__global__ __launch_bounds__(kDwThreads) void dw_wgrad_slab_kernel(const DwWgGeo* __restrict__ geo, const DwPtrs* __restrict__ ptrs,
                                                                   const DwItem* __restrict__ items, float* __restrict__ part) {
    __shared__ float smem[kDwThreads / 64][49];
    const DwItem it = items[blockIdx.x];
    const DwWgGeo g = geo[it.layer];
    const DwPtrs P = ptrs[it.layer];
    const int c = it.local / (int)g.nslab;
    const uint32_t slab = (uint32_t)it.local % g.nslab;
    const float* resid = (const float*)P.p[kWgResid];
    const float* ip = (const float*)P.p[kWgIp];
    switch (g.K) {       // uniform per workgroup
        case 1: dw_wgrad_slab<1>(g, resid, ip, c, slab, part, smem); break;
        case 3: dw_wgrad_slab<3>(g, resid, ip, c, slab, part, smem); break;
        case 5: dw_wgrad_slab<5>(g, resid, ip, c, slab, part, smem); break;
        default: dw_wgrad_slab<7>(g, resid, ip, c, slab, part, smem); break;
    }
}

// stage two: one thread per (channel, tap) of a layer, the slabs in slab order
__global__ __launch_bounds__(kDwThreads) void dw_wgrad_reduce_kernel(const DwWgGeo* __restrict__ geo, const DwPtrs* __restrict__ ptrs,
                                                                     const DwItem* __restrict__ items, const float* __restrict__ part) {
    const DwItem it = items[blockIdx.x];
    const DwWgGeo g = geo[it.layer];
    const uint32_t kk = (uint32_t)(g.K * g.K), e = (uint32_t)it.local * kDwThreads + threadIdx.x;
    if (e >= (uint32_t)g.C * kk) return;
    const uint32_t c = e / kk, t = e % kk;
    const float* p = part + g.part_off + (size_t)c * g.nslab * kk + t;
    float s = p[0];
    for (uint32_t q = 1; q < g.nslab; ++q) s += p[(size_t)q * kk];
    ((float*)ptrs[it.layer].p[kWgGrad])[e] = s;
}

struct DwWgPlan {
    std::vector<int64_t> key;
    size_t total = 0;
    bool uploaded = false;
    std::vector<DwWgGeo> geo;
    std::vector<DwItem> items, items2;
    size_t off_geo = 0, off_ptrs = 0, off_items = 0, off_items2 = 0, off_part = 0;
};

static int dw_wgrad_build(DwWgPlan& p, const pleas_dw_wgrad_layer* layers, int n) {
    p.geo.clear();
    p.items.clear();
    p.items2.clear();
    uint64_t part = 0;
    for (int i = 0; i < n; ++i) {
        const pleas_dw_wgrad_layer& l = layers[i];
        DwWgGeo g{};
        if (const int rc = dw_check_geometry("dw_wgrad_batch", l.N, l.C, l.Hin, l.Win, l.K, l.stride, l.pad, g.Ho, g.Wo); rc != PLEAS_OK)
            return rc;
        if (l.N <= 0) return bad_arg("dw_wgrad_batch: a layer without samples");
        g.N = l.N; g.C = l.C; g.Hin = l.Hin; g.Win = l.Win; g.K = l.K; g.stride = l.stride; g.pad = l.pad;
        g.rows = (uint32_t)((int64_t)l.N * g.Ho);
        g.rows_per_slab = (uint32_t)std::max(1, kDwSlabOutputs / g.Wo);
        g.nslab = (uint32_t)ceil_div(g.rows, g.rows_per_slab);
        g.part_off = (uint32_t)part;
        const uint64_t kk = (uint64_t)l.K * l.K, blocks = (uint64_t)l.C * g.nslab;
        part += blocks * kk;
        if (part >= (1ull << 30) || p.items.size() + blocks >= (1ull << 30)) return bad_arg("dw_wgrad_batch: too many workgroups");
        for (uint64_t b = 0; b < blocks; ++b) p.items.push_back(DwItem{i, (int)b});
        for (int64_t b = 0; b < ceil_div((int64_t)(l.C * kk), kDwThreads); ++b) p.items2.push_back(DwItem{i, (int)b});
        p.geo.push_back(g);
    }
    size_t off = 0;
    p.off_geo = off;    off += align256(p.geo.size() * sizeof(DwWgGeo));
    p.off_ptrs = off;   off += align256((size_t)n * sizeof(DwPtrs));
    p.off_items = off;  off += align256(p.items.size() * sizeof(DwItem));
    p.off_items2 = off; off += align256(p.items2.size() * sizeof(DwItem));
    p.off_part = off;   off += align256((size_t)part * sizeof(float));
    p.total = off;
    return PLEAS_OK;
}

static int dw_wgrad_check_list(const pleas_dw_wgrad_layer* layers, int n, bool pointers) {
    if (!layers || n <= 0) return bad_arg("dw_wgrad_batch: empty layer list");
    if (!pointers) return PLEAS_OK;
    for (int i = 0; i < n; ++i) {
        const pleas_dw_wgrad_layer& l = layers[i];
        if (!l.resid || !l.ip || !l.grad) return bad_arg("dw_wgrad_batch: null pointer");
        if (!dw_aligned16(l.resid) || !dw_aligned16(l.ip) || !dw_aligned16(l.grad))
            return bad_arg("dw_wgrad_batch: resid, ip and grad must be 16-byte aligned");
    }
    return PLEAS_OK;
}

static PlanCache<DwWgPlan, 1> g_dw_wg_plans;

template <class Layer, class Fill>
static int dw_upload_ptrs(const Layer* layers, int n, DwPtrs* table, hipStream_t stream, Fill&& fill) {
    for (int b0 = 0; b0 < n; b0 += kDwPtrBatch) {
        DwPtrBatch pb{};
        pb.base = b0;
        pb.count = std::min(kDwPtrBatch, n - b0);
        for (int t = 0; t < pb.count; ++t) fill(layers[b0 + t], pb.l[t]);
        hipLaunchKernelGGL(dw_set_ptrs_kernel, dim3(1), dim3(kDwPtrBatch * kDwMaxPtrs), 0, stream, table, pb);
        PLEAS_LAUNCH_CHECK("dw_set_ptrs_kernel");
    }
    return PLEAS_OK;
}

}  // namespace pleas

using namespace pleas;

extern "C" int pleas_dwconv2d_fwd(const float* x, const float* w, const float* bias, float* y, const float* scale, const float* shift,
                                  const float* res, float* z, int relu, int N, int C, int Hin, int Win, int K, int stride, int pad,
                                  void* stream_) {
    if (!x || !w) return bad_arg("dwconv2d_fwd: null x or w");
    if (!y && !z) return bad_arg("dwconv2d_fwd: neither y nor z to write");
    if ((scale == nullptr) != (shift == nullptr)) return bad_arg("dwconv2d_fwd: scale and shift come together");
    if (!z && (scale || res)) return bad_arg("dwconv2d_fwd: scale / shift / res without z");
    int Ho = 0, Wo = 0;
    if (const int rc = dw_check_geometry("dwconv2d_fwd", N, C, Hin, Win, K, stride, pad, Ho, Wo); rc != PLEAS_OK) return rc;
    if (!dw_aligned16(x) || !dw_aligned16(w) || !dw_aligned16(y) || !dw_aligned16(z) || !dw_aligned16(res))
        return bad_arg("dwconv2d_fwd: x, w, y, z and res must be 16-byte aligned");
    if (((uintptr_t)bias | (uintptr_t)scale | (uintptr_t)shift) & 3) return bad_arg("dwconv2d_fwd: bias, scale and shift must be 4-byte aligned");
    if (N == 0) return PLEAS_OK;
    DwFwdArgs a;
    a.x = x; a.w = w; a.bias = bias; a.y = y; a.scale = scale; a.shift = shift; a.res = res; a.z = z;
    a.relu = relu; a.C = C; a.Hin = Hin; a.Win = Win; a.Ho = Ho; a.Wo = Wo; a.pad = pad;
    a.strips = (uint32_t)ceil_div(Ho, kDwRows);
    a.items = (uint32_t)((int64_t)N * C * a.strips * Wo);
    const dim3 grid((unsigned)ceil_div(a.items, kDwThreads)), block(kDwThreads);
    hipStream_t stream = (hipStream_t)stream_;
    const double bytes = 4.0 * ((double)N * C * ((double)Hin * Win + (double)Ho * Wo * ((y ? 1 : 0) + (z ? 1 : 0) + (res ? 1 : 0))) + (double)C * K * K);
    ProfScope prof(kProfConv2d, 2.0 * N * C * Ho * Wo * K * K, bytes, stream);
#define PLEAS_DW_LAUNCH(KK, SS) hipLaunchKernelGGL((dw_fwd_kernel<KK, SS>), grid, block, 0, stream, a)
    switch (K * 2 + stride) {
        case 1 * 2 + 1: PLEAS_DW_LAUNCH(1, 1); break;
        case 1 * 2 + 2: PLEAS_DW_LAUNCH(1, 2); break;
        case 3 * 2 + 1: PLEAS_DW_LAUNCH(3, 1); break;
        case 3 * 2 + 2: PLEAS_DW_LAUNCH(3, 2); break;
        case 5 * 2 + 1: PLEAS_DW_LAUNCH(5, 1); break;
        case 5 * 2 + 2: PLEAS_DW_LAUNCH(5, 2); break;
        case 7 * 2 + 1: PLEAS_DW_LAUNCH(7, 1); break;
        default: PLEAS_DW_LAUNCH(7, 2); break;
    }
#undef PLEAS_DW_LAUNCH
    PLEAS_LAUNCH_CHECK("dw_fwd_kernel");
    return PLEAS_OK;
}

extern "C" size_t pleas_dw_fwd_batch_ws_bytes(const pleas_dw_layer* layers, int n_layers) {
    if (dw_fwd_check_list(layers, n_layers, false) != PLEAS_OK) return 0;
    DwFwdPlan p;
    if (dw_fwd_build(p, layers, n_layers) != PLEAS_OK) return 0;
    return p.total;
}

extern "C" int pleas_dw_fwd_batch(const pleas_dw_layer* layers, int n_layers, float* loss, void* ws, size_t ws_bytes, int ws_fresh,
                                  void* stream_) {
    if (const int rc = dw_fwd_check_list(layers, n_layers, true); rc != PLEAS_OK) return rc;
    if (!loss) return bad_arg("dw_fwd_batch: null loss");
    if (ws && !dw_aligned16(ws)) return bad_arg("dw_fwd_batch: the workspace must be 16-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    std::lock_guard<std::mutex> lk(g_dw_mu);
    std::vector<int64_t> key;
    key.push_back(n_layers);
    key.push_back((int64_t)(uintptr_t)ws);
    for (int i = 0; i < n_layers; ++i) {
        const pleas_dw_layer& l = layers[i];
        for (int v : {l.N, l.C, l.Hin, l.Win, l.K, l.stride, l.pad, l.Csrc, l.n_merged}) key.push_back(v);
        int32_t bits[2];
        std::memcpy(&bits[0], &l.dscale, 4);
        std::memcpy(&bits[1], &l.loss_scale, 4);
        key.push_back(bits[0]);
        key.push_back(bits[1]);
    }
    DwFwdPlan* hit = nullptr;
    if (const int rc = g_dw_fwd_plans.get(key, hit, [&](DwFwdPlan& p) { return dw_fwd_build(p, layers, n_layers); }); rc != PLEAS_OK)
        return rc;
    DwFwdPlan& P = *hit;
    if (const int rc = g_dw_fwd_plans.prepare(P, "dw_fwd_batch", ws, ws_bytes, ws_fresh, stream, [&] {
            return std::vector<PlanTable>{plan_table(P.off_geo, P.geo), plan_table(P.off_items, P.items)};
        });
        rc != PLEAS_OK)
        return rc;
    char* base = (char*)ws;
    DwPtrs* ptrs = reinterpret_cast<DwPtrs*>(base + P.off_ptrs);
    if (const int rc = dw_upload_ptrs(layers, n_layers, ptrs, stream, [](const pleas_dw_layer& l, DwPtrs& d) {
            d.p[kIp] = l.ip; d.p[kW] = l.w; d.p[kBias] = l.bias; d.p[kO1] = l.o1; d.p[kO2] = l.o2;
            d.p[kRow1] = l.row1; d.p[kRow2] = l.row2; d.p[kResid] = l.resid;
        });
        rc != PLEAS_OK)
        return rc;
    const DwFwdGeo* geo = reinterpret_cast<const DwFwdGeo*>(base + P.off_geo);
    double* parts = reinterpret_cast<double*>(base + P.off_parts);
    hipLaunchKernelGGL(dw_fwd_batch_kernel, dim3((unsigned)P.items.size()), dim3(kDwThreads), 0, stream, geo, ptrs,
                       reinterpret_cast<const DwItem*>(base + P.off_items), parts);
    PLEAS_LAUNCH_CHECK("dw_fwd_batch_kernel");
    hipLaunchKernelGGL(dw_loss_kernel, dim3((unsigned)n_layers), dim3(64), 0, stream, geo, parts, loss);
    PLEAS_LAUNCH_CHECK("dw_loss_kernel");
    return PLEAS_OK;
}

extern "C" size_t pleas_dw_wgrad_batch_ws_bytes(const pleas_dw_wgrad_layer* layers, int n_layers) {
    if (dw_wgrad_check_list(layers, n_layers, false) != PLEAS_OK) return 0;
    DwWgPlan p;
    if (dw_wgrad_build(p, layers, n_layers) != PLEAS_OK) return 0;
    return p.total;
}

extern "C" int pleas_dw_wgrad_batch(const pleas_dw_wgrad_layer* layers, int n_layers, void* ws, size_t ws_bytes, int ws_fresh,
                                    void* stream_) {
    if (const int rc = dw_wgrad_check_list(layers, n_layers, true); rc != PLEAS_OK) return rc;
    if (ws && !dw_aligned16(ws)) return bad_arg("dw_wgrad_batch: the workspace must be 16-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    std::lock_guard<std::mutex> lk(g_dw_mu);
    std::vector<int64_t> key;
    key.push_back(n_layers);
    key.push_back((int64_t)(uintptr_t)ws);
    for (int i = 0; i < n_layers; ++i) {
        const pleas_dw_wgrad_layer& l = layers[i];
        for (int v : {l.N, l.C, l.Hin, l.Win, l.K, l.stride, l.pad}) key.push_back(v);
    }
    DwWgPlan* hit = nullptr;
    if (const int rc = g_dw_wg_plans.get(key, hit, [&](DwWgPlan& p) { return dw_wgrad_build(p, layers, n_layers); }); rc != PLEAS_OK)
        return rc;
    DwWgPlan& P = *hit;
    if (const int rc = g_dw_wg_plans.prepare(P, "dw_wgrad_batch", ws, ws_bytes, ws_fresh, stream, [&] {
            return std::vector<PlanTable>{plan_table(P.off_geo, P.geo), plan_table(P.off_items, P.items),
                                          plan_table(P.off_items2, P.items2)};
        });
        rc != PLEAS_OK)
        return rc;
    char* base = (char*)ws;
    DwPtrs* ptrs = reinterpret_cast<DwPtrs*>(base + P.off_ptrs);
    if (const int rc = dw_upload_ptrs(layers, n_layers, ptrs, stream, [](const pleas_dw_wgrad_layer& l, DwPtrs& d) {
            d.p[kWgResid] = l.resid; d.p[kWgIp] = l.ip; d.p[kWgGrad] = l.grad;
        });
        rc != PLEAS_OK)
        return rc;
    const DwWgGeo* geo = reinterpret_cast<const DwWgGeo*>(base + P.off_geo);
    float* part = reinterpret_cast<float*>(base + P.off_part);
    hipLaunchKernelGGL(dw_wgrad_slab_kernel, dim3((unsigned)P.items.size()), dim3(kDwThreads), 0, stream, geo, ptrs,
                       reinterpret_cast<const DwItem*>(base + P.off_items), part);
    PLEAS_LAUNCH_CHECK("dw_wgrad_slab_kernel");
    hipLaunchKernelGGL(dw_wgrad_reduce_kernel, dim3((unsigned)P.items2.size()), dim3(kDwThreads), 0, stream, geo, ptrs,
                       reinterpret_cast<const DwItem*>(base + P.off_items2), part);
    PLEAS_LAUNCH_CHECK("dw_wgrad_reduce_kernel");
    return PLEAS_OK;
}
