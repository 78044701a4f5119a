// Closed-form fit of depthwise layers on gfx950 (MI355X): per-channel normal equations, accumulated over the batches by one grouped
// launch per batch, and a batched tiny Cholesky.
//
//   v_r in R^D, D = K*K + 2, per channel c and output pixel r = (n, oy, ox):
//     v_r[ky*K + kx] = ip[n][c][oy*s + ky - p][ox*s + kx - p]  (0 outside the image),  v_r[K*K] = 1,
//     v_r[K*K + 1]   = tgt[n][c][oy][ox] = (float)(([row1[c] >= 0] o1 + [row2[c] >= 0] o2) * coef), coef = 0.5 below n_merged:
//                      the fp32 value pleas_merge_blocks stores, never materialised
//   S[c] += sum_r v_r v_r^T     double S[C][D][D], LOWER triangle with the diagonal; the strict upper triangle is not touched
//                                                                                                   pleas_dw_normal_eq_accum
//   (G_T + ridge * mean(diag G_T) I) x = h_T per channel, x rounded once to fp32 into w[c][:] (and bias[c])
//                                                                              pleas_dw_normal_eq_solve / pleas_dw_normal_eq_solve_host
//
// Arithmetic: every fp32 x fp32 product is exact in fp64 and every sum is an fp64 sum.  No atomics.
//
// Form of the accumulate kernel.  v is padded with zeros to NB = 1 / 2 / 4 blocks of 16 entries (K = 1 and 3 / 5 / 7) and S[c] is
// cut into 16 x 16 tiles, of which the NB (NB + 1) / 2 on and below the diagonal are computed, each by v_mfma_f64_16x16x4_f64:
// lane l of a wave holds entry (l & 15) of every block of the pixel (l >> 4) of a group of FOUR consecutive pixels, ONE load per
// block, and passes it as the A operand (rows) of the tiles of its block row and as the B operand (columns) of those of its block
// column -- on a diagonal tile the same register twice.  The tile sums over the lanes inside the matrix unit: no shuffle tree.
// A work item (one workgroup of 4 waves) is one (channel, slab of kDwNeqSlab consecutive output pixels of the channel, counted
// over (n, oy, ox)); wave q takes the slab's pixel groups q, q + 4, ...  A lane walks (n, oy, ox) incrementally.  One kernel per
// kernel size (its own register count); the loads of kDwNeqUnroll pixel groups are issued together, without a branch between them.
//
// Summation order (the same bits run after run, grouped or alone; the split depends on the geometry alone):
//   per wave     its pixel groups ascending, one MFMA per group and tile: the four pixels of a group enter the accumulator in the
//                matrix unit's fixed order
//   per slab     the four waves' tiles in wave order, from 0                                   -> partial [C][slabs][tiles][16][16]
//   per entry    the slabs of the channel in slab order, from 0, and that sum is added to S    (stage two, one thread per entry)
// Two launches into one S add the second launch's sum to what the first left.  Two entries of ONE launch may not share an S.
//
// Solve: one wave per channel, four channels to a workgroup, the system in LDS as a packed triangle (dw_neq_solve.hpp).
#include <mutex>

#include "common.hpp"
#include "dw_neq_solve.hpp"

namespace pleas {

constexpr int kDwNeqThreads = 256;
constexpr int kDwNeqSlab = 4096;          // output pixels of a channel per work item
constexpr int kDwNeqUnroll = 4;           // pixel groups of a wave whose loads are in flight together
constexpr int kDwNeqPtrBatch = 16;        // layers whose addresses ride in one launch of the pointer kernel
constexpr int kDwNeqPtrs = 6;

typedef double f64x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) double gdouble;

struct DwNeqItem {       // one workgroup of a grouped launch
    int layer, local;
};
struct DwNeqPtrs {
    const void* p[kDwNeqPtrs];
};
struct DwNeqPtrBatch {
    int base, count;
    DwNeqPtrs l[kDwNeqPtrBatch];
};
enum { kNqIp = 0, kNqO1, kNqO2, kNqRow1, kNqRow2, kNqS };

__global__ void dw_neq_set_ptrs_kernel(DwNeqPtrs* table, const DwNeqPtrBatch b) {
    const int t = threadIdx.x;
    if (t < b.count * kDwNeqPtrs) table[b.base + t / kDwNeqPtrs].p[t % kDwNeqPtrs] = b.l[t / kDwNeqPtrs].p[t % kDwNeqPtrs];
}

struct DwNeqGeo {
    int N, C, Hin, Win, Ho, Wo, K, stride, pad, Csrc, n_merged;
    int nb, ntile;                     // blocks of 16 entries of v; tiles on and below the diagonal
    uint32_t M, nslab;                 // output pixels of a channel; slabs of a channel
    uint64_t part_off;                 // the layer's partials [C][nslab][ntile][256], in doubles
};

constexpr int dw_neq_blocks(int K) { return K <= 3 ? 1 : K == 5 ? 2 : 4; }

// stage one: one (channel, slab) -> its ntile partial tiles.  No branch stands between a load and the next: a lane whose entry is
// not a tap inside the image (or not the target) loads element 0 of the tensor and drops the value.
template <int K>
__device__ __forceinline__ void dw_neq_slab(const DwNeqGeo& g, const DwNeqPtrs& P, const int c, const uint32_t slab,
                                            double* __restrict__ part, double (*smem)[64]) {
    constexpr int NB = dw_neq_blocks(K), NT = NB * (NB + 1) / 2, KK = K * K, TB = (KK + 1) / 16;      // TB: the target's block
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e0 = lane & 15, sub = lane >> 4;
    // what entry b * 16 + e0 of v is: a tap (dy, dx relative to the output pixel's top-left input), the one, the target, or padding
    bool tap[NB];
    int dy[NB], dx[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int e = b * 16 + e0;
        tap[b] = e < KK;
        dy[b] = tap[b] ? e / K - g.pad : 0;
        dx[b] = tap[b] ? e % K - g.pad : 0;
    }
    const bool is_one = TB * 16 + e0 == KK, is_tgt = TB * 16 + e0 == KK + 1;      // (KK and KK + 1 share a block: KK % 16 is 1 or 9)
    const cgfloat* ip = PLEAS_GLOBAL(P.p[kNqIp]);
    const cgfloat* o1 = PLEAS_GLOBAL(P.p[kNqO1]);
    const cgfloat* o2 = PLEAS_GLOBAL(P.p[kNqO2]);
    const int r1 = PLEAS_GLOBAL_I(P.p[kNqRow1])[c], r2 = PLEAS_GLOBAL_I(P.p[kNqRow2])[c];
    const float coef = c < g.n_merged ? 0.5f : 1.0f;
    const uint32_t Ho = (uint32_t)g.Ho, Wo = (uint32_t)g.Wo, hw = Ho * Wo;
    const uint32_t first = slab * (uint32_t)kDwNeqSlab, end = min(first + (uint32_t)kDwNeqSlab, g.M);
    uint32_t r = first + (uint32_t)wave * 4u + (uint32_t)sub;
    uint32_t n = r / hw, oy = (r % hw) / Wo, ox = (r % hw) % Wo;

    f64x4_t acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f64x4_t{0.0, 0.0, 0.0, 0.0};

    // kDwNeqUnroll pixel groups per trip: their loads are all issued before the first matrix instruction waits for one (a wave has
    // one load per group and block in flight otherwise, and the kernel is bound by their latency).  A group past the slab's end
    // adds 0 * 0 to every accumulator: the sums are those of the groups taken one at a time.
    for (uint32_t base = first + (uint32_t)wave * 4u; base < end; base += 16u * kDwNeqUnroll) {      // uniform over the wave
        float f[kDwNeqUnroll][NB], ta[kDwNeqUnroll], tb[kDwNeqUnroll];
        bool in[kDwNeqUnroll][NB], in1[kDwNeqUnroll], in2[kDwNeqUnroll], alive[kDwNeqUnroll];
#pragma unroll
        for (int u = 0; u < kDwNeqUnroll; ++u) {
            const bool live = alive[u] = r < end;          // (then n < N: r < M)
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const int iy = (int)oy * g.stride + dy[b], ix = (int)ox * g.stride + dx[b];
                in[u][b] = live && tap[b] && iy >= 0 && iy < g.Hin && ix >= 0 && ix < g.Win;
                const uint32_t at = ((n * (uint32_t)g.C + (uint32_t)c) * (uint32_t)g.Hin + (uint32_t)iy) * (uint32_t)g.Win + (uint32_t)ix;
                f[u][b] = ip[in[u][b] ? at : 0u];
            }
            const uint32_t px = oy * Wo + ox;
            in1[u] = live && is_tgt && r1 >= 0;
            in2[u] = live && is_tgt && r2 >= 0;
            ta[u] = o1[in1[u] ? (n * (uint32_t)g.Csrc + (uint32_t)r1) * hw + px : 0u];
            tb[u] = o2[in2[u] ? (n * (uint32_t)g.Csrc + (uint32_t)r2) * hw + px : 0u];
            r += 16u;
            ox += 16u;
            if (ox >= Wo) {
                const uint32_t q = ox / Wo;
                ox -= q * Wo;
                oy += q;
                if (oy >= Ho) {
                    const uint32_t q2 = oy / Ho;
                    oy -= q2 * Ho;
                    n += q2;
                }
            }
        }
        // every load above is a load on every lane (the values pass an empty statement the compiler cannot make conditional)
#pragma unroll
        for (int u = 0; u < kDwNeqUnroll; ++u) {
#pragma unroll
            for (int b = 0; b < NB; ++b) asm volatile("" : "+v"(f[u][b]));
            asm volatile("" : "+v"(ta[u]), "+v"(tb[u]));
        }
#pragma unroll
        for (int u = 0; u < kDwNeqUnroll; ++u) {
            double v[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) v[b] = (double)(in[u][b] ? f[u][b] : 0.f);
            const float tg = ((in1[u] ? ta[u] : 0.f) + (in2[u] ? tb[u] : 0.f)) * coef;
            if (alive[u] && is_tgt) v[TB] = (double)tg;
            if (alive[u] && is_one) v[TB] = 1.0;
            int t = 0;
#pragma unroll
            for (int a = 0; a < NB; ++a)
#pragma unroll
                for (int b = 0; b <= a; ++b, ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[a], v[b], acc[t], 0, 0, 0);
        }
    }
    // the four waves in wave order; thread (reg, lane) holds row (lane >> 4) + 4 reg, column lane & 15 of a tile
    const int reg = wave, row = (lane >> 4) + 4 * reg, col = lane & 15;
    double* out = part + g.part_off + ((uint64_t)c * g.nslab + slab) * (uint64_t)(NT * 256);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int q = 0; q < 4; ++q) smem[wave * 4 + q][lane] = acc[t][q];
        __syncthreads();
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < kDwNeqThreads / 64; ++w) s += smem[w * 4 + reg][lane];
        out[t * 256 + row * 16 + col] = s;
        __syncthreads();
    }
}


// one kernel per kernel size (each at its own register count: 8 / 8 / 24 / 80 accumulator registers), over the items of its layers
template <int K>
__global__ __launch_bounds__(kDwNeqThreads) void dw_neq_slab_kernel(const DwNeqGeo* __restrict__ geo, const DwNeqPtrs* __restrict__ ptrs,
                                                                    const DwNeqItem* __restrict__ items, double* __restrict__ part) {
    __shared__ double smem[kDwNeqThreads / 64 * 4][64];      // [wave * 4 + register][lane]: one tile of each of the four waves
    const DwNeqItem it = items[blockIdx.x];
    const DwNeqGeo g = geo[it.layer];
    const DwNeqPtrs P = ptrs[it.layer];
    const int c = it.local / (int)g.nslab;
    const uint32_t slab = (uint32_t)it.local % g.nslab;
    dw_neq_slab<K>(g, P, c, slab, part, smem);
}

// stage two: one thread per (channel, i, j) of a layer's S; j <= i: the slabs in slab order from 0, then S += that sum
__global__ __launch_bounds__(kDwNeqThreads) void dw_neq_reduce_kernel(const DwNeqGeo* __restrict__ geo, const DwNeqPtrs* __restrict__ ptrs,
                                                                      const DwNeqItem* __restrict__ items, const double* __restrict__ part) {
    const DwNeqItem it = items[blockIdx.x];
    const DwNeqGeo g = geo[it.layer];
    const uint32_t D = (uint32_t)(g.K * g.K + 2), e = (uint32_t)it.local * kDwNeqThreads + threadIdx.x;
    if (e >= (uint32_t)g.C * D * D) return;
    const uint32_t c = e / (D * D), i = (e % (D * D)) / D, j = e % D;
    if (j > i) return;
    const uint32_t a = i >> 4, b = j >> 4, tile = a * (a + 1) / 2 + b;
    const uint64_t per_slab = (uint64_t)g.ntile * 256;
    const double* p = part + g.part_off + (uint64_t)c * g.nslab * per_slab + tile * 256 + (i & 15) * 16 + (j & 15);
    double s = 0.0;
    for (uint32_t q = 0; q < g.nslab; ++q) s += p[q * per_slab];
    gdouble* S = (gdouble*)ptrs[it.layer].p[kNqS];
    S[e] += s;
}

struct DwNeqPlan {
    std::vector<int64_t> key;
    size_t total = 0;
    bool uploaded = false;
    std::vector<DwNeqGeo> geo;
    std::vector<DwNeqItem> items, items2;      // items: those of the layers with K = 1 first, then 3, 5, 7
    size_t count[4] = {0, 0, 0, 0};            // items per kernel size
    size_t off_geo = 0, off_ptrs = 0, off_items = 0, off_items2 = 0, off_part = 0;
};

// geometry checks: those of the depthwise forwards (csrc/dwconv.hip), one message per refusal
static int dw_neq_check_geometry(const pleas_dw_neq_layer& l, int& Ho, int& Wo) {
    if (l.N <= 0 || l.C <= 0 || l.Hin <= 0 || l.Win <= 0) return bad_arg("dw_normal_eq: sizes must be positive");
    if (l.K < 1 || l.K > 7 || l.K % 2 == 0) return bad_arg("dw_normal_eq: the kernel must be odd and at most 7 x 7");
    if (l.stride != 1 && l.stride != 2) return bad_arg("dw_normal_eq: the stride must be 1 or 2");
    if (l.pad < 0 || l.pad > l.K / 2) return bad_arg("dw_normal_eq: the padding must lie in 0 .. K / 2");
    Ho = (l.Hin + 2 * l.pad - l.K) / l.stride + 1;
    Wo = (l.Win + 2 * l.pad - l.K) / l.stride + 1;
    if (l.Hin + 2 * l.pad < l.K || l.Win + 2 * l.pad < l.K || Ho <= 0 || Wo <= 0)
        return bad_arg("dw_normal_eq: the kernel does not fit the padded image");
    const int64_t lim = 1ll << 30, N = l.N;
    if (N * l.C >= lim || N * l.C * (int64_t)l.Hin * l.Win >= lim || N * l.C * (int64_t)Ho * Wo >= lim)
        return bad_arg("dw_normal_eq: the input and the output must each hold fewer than 2^30 elements");
    if (l.Csrc <= 0 || l.n_merged < 0 || l.n_merged > l.C) return bad_arg("dw_normal_eq: Csrc / n_merged out of range");
    if (N * l.Csrc * (int64_t)Ho * Wo >= lim) return bad_arg("dw_normal_eq: a source output of 2^30 elements or more");
    return PLEAS_OK;
}

static int dw_neq_build(DwNeqPlan& p, const pleas_dw_neq_layer* layers, int n) {
    p.geo.clear();
    p.items.clear();
    p.items2.clear();
    std::vector<DwNeqItem> by_class[4];
    uint64_t part = 0, total_blocks = 0;
    for (int i = 0; i < n; ++i) {
        const pleas_dw_neq_layer& l = layers[i];
        DwNeqGeo g{};
        if (const int rc = dw_neq_check_geometry(l, g.Ho, g.Wo); rc != PLEAS_OK) return rc;
        g.N = l.N; g.C = l.C; g.Hin = l.Hin; g.Win = l.Win; g.K = l.K; g.stride = l.stride; g.pad = l.pad;
        g.Csrc = l.Csrc; g.n_merged = l.n_merged;
        g.nb = dw_neq_blocks(l.K);
        g.ntile = g.nb * (g.nb + 1) / 2;
        g.M = (uint32_t)((int64_t)l.N * g.Ho * g.Wo);
        g.nslab = (uint32_t)ceil_div(g.M, kDwNeqSlab);
        g.part_off = part;
        const uint64_t blocks = (uint64_t)l.C * g.nslab, D = (uint64_t)l.K * l.K + 2;
        part += blocks * g.ntile * 256;
        total_blocks += blocks;
        if (part >= (1ull << 32) || total_blocks >= (1ull << 30) || (uint64_t)l.C * D * D >= (1ull << 30))
            return bad_arg("dw_normal_eq: too many workgroups");
        std::vector<DwNeqItem>& mine = by_class[l.K / 2];
        for (uint64_t b = 0; b < blocks; ++b) mine.push_back(DwNeqItem{i, (int)b});
        for (int64_t b = 0; b < ceil_div((int64_t)(l.C * D * D), kDwNeqThreads); ++b) p.items2.push_back(DwNeqItem{i, (int)b});
        p.geo.push_back(g);
    }
    for (int k = 0; k < 4; ++k) {
        p.count[k] = by_class[k].size();
        p.items.insert(p.items.end(), by_class[k].begin(), by_class[k].end());
    }
    size_t off = 0;
    p.off_geo = off;    off += align256(p.geo.size() * sizeof(DwNeqGeo));
    p.off_ptrs = off;   off += align256((size_t)n * sizeof(DwNeqPtrs));
    p.off_items = off;  off += align256(p.items.size() * sizeof(DwNeqItem));
    p.off_items2 = off; off += align256(p.items2.size() * sizeof(DwNeqItem));
    p.off_part = off;   off += align256((size_t)part * sizeof(double));
    p.total = off;
    return PLEAS_OK;
}

static bool dw_neq_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int dw_neq_check_list(const pleas_dw_neq_layer* layers, int n, bool pointers) {
    if (!layers || n <= 0) return bad_arg("dw_normal_eq: empty layer list");
    if (!pointers) return PLEAS_OK;
    for (int i = 0; i < n; ++i) {
        const pleas_dw_neq_layer& l = layers[i];
        if (!l.ip || !l.o1 || !l.o2 || !l.row1 || !l.row2 || !l.S) return bad_arg("dw_normal_eq_accum: null pointer");
        if (!dw_neq_aligned16(l.ip) || !dw_neq_aligned16(l.o1) || !dw_neq_aligned16(l.o2) || !dw_neq_aligned16(l.S))
            return bad_arg("dw_normal_eq_accum: ip, o1, o2 and S must be 16-byte aligned");
        if (((uintptr_t)l.row1 | (uintptr_t)l.row2) & 3) return bad_arg("dw_normal_eq_accum: row maps must be 4-byte aligned");
        if (l.n_merged < 0 || l.n_merged > l.C) return bad_arg("dw_normal_eq_accum: n_merged out of range");
    }
    return PLEAS_OK;
}

static std::mutex g_dw_neq_mu;
static PlanCache<DwNeqPlan, 1> g_dw_neq_plans;

// ------------------------------------------------------------------------------------------------------------------ solve
constexpr int kDwNeqSolveWaves = 4;       // channels of a workgroup

__global__ __launch_bounds__(kDwNeqSolveWaves * 64) void dw_neq_solve_kernel(const double* __restrict__ S, const int C, const int K,
                                                                             const int has_bias, const double ridge,
                                                                             float* __restrict__ w, float* __restrict__ bias,
                                                                             int* __restrict__ status) {
    __shared__ double a[kDwNeqSolveWaves][kDwNeqTri];
    __shared__ double x[kDwNeqSolveWaves][kDwNeqMaxT];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = blockIdx.x * kDwNeqSolveWaves + wave;
    const bool mine = c < C;
    const int cc = mine ? c : C - 1;       // a wave past the last channel walks the last one again (the barriers are the workgroup's)
    const int KK = K * K, D = KK + 2;
    const bool ok = dw_neq_solve_channel(S + (size_t)cc * D * D, K, has_bias, ridge, a[wave], x[wave], lane, 64, [] { __syncthreads(); });
    if (!mine) return;
    if (lane == 0) status[c] = ok ? 0 : 1;
    if (!ok) return;
    if (lane < KK) w[(size_t)c * KK + lane] = (float)x[wave][lane];
    if (has_bias && lane == 0) bias[c] = (float)x[wave][KK];
}

static int dw_neq_solve_check(const double* S, int C, int K, int has_bias, double ridge, const float* w, const float* bias,
                              const int* status) {
    if (!S || !w || !status) return bad_arg("dw_normal_eq_solve: null S, w or status");
    if (C <= 0) return bad_arg("dw_normal_eq_solve: no channels");
    if (K < 1 || K > 7 || K % 2 == 0) return bad_arg("dw_normal_eq_solve: the kernel must be odd and at most 7 x 7");
    if (has_bias && !bias) return bad_arg("dw_normal_eq_solve: has_bias without a bias to write");
    if (!(ridge >= 0.0)) return bad_arg("dw_normal_eq_solve: the ridge must not be negative");
    if (!dw_neq_aligned16(S) || (((uintptr_t)w | (uintptr_t)bias | (uintptr_t)status) & 3))
        return bad_arg("dw_normal_eq_solve: S must be 16-byte aligned, w, bias and status 4-byte aligned");
    return PLEAS_OK;
}

}  // namespace pleas

using namespace pleas;

extern "C" size_t pleas_dw_normal_eq_ws_bytes(const pleas_dw_neq_layer* layers, int n_layers) {
    if (dw_neq_check_list(layers, n_layers, false) != PLEAS_OK) return 0;
    DwNeqPlan p;
    if (dw_neq_build(p, layers, n_layers) != PLEAS_OK) return 0;
    return p.total;
}

extern "C" int pleas_dw_normal_eq_accum(const pleas_dw_neq_layer* layers, int n_layers, void* ws, size_t ws_bytes, int ws_fresh,
                                        void* stream_) {
    if (const int rc = dw_neq_check_list(layers, n_layers, true); rc != PLEAS_OK) return rc;
    if (ws && !dw_neq_aligned16(ws)) return bad_arg("dw_normal_eq_accum: the workspace must be 16-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    std::lock_guard<std::mutex> lk(g_dw_neq_mu);
    std::vector<int64_t> key;
    key.push_back(n_layers);
    key.push_back((int64_t)(uintptr_t)ws);
    for (int i = 0; i < n_layers; ++i) {
        const pleas_dw_neq_layer& l = layers[i];
        for (int v : {l.N, l.C, l.Hin, l.Win, l.K, l.stride, l.pad, l.Csrc, l.n_merged}) key.push_back(v);
    }
    DwNeqPlan* hit = nullptr;
    if (const int rc = g_dw_neq_plans.get(key, hit, [&](DwNeqPlan& p) { return dw_neq_build(p, layers, n_layers); }); rc != PLEAS_OK)
        return rc;
    DwNeqPlan& P = *hit;
    if (const int rc = g_dw_neq_plans.prepare(P, "dw_normal_eq_accum", ws, ws_bytes, ws_fresh, stream, [&] {
            return std::vector<PlanTable>{plan_table(P.off_geo, P.geo), plan_table(P.off_items, P.items),
                                          plan_table(P.off_items2, P.items2)};
        });
        rc != PLEAS_OK)
        return rc;
    char* base = (char*)ws;
    DwNeqPtrs* ptrs = reinterpret_cast<DwNeqPtrs*>(base + P.off_ptrs);
    for (int b0 = 0; b0 < n_layers; b0 += kDwNeqPtrBatch) {
        DwNeqPtrBatch pb{};
        pb.base = b0;
        pb.count = std::min(kDwNeqPtrBatch, n_layers - b0);
        for (int t = 0; t < pb.count; ++t) {
            const pleas_dw_neq_layer& l = layers[b0 + t];
            DwNeqPtrs& d = pb.l[t];
            d.p[kNqIp] = l.ip; d.p[kNqO1] = l.o1; d.p[kNqO2] = l.o2; d.p[kNqRow1] = l.row1; d.p[kNqRow2] = l.row2; d.p[kNqS] = l.S;
        }
        hipLaunchKernelGGL(dw_neq_set_ptrs_kernel, dim3(1), dim3(kDwNeqPtrBatch * kDwNeqPtrs), 0, stream, ptrs, pb);
        PLEAS_LAUNCH_CHECK("dw_neq_set_ptrs_kernel");
    }
    const DwNeqGeo* geo = reinterpret_cast<const DwNeqGeo*>(base + P.off_geo);
    double* part = reinterpret_cast<double*>(base + P.off_part);
    const DwNeqItem* items = reinterpret_cast<const DwNeqItem*>(base + P.off_items);
    size_t at = 0;
#define PLEAS_DW_NEQ_LAUNCH(KK, k)                                                                                                  \
    if (P.count[k]) {                                                                                                              \
        hipLaunchKernelGGL(dw_neq_slab_kernel<KK>, dim3((unsigned)P.count[k]), dim3(kDwNeqThreads), 0, stream, geo, ptrs, items + at, \
                           part);                                                                                                  \
        at += P.count[k];                                                                                                          \
    }
    PLEAS_DW_NEQ_LAUNCH(1, 0)
    PLEAS_DW_NEQ_LAUNCH(3, 1)
    PLEAS_DW_NEQ_LAUNCH(5, 2)
    PLEAS_DW_NEQ_LAUNCH(7, 3)
#undef PLEAS_DW_NEQ_LAUNCH
    PLEAS_LAUNCH_CHECK("dw_neq_slab_kernel");
    hipLaunchKernelGGL(dw_neq_reduce_kernel, dim3((unsigned)P.items2.size()), dim3(kDwNeqThreads), 0, stream, geo, ptrs,
                       reinterpret_cast<const DwNeqItem*>(base + P.off_items2), part);
    PLEAS_LAUNCH_CHECK("dw_neq_reduce_kernel");
    return PLEAS_OK;
}

extern "C" int pleas_dw_normal_eq_solve(const double* S, int C, int K, int has_bias, double ridge, float* w, float* bias, int* status,
                                        void* stream_) {
    if (const int rc = dw_neq_solve_check(S, C, K, has_bias, ridge, w, bias, status); rc != PLEAS_OK) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(dw_neq_solve_kernel, dim3((unsigned)ceil_div(C, kDwNeqSolveWaves)), dim3(kDwNeqSolveWaves * 64), 0, stream, S, C,
                       K, has_bias, ridge, w, bias, status);
    PLEAS_LAUNCH_CHECK("dw_neq_solve_kernel");
    return PLEAS_OK;
}

extern "C" int pleas_dw_normal_eq_solve_host(const double* S, int C, int K, int has_bias, double ridge, float* w, float* bias,
                                             int* status, void* /*stream: none, the arguments are host memory*/) {
    if (const int rc = dw_neq_solve_check(S, C, K, has_bias, ridge, w, bias, status); rc != PLEAS_OK) return rc;
    const int KK = K * K, D = KK + 2;
    std::vector<double> a(kDwNeqTri), x(kDwNeqMaxT);
    for (int c = 0; c < C; ++c) {
        const bool ok = dw_neq_solve_channel(S + (size_t)c * D * D, K, has_bias, ridge, a.data(), x.data(), 0, 1, [] {});
        status[c] = ok ? 0 : 1;
        if (!ok) continue;
        for (int t = 0; t < KK; ++t) w[(size_t)c * KK + t] = (float)x[t];
        if (has_bias) bias[c] = (float)x[KK];
    }
    return PLEAS_OK;
}
