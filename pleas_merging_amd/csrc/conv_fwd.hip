// PLeaS layer fitting on gfx950: forward of ALL merged layers of one update + regression target +
// residual + loss in one grouped fp32-MFMA launch.
//
// Replaces, per layer and per update (pleas/methods/pleas_merging.py):
//   :281  out   = layer(ip)                              (vendor conv / linear)
//   :116-123, :147  op = block-merge of the two source layers' outputs   (index_select x4 + cat)
//   :282  loss  = mean((out - op)^2)
//   first node of :287   resid = 2 (out - op) / numel
// `out` and `op` are never written: the epilogue gathers/averages the source outputs, forms the
// residual in registers, stores ONLY the residual (input of pleas_wgrad_batch) and one partial
// sum of squares per workgroup.
//
// Formulation: implicit GEMM  out[co][P] = sum_k W[co][k] * U[k][P],  P = (n, oh, ow) flattened,
// k = (ci, kh, kw) in the standard weight order.  A workgroup owns TM output channels x 128 pixels;
// W rows are K-contiguous (A operand, 16-B LDS reads feeding four MFMA steps: the NT core of nt_tile.hpp);
// U is read in place from the NCHW input: a thread owns ONE pixel for the whole K loop (its (n, oh, ow)
// is decoded once) and walks (ci, kh, kw) incrementally, so consecutive lanes read consecutive
// addresses for stride-1 layers; its 16 values of a chunk are one contiguous run of the [pixel][k] LDS
// tile (four 16-B stores), so BOTH operands are read back with the 16-B / four-MFMA-step pattern of
// nt_mma_fp32 (the flat forms below hand the core's exact step their own B sources).  The epilogue goes
// through LDS once to turn the accumulator layout (one pixel per lane) into 16-B runs along the pixel
// axis for the target gathers and the residual stores.
// Items of all layers are sorted longest-first into one grid.
//
// Work: 2*Cout*Cin*KH*KW*N*HWo flop per layer (same as the weight gradient), fp32-MFMA bound.
#include <algorithm>
#include <mutex>
#include <vector>

#include "fwd_schedule.hpp"
#include "nt_tile.hpp"

namespace pleas {

typedef short s16x4_t __attribute__((ext_vector_type(4)));   // what ds_read_tr16_b64 returns
typedef short s16x8_t __attribute__((ext_vector_type(8)));

// W tile rows: [TM][kLds] (k contiguous); U tile rows: [fTN pixels][kLds] (k contiguous: a thread's 16 k values of its pixel are one run)
constexpr int fTN = 128;

// What the epilogue of a tile does: ONE compile-time mode per kernel, so that no mode's kernel carries another's code.
//   mode       | entry point                | per-row operands | stores
//   -----------+----------------------------+------------------+-------------------------------------------------------
//   Fit        | pleas_fwd_batch            | block maps       | residual 2 (out - target) / numel, one loss partial
//   Conv       | pleas_conv2d_fwd           | none             | y = conv(x, w) + bias
//   ConvImage  | pleas_conv2d_bn_act_fwd    | scale, shift     | y and z = act(fma(y, scale, shift) (+ identity))
//   Image      | pleas_conv2d_act_fwd       | scale, shift     | z alone
//   ConvStats  | pleas_conv2d_bn_stats_fwd  | none             | y, and per tile and channel the sums of y and y^2 (fp64)
// y goes where Fit's residual goes (`resid`).  z is bn_act_kernel's arithmetic (elementwise.hip) on the value still in registers; the
// tile sums are what bn_stats_partial_kernel (bn_train.hip) would read y back for, taken from LDS in a fixed order, no atomics.
enum class FwdMode : int { Fit = 0, Conv = 1, ConvImage = 2, Image = 3, ConvStats = 4 };
constexpr int fModes = 5;
constexpr bool fwd_has_target(FwdMode m) { return m == FwdMode::Fit; }
constexpr bool fwd_has_image(FwdMode m) { return m == FwdMode::ConvImage || m == FwdMode::Image; }
constexpr bool fwd_stores_y(FwdMode m) { return m != FwdMode::Image; }
constexpr bool fwd_has_stats(FwdMode m) { return m == FwdMode::ConvStats; }

struct FwdLayerDev {
    const float* ip;      // merged input  [N][Cin][Hin][Win]
    const float* w;       // [Cout][Kd], Kd = Cin*KH*KW
    const float* bias;    // [Cout] or null
    const float* o1;      // source outputs [N][Csrc][HWo]
    const float* o2;
    const int32_t* row1;  // [Cout] block maps of the output axis (-1 = absent)
    const int32_t* row2;
    float* resid;         // [N][Cout][HWo]: Fit's residual, y of the modes that store it (null under Image)
    int Cout, Cin, Hin, Win, Hout, Wout, KH, KW, stride, pad, Csrc, n_merged;
    uint32_t HWo, Ptot, Kd;
    float dscale;         // 2 / (numel * world)
    int variant;          // bit0: TM == 64, bit1: scalar W loads, bit2: W is kernel-position-major [Cout][KH*KW][Cin],
                          // bit3: flat-shift tile (fwd_flat_tile), bits 4-5: its KIND
    int part_base;        // first loss-partial slot of this layer
    // the image modes: z = act(y * bn_scale[co] + bn_shift[co] (+ bn_res)) to `bn_z`
    int bn_relu;             // activation after the affine map (+ identity): a PLEAS_ACT_* code
    const float* bn_scale;   // [Cout]
    const float* bn_shift;   // [Cout]
    const float* bn_res;     // [N][Cout][HWo] or null
    float* bn_z;             // [N][Cout][HWo]
    // ConvStats: `st_part` [pixel tile][2][Cout][2] doubles -- segment 0 for the batch the tile's first pixel belongs to, segment 1
    // for the next one (`st_pb` pixels per batch, >= fTN or all of them)
    double* st_part;
    uint32_t st_pb;
};
struct FwdItemDev {
    int layer, tm, tp, slot;  // slot: loss-partial index
};

// ---- shared by both tile forms: the epilogue and its per-row operands.  A thread owns the TM / 8 output channels
// tid / 32 + 8 j of its tile; per channel the epilogue takes two 32-bit values and the bias: the channel's rows in the two sources'
// outputs (the block maps; -1 = absent), or, in the image modes, its BatchNorm scale and shift
template <int TM, bool IMAGE>
struct FwdRowOps {
    int row1[TM / 8], row2[TM / 8];
    float bias[TM / 8];
};
template <int TM>
struct FwdRowOps<TM, true> {
    float scale[TM / 8], shift[TM / 8];
    float bias[TM / 8];
};
template <int TM, FwdMode MODE = FwdMode::Fit>
__device__ __forceinline__ void fwd_load_maps(const FwdLayerDev& L, const int i0, FwdRowOps<TM, fwd_has_image(MODE)>& ops) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < TM / 8; ++j) {
        const int co = min(i0 + (tid >> 5) + 8 * j, L.Cout - 1);
        if constexpr (fwd_has_image(MODE)) {
            ops.scale[j] = PLEAS_GLOBAL(L.bn_scale)[co];
            ops.shift[j] = PLEAS_GLOBAL(L.bn_shift)[co];
        } else {
            // the modes without a target have no block maps: every source row is absent, the target is zero
            ops.row1[j] = L.row1 ? PLEAS_GLOBAL_I(L.row1)[co] : -1;
            ops.row2[j] = L.row2 ? PLEAS_GLOBAL_I(L.row2)[co] : -1;
        }
        ops.bias[j] = L.bias ? PLEAS_GLOBAL(L.bias)[co] : 0.f;
    }
}

// Without a target the epilogue is bias + store and leaves no loss partial; the image modes' identity takes the target's gather
// slots; the statistics pass sums the fp32 values that were stored, split at a batch boundary.
template <int TM, FwdMode MODE = FwdMode::Fit>
__device__ __forceinline__ void fwd_epilogue(const FwdLayerDev& L, const FwdItemDev& it, f32x16 (&acc)[TM / 64][2],
                                             const FwdRowOps<TM, fwd_has_image(MODE)>& ops, float* smem, float* __restrict__ partials) {
    constexpr int MTM = TM / 64;
    constexpr int ROWS = TM / 8, GB = 8, NB = ROWS / GB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int i0 = it.tm * TM;
    const uint32_t p0 = (uint32_t)it.tp * fTN;
    // ---- epilogue.  Accumulators hold one pixel per lane; go through LDS once ([co][pixel], stride 132) so that
    //      each thread then owns 4 consecutive pixels of one output channel: 16-B target gathers, 16-B residual stores.
    constexpr int EL = 132;
    float* Ct = smem;  // [TM][EL] floats <= the staging buffers just released by the last barrier of the K loop
    auto spill_acc = [&]() {
#pragma unroll
        for (int sm = 0; sm < MTM; ++sm)
#pragma unroll
            for (int sn = 0; sn < 2; ++sn)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int lco = wm * (TM / 2) + sm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    Ct[lco * EL + wn * 64 + sn * 32 + (lane & 31)] = acc[sm][sn][r];
                }
        __syncthreads();
    };
    float sq = 0.f;
    // the statistics pass gives TM / 256 threads to a channel row; that row's bias is requested here, ahead of the spill
    constexpr int SPR = kThreads / TM;       // threads per row of the statistics pass
    float st_bias = 0.f;
    if constexpr (fwd_has_stats(MODE)) st_bias = L.bias ? PLEAS_GLOBAL(L.bias)[min(i0 + tid / SPR, L.Cout - 1)] : 0.f;
    // The image's activation (bn_relu is 0, 1 or 2: fwd_describe).  The ReLU arm is the select it always was; ReLU6 is two more
    // selects against launch-uniform bounds that the other codes never reach (-inf / +inf), so every arm is straight-line code: a
    // branch around a clamp of its own costs the unrolled pass registers (an occupancy step on the 128-row forms).  Both
    // comparisons are false for a NaN: it stays, as in relu6_keep_nan -- whose values these are.
    const bool relu1 = fwd_has_image(MODE) && L.bn_relu == PLEAS_ACT_RELU, relu6 = fwd_has_image(MODE) && L.bn_relu == PLEAS_ACT_RELU6;
    const float act_lo = relu6 ? 0.f : -__builtin_inff(), act_hi = relu6 ? 6.f : __builtin_inff();
    auto act6 = [&](const float v) {
        const float f = v < act_lo ? 0.f : v;
        return f > act_hi ? 6.f : f;
    };
    const bool vec_ok = (L.HWo % 4 == 0);   // then a 4-pixel group never straddles samples and is 16-B aligned
    const int pg = (tid & 31) * 4;           // pixel group of this thread
    const uint32_t Pg = p0 + pg;
    const bool gin = Pg < L.Ptot;
    const uint32_t gn = gin ? Pg / L.HWo : 0u, gp = gin ? Pg - gn * L.HWo : 0u;
    // Each thread owns TM/8 output channels (lco = tid/32 + 8 j) x 4 pixels.  Order, chosen so that global-memory latency
    // is exposed once instead of once per step: block maps + bias -> first batch of target gathers (8 channels, branch
    // free: absent / out-of-range rows read element 0 and are masked) -> accumulators through LDS (the gathers are in
    // flight meanwhile) -> second batch issued -> first consumed -> second consumed.
    if (vec_ok) {
        f32x4 ta[NB][GB], tb[NB][GB];
        // per-thread bases: the (sample, pixel group) part of every address is the same for all of the thread's channels, so a
        // gather / store address is the tensor's uniform base pointer + ONE 32-bit multiply-add in bytes (the plan builder
        // refuses tensors of 4 GB and more)
        const uint32_t hw4 = 4u * L.HWo;
        const uint32_t gbase = 4u * (gn * (uint32_t)L.Csrc * L.HWo + gp);
        const uint32_t rbase = 4u * ((gn * (uint32_t)L.Cout + (uint32_t)i0 + (uint32_t)(tid >> 5)) * L.HWo + gp);
        // the image modes: the identity (shaped like the output) stands where the first source's outputs are gathered from
        const bool has_res = fwd_has_image(MODE) && L.bn_res != nullptr;
        const char* o1b = reinterpret_cast<const char*>(fwd_has_image(MODE) ? (has_res ? L.bn_res : L.ip) : L.o1);
        const char* o2b = reinterpret_cast<const char*>(L.o2);
        char* rb_ = reinterpret_cast<char*>(L.resid);
        char* zb_ = reinterpret_cast<char*>(L.bn_z);
        auto gather = [&](const int bt) {
#pragma unroll
            for (int u = 0; u < GB; ++u) {
                const int j = bt * GB + u;
                if constexpr (fwd_has_image(MODE)) {
                    // unconditional load from a valid address (the output's own offset into the identity; the first floats
                    // of the input for rows / pixels outside the layer and when there is no identity -- then voided by a
                    // select): no branch around a load
                    const bool live = has_res && gin && i0 + (tid >> 5) + 8 * j < L.Cout;
                    const uint32_t oz = live ? rbase + (uint32_t)(8 * j) * hw4 : 0u;
                    const f32x4 idn = *(const __attribute__((address_space(1))) f32x4*)(o1b + oz);
                    ta[bt][u] = has_res ? idn : f32x4{0.f, 0.f, 0.f, 0.f};
                } else if constexpr (!fwd_has_target(MODE)) {
                    ta[bt][u] = tb[bt][u] = f32x4{0.f, 0.f, 0.f, 0.f};
                } else {
                    const uint32_t oa = (gin && ops.row1[j] >= 0) ? gbase + (uint32_t)ops.row1[j] * hw4 : 0u;
                    const uint32_t ob = (gin && ops.row2[j] >= 0) ? gbase + (uint32_t)ops.row2[j] * hw4 : 0u;
                    ta[bt][u] = *(const __attribute__((address_space(1))) f32x4*)(o1b + oa);
                    tb[bt][u] = *(const __attribute__((address_space(1))) f32x4*)(o2b + ob);
                }
            }
        };
        auto consume = [&](const int bt) {
#pragma unroll
            for (int u = 0; u < GB; ++u) {
                const int j = bt * GB + u;
                const int lco = (tid >> 5) + 8 * j, co = i0 + lco;
                const bool live = gin && co < L.Cout;
                if constexpr (fwd_has_image(MODE)) {
                    const f32x4 o = *reinterpret_cast<const f32x4*>(Ct + lco * EL + pg);
                    f32x4 y, z;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        y[e] = o[e] + ops.bias[j];
                        const float sm = fmaf(y[e], ops.scale[j], ops.shift[j]) + ta[bt][u][e];
                        z[e] = act6(relu1 ? fmaxf(sm, 0.f) : sm);
                    }
                    if (live) {
                        if constexpr (fwd_stores_y(MODE)) *(__attribute__((address_space(1))) f32x4*)(rb_ + (rbase + (uint32_t)(8 * j) * hw4)) = y;
                        *(__attribute__((address_space(1))) f32x4*)(zb_ + (rbase + (uint32_t)(8 * j) * hw4)) = z;
                    }
                } else {
                    // target = (o1 * [present] + o2 * [present]) * coef, coef in {0.5, 1}: folding coef into the two factors is
                    // exact (power of two), so  fma(o2, cb, o1 * ca)  rounds once, like the sum it replaces
                    const float coef = co < L.n_merged ? 0.5f : 1.0f;
                    const float ca = ops.row1[j] >= 0 ? coef : 0.f, cb = ops.row2[j] >= 0 ? coef : 0.f;
                    const f32x4 o = *reinterpret_cast<const f32x4*>(Ct + lco * EL + pg);
                    f32x4 d;
                    float s4 = 0.f;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float dd = (o[e] + ops.bias[j]) - fmaf(tb[bt][u][e], cb, ta[bt][u][e] * ca);
                        s4 = fmaf(dd, dd, s4);
                        d[e] = L.dscale * dd;
                    }
                    sq += live ? s4 : 0.f;
                    if (live) *(__attribute__((address_space(1))) f32x4*)(rb_ + (rbase + (uint32_t)(8 * j) * hw4)) = d;
                }
            }
        };
        gather(0);
        spill_acc();
        if constexpr (NB > 1) gather(1);
        consume(0);
        if constexpr (NB > 1) consume(1);
    } else {
        spill_acc();
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            const int lco = (tid >> 5) + 8 * j, co = i0 + lco;
            if (co >= L.Cout || !gin) continue;
            const float coef = co < L.n_merged ? 0.5f : 1.0f;
            const f32x4 o = *reinterpret_cast<const f32x4*>(Ct + lco * EL + pg);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t Pe = Pg + e;
                if (Pe >= L.Ptot) break;
                const uint32_t n = Pe / L.HWo, p = Pe - n * L.HWo;
                if constexpr (fwd_has_image(MODE)) {
                    const size_t at = ((size_t)n * L.Cout + co) * L.HWo + p;
                    const float y = o[e] + ops.bias[j];
                    const float sm = fmaf(y, ops.scale[j], ops.shift[j]) + (L.bn_res ? PLEAS_GLOBAL(L.bn_res)[at] : 0.f);
                    if constexpr (fwd_stores_y(MODE)) PLEAS_GLOBAL_W(L.resid)[at] = y;
                    PLEAS_GLOBAL_W(L.bn_z)[at] = act6(relu1 ? fmaxf(sm, 0.f) : sm);
                } else {
                    float a = 0.f, b = 0.f;
                    if (ops.row1[j] >= 0) a = PLEAS_GLOBAL(L.o1)[((size_t)n * L.Csrc + ops.row1[j]) * L.HWo + p];
                    if (ops.row2[j] >= 0) b = PLEAS_GLOBAL(L.o2)[((size_t)n * L.Csrc + ops.row2[j]) * L.HWo + p];
                    const float dd = (o[e] + ops.bias[j]) - (a + b) * coef;
                    sq = fmaf(dd, dd, sq);
                    PLEAS_GLOBAL_W(L.resid)[((size_t)n * L.Cout + co) * L.HWo + p] = L.dscale * dd;
                }
            }
        }
    }
    if constexpr (fwd_has_stats(MODE)) {
        // Thread (row r, part q) sums NCH 16-byte groups of its row: q's groups are q * NCH .. + NCH - 1, visited from a start
        // that is rotated per q so that the 16 lanes of a ds_read_b128 group fall on 16 different bank quads (rows are 33 quads
        // apart).  The order is a function of (r, q) alone: the same bits run after run.
        constexpr int NCH = 32 / SPR;
        const int r = tid / SPR, q = tid % SPR;
        const int skew = (NCH / 2) * (SPR == 2 ? q : q >> 1);
        // live pixels of the tile: [0, n0) belong to the first batch it touches, [n0, n1) to the next one
        const uint32_t bnext = (p0 / L.st_pb + 1u) * L.st_pb;
        const uint32_t n1 = min(L.Ptot - p0, (uint32_t)fTN), n0 = min(bnext - p0, n1);
        double a0 = 0.0, b0 = 0.0, a1 = 0.0, b1 = 0.0;
        const float* row = Ct + r * EL + q * NCH * 4;
        if (n0 == (uint32_t)fTN) {           // block-uniform: a whole tile inside one batch, nothing to select
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const f32x4 o = *reinterpret_cast<const f32x4*>(row + 4 * ((i + skew) % NCH));
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const double v = (double)(o[e] + st_bias);
                    a0 += v;
                    b0 = fma(v, v, b0);
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int g = (i + skew) % NCH;
                const f32x4 o = *reinterpret_cast<const f32x4*>(row + 4 * g);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t px = (uint32_t)(4 * (q * NCH + g) + e);
                    const double v = (double)(o[e] + st_bias);
                    const double v0 = px < n0 ? v : 0.0, v1 = (px >= n0 && px < n1) ? v : 0.0;
                    a0 += v0;
                    b0 = fma(v0, v0, b0);
                    a1 += v1;
                    b1 = fma(v1, v1, b1);
                }
            }
        }
        // the row's SPR parts: a butterfly over adjacent lanes (every lane ends with the same sum, formed in the same order)
#pragma unroll
        for (int off = 1; off < SPR; off <<= 1) {
            a0 += __shfl_xor(a0, off);
            b0 += __shfl_xor(b0, off);
            a1 += __shfl_xor(a1, off);
            b1 += __shfl_xor(b1, off);
        }
        const int co = i0 + r;
        if (q == 0 && co < L.Cout) {
            double* seg = L.st_part + ((size_t)it.tp * 2 * L.Cout + co) * 2;
            seg[0] = a0;
            seg[1] = b0;
            if (n1 > n0) {                   // block-uniform: the tile reaches into the next batch
                seg[(size_t)L.Cout * 2 + 0] = a1;
                seg[(size_t)L.Cout * 2 + 1] = b1;
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sq += __shfl_xor(sq, off);
    __syncthreads();  // everyone is done with Ct: reuse its first floats for the block sum
    if (lane == 0) smem[wave] = sq;
    __syncthreads();
    if (tid == 0 && partials) partials[L.part_base + it.slot] = (smem[0] + smem[1]) + (smem[2] + smem[3]);
}

// The weight rows a thread stages per chunk, for both tile forms: LPR lanes share a row's 32 k (VEC floats each), the 256 threads
// cover RPP rows per pass and the tile's TM rows in PASS passes.  SPLIT_ROWS: the rows of a pass are permuted so that the split
// planes are written without bank conflicts (split_stage_row, common.hpp).
template <int TM, int VEC, bool SPLIT_ROWS = false>
struct FwdWeightRows {
    static constexpr int LPR = kBK / VEC, RPP = kThreads / LPR, PASS = TM / RPP;
    int arow, acol;           // first row of this thread in the tile, its k offset in the chunk
    unsigned oka = 0;         // bit q: row arow + q * RPP is a channel of the layer
    uint32_t offa[PASS];      // where that row starts in W (clamped to the last channel: loads stay in bounds, oka masks them)
    __device__ __forceinline__ FwdWeightRows(const FwdLayerDev& L, const int i0) {
        const int tid = threadIdx.x;
        arow = SPLIT_ROWS ? split_stage_row(tid / LPR) : tid / LPR;
        acol = (tid % LPR) * VEC;
#pragma unroll
        for (int q = 0; q < PASS; ++q) {
            const int gi = i0 + arow + q * RPP;
            if (gi < L.Cout) oka |= 1u << q;
            offa[q] = (uint32_t)min(gi, L.Cout - 1) * L.Kd;
        }
    }
};

template <int TM, int VECA, FwdMode MODE = FwdMode::Fit>
__device__ __forceinline__ void fwd_tile(const FwdLayerDev& L, const FwdItemDev& it, float* smem, float* __restrict__ partials) {
    constexpr int MTM = TM / 64;
    using WRows = FwdWeightRows<TM, VECA>;
    constexpr int RPP = WRows::RPP, PASS = WRows::PASS;
    float* As = smem;                      // [2][TM][kLds]
    float* Bs = smem + 2 * TM * kLds;      // [2][fTN][kLds]
    const int tid = threadIdx.x;
    const int i0 = it.tm * TM;
    const uint32_t p0 = (uint32_t)it.tp * fTN;
    const uint32_t HWi = (uint32_t)L.Hin * L.Win;
    const int R = L.KH * L.KW;
    const bool kpos = (L.variant & 4) != 0;
    const int nchunks = (int)((L.Kd + kBK - 1) / kBK);

    // ---- A (weights) staging: rows co, k contiguous
    const WRows wr(L, i0);
    const int arow = wr.arow, acol = wr.acol;
    float ra[PASS][VECA];
    // ---- B (input) staging: this thread's pixel and half of the chunk's k rows
    const int bpix = tid & 127;
    const int bhalf = __builtin_amdgcn_readfirstlane(tid >> 7);  // wave-uniform: the k walk below stays on the scalar unit
    const uint32_t P = p0 + bpix;
    const bool pin = P < L.Ptot;
    const uint32_t pn = pin ? P / L.HWo : 0u, pp = pin ? P - pn * L.HWo : 0u;
    const int oh = (int)(pp / (uint32_t)L.Wout), ow = (int)(pp - (uint32_t)oh * L.Wout);
    const int ih0 = oh * L.stride - L.pad, iw0 = ow * L.stride - L.pad;
    const size_t pbase = (size_t)pn * L.Cin * HWi;
    float rb[16];
    unsigned okb = 0;
    bool kina = false;
    // per-pixel tap table for kernels larger than 1x1 (KH*KW <= 64, checked on the host)
    unsigned long long tapmask = 0;
    const long long pixoff = (long long)ih0 * L.Win + iw0;
    for (int r = 0; r < R; ++r) {
        const int kh = r / L.KW, kw = r - kh * L.KW;
        const bool ok = pin && ih0 + kh >= 0 && ih0 + kh < L.Hin && iw0 + kw >= 0 && iw0 + kw < L.Win;
        tapmask |= (unsigned long long)ok << r;
    }

    f32x16 acc[MTM][2];
    nt_zero(acc);

    auto load_chunk = [&](int c) {
        {
            // kernel-position-major weights: chunk c = (channel block c / R, tap c % R); its 32 k values sit at
            // [tap][block * 32 ..] of the weight row
            const uint32_t k = kpos ? (uint32_t)(c % R) * L.Cin + (uint32_t)(c / R) * kBK + acol : (uint32_t)c * kBK + acol;
            kina = k < L.Kd;
            const uint32_t kc = kina ? k : 0u;
#pragma unroll
            for (int q = 0; q < PASS; ++q) {
                if constexpr (VECA == 4) {
                    const f32x4 v = *(const __attribute__((address_space(1))) f32x4*)(PLEAS_GLOBAL(L.w) + wr.offa[q] + kc);
#pragma unroll
                    for (int e = 0; e < 4; ++e) ra[q][e] = v[e];
                } else {
                    ra[q][0] = PLEAS_GLOBAL(L.w)[wr.offa[q] + kc];
                }
            }
        }
        {
            // Every lane of a wave walks the SAME k values (wave-uniform ci, kh, kw); only the pixel differs.
            // Loads are unconditional: an out-of-range tap reads element 0 (offset masked to zero, no branch) and is
            // zeroed when the tile is written to LDS.
            const uint32_t k = (uint32_t)c * kBK + bhalf * 16;
            okb = 0;
            if (R == 1 || kpos) {
                // ONE tap per chunk (1x1 / Linear, or kernel-position-major weights: channel block c / R, tap c % R; the
                // taps of a channel block run back to back, so their shifted re-reads of the same input rows hit L1/L2).
                // Per thread: one masked base offset per chunk; per load: + a wave-uniform channel offset.
                const int cb = kpos ? c / R : c;
                const int r = kpos ? c - cb * R : 0;
                const int kh = r / L.KW, kw = r - kh * L.KW;
                const bool ok_tap = (tapmask >> r) & 1ull;
                const uint32_t ch0 = (uint32_t)cb * kBK + bhalf * 16;
                const long long voff = ok_tap ? (long long)pbase + pixoff + (kh * L.Win + kw) : 0ll;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const uint32_t ch = ch0 + q;
                    const bool ok = ok_tap && ch < (uint32_t)L.Cin;
                    okb |= (ok ? 1u : 0u) << q;
                    const long long lin = (long long)min(ch, (uint32_t)L.Cin - 1u) * HWi;   // scalar; masked lanes read ip[lin]
                    rb[q] = PLEAS_GLOBAL(L.ip)[voff + lin];
                }
            } else {
                // general kernel: the tap validity of this thread's pixel is a precomputed bit mask and its pixel
                // offset a constant; (ci, r, kh, kw) are wave-uniform and walk on the scalar unit
                int ci = (int)(k / (uint32_t)R);
                int r = (int)(k - (uint32_t)ci * R);
                int kh = r / L.KW, kw = r - kh * L.KW;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const bool ok = ((tapmask >> r) & 1ull) && (k + q) < L.Kd;
                    okb |= (ok ? 1u : 0u) << q;
                    const long long lin = (long long)ci * HWi + kh * L.Win + kw;   // scalar
                    const size_t off = (size_t)((long long)pbase + pixoff + lin) & (size_t)(-(long long)ok);
                    rb[q] = PLEAS_GLOBAL(L.ip)[off];
                    ++r;
                    ++kw;
                    const int cw = kw == L.KW;
                    kw = cw ? 0 : kw;
                    kh += cw;
                    const int cr = r == R;
                    r = cr ? 0 : r;
                    kh = cr ? 0 : kh;
                    ci += cr;
                }
            }
        }
    };
    auto store_chunk = [&](int buf) {
        float* a = As + buf * TM * kLds;
        float* b = Bs + buf * fTN * kLds;
#pragma unroll
        for (int q = 0; q < PASS; ++q) {
            const bool ok = kina && ((wr.oka >> q) & 1u);
            const int row = arow + q * RPP;
            if constexpr (VECA == 4) {
                f32x4 v = {ok ? ra[q][0] : 0.f, ok ? ra[q][1] : 0.f, ok ? ra[q][2] : 0.f, ok ? ra[q][3] : 0.f};
                *reinterpret_cast<f32x4*>(a + row * kLds + acol) = v;
            } else {
                a[row * kLds + acol] = ok ? ra[q][0] : 0.f;
            }
        }
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = ((okb >> (q4 * 4 + e)) & 1u) ? rb[q4 * 4 + e] : 0.f;
            *reinterpret_cast<f32x4*>(b + bpix * kLds + bhalf * 16 + q4 * 4) = v;
        }
    };
    auto compute = [&](int buf) { nt_mma_fp32<TM, fTN>(As, Bs, buf, acc); };

    // nt_pipeline<0>'s order with the last chunk taken out of the loop: the block maps and biases of the epilogue are requested
    // before the LAST chunk's MFMAs (no staging loads are in flight then), so that their round trip is covered by that chunk
    // instead of opening the epilogue.  (Requested from nt_pipeline's compute callback they are live across its loop: the 128-row
    // forms then spill 164-320 B per lane.)
    load_chunk(0);
    store_chunk(0);
    __syncthreads();
    FwdRowOps<TM, fwd_has_image(MODE)> ops;
    for (int c = 0; c + 1 < nchunks; ++c) {
        const int buf = c & 1;
        load_chunk(c + 1);
        compute(buf);
        store_chunk(buf ^ 1);
        __syncthreads();
    }
    fwd_load_maps<TM, MODE>(L, i0, ops);
    compute((nchunks - 1) & 1);
    __syncthreads();

    fwd_epilogue<TM, MODE>(L, it, acc, ops, smem, partials);
}


// ------------------------------------------------------------------------------------------------------------------
// "Flat-shift" tile: stride-1, same-size convolutions (1x1, 3x3 pad 1, 5x5 pad 2 ...) with Cin % 32 == 0 -- 97 % of a
// ResNet's merged-layer flops.  For a fixed channel the HW pixels of a sample are contiguous, and tap (kh, kw) of a
// stride-1 same-size convolution reads the SAME flat pixel run shifted by delta = (kh - pad) * W + (kw - pad).  So the
// input operand of a whole channel block (32 channels x all KH*KW taps) is ONE LDS image
//     Bs[k][j],  j = 0 .. 128 + 2 * halo,   halo = pad * (W + 1),   holding flat pixels p0 - halo .. p0 + 127 + halo,
// loaded once per channel block (16-B loads along the pixel axis for 1x1 layers, 9x fewer loads than one gather per tap
// for 3x3), and the MFMA B fragment of tap r is a plain ds_read_b32 at  Bs[k][halo + pixel + delta_r].  Border taps
// (left / right column, top / bottom row, neighbouring sample) are not masked value by value: a lane whose pixel does not
// have tap r reads the row's ZERO COLUMN instead (one select on the address per tap and 32-pixel fragment).
// Weights: kernel-position-major chunks (tap r, channel block) exactly as in fwd_tile; accumulators and epilogue shared.
constexpr int fFlatRow1 = 132;     // Bs row stride of 1x1 layers: 128 pixels + zero column, 16-B aligned rows
constexpr int fFlatPix = 36;       // k x k image since round 4: [column][36] -- a pixel's 32 channels contiguous (+ 4 pad: 16-byte
                                   // aligned rows, conflict-free ds_read_b128 as for the weight tile), so that ONE 16-byte LDS read
                                   // feeds four MFMA steps instead of four 4-byte reads (an LDS read costs the SIMD ~10 cycles
                                   // whatever its width)
constexpr int fFlatColsK = 248;    // columns of that image: 128 + 2 * halo data columns + one zero row
// KIND 0: 1x1, 16-B loads along the pixel axis (HW % 4 == 0), two images (double buffer)
// KIND 1: 1x1, scalar loads (HW % 4 != 0, e.g. 7 x 7), two images
// KIND 2: k x k, scalar loads, ONE image per channel block shared by all taps
// SPLIT = 1 / 2 (pleas_arith(PLEAS_ARITH_SPLIT_BF16 / _EXACT); KIND 0 and 2): every chunk goes to LDS as three bf16 planes
// (common.hpp), ONE image per operand (two barriers per chunk), six / nine v_mfma_f32_32x32x16_bf16 per 16-deep k step.
//   weights:      [TM][kSplitRow] rows (3 planes x 32 k), fragments by ds_read_b128 -- the operand map of the MFMA
//   k x k input:  [column][kSplitRow], a pixel's 32 channels contiguous per plane: the same 16-byte fragment reads
//   1 x 1 input:  [plane][k][fSplitPixRow] (pixels contiguous, as they come from memory: 8-byte writes), fragments by
//                 ds_read_b64_tr_b16 -- the hardware transposes 4 k x 16 pixels per 16-lane group
constexpr int fSplitPixRow = 160;  // bf16 per k row of the 1 x 1 split image: 128 pixels + 32 pad = 320 B (rows 16 banks apart:
                                   // the four rows x eight 8-byte column chunks of a half-wave's transposed read hit 32 distinct bank pairs)
template <int TM, int KIND, int SPLIT = 0, FwdMode MODE = FwdMode::Fit>
__device__ __forceinline__ void fwd_flat_tile(const FwdLayerDev& L, const FwdItemDev& it, float* smem, float* __restrict__ partials) {
    static_assert(!SPLIT || KIND != 1, "the scalar 1 x 1 form (7 x 7 images) has no split variant");
    constexpr int MTM = TM / 64;
    using WRows = FwdWeightRows<TM, 4, SPLIT != 0>;                      // weight staging: 16-B loads
    constexpr int RPP = WRows::RPP, PASS = WRows::PASS;
    constexpr int Lr = KIND == 2 ? fFlatPix : fFlatRow1;                // compile-time: LDS offsets are immediates
    constexpr int jz = KIND == 2 ? fFlatColsK - 1 : Lr - 1;              // the zero column (k x k: the zero ROW of the image)
    constexpr int NBUF = KIND == 2 ? 1 : 2;
    constexpr int MCOL = KIND == 2 ? 4 : 2;                              // scalar form: column passes of 64 lanes
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int i0 = it.tm * TM;
    const uint32_t p0 = (uint32_t)it.tp * fTN;
    const int R = KIND == 2 ? L.KH * L.KW : 1;
    const int W = L.Win;
    const uint32_t HW = L.HWo;                       // == Hin * Win
    const int halo = KIND == 2 ? L.pad * (W + 1) : 0;
    const int span = fTN + 2 * halo;                 // data columns of a Bs row
    const int CB = L.Cin / kBK;
    const int nchunks = CB * R;
    float* As = smem;                                // [2][TM][kLds]
    float* Bs = smem + 2 * TM * kLds;                // 1x1: [NBUF][32][Lr]; k x k: [fFlatColsK][fFlatPix]
    __bf16* As16 = reinterpret_cast<__bf16*>(smem);  // SPLIT: [TM][kSplitRow]
    __bf16* Bs16 = As16 + TM * kSplitRow;            // SPLIT: k x k [fFlatColsK][kSplitRow]; 1 x 1 [3][32][fSplitPixRow]

    // ---- A (weights) staging, as in fwd_tile with VECA = 4
    const WRows wr(L, i0);
    const int arow = wr.arow, acol = wr.acol;
    f32x4 ra0[PASS], ra1[PASS];    // two register sets: the weights of chunk c + 2 are requested while chunk c computes
    // ---- B (input) staging.
    //   KIND 0: thread = (row tid / 32 + 8 i, pixel group tid % 32), i < 4: four 16-B loads per chunk
    //   else  : wave w owns rows 8 w .. 8 w + 7, lane covers columns lane + 64 m (columns >= span unused)
    uint32_t voff[MCOL];
    unsigned vok = 0;
    constexpr int NRB = KIND == 0 ? 16 : 8 * MCOL;
    float rb0[NRB], rb1[KIND == 2 ? 1 : NRB];   // 1x1 forms: two sets as well (a new image every chunk)
    if constexpr (KIND == 0) {
        const uint32_t P4 = p0 + 4u * (tid & 31);
        const bool ok = P4 < L.Ptot;
        const uint32_t n = ok ? P4 / HW : 0u, p = ok ? P4 - n * HW : 0u;
        voff[0] = ok ? n * (uint32_t)L.Cin * HW + p + (uint32_t)(tid >> 5) * HW : 0u;
        voff[1] = 0;
        vok = ok ? 1u : 0u;
    } else {
#pragma unroll
        for (int m = 0; m < MCOL; ++m) {
            const int j = lane + 64 * m;
            const long long Pv = (long long)p0 - halo + j;
            const bool ok = j < span && Pv >= 0 && Pv < (long long)L.Ptot;
            const uint32_t n = ok ? (uint32_t)Pv / HW : 0u, p = ok ? (uint32_t)Pv - n * HW : 0u;
            voff[m] = ok ? n * (uint32_t)L.Cin * HW + p : 0u;
            vok |= (ok ? 1u : 0u) << m;
        }
    }
    const int M = (span + 63) / 64;                    // scalar form: column passes that hold data (wave-uniform)

    // ---- MFMA-side view of this lane's two pixels (fragments sn = 0, 1): LDS column and tap validity
    int jb[2];
    unsigned tapok[2];
#pragma unroll
    for (int sn = 0; sn < 2; ++sn) {
        const int q = wn * 64 + sn * 32 + (lane & 31);
        const uint32_t P = p0 + q;
        jb[sn] = halo + q;
        unsigned mask = 0;
        if (P < L.Ptot) {
            if constexpr (KIND == 2) {
                const uint32_t n = P / HW, pp = P - n * HW;
                const int oh = (int)(pp / (uint32_t)W), ow = (int)(pp - (uint32_t)oh * W);
                for (int r = 0; r < R; ++r) {
                    const int kh = r / L.KW, kw = r - kh * L.KW;
                    const int ih = oh + kh - L.pad, iw = ow + kw - L.pad;
                    mask |= (unsigned)(ih >= 0 && ih < L.Hin && iw >= 0 && iw < W) << r;
                }
            } else {
                mask = 1u;
            }
        }
        tapok[sn] = mask;
    }

    f32x16 acc[MTM][2];
    nt_zero(acc);

    auto load_a = [&](int cb, int r, f32x4 (&ra)[PASS]) {
        const uint32_t k = (uint32_t)r * L.Cin + (uint32_t)cb * kBK + acol;    // kernel-position-major (== plain for 1x1)
#pragma unroll
        for (int q = 0; q < PASS; ++q) ra[q] = *(const __attribute__((address_space(1))) f32x4*)(PLEAS_GLOBAL(L.w) + wr.offa[q] + k);
    };
    // Tiles whose rows / pixels all exist store their staged values as they are (block-uniform tests): every select that is
    // not executed is vector-pipe time the fp32 MFMAs get back (a vector instruction costs ~4.5 cycles of it).
    const bool full_a = i0 + TM <= L.Cout;
    const bool full_b = p0 + fTN <= L.Ptot;
    auto store_a = [&](int buf, const f32x4 (&ra)[PASS]) {
        if constexpr (SPLIT) {
#pragma unroll
            for (int q = 0; q < PASS; ++q) {
                const bool ok = full_a || ((wr.oka >> q) & 1u);
                split3_store4(As16 + (arow + q * RPP) * kSplitRow, acol, ok ? ra[q][0] : 0.f, ok ? ra[q][1] : 0.f,
                              ok ? ra[q][2] : 0.f, ok ? ra[q][3] : 0.f);
            }
            return;
        }
        float* a = As + buf * TM * kLds;
        if (full_a) {
#pragma unroll
            for (int q = 0; q < PASS; ++q) *reinterpret_cast<f32x4*>(a + (arow + q * RPP) * kLds + acol) = ra[q];
            return;
        }
#pragma unroll
        for (int q = 0; q < PASS; ++q) {
            const bool ok = (wr.oka >> q) & 1u;
            const f32x4 v = {ok ? ra[q][0] : 0.f, ok ? ra[q][1] : 0.f, ok ? ra[q][2] : 0.f, ok ? ra[q][3] : 0.f};
            *reinterpret_cast<f32x4*>(a + (arow + q * RPP) * kLds + acol) = v;
        }
    };
    auto load_b = [&](int cb, auto& rb) {
        const cgfloat* base = PLEAS_GLOBAL(L.ip) + (size_t)cb * kBK * HW;
        if constexpr (KIND == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4 v = *(const __attribute__((address_space(1))) f32x4*)(base + voff[0] + (uint32_t)(8 * i) * HW);
#pragma unroll
                for (int e = 0; e < 4; ++e) rb[4 * i + e] = v[e];
            }
        } else {
            const cgfloat* wbase = base + (size_t)(8 * wave) * HW;     // wave-uniform row block
#pragma unroll
            for (int kr = 0; kr < 8; ++kr)
#pragma unroll
                for (int m = 0; m < MCOL; ++m)
                    if (m < M) rb[kr * MCOL + m] = wbase[(size_t)kr * HW + voff[m]];
        }
    };
    auto store_b = [&](int buf, const auto& rb) {
        if constexpr (SPLIT && KIND == 0) {
            // this thread holds k rows tid / 32 + 8 i of pixels 4 (tid % 32) .. + 3: per row and plane one 8-byte write
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                uint32_t lo[3], hi[3];
                split3_pair(vok ? rb[4 * i] : 0.f, vok ? rb[4 * i + 1] : 0.f, lo);
                split3_pair(vok ? rb[4 * i + 2] : 0.f, vok ? rb[4 * i + 3] : 0.f, hi);
#pragma unroll
                for (int p = 0; p < 3; ++p)
                    *reinterpret_cast<u32x2_t*>(Bs16 + (p * kBK + (tid >> 5) + 8 * i) * fSplitPixRow + 4 * (tid & 31)) = u32x2_t{lo[p], hi[p]};
            }
            return;
        } else if constexpr (SPLIT && KIND == 2) {
            // channels 8 wave .. + 7 of columns lane + 64 m: per column and plane ONE 16-byte write
#pragma unroll
            for (int m = 0; m < MCOL; ++m)
                if (m < M && lane + 64 * m < span) {
                    const bool ok = (vok >> m) & 1u;
                    uint32_t w[4][3];
#pragma unroll
                    for (int h = 0; h < 4; ++h)
                        split3_pair(ok ? rb[(2 * h) * MCOL + m] : 0.f, ok ? rb[(2 * h + 1) * MCOL + m] : 0.f, w[h]);
#pragma unroll
                    for (int p = 0; p < 3; ++p)
                        *reinterpret_cast<u32x4_t*>(Bs16 + (lane + 64 * m) * kSplitRow + p * 32 + 8 * wave) =
                            u32x4_t{w[0][p], w[1][p], w[2][p], w[3][p]};
                }
            return;
        }
        float* b = Bs + buf * kBK * Lr;
        if constexpr (KIND == 0) {
            if (full_b) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f32x4 v = {rb[4 * i], rb[4 * i + 1], rb[4 * i + 2], rb[4 * i + 3]};
                    *reinterpret_cast<f32x4*>(b + ((tid >> 5) + 8 * i) * Lr + 4 * (tid & 31)) = v;
                }
                return;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4 v = {vok ? rb[4 * i] : 0.f, vok ? rb[4 * i + 1] : 0.f, vok ? rb[4 * i + 2] : 0.f, vok ? rb[4 * i + 3] : 0.f};
                *reinterpret_cast<f32x4*>(b + ((tid >> 5) + 8 * i) * Lr + 4 * (tid & 31)) = v;
            }
        } else if constexpr (KIND == 2) {
            // this thread holds channels 8 wave .. + 7 of columns lane + 64 m: two 16-byte runs of the column's row
#pragma unroll
            for (int m = 0; m < MCOL; ++m)
                if (m < M && lane + 64 * m < span) {
                    const bool ok = (vok >> m) & 1u;
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const f32x4 v = {ok ? rb[(4 * h + 0) * MCOL + m] : 0.f, ok ? rb[(4 * h + 1) * MCOL + m] : 0.f,
                                         ok ? rb[(4 * h + 2) * MCOL + m] : 0.f, ok ? rb[(4 * h + 3) * MCOL + m] : 0.f};
                        *reinterpret_cast<f32x4*>(b + (lane + 64 * m) * fFlatPix + 8 * wave + 4 * h) = v;
                    }
                }
        } else {
#pragma unroll
            for (int kr = 0; kr < 8; ++kr)
#pragma unroll
                for (int m = 0; m < MCOL; ++m)
                    if (m < M && lane + 64 * m < span)
                        b[(8 * wave + kr) * Lr + lane + 64 * m] = ((vok >> m) & 1u) ? rb[kr * MCOL + m] : 0.f;
        }
    };
    // tap offsets of a k x k layer without a division per chunk: tap r -> r + 1 is one pixel to the right, or (at the end of a
    // kernel row) W - KW + 1 pixels on; taps are visited in order 0 .. R - 1 per channel block (all scalar-unit arithmetic)
    const int delta0 = -(L.pad * W + L.pad);
    auto tap_delta = [&](int r) {
        if constexpr (KIND != 2) return 0;
        int kh = 0, rr = r;
        while (rr >= L.KW) { rr -= L.KW; ++kh; }      // r < 32, KW >= 3: at most a few scalar steps
        return delta0 + kh * W + rr;
    };
    // One chunk.  A lane whose tap (k x k) or pixel (1 x 1: past the tensor's end) is not there takes 0 by reading the image's zero
    // row / the row's zero column: one select on the address per tap and fragment instead of one per value, made here, outside
    // the k loops.  Exact: the core's step (nt_mma_fp32_from) with this form's B source.  Split: written out -- unlike
    // nt_mma_split it reads all A fragments of a k group before the B fragments, and the 1 x 1 form's B fragments pixel fragment
    // by pixel fragment; that order is kept.
    auto compute = [&](int abuf, int bbuf, int r) {
        const int delta = tap_delta(r);
        const bool ok0 = (tapok[0] >> r) & 1u, ok1 = (tapok[1] >> r) & 1u;
        if constexpr (SPLIT) {
            const __bf16* a16 = As16 + (wm * (TM / 2) + (lane & 31)) * kSplitRow + 8 * (lane >> 5);
#pragma unroll
            for (int g16 = 0; g16 < kBK / 16; ++g16) {
                bf16x8_t sa[MTM][3], sb[2][3];
#pragma unroll
                for (int p = 0; p < 3; ++p)
#pragma unroll
                    for (int s_ = 0; s_ < MTM; ++s_) sa[s_][p] = *reinterpret_cast<const bf16x8_t*>(a16 + s_ * 32 * kSplitRow + p * 32 + g16 * 16);
                if constexpr (KIND == 2) {
                    // [column][kSplitRow] image: this lane's (shifted) column per fragment, read like the weights
                    const __bf16* c0 = Bs16 + (ok0 ? jb[0] + delta : jz) * kSplitRow + 8 * (lane >> 5) + g16 * 16;
                    const __bf16* c1 = Bs16 + (ok1 ? jb[1] + delta : jz) * kSplitRow + 8 * (lane >> 5) + g16 * 16;
#pragma unroll
                    for (int p = 0; p < 3; ++p) {
                        sb[0][p] = *reinterpret_cast<const bf16x8_t*>(c0 + p * 32);
                        sb[1][p] = *reinterpret_cast<const bf16x8_t*>(c1 + p * 32);
                    }
                } else {
                    // transposed reads: lane 4 q + pp of a 16-lane group supplies row q, columns 4 pp .. + 3 of the group's
                    // 4 k x 16 pixel block and receives its own pixel's four k; two reads give the lane its 8 k
                    const int u = (lane >> 4) & 1, q = (lane >> 2) & 3, pp = lane & 3;
                    const int krow = g16 * 16 + 8 * (lane >> 5) + q;
#pragma unroll
                    for (int sn = 0; sn < 2; ++sn)
#pragma unroll
                        for (int p = 0; p < 3; ++p) {
                            const __bf16* base = Bs16 + (p * kBK + krow) * fSplitPixRow + wn * 64 + sn * 32 + 16 * u + 4 * pp;
                            const s16x4_t lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(base));
                            const s16x4_t hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(base + 4 * fSplitPixRow));
                            const s16x8_t both = {lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], hi4[2], hi4[3]};
                            sb[sn][p] = __builtin_bit_cast(bf16x8_t, both);
                        }
                }
#pragma unroll
                for (int sm = 0; sm < MTM; ++sm) {
                    acc[sm][0] = split3_mfma<split_products(SPLIT)>(sa[sm], sb[0], acc[sm][0]);
                    acc[sm][1] = split3_mfma<split_products(SPLIT)>(sa[sm], sb[1], acc[sm][1]);
                }
                // nine products: nothing moves across the end of a k group.  Left to itself the scheduler keeps three values more
                // alive than the 256 registers of two workgroups per CU hold (the plain 128-row 1 x 1 kernel spilled 12 bytes).
                if constexpr (SPLIT == 2) __builtin_amdgcn_sched_barrier(0);
            }
        } else {
            const float* a = As + abuf * TM * kLds + (wm * (TM / 2) + (lane & 31)) * kLds + 4 * (lane >> 5);
            if constexpr (KIND == 2) {
                // [column][k] image: a lane's four k of an MFMA group are ONE 16-byte read of its (shifted) column
                const float* c[2] = {Bs + (ok0 ? jb[0] + delta : jz) * fFlatPix + 4 * (lane >> 5),
                                     Bs + (ok1 ? jb[1] + delta : jz) * fFlatPix + 4 * (lane >> 5)};
                nt_mma_fp32_from<TM, fTN>(a, [&](int sn, int kk) { return *reinterpret_cast<const f32x4*>(c[sn] + kk * 8); }, acc);
            } else {
                // 1 x 1 (one tap, no shift), [k][pixel] image: four 4-byte reads at stride Lr; half-wave h takes k = 8 kk + e + 4 h
                const float* bb = Bs + bbuf * kBK * Lr + 4 * (lane >> 5) * Lr;
                const float* c[2] = {bb + (ok0 ? jb[0] : jz), bb + (ok1 ? jb[1] : jz)};
                nt_mma_fp32_from<TM, fTN>(a, [&](int sn, int kk) {
                    return f32x4{c[sn][(kk * 8 + 0) * Lr], c[sn][(kk * 8 + 1) * Lr], c[sn][(kk * 8 + 2) * Lr], c[sn][(kk * 8 + 3) * Lr]};
                }, acc);
            }
        }
    };

    // zero column of every row of every image (never overwritten: data columns end at span - 1 < jz); k x k: the zero row
    if constexpr (SPLIT) {
        if constexpr (KIND == 2) {       // the zero row of the split image: 3 planes x 32 k
            if (tid < 12) *reinterpret_cast<u32x4_t*>(Bs16 + jz * kSplitRow + 8 * tid) = u32x4_t{0u, 0u, 0u, 0u};
        }                                // 1 x 1: pixels past the tensor's end are stored as zeros (no zero column)
    } else if constexpr (KIND == 2) {
        if (tid < fFlatPix / 4) *reinterpret_cast<f32x4*>(Bs + jz * fFlatPix + 4 * tid) = f32x4{0.f, 0.f, 0.f, 0.f};
    } else if (tid < kBK * NBUF) Bs[tid * Lr + jz] = 0.f;
    load_a(0, 0, ra0);
    load_b(0, rb0);
    store_a(0, ra0);
    store_b(0, rb0);
    __syncthreads();
    FwdRowOps<TM, fwd_has_image(MODE)> ops;
    // Software pipeline, two chunks deep for the global loads: while chunk c computes, the operands of chunk c + 1 are in
    // flight or in registers (requested one iteration earlier) and those of chunk c + 2 are requested.  k x k forms load
    // the input image of the next channel block two taps before its first use.
    int bsel = 0;
    int r1 = R > 1 ? 1 : 0, cb1 = R > 1 ? 0 : 1;       // (channel block, tap) of chunk c + 1
    if (nchunks > 1) {
        load_a(cb1, r1, ra1);
        if constexpr (KIND != 2) load_b(cb1, rb1);
    }
    auto step = [&](int c, int r, f32x4 (&ra_next)[PASS], f32x4 (&ra_far)[PASS], auto& rb_next, auto& rb_far) {
        // chunk c computes; chunk c + 1 (operands in *_next) is stored afterwards; chunk c + 2 is requested into *_far
        int r2 = r1 + 1, cb2 = cb1;
        if (r2 == R) { r2 = 0; ++cb2; }
        const bool far = c + 2 < nchunks;
        const bool newb = r1 == 0;                   // chunk c + 1 starts a new channel block
        if (far) load_a(cb2, r2, ra_far);
        if constexpr (KIND != 2) {
            if (far) load_b(cb2, rb_far);
        } else {
            // the image of block cb1 + 1 (first used by chunk c + 1 + (R - r1)) is requested when chunk c + 1 is its
            // block's second-to-last tap, i.e. two chunks before the store below needs it
            if (r1 == R - 2 && cb1 + 1 < CB) load_b(cb1 + 1, rb0);     // ONE register set: an image per R chunks
        }
        compute(c & 1, bsel, r);
        if constexpr (SPLIT) {
            __syncthreads();                         // every wave is done reading the (single) images
            store_a(0, ra_next);
            if (newb) {
                if constexpr (KIND == 2) store_b(0, rb0);
                else store_b(0, rb_next);
            }
            __syncthreads();
            r1 = r2;
            cb1 = cb2;
            return;
        }
        store_a((c + 1) & 1, ra_next);
        if (newb) {
            if constexpr (NBUF == 2) {
                bsel ^= 1;
                store_b(bsel, rb_next);
            } else {
                __syncthreads();                     // every wave is done reading the single image
                store_b(0, rb0);
            }
        }
        __syncthreads();
        r1 = r2;
        cb1 = cb2;
    };
    int r = 0;
    int c = 0;
    for (; c + 2 < nchunks; c += 2) {
        const int ra_ = r1;                          // tap of chunk c + 1, read before step() advances it
        step(c, r, ra1, ra0, rb1, rb0);
        const int rb_ = r1;
        step(c + 1, ra_, ra0, ra1, rb0, rb1);
        r = rb_;
    }
    if (c + 1 < nchunks) {
        const int ra_ = r1;
        step(c, r, ra1, ra0, rb1, rb0);
        r = ra_;
    }
    fwd_load_maps<TM, MODE>(L, i0, ops);                    // epilogue operands, requested under the last chunk's MFMAs
    compute((nchunks - 1) & 1, bsel, r);
    __syncthreads();
    fwd_epilogue<TM, MODE>(L, it, acc, ops, smem, partials);
}

// One kernel per tile form (register allocation and LDS are then per form, not the maximum over all of them); the host
// launches each form's slice of the item list.  The form ids are ABI (pleas_fwd_plan_units, pleas_fwd_plan_lanes); what a
// form IS stands in this table and nowhere else.
struct FwdForm {
    bool flat;        // fwd_flat_tile, else the general fwd_tile
    int tm;           // output channels of a tile
    int sub;          // general: floats per weight load (VECA); flat: KIND
    bool split;       // split-bf16 kernels exist (launched under pleas_arith(PLEAS_ARITH_SPLIT_BF16 / _EXACT); the other forms
                      // run their exact kernel in the same launch group)
    int occupancy[3]; // workgroups per CU the exact / the six-product / the nine-product kernel is compiled for
    double weight;    // expected duration per unit of MFMA work (measured on the ResNet-101 list, each form alone): the general
                      // tile (stride-2 layers: few, long items; stem: scalar weight loads) runs at ~0.4x the flat forms' rate,
                      // the scalar-pixel 1 x 1 form (7 x 7 images) at ~0.5x
};
constexpr int fForms = 10;
constexpr FwdForm kFwdForms[fForms] = {
    {false, 128, 4, false, {2, 2, 2}, 2.5}, {false, 64, 4, false, {2, 2, 2}, 2.5},
    {false, 128, 1, false, {2, 2, 2}, 2.5}, {false, 64, 1, false, {2, 2, 2}, 2.5},
    {true, 128, 0, true, {2, 2, 2}, 1.0},   {true, 128, 1, false, {2, 2, 2}, 2.0}, {true, 128, 2, true, {2, 2, 2}, 1.0},
    {true, 64, 0, true, {2, 3, 3}, 1.0},    {true, 64, 1, false, {2, 2, 2}, 2.0},  {true, 64, 2, true, {2, 3, 3}, 1.0},
};
// the id of FwdLayerDev::variant's form
constexpr int fwd_form_of(int variant) {
    if (variant & 8) return ((variant & 1) ? 7 : 4) + ((variant >> 4) & 3);
    return variant & 3;
}
// row f of the table describes what fwd_describe's variant bits call form f
constexpr bool fwd_forms_match_variants() {
    for (int f = 0; f < fForms; ++f) {
        const FwdForm& F = kFwdForms[f];
        const int variant = (F.tm == 64 ? 1 : 0) | (F.flat ? 8 | (F.sub << 4) : (F.sub == 1 ? 2 : 0));
        if (fwd_form_of(variant) != f || (F.split && !(F.flat && F.sub != 1))) return false;
    }
    return true;
}
static_assert(fwd_forms_match_variants(), "kFwdForms is indexed by the form id");
template <int FORM, int SPLIT = 0>
__global__ __launch_bounds__(kThreads, kFwdForms[FORM].occupancy[SPLIT]) void fwd_batch_kernel(const FwdLayerDev* __restrict__ layers,
                                                             const FwdItemDev* __restrict__ items,
                                                             float* __restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const FwdItemDev it = items[blockIdx.x];
    if (it.layer < 0) return;   // padding of the XCD-aware item order
    const FwdLayerDev L = layers[it.layer];
    constexpr FwdForm F = kFwdForms[FORM];
    if constexpr (F.flat) fwd_flat_tile<F.tm, F.sub, SPLIT>(L, it, smem, partials);
    else fwd_tile<F.tm, F.sub>(L, it, smem, partials);
}
// A plain convolution (pleas_conv2d_fwd): ONE layer, described in the kernel arguments; the work item is the block index
// (output-channel tile fastest, as in the grouped plan), no tables, no target, no loss.
template <int FORM, int SPLIT, FwdMode MODE>
__global__ __launch_bounds__(kThreads, kFwdForms[FORM].occupancy[SPLIT]) void conv2d_fwd_kernel(const FwdLayerDev L, const int tms) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const FwdItemDev it{0, (int)(blockIdx.x % (unsigned)tms), (int)(blockIdx.x / (unsigned)tms), 0};
    constexpr FwdForm F = kFwdForms[FORM];
    static_assert(!fwd_has_target(MODE), "the fit has its own kernel: tables of layers and items, loss partials");
    if constexpr (F.flat) fwd_flat_tile<F.tm, F.sub, SPLIT, MODE>(L, it, smem, nullptr);
    else fwd_tile<F.tm, F.sub, MODE>(L, it, smem, nullptr);
}
// The kernels of a form, [arithmetic = pleas_arith's mode]: a form without split kernels keeps its exact one there.
struct FwdFormKernels {
    void (*batch[3])(const FwdLayerDev*, const FwdItemDev*, float*);
    void (*conv2d[fModes][3])(const FwdLayerDev, const int);      // [FwdMode][arithmetic]; none for Fit (`batch`)
};
template <int FORM>
static constexpr FwdFormKernels fwd_form_kernels() {
    constexpr int S = kFwdForms[FORM].split ? 1 : 0, S9 = kFwdForms[FORM].split ? 2 : 0;
    using M = FwdMode;
    return {{fwd_batch_kernel<FORM, 0>, fwd_batch_kernel<FORM, S>, fwd_batch_kernel<FORM, S9>},
            {{nullptr, nullptr, nullptr},
             {conv2d_fwd_kernel<FORM, 0, M::Conv>, conv2d_fwd_kernel<FORM, S, M::Conv>, conv2d_fwd_kernel<FORM, S9, M::Conv>},
             {conv2d_fwd_kernel<FORM, 0, M::ConvImage>, conv2d_fwd_kernel<FORM, S, M::ConvImage>, conv2d_fwd_kernel<FORM, S9, M::ConvImage>},
             {conv2d_fwd_kernel<FORM, 0, M::Image>, conv2d_fwd_kernel<FORM, S, M::Image>, conv2d_fwd_kernel<FORM, S9, M::Image>},
             {conv2d_fwd_kernel<FORM, 0, M::ConvStats>, conv2d_fwd_kernel<FORM, S, M::ConvStats>, conv2d_fwd_kernel<FORM, S9, M::ConvStats>}}};
}
static const FwdFormKernels kFwdKernels[fForms] = {fwd_form_kernels<0>(), fwd_form_kernels<1>(), fwd_form_kernels<2>(), fwd_form_kernels<3>(),
                                                   fwd_form_kernels<4>(), fwd_form_kernels<5>(), fwd_form_kernels<6>(), fwd_form_kernels<7>(),
                                                   fwd_form_kernels<8>(), fwd_form_kernels<9>()};
// side streams of the library for the concurrent forms (+ the caller's stream = four hardware queues)
constexpr int fLanes = 3;
static SideStreams<fLanes> g_fwd_side;

// loss[l] = scale[l] * sum of this layer's partials (fixed order, fp64 combine)
struct FwdLossDev {
    int begin, count;
    float scale;
    int pad;
};
__global__ __launch_bounds__(64) void fwd_loss_kernel(const float* __restrict__ partials, const FwdLossDev* __restrict__ ld,
                                                      float* __restrict__ loss) {
    const FwdLossDev d = ld[blockIdx.x];
    double s = 0.0;
    for (int i = threadIdx.x; i < d.count; i += 64) s += (double)partials[d.begin + i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if (threadIdx.x == 0) loss[blockIdx.x] = (float)(s * (double)d.scale);
}

constexpr int fPtrBatch = 56;
struct FwdPtrBatch {
    int base, count;
    const float* ip[fPtrBatch];
    const float* w[fPtrBatch];
    const float* bias[fPtrBatch];
    const float* o1[fPtrBatch];
    const float* o2[fPtrBatch];
    const int32_t* row1[fPtrBatch];
    const int32_t* row2[fPtrBatch];
    float* resid[fPtrBatch];
};
__global__ void fwd_set_ptrs_kernel(FwdLayerDev* __restrict__ layers, const FwdPtrBatch b) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < b.count) {
        FwdLayerDev& L = layers[b.base + t];
        L.ip = b.ip[t];
        L.w = b.w[t];
        L.bias = b.bias[t];
        L.o1 = b.o1[t];
        L.o2 = b.o2[t];
        L.row1 = b.row1[t];
        L.row2 = b.row2[t];
        L.resid = b.resid[t];
    }
}

struct FwdPlan {
    std::vector<int64_t> key;
    std::vector<FwdLayerDev> layers;
    std::vector<FwdItemDev> items;
    std::vector<FwdLossDev> loss;
    size_t off_layers = 0, off_items = 0, off_loss = 0, off_parts = 0, total = 0;
    int form_begin[fForms] = {0}, form_count[fForms] = {0};
    size_t form_lds[fForms] = {0};
    std::vector<float> item_work;      // per item (aligned with `items`): relative duration, 0 for padding
    std::vector<FwdUnit> units;        // in launch order (fwd_schedule.hpp)
    double flops = 0, bytes = 0;
    int n_parts = 0;
    bool uploaded = false;
    int split = 0;                     // pleas_arith's mode the plan was built under: 1 / 2, the flat forms launch those split kernels
    // lanes from MEASURED durations: launch kFwdCalibAt of a plan brackets every unit's kernel with events on its lane; a
    // later launch that finds them complete deals the forms again, longest measured duration first
    int launches = 0, calib = 0;       // calib: 0 not measured yet, 1 events recorded, 2 lanes dealt from measurements
    // the calibration launch's events, around every unit's kernel on its lane.  They belong to the PLAN (a slot of the plan
    // cache, alive for the process): two plans that calibrate at the same time must not read each other's timings.
    hipEvent_t t0[kFwdMaxUnits], t1[kFwdMaxUnits];
    int timed = 0;                     // 0 events not created yet, 1 created, -1 creation failed (no calibration)
    bool timing_events() {
        if (timed == 0) {
            timed = 1;
            for (int u = 0; u < kFwdMaxUnits && timed == 1; ++u)
                if (hipEventCreate(&t0[u]) != hipSuccess || hipEventCreate(&t1[u]) != hipSuccess) timed = -1;
        }
        return timed == 1;
    }
    FwdFormItems form_items() const { return FwdFormItems{fForms, form_begin, form_count, item_work.data()}; }
};
static PlanCache<FwdPlan, 1> g_fplans;
static FwdCalibStore g_fcalib;

// Geometry checks, tile height, tile form and LDS bytes of ONE layer (shared by the grouped plan and the plain convolution).
static int fwd_describe(const pleas_fwd_layer& l, FwdLayerDev& d, size_t& lds_bytes, int& TM_out) {
    if (l.N <= 0 || l.Cout <= 0 || l.Cin <= 0 || l.Hin <= 0 || l.Win <= 0 || l.KH <= 0 || l.KW <= 0 || l.stride <= 0 ||
        l.pad < 0 || l.Csrc <= 0 || l.n_merged < 0)
        return bad_arg("conv_fwd: layer geometry");
    const int Hout = (l.Hin + 2 * l.pad - l.KH) / l.stride + 1, Wout = (l.Win + 2 * l.pad - l.KW) / l.stride + 1;
    if (Hout <= 0 || Wout <= 0) return bad_arg("conv_fwd: empty output");
    if (l.KH * l.KW > 64) return bad_arg("conv_fwd: kernels larger than 64 taps are not supported");
    const int64_t HWo = (int64_t)Hout * Wout, Ptot = (int64_t)l.N * HWo, Kd = (int64_t)l.Cin * l.KH * l.KW;
    if (Ptot >= (1ll << 31) || (int64_t)l.Cout * Kd >= (1ll << 32)) return bad_arg("conv_fwd: tensor too large");
    if (Ptot * std::max(l.Cout, l.Csrc) >= (1ll << 30)) return bad_arg("conv_fwd: outputs of 4 GB and more per call are not supported");
    d.Cout = l.Cout; d.Cin = l.Cin; d.Hin = l.Hin; d.Win = l.Win; d.Hout = Hout; d.Wout = Wout;
    d.KH = l.KH; d.KW = l.KW; d.stride = l.stride; d.pad = l.pad; d.Csrc = l.Csrc; d.n_merged = l.n_merged;
    d.HWo = (uint32_t)HWo; d.Ptot = (uint32_t)Ptot; d.Kd = (uint32_t)Kd;
    d.dscale = l.dscale;
    // short-K layers (1x1 with few input channels) are bound by their epilogue's memory traffic, not by the MFMAs:
    // 64-row tiles (52 KB of LDS, <= 132 registers) let THREE workgroups share a CU and overlap more of it
    // (round 5: 128-row tiles for them too are 1.6 % faster per launch group in both arithmetics -- half the tiles re-read and, under
    // the split arithmetic, re-convert each input chunk: 2.570 -> 2.529 ms exact, 1.884 -> 1.837 ms split,
    // profiles/r05_exp_source_conv.txt -- so 64-row tiles remain for Cout <= 64 only)
    const int TM = l.Cout > 64 ? 128 : 64;
    d.variant = (TM == 64 ? 1 : 0) | (Kd % 4 == 0 ? 0 : 2);
    if (l.flags & PLEAS_FWD_KPOS_MAJOR) {
        if (l.Cin % kBK != 0) return bad_arg("conv_fwd: kernel-position-major weights need Cin % 32 == 0");
        d.variant |= 4;
    }
    lds_bytes = (size_t)(2 * TM * kLds + 2 * fTN * kLds) * sizeof(float);  // >= TM*132 floats (epilogue)
    {
        // flat-shift form: stride 1, square odd kernel with "same" padding, whole 32-channel blocks, and (for k > 1)
        // kernel-position-major weights; its LDS must not exceed the general form's (two workgroups per CU)
        const int R = l.KH * l.KW;
        const bool same = l.stride == 1 && l.KH == l.KW && (l.KH & 1) && l.pad == (l.KH - 1) / 2;
        const int halo = l.pad * (l.Win + 1);
        const int kind = R > 1 ? 2 : (HWo % 4 == 0 ? 0 : 1);
        const int Lr = kind == 2 ? fFlatColsK : fFlatRow1;      // k x k: columns of the [column][36] image, zero row included
        const size_t flat_lds = std::max((size_t)(2 * TM * kLds + (kind == 2 ? fFlatColsK * fFlatPix : 2 * kBK * Lr)) * sizeof(float),
                                         (size_t)TM * 132 * sizeof(float));
        if (same && l.Cin % kBK == 0 && R <= 32 && (R == 1 || (l.flags & PLEAS_FWD_KPOS_MAJOR)) &&
            fTN + 2 * halo < Lr && flat_lds <= lds_bytes && (int64_t)l.N * l.Cin * HWo < (1ll << 32)) {
            d.variant |= 8 | (kind << 4);
            lds_bytes = flat_lds;
            if (arith_mode() != 0 && kind != 1) {
                // split-bf16 images (fwd_flat_tile<.., SPLIT = 1 / 2>): weights [TM][kSplitRow] + input k x k [columns][kSplitRow] /
                // 1 x 1 [3][32][fSplitPixRow] bf16, ONE image each; the epilogue stages [TM][132] floats in the same memory
                const size_t img = (size_t)(TM * kSplitRow + (kind == 2 ? fFlatColsK * kSplitRow : 3 * kBK * fSplitPixRow)) * sizeof(__bf16);
                lds_bytes = std::max(img, (size_t)TM * 132 * sizeof(float));
            }
        }
    }
    TM_out = TM;
    return PLEAS_OK;
}

static std::mutex g_fplan_mu;

static int build_fwd_plan(FwdPlan& P, const pleas_fwd_layer* ly, int n) {
    P.split = arith_mode();
    P.layers.assign(n, FwdLayerDev());
    P.items.clear();
    for (int f = 0; f < fForms; ++f) P.form_begin[f] = P.form_count[f] = 0;
    P.loss.assign(n, FwdLossDev());
    P.flops = P.bytes = 0;
    std::vector<XcdWork<FwdItemDev>> work[fForms];
    double form_work[fForms] = {0};
    for (int f = 0; f < fForms; ++f) P.form_lds[f] = 0;
    int parts = 0;
    for (int i = 0; i < n; ++i) {
        const pleas_fwd_layer& l = ly[i];
        FwdLayerDev& d = P.layers[i];
        size_t lds_bytes = 0;
        int TM = 128;
        if (const int rc = fwd_describe(l, d, lds_bytes, TM); rc != PLEAS_OK) return rc;
        const int64_t Ptot = d.Ptot, Kd = d.Kd;
        d.part_base = parts;
        const int tms = (int)ceil_div(l.Cout, TM), tps = (int)ceil_div(Ptot, fTN);
        int slot = 0;
        // Within a layer the output-channel tile runs fastest: with workgroup b on XCD b % 8, an XCD then keeps meeting the
        // same few weight tiles, which stay in its L2, while every input tile is streamed once per XCD that needs it.
        const int form = fwd_form_of(d.variant);
        for (int tp = 0; tp < tps; ++tp)
            for (int tm = 0; tm < tms; ++tm) {
                XcdWork<FwdItemDev> w;
                w.it = FwdItemDev{i, tm, tp, slot++};
                w.w = (double)ceil_div(Kd, kBK) * TM;
                // all items of a layer re-read its weights (and, across tm, its input): keep them on one XCD; layers
                // with many pixel tiles are cut into runs of 32 tiles so that the 8 queues still balance
                w.key = (int64_t)i * 65536 + tp / 32;
                work[form].push_back(w);
                form_work[form] += w.w;
            }
        P.loss[i] = FwdLossDev{parts, slot, l.loss_scale, 0};
        parts += slot;
        P.form_lds[form] = std::max(P.form_lds[form], lds_bytes);
        P.flops += 2.0 * l.Cout * (double)Kd * (double)Ptot;
        P.bytes += ((double)l.Cin * l.N * l.Hin * l.Win + 3.0 * l.Cout * (double)Ptot) * sizeof(float);
    }
    // Off by default for this kernel (PLEAS_XCD_ORDER=1 turns it on): it cuts FETCH_SIZE by 32 % (8.3 -> 6.1 GB per launch)
    // but costs 1-4 % of time -- co-resident workgroups of one layer reach their latency-bound epilogues together,
    // while the plain longest-first order mixes layers on a CU.
    for (int f = 0; f < fForms; ++f) {
        P.form_begin[f] = (int)P.items.size();
        std::vector<FwdItemDev> part = xcd_order_items(work[f], FwdItemDev{-1, 0, 0, 0}, /*by_default=*/false);
        P.items.insert(P.items.end(), part.begin(), part.end());
        P.form_count[f] = (int)part.size();
    }
    P.item_work.assign(P.items.size(), 0.f);
    for (size_t k = 0; k < P.items.size(); ++k)
        if (P.items[k].layer >= 0) {
            const FwdLayerDev& d = P.layers[P.items[k].layer];
            P.item_work[k] = (float)(ceil_div(d.Kd, kBK) * kFwdForms[fwd_form_of(d.variant)].tm);
        }
    // launch order: the form with the most work first (its tail is then covered by nothing, the small ones' tails are short).
    // The forms' static weights deal the FIRST launches of a plan only; launch kFwdCalibAt measures every form on its lane and
    // the lanes are dealt again from those durations (pleas_fwd_batch).
    P.units.clear();
    for (int f = 0; f < fForms; ++f)
        if (P.form_count[f] > 0)
            P.units.push_back(FwdUnit{f, P.form_begin[f], P.form_count[f], 0, form_work[f] * kFwdForms[f].weight});
    fwd_deal_lanes(P.units, fLanes + 1);
    P.launches = P.calib = 0;
    P.n_parts = parts;
    size_t off = 0;
    P.off_layers = off;
    off = align256(off + P.layers.size() * sizeof(FwdLayerDev));
    P.off_items = off;
    off = align256(off + P.items.size() * sizeof(FwdItemDev));
    P.off_loss = off;
    off = align256(off + P.loss.size() * sizeof(FwdLossDev));
    P.off_parts = off;
    P.total = off + (size_t)parts * sizeof(float);
    P.uploaded = false;
    return PLEAS_OK;
}

}  // namespace pleas

using namespace pleas;

extern "C" int pleas_fwd_plan_lanes(double* form_ms, int* form_lane, int* form_items) {
    if (!form_ms || !form_lane || !form_items) return bad_arg("fwd_plan_lanes: null pointer");
    std::lock_guard<std::mutex> lk(g_fplan_mu);
    if (!g_fplans.last) return bad_arg("fwd_plan_lanes: no grouped forward has run yet");
    const FwdPlan& P = *g_fplans.last;
    for (int f = 0; f < fForms; ++f) {
        form_ms[f] = 0;
        form_lane[f] = 0;
        form_items[f] = P.form_count[f];
    }
    for (const auto& u : P.units) {      // a form cut into slices: summed duration, lanes as decimal digits (lane + 1 each)
        form_ms[u.form] += u.ms;
        form_lane[u.form] = form_lane[u.form] * 10 + u.lane + 1;
    }
    return P.calib;
}

extern "C" int pleas_fwd_plan_units(const pleas_fwd_layer* layers, int n_layers, const double* form_ms, int* units, int max_units) {
    if (!layers || n_layers <= 0 || !units || max_units <= 0) return bad_arg("fwd_plan_units: empty layer list / null output");
    FwdPlan tmp;
    const int rc = build_fwd_plan(tmp, layers, n_layers);
    if (rc != PLEAS_OK) return rc;
    if (form_ms) {       // as if the calibration launch had measured these per-form durations
        for (auto& u : tmp.units) u.ms = form_ms[u.form];
        (void)fwd_schedule_measured(tmp.units, tmp.form_items(), fLanes + 1, kFwdMaxUnits);      // unusable measurements: the static units stay
    }
    const int n = (int)std::min<size_t>(tmp.units.size(), (size_t)max_units);
    for (int i = 0; i < n; ++i) {
        units[4 * i + 0] = tmp.units[i].form;
        units[4 * i + 1] = tmp.units[i].begin;
        units[4 * i + 2] = tmp.units[i].count;
        units[4 * i + 3] = tmp.units[i].lane;
    }
    return (int)tmp.units.size();
}

extern "C" size_t pleas_fwd_batch_ws_bytes(const pleas_fwd_layer* layers, int n_layers) {
    if (!layers || n_layers <= 0) return 0;
    FwdPlan tmp;
    if (build_fwd_plan(tmp, layers, n_layers) != PLEAS_OK) return 0;
    return tmp.total;
}

// One plain convolution call: the operands, the geometry, the mode and that mode's operands.
struct Conv2dCall {
    FwdMode mode;
    const float *x, *w, *bias;
    float* y;                                    // null under Image
    int N, Cin, Hin, Win, Cout, KH, KW, stride, pad, flags;
    void* stream;
    const float *scale = nullptr, *shift = nullptr, *res = nullptr;      // the image modes: res may be null
    float* z = nullptr;
    int relu = 0;                                // activation after the map: a PLEAS_ACT_* code (other values: ReLU)
};
// its description; ConvStats: the caller sets d.st_part / d.st_pb once its own refusals are past
struct Conv2dPlan { FwdLayerDev d; size_t lds = 0; int TM = 128; };

// Every refusal of a call, and its description; no HIP call.
static int conv2d_describe(const Conv2dCall& c, Conv2dPlan& p) {
    FwdLayerDev& d = p.d;
    if (!c.x || !c.w || (!c.y && fwd_stores_y(c.mode))) return bad_arg("conv2d_fwd: null pointer");
    if (((uintptr_t)c.w & 15) != 0 || ((uintptr_t)c.x & 15) != 0)
        return bad_arg(fwd_has_stats(c.mode) ? "conv2d_bn_stats_fwd: x and w must be 16-byte aligned" : "conv2d_fwd: x and w must be 16-byte aligned");
    if (fwd_has_image(c.mode) && ((((uintptr_t)c.y | (uintptr_t)c.z | (uintptr_t)c.res) & 15) != 0))
        return bad_arg("conv2d_bn_act_fwd: y, z and res must be 16-byte aligned");
    pleas_fwd_layer l{};      // the geometry alone is read
    l.N = c.N; l.Cout = c.Cout; l.Cin = c.Cin; l.Hin = c.Hin; l.Win = c.Win; l.KH = c.KH; l.KW = c.KW; l.stride = c.stride; l.pad = c.pad;
    l.Csrc = 1; l.dscale = 1.f; l.flags = c.flags;
    d = FwdLayerDev{};
    if (const int rc = fwd_describe(l, d, p.lds, p.TM); rc != PLEAS_OK) return rc;
    // no block maps: every source row is absent (fwd_load_maps), the masked gathers read the first floats of x
    d.ip = c.x; d.w = c.w; d.bias = c.bias; d.o1 = c.x; d.o2 = c.x; d.resid = c.y;
    d.bn_scale = c.scale; d.bn_shift = c.shift; d.bn_res = c.res; d.bn_z = c.z; d.bn_relu = c.relu == PLEAS_ACT_RELU6 ? PLEAS_ACT_RELU6 : (c.relu ? PLEAS_ACT_RELU : PLEAS_ACT_NONE);
    return PLEAS_OK;
}

static int conv2d_enqueue(const Conv2dCall& c, const Conv2dPlan& p) {
    const FwdLayerDev& d = p.d;
    const int tms = (int)ceil_div(c.Cout, p.TM), tps = (int)ceil_div((int64_t)d.Ptot, fTN);
    const dim3 grid((unsigned)((int64_t)tms * tps));
    hipStream_t st = (hipStream_t)c.stream;
    const double out_floats = (double)c.Cout * d.Ptot;
    ProfScope prof(kProfConv2d, 2.0 * c.Cout * (double)d.Kd * (double)d.Ptot,
                   ((double)c.Cin * c.N * c.Hin * c.Win + out_floats * ((c.mode == FwdMode::ConvImage ? 2.0 : 1.0) + (c.res ? 1.0 : 0.0))) * sizeof(float), st);
    hipLaunchKernelGGL(kFwdKernels[fwd_form_of(d.variant)].conv2d[(int)c.mode][arith_mode()], grid, dim3(kThreads), p.lds, st, d, tms);
    PLEAS_LAUNCH_CHECK("conv2d_fwd_kernel");
    return PLEAS_OK;
}

static int conv2d_launch(const Conv2dCall& c) {
    Conv2dPlan p;
    if (const int rc = conv2d_describe(c, p); rc != PLEAS_OK) return rc;
    return conv2d_enqueue(c, p);
}

extern "C" int pleas_conv2d_fwd(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int Hin, int Win,
                                int Cout, int KH, int KW, int stride, int pad, int flags, void* stream_) {
    return conv2d_launch(Conv2dCall{FwdMode::Conv, x, w, bias, y, N, Cin, Hin, Win, Cout, KH, KW, stride, pad, flags, stream_});
}

extern "C" int pleas_conv2d_bn_act_fwd(const float* x, const float* w, const float* bias, float* y, const float* scale,
                                       const float* shift, const float* res, float* z, int relu, int N, int Cin, int Hin,
                                       int Win, int Cout, int KH, int KW, int stride, int pad, int flags, void* stream_) {
    if (!scale || !shift || !z) return bad_arg("conv2d_bn_act_fwd: null pointer");
    return conv2d_launch(Conv2dCall{FwdMode::ConvImage, x, w, bias, y, N, Cin, Hin, Win, Cout, KH, KW, stride, pad, flags, stream_,
                                    scale, shift, res, z, relu});
}

extern "C" int pleas_conv2d_act_fwd(const float* x, const float* w, const float* bias, const float* scale, const float* shift,
                                    const float* res, float* z, int relu, int N, int Cin, int Hin, int Win, int Cout, int KH,
                                    int KW, int stride, int pad, int flags, void* stream_) {
    if (!scale || !shift || !z) return bad_arg("conv2d_act_fwd: null pointer");
    return conv2d_launch(Conv2dCall{FwdMode::Image, x, w, bias, nullptr, N, Cin, Hin, Win, Cout, KH, KW, stride, pad, flags, stream_,
                                    scale, shift, res, z, relu});
}

// Workspace of pleas_conv2d_bn_stats_fwd, in doubles: what bn_train_finalize_kernel takes with S = 1 -- the sums per (batch,
// channel) [batches][1][Cout][2] and its moments tail [batches][Cout][2] -- then the tiles' partial slab [pixel tiles][2][Cout][2].
static size_t conv_bn_stats_head(int Cout, int batches) { return (size_t)batches * Cout * 4; }

extern "C" size_t pleas_conv2d_bn_stats_ws_bytes(int N, int Cout, int Hout, int Wout, int batches) {
    if (N <= 0 || Cout <= 0 || Hout <= 0 || Wout <= 0 || batches <= 0) return 0;
    const int64_t tiles = ceil_div((int64_t)N * Hout * Wout, fTN);
    return (conv_bn_stats_head(Cout, batches) + (size_t)tiles * 2 * Cout * 2) * sizeof(double);
}

extern "C" int pleas_conv2d_bn_stats_fwd(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int Hin, int Win,
                                         int Cout, int KH, int KW, int stride, int pad, int flags, int batches, const float* gamma,
                                         const float* beta, double eps, double momentum, float* running_mean, float* running_var,
                                         int64_t* num_batches_tracked, float* scale, float* shift, void* ws, size_t ws_bytes,
                                         void* stream_) {
    // every refusal comes before the first HIP call: nothing is enqueued for a call that is turned down
    if (!x || !w || !y || !scale || !shift) return bad_arg("conv2d_bn_stats_fwd: null pointer");
    if (batches < 1 || batches > 65535) return bad_arg("conv2d_bn_stats_fwd: batches");
    if (N <= 0 || N % batches != 0) return bad_arg("conv2d_bn_stats_fwd: the samples do not split into the batches");
    if ((running_mean == nullptr) != (running_var == nullptr))
        return bad_arg("conv2d_bn_stats_fwd: running_mean / running_var: both or neither");
    Conv2dCall c{FwdMode::ConvStats, x, w, bias, y, N, Cin, Hin, Win, Cout, KH, KW, stride, pad, flags, stream_};
    Conv2dPlan p;
    if (const int rc = conv2d_describe(c, p); rc != PLEAS_OK) return rc;
    FwdLayerDev& d = p.d;
    const int64_t per_batch = (int64_t)(N / batches) * d.HWo;      // values per channel and batch
    if (per_batch <= 1) return bad_arg("conv2d_bn_stats_fwd: more than one value per channel is needed");
    // a tile has two segments: it may touch two batches, not three
    if (batches > 1 && per_batch < fTN)
        return bad_arg("conv2d_bn_stats_fwd: batches of fewer than 128 pixels cannot share a forward (fold them after pleas_conv2d_fwd)");
    const size_t need = pleas_conv2d_bn_stats_ws_bytes(N, Cout, d.Hout, d.Wout, batches);
    if (!ws || ws_bytes < need) return workspace_too_small("conv2d_bn_stats_fwd", need);
    if ((uintptr_t)ws & 7) return bad_arg("conv2d_bn_stats_fwd: workspace must be 8-byte aligned");
    double* sums = (double*)ws;
    d.st_part = sums + conv_bn_stats_head(Cout, batches);
    d.st_pb = (uint32_t)per_batch;
    if (const int rc = conv2d_enqueue(c, p); rc != PLEAS_OK) return rc;
    return bn_fold_tile_partials(d.st_part, fTN, d.Ptot, (uint32_t)per_batch, Cout, batches, sums, gamma, beta, eps, momentum,
                                 running_mean, running_var, num_batches_tracked, scale, shift, (hipStream_t)stream_);
}

// The calibration launch's events: all complete?  Then the plan's units take their measured durations, long ones are cut and
// the lanes dealt again, and the result is published for other fitters on the same geometry.
static void fwd_adopt_measurements(FwdPlan& P) {
    if (P.calib != 1) return;
    const int active = (int)P.units.size();
    bool ready = true;
    for (int u = 0; ready && u < active; ++u) ready = hipEventQuery(P.t1[u]) == hipSuccess;
    if (ready) {
        for (int u = 0; u < active; ++u) {
            float ms = 0.f;
            P.units[u].ms = hipEventElapsedTime(&ms, P.t0[u], P.t1[u]) == hipSuccess ? ms : 0.0;
        }
        P.calib = 2;
        if (fwd_schedule_measured(P.units, P.form_items(), fLanes + 1, kFwdMaxUnits))      // else: static lanes kept, nothing published
            g_fcalib.publish(P.key, P.units);
    }
    (void)hipGetLastError();   // hipEventQuery's "not ready" is not an error of this call
}

// The forms are independent grids.  Back to back on one stream each would wait for the previous one's LAST workgroup (a
// stride-2 3x3 layer has 28 items of 144 chunks: half a millisecond of tail on an empty chip), so every form but the largest
// goes to one of THREE side streams of the library (fork / join with events around the group; the runtime multiplexes a
// process's streams onto four hardware queues, so more lanes would only queue up behind each other): forms are dealt to the
// least-loaded lane, largest first, and the long items of the small forms run beside the large forms' thousands of short
// ones, as in one grid.  Launch kFwdCalibAt of a plan also brackets every unit with the plan's timing events.
static int fwd_launch_units(FwdPlan& P, const FwdLayerDev* dl, const FwdItemDev* items, float* parts, hipStream_t stream) {
    ProfScope prof(kProfConvFwd, P.flops, P.bytes, stream);
    SideStreams<fLanes>::Set& side = g_fwd_side.current();
    const int active = (int)P.units.size();
    const bool fork = active > 1 && side.ok;
    const bool measure = fork && P.calib == 0 && P.launches == kFwdCalibAt && active <= kFwdMaxUnits && P.timing_events();
    if (fork) PLEAS_HIP_CHECK(hipEventRecord(side.forked, stream));
    bool lane_used[fLanes + 1] = {false};
    for (int o = 0; o < active; ++o) {
        const FwdUnit& un = P.units[o];
        const int lane = fork ? un.lane : 0;          // lane 0 = the caller's stream
        hipStream_t st = lane == 0 ? stream : side.streams[lane - 1];
        if (lane > 0 && !lane_used[lane]) PLEAS_HIP_CHECK(hipStreamWaitEvent(st, side.forked, 0));
        lane_used[lane] = true;
        if (measure) PLEAS_HIP_CHECK(hipEventRecord(P.t0[o], st));
        hipLaunchKernelGGL(kFwdKernels[un.form].batch[P.split], dim3((unsigned)un.count), dim3(kThreads), P.form_lds[un.form], st,
                           dl, items + un.begin, parts);
        if (measure) PLEAS_HIP_CHECK(hipEventRecord(P.t1[o], st));
    }
    if (measure) P.calib = 1;
    for (int lane = 1; lane <= fLanes; ++lane)
        if (lane_used[lane]) {
            PLEAS_HIP_CHECK(hipEventRecord(side.joined[lane - 1], side.streams[lane - 1]));
            PLEAS_HIP_CHECK(hipStreamWaitEvent(stream, side.joined[lane - 1], 0));
        }
    return PLEAS_OK;
}

extern "C" int pleas_fwd_batch(const pleas_fwd_layer* layers, int n_layers, float* loss, void* ws, size_t ws_bytes,
                               int ws_fresh, void* stream_) {
    if (!layers || n_layers <= 0 || !loss) return bad_arg("conv_fwd: empty layer list");
    for (int i = 0; i < n_layers; ++i) {
        const pleas_fwd_layer& l = layers[i];
        if (!l.ip || !l.w || !l.o1 || !l.o2 || !l.row1 || !l.row2 || !l.resid) return bad_arg("conv_fwd: null pointer");
        if (((uintptr_t)l.w & 15) != 0) return bad_arg("conv_fwd: weights must be 16-byte aligned");
        if (((uintptr_t)l.ip & 15) != 0) return bad_arg("conv_fwd: the merged input must be 16-byte aligned");
    }
    hipStream_t stream = (hipStream_t)stream_;
    std::lock_guard<std::mutex> lk(g_fplan_mu);
    std::vector<int64_t> key;
    key.push_back(n_layers);
    key.push_back((int64_t)(uintptr_t)ws);
    key.push_back(arith_mode());      // plans (LDS sizes, kernels) differ between the arithmetics
    for (int i = 0; i < n_layers; ++i) {
        const pleas_fwd_layer& l = layers[i];
        for (int v : {l.N, l.Cout, l.Cin, l.Hin, l.Win, l.KH, l.KW, l.stride, l.pad, l.Csrc, l.n_merged, l.flags})
            key.push_back(v);
        int32_t bits[2];
        std::memcpy(&bits[0], &l.dscale, 4);
        std::memcpy(&bits[1], &l.loss_scale, 4);
        key.push_back(bits[0]);
        key.push_back(bits[1]);
    }
    FwdPlan* hit = nullptr;
    if (const int rc = g_fplans.get(key, hit, [&](FwdPlan& p) { return build_fwd_plan(p, layers, n_layers); }); rc != PLEAS_OK)
        return rc;
    FwdPlan& P = *hit;
    if (P.calib == 0 && P.launches == 0)        // a new plan: start from what another fitter measured on this geometry
        if (const std::vector<FwdUnit>* measured = g_fcalib.find(P.key)) {
            P.units = *measured;
            P.calib = 2;
        }
    if (const int rc = g_fplans.prepare(P, "conv_fwd", ws, ws_bytes, ws_fresh, stream, [&] {
            return std::vector<PlanTable>{plan_table(P.off_layers, P.layers), plan_table(P.off_items, P.items),
                                          plan_table(P.off_loss, P.loss)};
        });
        rc != PLEAS_OK)
        return rc;
    char* base = (char*)ws;
    FwdLayerDev* dl = reinterpret_cast<FwdLayerDev*>(base + P.off_layers);
    for (int b0 = 0; b0 < n_layers; b0 += fPtrBatch) {
        FwdPtrBatch pb;
        pb.base = b0;
        pb.count = std::min(fPtrBatch, n_layers - b0);
        for (int t = 0; t < pb.count; ++t) {
            const pleas_fwd_layer& l = layers[b0 + t];
            pb.ip[t] = l.ip; pb.w[t] = l.w; pb.bias[t] = l.bias; pb.o1[t] = l.o1; pb.o2[t] = l.o2;
            pb.row1[t] = l.row1; pb.row2[t] = l.row2; pb.resid[t] = l.resid;
        }
        hipLaunchKernelGGL(fwd_set_ptrs_kernel, dim3(1), dim3(64), 0, stream, dl, pb);
        PLEAS_LAUNCH_CHECK("fwd_set_ptrs_kernel");
    }
    float* parts = reinterpret_cast<float*>(base + P.off_parts);
    ++P.launches;
    fwd_adopt_measurements(P);
    if (const int rc = fwd_launch_units(P, dl, reinterpret_cast<const FwdItemDev*>(base + P.off_items), parts, stream); rc != PLEAS_OK)
        return rc;
    PLEAS_LAUNCH_CHECK("fwd_batch_kernel");
    hipLaunchKernelGGL(fwd_loss_kernel, dim3(n_layers), dim3(64), 0, stream, parts,
                       reinterpret_cast<const FwdLossDev*>(base + P.off_loss), loss);
    PLEAS_LAUNCH_CHECK("fwd_loss_kernel");
    return PLEAS_OK;
}
