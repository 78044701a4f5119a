// The NT contraction tile of gram_tile, wgrad_tile, neq_tile, neq_lag_tile, lin_tile and the forward convolution's fwd_tile / fwd_flat_tile
// (DESIGN.md 3.1), device side: C[i][j] += sum_k A[i][k] * B[j][k] on a TM x TN tile.  256 threads = 2 x 2 waves, each wave
// (wm, wn) owns a TM/2 x TN/2 quarter as 32 x 32 MFMA tiles.  A K chunk of 32 goes global -> registers -> LDS; the kernels'
// loaders (what differs between them) stay with them.
//   exact fp32:  LDS [2][rows][kLds] floats per operand (double-buffered, one barrier per chunk), v_mfma_f32_32x32x2_f32
//   split bf16:  LDS [rows][kSplitRow] bf16 per operand (common.hpp; ONE image, two barriers per chunk: the next chunk
//                waits in registers), six or nine v_mfma_f32_32x32x16_bf16 per 16-deep k step (NPROD)
// The A operand always lies in LDS as above.  Where the exact step's B fragments come from is a B SOURCE, a callable of the
// tile: (sn, kk) -> f32x4 gives the four k of this lane's half-wave for 32-pixel fragment sn and k group kk.  nt_mma_fp32 is the
// instance that reads [row][kLds] rows; the flat forward tiles read shifted image rows and pixel-major images.  The split step
// has no source: the flat forward tile's split step reads its fragments in an order of its own and stays written out there.
#pragma once
#include "common.hpp"

namespace pleas {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef f32x16_t f32x16;
typedef f32x4 f32x4u __attribute__((aligned(4)));   // 16 bytes at a 4-byte-aligned address: still ONE global_load_dwordx4

constexpr int kBK = 32;      // K chunk (floats) staged per step
constexpr int kLds = 36;     // padded LDS row stride: 16-B aligned rows, conflict-free ds_read_b128
constexpr int kThreads = 256;

template <int MTM, int MTN>
__device__ __forceinline__ void nt_zero(f32x16 (&acc)[MTM][MTN]) {
#pragma unroll
    for (int a = 0; a < MTM; ++a)
#pragma unroll
        for (int b = 0; b < MTN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
}

// One chunk of buffer `buf`, exact arithmetic.  Lanes 0-31 feed k = 8kk+e, lanes 32-63 feed k = 8kk+4+e: any pairing of k is
// valid as long as A and B agree, and it lets one 16-B LDS read serve four MFMA steps.
// The part every tile shares: `a` is this lane's first A fragment in [row][kLds] rows; bsrc(sn, kk) is its B fragment.
template <int TM, int TN, class BSrc>
__device__ __forceinline__ void nt_mma_fp32_from(const float* a, BSrc&& bsrc, f32x16 (&acc)[TM / 64][TN / 64]) {
    constexpr int MTM = TM / 64, MTN = TN / 64;
#pragma unroll
    for (int kk = 0; kk < kBK / 8; ++kk) {
        f32x4 fa[MTM], fb[MTN];
#pragma unroll
        for (int s = 0; s < MTM; ++s) fa[s] = *reinterpret_cast<const f32x4*>(a + s * 32 * kLds + kk * 8);
#pragma unroll
        for (int s = 0; s < MTN; ++s) fb[s] = bsrc(s, kk);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int sm = 0; sm < MTM; ++sm)
#pragma unroll
                for (int sn = 0; sn < MTN; ++sn)
                    acc[sm][sn] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[sm][e], fb[sn][e], acc[sm][sn], 0, 0, 0);
    }
}
template <int TM, int TN>
__device__ __forceinline__ void nt_mma_fp32(const float* As, const float* Bs, int buf, f32x16 (&acc)[TM / 64][TN / 64]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;
    const float* a = As + buf * TM * kLds + (wm * (TM / 2) + (lane & 31)) * kLds + 4 * (lane >> 5);
    const float* b = Bs + buf * TN * kLds + (wn * (TN / 2) + (lane & 31)) * kLds + 4 * (lane >> 5);
    nt_mma_fp32_from<TM, TN>(a, [b](int sn, int kk) { return *reinterpret_cast<const f32x4*>(b + sn * 32 * kLds + kk * 8); }, acc);
}

// One chunk of the split images.  Lane (r, h) of k group g reads k = 16 g + 8 h .. + 7 of its row from each plane: the
// operand map of the MFMA.
template <int TM, int TN, int NPROD = 6>
__device__ __forceinline__ void nt_mma_split(const __bf16* As16, const __bf16* Bs16, f32x16 (&acc)[TM / 64][TN / 64]) {
    constexpr int MTM = TM / 64, MTN = TN / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;
    const __bf16* a16 = As16 + (wm * (TM / 2) + (lane & 31)) * kSplitRow + 8 * (lane >> 5);
    const __bf16* b16 = Bs16 + (wn * (TN / 2) + (lane & 31)) * kSplitRow + 8 * (lane >> 5);
#pragma unroll
    for (int g16 = 0; g16 < kBK / 16; ++g16) {
        bf16x8_t sa[MTM][3], sb[MTN][3];
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int s = 0; s < MTM; ++s) sa[s][p] = *reinterpret_cast<const bf16x8_t*>(a16 + s * 32 * kSplitRow + p * kBK + g16 * 16);
#pragma unroll
            for (int s = 0; s < MTN; ++s) sb[s][p] = *reinterpret_cast<const bf16x8_t*>(b16 + s * 32 * kSplitRow + p * kBK + g16 * 16);
        }
#pragma unroll
        for (int sm = 0; sm < MTM; ++sm)
#pragma unroll
            for (int sn = 0; sn < MTN; ++sn) acc[sm][sn] = split3_mfma<NPROD>(sa[sm], sb[sn], acc[sm][sn]);
    }
}

// K chunks [c_begin, c_end): load(c) brings chunk c into registers, store(buf) masks it into LDS, compute(buf) multiplies.
// The loads of chunk c + 1 stay in flight behind the MFMAs of chunk c.  SPLIT (1 or 2): one LDS image, so a second barrier (every
// wave is done reading it) comes before the store.
template <int SPLIT, class Load, class Store, class Compute>
__device__ __forceinline__ void nt_pipeline(int c_begin, int c_end, Load&& load, Store&& store, Compute&& compute) {
    if (c_begin < c_end) {
        load(c_begin);
        store(0);
    }
    __syncthreads();
    for (int c = c_begin; c < c_end; ++c) {
        const int buf = SPLIT ? 0 : (c - c_begin) & 1;
        const bool more = c + 1 < c_end;
        if (more) load(c + 1);
        compute(buf);
        if constexpr (SPLIT) __syncthreads();
        if (more) store(SPLIT ? 0 : buf ^ 1);
        __syncthreads();
    }
}

}  // namespace pleas
