// uint8 image batches to normalised fp32 NCHW on gfx950 (MI355X): table lookup, crop and horizontal flip in one pass.
//
//   dst[n][c][y][x] = lut[c][ src[n][y0 + y][x0 + xs][c] ],   xs = Wo-1-x for a flipped sample, else x      pleas_image_batch
//
// Replaces: `x.cuda()` of batches that CPU workers have run through ToTensor / Normalize / RandomCrop / RandomHorizontalFlip
// (pleas/methods/activation_matching.py:121, pleas/methods/pleas_merging.py:266 and the drivers' dataset transforms): the host
// ships uint8 (3 bytes per pixel instead of 12) and does no per-image arithmetic.
//
// HBM-bound: reads the window's bytes once, writes four times as many.  The only arithmetic is the lookup, so the result
// carries the table's bits whatever the compiler does; no atomics, no sums, every element written once.
//
// Work: the 256 threads of a workgroup form `by` teams of `bx` lanes, bx = the power of two at or above ceil(Wo / 16), at most
// 256; a team takes one row of the output at a time (one n, one y: Wo pixels of C planes).  Lane j takes pixels j, j + bx, ...
// byte by byte, four pixels (all their channels) loaded before the first is looked up, so the team's lanes read side by side
// and write 4-byte runs side by side into each plane.  One path for every C, layout, alignment, crop and flip.  Rows are dealt
// to teams along blockIdx.x, samples along blockIdx.y, both with grid strides: no division anywhere, 64-bit offsets throughout.
//
// Measured and dropped (profiles/image_batch_fast_vs_byte.json): a second path for interleaved 3-channel rows on a 16-byte
// boundary -- 48 bytes per lane step as three 16-byte loads, de-interleaved in registers, four 16-byte stores per plane -- ran
// at 0.97 to 1.01 of the byte path's time on 16 and 128 images of 224 x 224 x 3 (29 us at 128 images, the byte path then one
// pixel at a time; with four pixels of loads in flight it takes 20 us: profiles/image_batch_bench.json).
#include "common.hpp"

namespace pleas {

constexpr int kImgThreads = 256;
constexpr int kImgStep = 16;              // pixels of a row per lane of its team (bx = the power of two at or above Wo / 16)
constexpr int kImgAhead = 4;              // pixels a lane loads before it looks the first one up
constexpr int kImgMaxBlocks = 2048;       // about eight workgroups per CU; larger batches stride over the grid

typedef __attribute__((address_space(1))) const uint8_t gcu8;

template <int C>
__global__ __launch_bounds__(kImgThreads) void image_batch_kernel(const uint8_t* __restrict__ src_, float* __restrict__ dst_,
                                                                  const float* __restrict__ lut, const int32_t* __restrict__ origin,
                                                                  const uint8_t* __restrict__ flip, int64_t N, int H, int W, int Ho,
                                                                  int Wo, int log_bx, int planar) {
    __shared__ float table[C * 256];
    for (int i = threadIdx.x; i < C * 256; i += kImgThreads) table[i] = lut[i];
    __syncthreads();

    gcu8* src = (gcu8*)src_;
    gfloat* dst = PLEAS_GLOBAL_W(dst_);
    const int bx = 1 << log_bx, by = kImgThreads >> log_bx;
    const int tx = threadIdx.x & (bx - 1), ty = threadIdx.x >> log_bx;
    const uint64_t plane = (uint64_t)Ho * (uint64_t)Wo;      // elements of one dst plane
    // element (c, xs) of a row's window lies at src[base + c * cs + xs * ps]
    const int64_t cs = planar ? (int64_t)H * W : 1, ps = planar ? 1 : C;
    for (int64_t n = blockIdx.y; n < N; n += gridDim.y) {
        int64_t y0 = 0, x0 = 0;
        if (origin) {
            y0 = origin[2 * n];
            x0 = origin[2 * n + 1];
        }
        const bool fl = flip && flip[n];
        for (int64_t y = (int64_t)blockIdx.x * by + ty; y < Ho; y += (int64_t)gridDim.x * by) {
            gfloat* d = dst + (((uint64_t)n * C) * (uint64_t)Ho + (uint64_t)y) * (uint64_t)Wo;      // plane 0 of the row; plane c at + c * plane
            const int64_t base = planar ? ((n * C) * H + (y0 + y)) * W + x0 : ((n * H + (y0 + y)) * W + x0) * C;
            for (int x = tx; x < Wo; x += kImgAhead * bx) {
                uint32_t b[kImgAhead][C];
#pragma unroll
                for (int u = 0; u < kImgAhead; ++u) {
                    // clamped: the loads stay unconditional and inside the window, a pixel past Wo is not stored
                    const int xc = min(x + u * bx, Wo - 1);
                    const int64_t at = base + (int64_t)(fl ? Wo - 1 - xc : xc) * ps;
#pragma unroll
                    for (int c = 0; c < C; ++c) b[u][c] = src[at + c * cs];
                }
#pragma unroll
                for (int u = 0; u < kImgAhead; ++u) {
                    const int xu = x + u * bx;
                    if (xu < Wo) {
#pragma unroll
                        for (int c = 0; c < C; ++c) d[(uint64_t)c * plane + xu] = table[c * 256 + b[u][c]];
                    }
                }
            }
        }
    }
}

}  // namespace pleas

using namespace pleas;

extern "C" int pleas_image_batch(const uint8_t* src, float* dst, const float* lut, const int32_t* origin, const uint8_t* flip,
                                 int64_t N, int C, int H, int W, int Ho, int Wo, int layout, void* stream_) {
    if (N < 0) return bad_arg("image_batch: negative N");
    if (C < 1 || C > 4) return bad_arg("image_batch: C must lie in 1 .. 4");
    if (H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) return bad_arg("image_batch: H, W, Ho and Wo must be positive");
    if (Ho > H || Wo > W) return bad_arg("image_batch: the window (Ho, Wo) must fit inside the image (H, W)");
    if (layout != PLEAS_IMAGE_NHWC && layout != PLEAS_IMAGE_NCHW) return bad_arg("image_batch: unknown layout");
    if (N == 0) return PLEAS_OK;      // nothing to write
    if (!src || !dst || !lut) return bad_arg("image_batch: null src, dst or lut");
    if ((uintptr_t)dst & 15) return bad_arg("image_batch: dst must be 16-byte aligned");
    if ((double)N * C * H * W >= 4.0e18 || (double)N * C * Ho * Wo >= 1.0e18)
        return bad_arg("image_batch: src or dst does not fit a 64-bit byte offset");
    const int lanes = (int)ceil_div(Wo, kImgStep);
    int log_bx = 0;
    while ((1 << log_bx) < lanes && (1 << log_bx) < kImgThreads) ++log_bx;
    const int by = kImgThreads >> log_bx;
    const unsigned gx = (unsigned)std::min<int64_t>(ceil_div(Ho, by), kImgMaxBlocks);
    const dim3 grid(gx, (unsigned)std::min<int64_t>(N, std::max<int64_t>(kImgMaxBlocks / gx, 1)));
    const int planar = layout == PLEAS_IMAGE_NCHW ? 1 : 0;
    hipStream_t stream = (hipStream_t)stream_;
#define PLEAS_IMAGE_LAUNCH(CH)                                                                                                      \
    hipLaunchKernelGGL(image_batch_kernel<CH>, grid, dim3(kImgThreads), 0, stream, src, dst, lut, origin, flip, N, H, W, Ho, Wo, log_bx, \
                       planar)
    switch (C) {
        case 1: PLEAS_IMAGE_LAUNCH(1); break;
        case 2: PLEAS_IMAGE_LAUNCH(2); break;
        case 3: PLEAS_IMAGE_LAUNCH(3); break;
        default: PLEAS_IMAGE_LAUNCH(4); break;
    }
#undef PLEAS_IMAGE_LAUNCH
    PLEAS_LAUNCH_CHECK("image_batch_kernel");
    return PLEAS_OK;
}
