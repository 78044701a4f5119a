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
#include "resample_plan.hpp"

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

// ---- pleas_image_resample: PIL's 8-bit bilinear resampling of a ragged batch in two launches (plan: resample_plan.hpp).
//
//   rows    ws[s][r][x][c]      = clip8(2^21 + sum_j kh[x][j] * src_s[row0 + r][lo_x + j][c])      r over the source rows the window reads
//   planes  dst[s][c][y][x]     = lut[c][ clip8(2^21 + sum_j kv[y][j] * ws[s][lo_y + j][xs][c]) ],   xs = Wo-1-x for a flipped sample
//
// Replaces: RandomResizedCrop / Resize + CenterCrop on the CPU workers of the drivers' loaders
// (experiments/shared_label_space/run_domainnet.py:204-214, experiments/datasets/interface.py:14-18), whose images come in every size.
//
// int32 multiply-adds only (the sum stays below 2^31: 2^21 + 255 * (2^22 + ksize)), no atomics, no floating point but the
// table's values, every byte of ws and every element of dst written once.  A workgroup takes items (sample, first row, rows)
// from the plan's table with a grid stride, so samples of very different sizes share the grid by their rows; inside an item
// the 256 threads form `by` teams of `bx` lanes as in image_batch_kernel: a team takes a row, its lanes run along x side by
// side (4-byte runs into each plane of dst).  Everything indexed with comes from the plan, which the host validated.
//
// pleas_image_resample_chain (at the end of this file) runs two such resamplings in a row: a ragged form of the rows kernel and
// resample_bytes_kernel make the uint8 image between them, then the two kernels above run on it.
constexpr int kResMaxBlocks = 8192;
constexpr int kResStep = 4;               // outputs of a row per lane of its team (bx = the power of two at or above Wo / 4)

typedef __attribute__((address_space(1))) uint8_t gu8;

__device__ __forceinline__ int64_t plan64(gcint* p) { return (int64_t)(uint32_t)p[0] | ((int64_t)p[1] << 32); }
__device__ __forceinline__ int clip8_dev(int v) { return min(max(v >> resample::kPrecisionBits, 0), 255); }

// the team of a row of `outputs` elements, kResStep to a lane: log2 of the power of two at or above outputs / kResStep, at most 8
__device__ __forceinline__ int team_log(int outputs) {
    const int lanes = (outputs + kResStep - 1) / kResStep;
    return lanes <= 1 ? 0 : min(32 - __clz(lanes - 1), 8);
}

// kRagged = false: the rows pass of a plan, every sample Wo = the header's wide, teams of 1 << log_bx lanes.
// kRagged = true: the rows pass of a chain's stage-1 section, sample s its own kSWo wide, the team sized per item from it.
template <int C, bool kRagged>
__global__ __launch_bounds__(kImgThreads) void resample_rows_kernel(const uint8_t* __restrict__ src_, const int32_t* __restrict__ plan_,
                                                                    uint8_t* __restrict__ ws_, int log_bx) {
    using namespace resample;
    gcint* plan = PLEAS_GLOBAL_I(plan_);
    gcu8* src = (gcu8*)src_;
    gu8* ws = (gu8*)ws_;
    const int items = plan[kHItemsH];
    gcint* table = plan + plan[kHOffItemsH];
    for (int it = blockIdx.x; it < items; it += gridDim.x) {
        gcint* sm = plan + plan[kHOffSamples] + (int64_t)table[3 * it] * kSampleWords;
        const int Wo = kRagged ? sm[kSWo] : plan[kHWo];
        if (kRagged) log_bx = team_log(Wo);
        const int bx = 1 << log_bx, by = kImgThreads >> log_bx;
        const int tx = threadIdx.x & (bx - 1), ty = threadIdx.x >> log_bx;
        const int r0 = table[3 * it + 1], r1 = r0 + table[3 * it + 2];
        gcu8* img = src + plan64(sm + kSSrcLo);
        gu8* rows = ws + plan64(sm + kSWsLo);
        gcint* hb = plan + sm[kSOffHB];
        gcint* hk = plan + sm[kSOffHK];
        const int ks = sm[kSKsH], W = sm[kSW], row0 = sm[kSRow0];
        for (int r = r0 + ty; r < r1; r += by) {
            gcu8* in = img + (int64_t)(row0 + r) * W * C;
            gu8* out = rows + (int64_t)r * Wo * C;
            for (int x = tx; x < Wo; x += bx) {
                const int lo = hb[2 * x], n = hb[2 * x + 1];
                gcint* k = hk + (int64_t)x * ks;
                gcu8* p = in + (int64_t)lo * C;
                int acc[C];
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] = 1 << (kPrecisionBits - 1);
                for (int j = 0; j < n; ++j) {
                    const int kj = k[j];
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[c] += kj * (int)p[j * C + c];
                }
#pragma unroll
                for (int c = 0; c < C; ++c) out[x * C + c] = (uint8_t)clip8_dev(acc[c]);
            }
        }
    }
}

// The bytes pass of a chain's stage-1 section: scratch [rows_s][w_s][C] -> intermediate uint8 [h_s][w_s][C].  A row is w_s * C
// bytes, each the same sum down its column whatever channel it belongs to, so one kernel serves every C; a team's lanes run
// along the bytes side by side.  No table, no flip: the intermediate is the image PIL would hold between the two resizes.
__global__ __launch_bounds__(kImgThreads) void resample_bytes_kernel(const uint8_t* __restrict__ ws_, const int32_t* __restrict__ plan_,
                                                                     uint8_t* __restrict__ mid_) {
    using namespace resample;
    gcint* plan = PLEAS_GLOBAL_I(plan_);
    gcu8* ws = (gcu8*)ws_;
    gu8* mid = (gu8*)mid_;
    const int C = plan[kHC], items = plan[kHItemsV];
    gcint* table = plan + plan[kHOffItemsV];
    for (int it = blockIdx.x; it < items; it += gridDim.x) {
        gcint* sm = plan + plan[kHOffSamples] + (int64_t)table[3 * it] * kSampleWords;
        const int rb = sm[kSWo] * C;      // bytes of a row: at most 4 * 16384
        const int log_bx = team_log(rb);
        const int bx = 1 << log_bx, by = kImgThreads >> log_bx;
        const int tx = threadIdx.x & (bx - 1), ty = threadIdx.x >> log_bx;
        const int y0 = table[3 * it + 1], y1 = y0 + table[3 * it + 2];
        gcu8* rows = ws + plan64(sm + kSWsLo);
        gu8* out = mid + plan64(sm + kSMidLo);
        gcint* vb = plan + sm[kSOffVB];
        gcint* vk = plan + sm[kSOffVK];
        const int ks = sm[kSKsV];
        for (int y = y0 + ty; y < y1; y += by) {
            const int lo = vb[2 * y], n = vb[2 * y + 1];
            gcint* k = vk + (int64_t)y * ks;
            for (int b = tx; b < rb; b += bx) {
                gcu8* p = rows + (int64_t)lo * rb + b;
                int acc = 1 << (kPrecisionBits - 1);
                for (int j = 0; j < n; ++j) acc += k[j] * (int)p[(int64_t)j * rb];
                out[(int64_t)y * rb + b] = (uint8_t)clip8_dev(acc);
            }
        }
    }
}

template <int C>
__global__ __launch_bounds__(kImgThreads) void resample_planes_kernel(const uint8_t* __restrict__ ws_, const int32_t* __restrict__ plan_,
                                                                      const float* __restrict__ lut, const uint8_t* __restrict__ flip,
                                                                      float* __restrict__ dst_, int log_bx) {
    using namespace resample;
    __shared__ float lds_table[C * 256];
    for (int i = threadIdx.x; i < C * 256; i += kImgThreads) lds_table[i] = lut[i];
    __syncthreads();

    gcint* plan = PLEAS_GLOBAL_I(plan_);
    gcu8* ws = (gcu8*)ws_;
    gfloat* dst = PLEAS_GLOBAL_W(dst_);
    const int bx = 1 << log_bx, by = kImgThreads >> log_bx;
    const int tx = threadIdx.x & (bx - 1), ty = threadIdx.x >> log_bx;
    const int Ho = plan[kHHo], Wo = plan[kHWo], items = plan[kHItemsV];
    const uint64_t plane = (uint64_t)Ho * (uint64_t)Wo;
    gcint* table = plan + plan[kHOffItemsV];
    for (int it = blockIdx.x; it < items; it += gridDim.x) {
        const int s = table[3 * it];
        gcint* sm = plan + plan[kHOffSamples] + (int64_t)s * kSampleWords;
        const int y0 = table[3 * it + 1], y1 = y0 + table[3 * it + 2];
        gcu8* rows = ws + plan64(sm + kSWsLo);
        gcint* vb = plan + sm[kSOffVB];
        gcint* vk = plan + sm[kSOffVK];
        const int ks = sm[kSKsV];
        const bool fl = flip && flip[s];
        for (int y = y0 + ty; y < y1; y += by) {
            const int lo = vb[2 * y], n = vb[2 * y + 1];
            gcint* k = vk + (int64_t)y * ks;
            gfloat* d = dst + (((uint64_t)s * C) * (uint64_t)Ho + (uint64_t)y) * (uint64_t)Wo;      // plane 0 of the row
            for (int x = tx; x < Wo; x += bx) {
                gcu8* p = rows + ((int64_t)lo * Wo + (fl ? Wo - 1 - x : x)) * C;
                int acc[C];
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] = 1 << (kPrecisionBits - 1);
                for (int j = 0; j < n; ++j) {
                    const int kj = k[j];
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[c] += kj * (int)p[(int64_t)j * Wo * C + c];
                }
#pragma unroll
                for (int c = 0; c < C; ++c) d[(uint64_t)c * plane + x] = lds_table[c * 256 + clip8_dev(acc[c])];
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

extern "C" size_t pleas_resample_plan_bytes(const int32_t* geom, int64_t N, int Ho, int Wo) {
    resample::Layout L;
    if (const char* e = resample::layout_of(geom, N, Ho, Wo, L)) {
        bad_arg(e);
        return 0;
    }
    return (size_t)L.words * 4;
}

extern "C" int pleas_resample_plan(const int32_t* geom, const int64_t* src_offset, int64_t N, int C, int Ho, int Wo, int64_t src_bytes,
                                   void* plan, size_t plan_bytes) {
    if (const char* e = resample::build_plan(geom, src_offset, N, C, Ho, Wo, src_bytes, (int32_t*)plan, plan_bytes)) return bad_arg(e);
    return PLEAS_OK;
}

extern "C" int pleas_resample_plan_info(const void* plan_, size_t plan_bytes, int64_t* info) {
    const int32_t* plan = (const int32_t*)plan_;
    if (const char* e = resample::check_header(plan, plan_bytes)) return bad_arg(e);
    if (!info) return bad_arg("image_resample: null info");
    using namespace resample;
    info[0] = plan[kHN], info[1] = plan[kHC], info[2] = plan[kHHo], info[3] = plan[kHWo];
    info[4] = pair64(plan + kHSrcLo), info[5] = pair64(plan + kHWsLo), info[6] = plan[kHItemsH], info[7] = plan[kHItemsV];
    return PLEAS_OK;
}

extern "C" int pleas_image_resample_host(const uint8_t* src, const void* plan_, size_t plan_bytes, const float* lut, const uint8_t* flip,
                                         float* dst_f32, uint8_t* dst_u8) {
    const int32_t* plan = (const int32_t*)plan_;
    if (const char* e = resample::check_header(plan, plan_bytes)) return bad_arg(e);
    if (plan[resample::kHN] == 0) return PLEAS_OK;
    if (!src || !lut || !dst_f32) return bad_arg("image_resample_host: null src, lut or dst");
    std::vector<uint8_t> ws((size_t)resample::pair64(plan + resample::kHWsLo));
    resample::execute(src, plan, lut, flip, dst_f32, dst_u8, ws.data());
    return PLEAS_OK;
}

extern "C" int pleas_image_resample(const uint8_t* src, const void* plan_dev, const void* plan_host, size_t plan_bytes, const float* lut,
                                    const uint8_t* flip, float* dst, void* ws, size_t ws_bytes, void* stream_) {
    using namespace resample;
    const int32_t* plan = (const int32_t*)plan_host;
    if (const char* e = check_header(plan, plan_bytes)) return bad_arg(e);
    if (plan[kHN] == 0) return PLEAS_OK;      // nothing to write
    if (!src || !plan_dev || !lut || !dst) return bad_arg("image_resample: null src, plan, lut or dst");
    if (((uintptr_t)plan_dev & 3)) return bad_arg("image_resample: the device plan must be 4-byte aligned");
    if ((uintptr_t)dst & 15) return bad_arg("image_resample: dst must be 16-byte aligned");
    const size_t need = (size_t)pair64(plan + kHWsLo);
    if (!ws || ws_bytes < need) return workspace_too_small("image_resample", need);
    const int C = plan[kHC], Wo = plan[kHWo];
    const int lanes = (int)ceil_div(Wo, kResStep);
    int log_bx = 0;
    while ((1 << log_bx) < lanes && (1 << log_bx) < kImgThreads) ++log_bx;
    const dim3 grid_h((unsigned)std::min(plan[kHItemsH], kResMaxBlocks)), grid_v((unsigned)std::min(plan[kHItemsV], kResMaxBlocks));
    hipStream_t stream = (hipStream_t)stream_;
#define PLEAS_RESAMPLE_LAUNCH(CH)                                                                                                    \
    hipLaunchKernelGGL((resample_rows_kernel<CH, false>), grid_h, dim3(kImgThreads), 0, stream, src, (const int32_t*)plan_dev, (uint8_t*)ws,   \
                       log_bx);                                                                                                      \
    hipLaunchKernelGGL(resample_planes_kernel<CH>, grid_v, dim3(kImgThreads), 0, stream, (const uint8_t*)ws,                         \
                       (const int32_t*)plan_dev, lut, flip, dst, log_bx)
    switch (C) {
        case 1: PLEAS_RESAMPLE_LAUNCH(1); break;
        case 2: PLEAS_RESAMPLE_LAUNCH(2); break;
        case 3: PLEAS_RESAMPLE_LAUNCH(3); break;
        default: PLEAS_RESAMPLE_LAUNCH(4); break;
    }
#undef PLEAS_RESAMPLE_LAUNCH
    PLEAS_LAUNCH_CHECK("resample kernels");
    return PLEAS_OK;
}

// ---- pleas_image_resample_chain: Resize -> RandomResizedCrop as two PIL resamplings with a uint8 image in between, four launches
//
//   rows 1    ws1[s][r][x][c]  = clip8(2^21 + sum_j kh1[x][j] * src_s[row0 + r][lo_x + j][c])       x over the box's w_s columns of the
//   bytes 1   mid[s][y][x][c]  = clip8(2^21 + sum_j kv1[y][j] * ws1[s][lo_y + j][x][c])             virtual H1 x W1 image, y over its h_s rows
//   rows 2, planes 2           = the two kernels of pleas_image_resample on mid, under the chain's stage-2 plan
//
// Replaces: Resize(256) -> RandomResizedCrop(224) on the CPU workers of the drivers' train loaders
// (experiments/datasets/interface.py, cub.py, nabird.py, oxford_pets.py, stanford_dogs.py, domainnet.py).
extern "C" size_t pleas_resample_chain_plan_bytes(const int32_t* geom, int64_t N, int Ho, int Wo) {
    resample::ChainLayout L;
    if (const char* e = resample::chain_layout_of(geom, N, Ho, Wo, L)) {
        bad_arg(e);
        return 0;
    }
    return (size_t)L.words * 4;
}

extern "C" int pleas_resample_chain_plan(const int32_t* geom, const int64_t* src_offset, int64_t N, int C, int Ho, int Wo,
                                         int64_t src_bytes, void* plan, size_t plan_bytes) {
    if (const char* e = resample::build_chain_plan(geom, src_offset, N, C, Ho, Wo, src_bytes, (int32_t*)plan, plan_bytes)) return bad_arg(e);
    return PLEAS_OK;
}

extern "C" int pleas_resample_chain_plan_info(const void* plan_, size_t plan_bytes, int64_t* info) {
    const int32_t* plan = (const int32_t*)plan_;
    if (const char* e = resample::check_chain_header(plan, plan_bytes)) return bad_arg(e);
    if (!info) return bad_arg("image_resample_chain: null info");
    using namespace resample;
    const int32_t* p1 = plan + plan[kCOff1];
    const int32_t* p2 = plan + plan[kCOff2];
    info[0] = plan[kCN], info[1] = plan[kCC], info[2] = plan[kCHo], info[3] = plan[kCWo];
    info[4] = pair64(plan + kCSrcLo), info[5] = pair64(plan + kCWsLo), info[6] = pair64(plan + kCMidLo);
    info[7] = p1[kHItemsH], info[8] = p1[kHItemsV], info[9] = p2[kHItemsH], info[10] = p2[kHItemsV];
    return PLEAS_OK;
}

extern "C" int pleas_image_resample_chain_host(const uint8_t* src, const void* plan_, size_t plan_bytes, const float* lut,
                                               const uint8_t* flip, float* dst_f32, uint8_t* dst_u8, uint8_t* mid_u8) {
    using namespace resample;
    const int32_t* plan = (const int32_t*)plan_;
    if (const char* e = check_chain_header(plan, plan_bytes)) return bad_arg(e);
    if (plan[kCN] == 0) return PLEAS_OK;
    if (!src || !lut || !dst_f32) return bad_arg("image_resample_chain_host: null src, lut or dst");
    std::vector<uint8_t> ws((size_t)pair64(plan + kCWsLo));
    execute_chain(src, plan, lut, flip, dst_f32, dst_u8, ws.data());
    if (mid_u8) std::memcpy(mid_u8, ws.data() + pair64(plan + kCMidAtLo), (size_t)pair64(plan + kCMidLo));
    return PLEAS_OK;
}

extern "C" int pleas_image_resample_chain(const uint8_t* src, const void* plan_dev_, const void* plan_host, size_t plan_bytes,
                                          const float* lut, const uint8_t* flip, float* dst, void* ws_, size_t ws_bytes, void* stream_) {
    using namespace resample;
    const int32_t* plan = (const int32_t*)plan_host;
    if (const char* e = check_chain_header(plan, plan_bytes)) return bad_arg(e);
    if (plan[kCN] == 0) return PLEAS_OK;      // nothing to write
    if (!src || !plan_dev_ || !lut || !dst) return bad_arg("image_resample_chain: null src, plan, lut or dst");
    if (((uintptr_t)plan_dev_ & 3)) return bad_arg("image_resample_chain: the device plan must be 4-byte aligned");
    if ((uintptr_t)dst & 15) return bad_arg("image_resample_chain: dst must be 16-byte aligned");
    const size_t need = (size_t)pair64(plan + kCWsLo);
    if (!ws_ || ws_bytes < need) return workspace_too_small("image_resample_chain", need);
    const int32_t* p1 = plan + plan[kCOff1];
    const int32_t* p2 = plan + plan[kCOff2];
    const int32_t* dev1 = (const int32_t*)plan_dev_ + plan[kCOff1];
    const int32_t* dev2 = (const int32_t*)plan_dev_ + plan[kCOff2];
    uint8_t* ws1 = (uint8_t*)ws_;
    uint8_t* mid = ws1 + pair64(plan + kCMidAtLo);
    uint8_t* ws2 = ws1 + pair64(plan + kCWs2AtLo);
    const int C = plan[kCC], Wo = plan[kCWo];
    const int lanes = (int)ceil_div(Wo, kResStep);
    int log_bx = 0;
    while ((1 << log_bx) < lanes && (1 << log_bx) < kImgThreads) ++log_bx;
    const dim3 grid_h1((unsigned)std::min(p1[kHItemsH], kResMaxBlocks)), grid_v1((unsigned)std::min(p1[kHItemsV], kResMaxBlocks));
    const dim3 grid_h2((unsigned)std::min(p2[kHItemsH], kResMaxBlocks)), grid_v2((unsigned)std::min(p2[kHItemsV], kResMaxBlocks));
    hipStream_t stream = (hipStream_t)stream_;
#define PLEAS_CHAIN_LAUNCH(CH)                                                                                                       \
    hipLaunchKernelGGL((resample_rows_kernel<CH, true>), grid_h1, dim3(kImgThreads), 0, stream, src, dev1, ws1, 0);                   \
    hipLaunchKernelGGL(resample_bytes_kernel, grid_v1, dim3(kImgThreads), 0, stream, (const uint8_t*)ws1, dev1, mid);                \
    hipLaunchKernelGGL((resample_rows_kernel<CH, false>), grid_h2, dim3(kImgThreads), 0, stream, (const uint8_t*)mid, dev2, ws2,     \
                       log_bx);                                                                                                      \
    hipLaunchKernelGGL(resample_planes_kernel<CH>, grid_v2, dim3(kImgThreads), 0, stream, (const uint8_t*)ws2, dev2, lut, flip, dst, \
                       log_bx)
    switch (C) {
        case 1: PLEAS_CHAIN_LAUNCH(1); break;
        case 2: PLEAS_CHAIN_LAUNCH(2); break;
        case 3: PLEAS_CHAIN_LAUNCH(3); break;
        default: PLEAS_CHAIN_LAUNCH(4); break;
    }
#undef PLEAS_CHAIN_LAUNCH
    PLEAS_LAUNCH_CHECK("resample chain kernels");
    return PLEAS_OK;
}
