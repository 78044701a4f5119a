// Host plan of pleas_image_resample (image.hip): PIL's 8-bit bilinear resampling of a ragged uint8 batch, as tables.
// Pure C++ -- no HIP include -- so that the arithmetic can be compiled, run and sanitised where there is no GPU
// (tests/resample_plan_check.cpp includes this file and nothing else of the library).
//
// One pass along an axis, input length `in`, output length `out` (PIL's precompute_coeffs + normalize_coeffs_8bpc for the
// bilinear filter, all in double):
//   scale = in / out;  fs = max(scale, 1);  support = fs;  ksize = 2 * ceil(support) + 1
//   output i:  center = (i + 0.5) * scale;  lo = max(0, (int)(center - support + 0.5));  hi = min(in, (int)(center + support + 0.5))
//              w_j = max(0, 1 - |(lo + j - center + 0.5) * (1 / fs)|),  j in [0, hi - lo);  ww = sum of the w_j in that order;
//              w_j /= ww when ww != 0;  k_j = (int)(0.5 + w_j * 2^22)
//              value = clamp((2^21 + sum_j k_j * in[lo + j]) >> 22, 0, 255)                          (int32; no overflow: 255 * (2^22 + ksize))
// The horizontal pass runs first, its result is stored as uint8, the vertical pass second.  Every product above is either
// exact (a power of two) or feeds a function call, so contraction into multiply-adds could not change a bit; the functions
// that compute in double switch it off all the same.
//
// Descriptor of a sample, kGeomWords int32:  H, W (image), y0, x0, h, w (box inside it), Hv, Wv (virtual output size the box
// is resampled to), oy, ox (origin of the Ho x Wo window of that output which is produced).  A resized crop has Hv x Wv =
// Ho x Wo and origin (0, 0); Resize + CenterCrop has the whole image as its box.
//
// The plan is position independent (offsets in int32 words from its start) and lives in caller memory:
//   header, kHeaderWords | samples, N x kSampleWords | horizontal items, 3 each | vertical items, 3 each |
//   per sample: horizontal bounds (x of the first tap in the IMAGE, taps) x Wo, coefficients Wo x ksize,
//               vertical bounds (first tap's row in the WORKSPACE, taps) x Ho, coefficients Ho x ksize
// An item is (sample, first row, rows): rows of the sample's workspace for the horizontal pass, rows of its output for the
// vertical one.  The workspace holds, per sample, the uint8 [rows][Wo][C] result of the horizontal pass for exactly the source
// rows the window's vertical pass reads.
//
// A CHAIN plan (pleas_image_resample_chain) is two resamplings with a uint8 image in between:
//   img.resize((W1, H1)).crop(box).resize((Wo, Ho))          descriptor, kChainGeomWords int32:  H, W, H1, W1, y0, x0, h, w
// as one position-independent blob:
//   chain header, kChainHeaderWords | stage-1 section | stage-2 plan
// The stage-1 section has the layout of a plan (its offsets count from the section's start) with its own magic word, because
// its output size is per sample: the box h x w of the virtual H1 x W1 image, kept in the sample record (kSWo, and the items'
// rows) with the sample's place in the intermediate buffer (kSMid*).  Its two item tables feed the ragged rows pass
// (src -> scratch [rows_s][w_s][C]) and the bytes pass (scratch -> intermediate uint8 [h_s][w_s][C], samples packed end to end).
// The stage-2 plan is an ordinary plan, unchanged: box = the whole intermediate image, Hv x Wv = Ho x Wo, origin 0, its source
// offsets pointing into the intermediate.  The workspace is three regions, each on a 16-byte boundary, whose offsets the chain
// header holds:  stage-1 scratch at 0 | intermediate | stage-2 scratch.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace pleas {
namespace resample {

constexpr int32_t kMagic = 0x53455250;      // "PRES"
constexpr int kGeomWords = 10;
constexpr int kHeaderWords = 16;
constexpr int kSampleWords = 16;
constexpr int kMaxSide = 16384;             // of an image and of a virtual output: keeps a table below 2^31 words
constexpr int64_t kMaxSamples = 1 << 20;
constexpr int kPrecisionBits = 22;

enum Geom { kGH = 0, kGW, kGY0, kGX0, kGh, kGw, kGHv, kGWv, kGOy, kGOx };
enum Header { kHMagic = 0, kHN, kHC, kHHo, kHWo, kHSrcLo, kHSrcHi, kHWsLo, kHWsHi, kHWords, kHItemsH, kHItemsV, kHOffItemsH,
              kHOffItemsV, kHOffSamples, kHReserved };
// kSWo, kSMidLo, kSMidHi: the stage-1 section of a chain only (zero in an ordinary plan, whose output width is the header's)
enum Sample { kSSrcLo = 0, kSSrcHi, kSWsLo, kSWsHi, kSW, kSRow0, kSRows, kSOffHB, kSOffHK, kSKsH, kSOffVB, kSOffVK, kSKsV,
              kSWo, kSMidLo, kSMidHi };

constexpr int32_t kChainMagic = 0x48435250;      // "PRCH"
constexpr int32_t kStage1Magic = 0x31535250;     // "PRS1": laid out like a plan, not one (output sizes are per sample)
constexpr int kChainGeomWords = 8;
constexpr int kChainHeaderWords = 24;
enum ChainGeom { kCGH = 0, kCGW, kCGH1, kCGW1, kCGY0, kCGX0, kCGh, kCGw };
// kCOff1, kCOff2: words from the blob's start to the stage-1 section and to the stage-2 plan; kCMidAt, kCWs2At: bytes from the
// workspace's start to the intermediate and to the stage-2 scratch; kCMid: bytes of the intermediate; kCWs: of the workspace
enum ChainHeader { kCMagic = 0, kCN, kCC, kCHo, kCWo, kCSrcLo, kCSrcHi, kCWsLo, kCWsHi, kCWords, kCOff1, kCOff2, kCMidAtLo, kCMidAtHi,
                   kCMidLo, kCMidHi, kCWs2AtLo, kCWs2AtHi };

struct Axis {
    double scale, fs;
    int ksize;
};

inline Axis axis_of(int in, int out) {
#pragma STDC FP_CONTRACT OFF
    Axis a;
    a.scale = (double)in / (double)out;
    a.fs = a.scale < 1.0 ? 1.0 : a.scale;
    a.ksize = 2 * (int)std::ceil(a.fs) + 1;
    return a;
}

// taps of output i: [lo, lo + n) of the input, n <= ksize
inline void axis_bounds(const Axis& a, int in, int i, int& lo, int& n) {
#pragma STDC FP_CONTRACT OFF
    const double center = (i + 0.5) * a.scale;
    lo = (int)(center - a.fs + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(center + a.fs + 0.5);
    if (hi > in) hi = in;
    n = hi - lo;
}

// the n integer coefficients of output i into k[0 .. ksize), the rest zero; `w` is scratch of ksize doubles
inline void axis_coeffs(const Axis& a, int i, int lo, int n, double* w, int32_t* k) {
#pragma STDC FP_CONTRACT OFF
    const double center = (i + 0.5) * a.scale, ss = 1.0 / a.fs;
    double ww = 0.0;
    for (int j = 0; j < n; ++j) {
        double x = (lo + j - center + 0.5) * ss;
        if (x < 0.0) x = -x;
        w[j] = x < 1.0 ? 1.0 - x : 0.0;
        ww += w[j];
    }
    for (int j = 0; j < n; ++j) {
        if (ww != 0.0) w[j] /= ww;
        k[j] = (int32_t)(0.5 + w[j] * (double)(1 << kPrecisionBits));      // bilinear: no negative weight
    }
    for (int j = n; j < a.ksize; ++j) k[j] = 0;
}

// rows of an item: enough outputs for a workgroup whatever Wo is
inline int rows_per_item_h(int Wo) { return std::min(256, std::max(4, (2048 + Wo - 1) / Wo)); }
inline int rows_per_item_v(int Wo) { return std::min(256, std::max(2, (1024 + Wo - 1) / Wo)); }

inline const char* check_sizes(int64_t N, int Ho, int Wo) {
    if (N < 0 || N > kMaxSamples) return "image_resample: N must lie in 0 .. 2^20";
    if (Ho < 1 || Wo < 1) return "image_resample: Ho and Wo must be positive";
    if (Ho > kMaxSide || Wo > kMaxSide) return "image_resample: Ho and Wo are at most 16384";
    return nullptr;
}

inline const char* check_geom(const int32_t* g, int Ho, int Wo) {
    if (g[kGH] < 1 || g[kGW] < 1 || g[kGh] < 1 || g[kGw] < 1 || g[kGHv] < 1 || g[kGWv] < 1)
        return "image_resample: image, box and virtual sizes must be positive";
    if (g[kGH] > kMaxSide || g[kGW] > kMaxSide) return "image_resample: a source side is at most 16384";
    if (g[kGHv] > kMaxSide || g[kGWv] > kMaxSide) return "image_resample: a virtual output side is at most 16384";
    if (g[kGY0] < 0 || g[kGX0] < 0 || (int64_t)g[kGY0] + g[kGh] > g[kGH] || (int64_t)g[kGX0] + g[kGw] > g[kGW])
        return "image_resample: the box must lie inside the image";
    if (g[kGOy] < 0 || g[kGOx] < 0 || (int64_t)g[kGOy] + Ho > g[kGHv] || (int64_t)g[kGOx] + Wo > g[kGWv])
        return "image_resample: the window must lie inside the virtual output";
    return nullptr;
}

struct Layout {
    struct Per {
        Axis ax, ay;
        int rlo, rows;      // source rows (of the box) the window's vertical pass reads: [rlo, rlo + rows)
    };
    std::vector<Per> per;
    int64_t items_h = 0, items_v = 0, words = 0;
};

// What one sample (descriptor g, window Ho x Wo) adds to a plan: its axes and source rows into p, its table words into `words`,
// its items into the two counts.  nullptr, or what is wrong.
inline const char* layout_sample(const int32_t* g, int Ho, int Wo, Layout::Per& p, int64_t& words, int64_t& items_h, int64_t& items_v) {
    if (const char* e = check_geom(g, Ho, Wo)) return e;
    p.ax = axis_of(g[kGw], g[kGWv]);
    p.ay = axis_of(g[kGh], g[kGHv]);
    int lo0, n0, lo1, n1;
    axis_bounds(p.ay, g[kGh], g[kGOy], lo0, n0);
    axis_bounds(p.ay, g[kGh], g[kGOy] + Ho - 1, lo1, n1);
    p.rlo = lo0;
    p.rows = lo1 + n1 - lo0;
    if (p.rows < 1 || n0 < 1) return "image_resample: an output row without taps";      // cannot happen for a valid box
    const int rh = rows_per_item_h(Wo), rv = rows_per_item_v(Wo);
    items_h += (p.rows + rh - 1) / rh;
    items_v += (Ho + rv - 1) / rv;
    words += 2 * (int64_t)Wo + (int64_t)Wo * p.ax.ksize + 2 * (int64_t)Ho + (int64_t)Ho * p.ay.ksize;
    return nullptr;
}

// Sizes of the plan of `geom` (validated here).  nullptr, or what is wrong.
inline const char* layout_of(const int32_t* geom, int64_t N, int Ho, int Wo, Layout& L) {
    if (const char* e = check_sizes(N, Ho, Wo)) return e;
    if (N > 0 && !geom) return "image_resample: null geometry";
    L.per.resize((size_t)N);
    L.items_h = L.items_v = 0;
    int64_t words = kHeaderWords + N * kSampleWords;
    for (int64_t s = 0; s < N; ++s)
        if (const char* e = layout_sample(geom + s * kGeomWords, Ho, Wo, L.per[(size_t)s], words, L.items_h, L.items_v)) return e;
    words += 3 * (L.items_h + L.items_v);
    if (words >= ((int64_t)1 << 31) / 4) return "image_resample: the plan does not fit 2^31 bytes";
    L.words = words;
    return nullptr;
}

inline int64_t pair64(const int32_t* p) { return (int64_t)(uint32_t)p[0] | ((int64_t)p[1] << 32); }
inline void set64(int32_t* p, int64_t v) {
    p[0] = (int32_t)(uint32_t)(v & 0xffffffff);
    p[1] = (int32_t)(v >> 32);
}

// The record (all but the source offset), the items and the tables of sample s, window Ho x Wo, whose tables begin at word
// `at` of `plan` and whose scratch begins at byte `ws` of the workspace; both move past the sample.
inline void fill_sample(int32_t* plan, int32_t* sm, int64_t s, const int32_t* g, const Layout::Per& p, int C, int Ho, int Wo, int64_t& at,
                        int64_t& ws, int32_t*& ih, int32_t*& iv, std::vector<double>& w) {
    const int rh = rows_per_item_h(Wo), rv = rows_per_item_v(Wo);
    set64(sm + kSWsLo, ws);
    ws += ((int64_t)p.rows * Wo * C + 15) / 16 * 16;
    sm[kSW] = g[kGW];
    sm[kSRow0] = g[kGY0] + p.rlo;
    sm[kSRows] = p.rows;
    for (int r = 0; r < p.rows; r += rh, ih += 3) ih[0] = (int32_t)s, ih[1] = r, ih[2] = std::min(rh, p.rows - r);
    for (int y = 0; y < Ho; y += rv, iv += 3) iv[0] = (int32_t)s, iv[1] = y, iv[2] = std::min(rv, Ho - y);
    w.resize((size_t)std::max(p.ax.ksize, p.ay.ksize));
    sm[kSOffHB] = (int32_t)at;
    at += 2 * (int64_t)Wo;
    sm[kSOffHK] = (int32_t)at;
    at += (int64_t)Wo * p.ax.ksize;
    sm[kSKsH] = p.ax.ksize;
    sm[kSOffVB] = (int32_t)at;
    at += 2 * (int64_t)Ho;
    sm[kSOffVK] = (int32_t)at;
    at += (int64_t)Ho * p.ay.ksize;
    sm[kSKsV] = p.ay.ksize;
    for (int x = 0; x < Wo; ++x) {
        int lo, n;
        axis_bounds(p.ax, g[kGw], g[kGOx] + x, lo, n);
        axis_coeffs(p.ax, g[kGOx] + x, lo, n, w.data(), plan + sm[kSOffHK] + (int64_t)x * p.ax.ksize);
        plan[sm[kSOffHB] + 2 * x] = g[kGX0] + lo;
        plan[sm[kSOffHB] + 2 * x + 1] = n;
    }
    for (int y = 0; y < Ho; ++y) {
        int lo, n;
        axis_bounds(p.ay, g[kGh], g[kGOy] + y, lo, n);
        axis_coeffs(p.ay, g[kGOy] + y, lo, n, w.data(), plan + sm[kSOffVK] + (int64_t)y * p.ay.ksize);
        plan[sm[kSOffVB] + 2 * y] = lo - p.rlo;
        plan[sm[kSOffVB] + 2 * y + 1] = n;
    }
}

// Writes the plan of N samples into plan[0 .. plan_bytes).  src_offset[s]: byte offset of sample s (packed uint8 [H][W][C]) in
// a buffer of src_bytes.  nullptr, or what is wrong (then the plan's magic is not set).
inline const char* build_plan(const int32_t* geom, const int64_t* src_offset, int64_t N, int C, int Ho, int Wo, int64_t src_bytes,
                              int32_t* plan, size_t plan_bytes) {
    if (C < 1 || C > 4) return "image_resample: C must lie in 1 .. 4";
    if (!plan || plan_bytes < (size_t)kHeaderWords * 4) return "image_resample: null or short plan memory";
    if ((uintptr_t)plan & 3) return "image_resample: plan memory must be 4-byte aligned";
    plan[kHMagic] = 0;
    if (src_bytes < 0) return "image_resample: negative source size";
    Layout L;
    if (const char* e = layout_of(geom, N, Ho, Wo, L)) return e;
    if (N > 0 && !src_offset) return "image_resample: null source offsets";
    if ((size_t)L.words * 4 > plan_bytes) return "image_resample: plan memory too small (ask pleas_resample_plan_bytes)";
    for (int64_t s = 0; s < N; ++s) {
        const int32_t* g = geom + s * kGeomWords;
        const int64_t bytes = (int64_t)g[kGH] * g[kGW] * C;
        if (src_offset[s] < 0 || src_offset[s] > src_bytes || bytes > src_bytes - src_offset[s])
            return "image_resample: a sample does not lie inside the source buffer";
    }
    std::memset(plan, 0, (size_t)L.words * 4);
    int32_t* samples = plan + kHeaderWords;
    int64_t at = kHeaderWords + N * kSampleWords;
    const int64_t off_items_h = at;
    at += 3 * L.items_h;
    const int64_t off_items_v = at;
    at += 3 * L.items_v;
    int32_t* ih = plan + off_items_h;
    int32_t* iv = plan + off_items_v;
    int64_t ws = 0;
    std::vector<double> w;
    for (int64_t s = 0; s < N; ++s) {
        int32_t* sm = samples + s * kSampleWords;
        set64(sm + kSSrcLo, src_offset[s]);
        fill_sample(plan, sm, s, geom + s * kGeomWords, L.per[(size_t)s], C, Ho, Wo, at, ws, ih, iv, w);
    }
    plan[kHN] = (int32_t)N;
    plan[kHC] = C;
    plan[kHHo] = Ho;
    plan[kHWo] = Wo;
    set64(plan + kHSrcLo, src_bytes);
    set64(plan + kHWsLo, ws);
    plan[kHWords] = (int32_t)L.words;
    plan[kHItemsH] = (int32_t)L.items_h;
    plan[kHItemsV] = (int32_t)L.items_v;
    plan[kHOffItemsH] = (int32_t)off_items_h;
    plan[kHOffItemsV] = (int32_t)off_items_v;
    plan[kHOffSamples] = kHeaderWords;
    plan[kHMagic] = kMagic;
    return nullptr;
}

// The header of a plan the caller hands back: what a launch checks on the host copy.
inline const char* check_header(const int32_t* plan, size_t plan_bytes) {
    if (!plan || plan_bytes < (size_t)kHeaderWords * 4 || ((uintptr_t)plan & 3)) return "image_resample: null, short or unaligned plan";
    if (plan[kHMagic] != kMagic) return "image_resample: not a plan (build it with pleas_resample_plan)";
    if (plan[kHWords] < kHeaderWords || (size_t)plan[kHWords] * 4 > plan_bytes) return "image_resample: the plan is longer than plan_bytes";
    if (plan[kHN] < 0 || plan[kHC] < 1 || plan[kHC] > 4 || plan[kHHo] < 1 || plan[kHWo] < 1 || plan[kHItemsH] < 0 || plan[kHItemsV] < 0 ||
        pair64(plan + kHWsLo) < 0 || pair64(plan + kHSrcLo) < 0)
        return "image_resample: damaged plan header";
    return nullptr;
}

inline uint8_t clip8(int32_t v) {
    v >>= kPrecisionBits;
    return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// The horizontal pass of a plan (ragged = false: every sample Wo wide) or of a chain's stage-1 section (ragged = true: sample s
// is its own kSWo wide), item by item as resample_rows_kernel does.
inline void execute_rows(const uint8_t* src, const int32_t* plan, uint8_t* ws, bool ragged) {
    const int C = plan[kHC];
    const int32_t* samples = plan + plan[kHOffSamples];
    const int32_t* items = plan + plan[kHOffItemsH];
    for (int32_t it = 0; it < plan[kHItemsH]; ++it) {
        const int32_t* sm = samples + (int64_t)items[3 * it] * kSampleWords;
        const uint8_t* img = src + pair64(sm + kSSrcLo);
        uint8_t* rows = ws + pair64(sm + kSWsLo);
        const int32_t* hb = plan + sm[kSOffHB];
        const int Wo = ragged ? sm[kSWo] : plan[kHWo];
        for (int r = items[3 * it + 1]; r < items[3 * it + 1] + items[3 * it + 2]; ++r) {
            const uint8_t* in = img + (int64_t)(sm[kSRow0] + r) * sm[kSW] * C;
            uint8_t* out = rows + (int64_t)r * Wo * C;
            for (int x = 0; x < Wo; ++x) {
                const int32_t* k = plan + sm[kSOffHK] + (int64_t)x * sm[kSKsH];
                for (int c = 0; c < C; ++c) {
                    int32_t acc = 1 << (kPrecisionBits - 1);
                    for (int j = 0; j < hb[2 * x + 1]; ++j) acc += k[j] * (int32_t)in[(int64_t)(hb[2 * x] + j) * C + c];
                    out[x * C + c] = clip8(acc);
                }
            }
        }
    }
}

// Executes a plan on the host, item by item as the two kernels do.  dst fp32 [N][C][Ho][Wo] through lut [C][256]; dst_u8 (or
// null) the resampled bytes [N][Ho][Wo][C], both after the flip.  `ws`: at least the header's workspace bytes.
inline void execute(const uint8_t* src, const int32_t* plan, const float* lut, const uint8_t* flip, float* dst, uint8_t* dst_u8,
                    uint8_t* ws) {
    const int C = plan[kHC], Ho = plan[kHHo], Wo = plan[kHWo];
    const int32_t* samples = plan + plan[kHOffSamples];
    execute_rows(src, plan, ws, false);
    const int32_t* items = plan + plan[kHOffItemsV];
    for (int32_t it = 0; it < plan[kHItemsV]; ++it) {
        const int64_t s = items[3 * it];
        const int32_t* sm = samples + s * kSampleWords;
        const uint8_t* rows = ws + pair64(sm + kSWsLo);
        const int32_t* vb = plan + sm[kSOffVB];
        const bool fl = flip && flip[s];
        for (int y = items[3 * it + 1]; y < items[3 * it + 1] + items[3 * it + 2]; ++y) {
            const int32_t* k = plan + sm[kSOffVK] + (int64_t)y * sm[kSKsV];
            for (int x = 0; x < Wo; ++x) {
                const int xs = fl ? Wo - 1 - x : x;
                for (int c = 0; c < C; ++c) {
                    int32_t acc = 1 << (kPrecisionBits - 1);
                    for (int j = 0; j < vb[2 * y + 1]; ++j) acc += k[j] * (int32_t)rows[((int64_t)(vb[2 * y] + j) * Wo + xs) * C + c];
                    const uint8_t v = clip8(acc);
                    dst[((s * C + c) * Ho + y) * (int64_t)Wo + x] = lut[c * 256 + v];
                    if (dst_u8) dst_u8[((s * Ho + y) * (int64_t)Wo + x) * C + c] = v;
                }
            }
        }
    }
}

// ---- chains: resize to (H1, W1), crop the box, resize to (Ho, Wo)

inline const char* check_chain_geom(const int32_t* g) {
    if (g[kCGH] < 1 || g[kCGW] < 1 || g[kCGH1] < 1 || g[kCGW1] < 1 || g[kCGh] < 1 || g[kCGw] < 1)
        return "image_resample_chain: image, first-stage and box sizes must be positive";
    if (g[kCGH] > kMaxSide || g[kCGW] > kMaxSide) return "image_resample_chain: a source side is at most 16384";
    if (g[kCGH1] > kMaxSide || g[kCGW1] > kMaxSide) return "image_resample_chain: a first-stage side is at most 16384";
    if (g[kCGY0] < 0 || g[kCGX0] < 0 || (int64_t)g[kCGY0] + g[kCGh] > g[kCGH1] || (int64_t)g[kCGX0] + g[kCGw] > g[kCGW1])
        return "image_resample_chain: the box must lie inside the first-stage image (H1 x W1)";
    return nullptr;
}

// the two ordinary descriptors of a chain's sample: stage 1 produces the box as a window of the whole image's resize,
// stage 2 resamples the whole intermediate image
inline void chain_stage_geoms(const int32_t* g, int Ho, int Wo, int32_t* g1, int32_t* g2) {
    const int32_t a[kGeomWords] = {g[kCGH], g[kCGW], 0, 0, g[kCGH], g[kCGW], g[kCGH1], g[kCGW1], g[kCGY0], g[kCGX0]};
    std::memcpy(g1, a, sizeof a);
    g2[kGH] = g2[kGh] = g[kCGh];
    g2[kGW] = g2[kGw] = g[kCGw];
    g2[kGY0] = g2[kGX0] = g2[kGOy] = g2[kGOx] = 0;
    g2[kGHv] = Ho;
    g2[kGWv] = Wo;
}

struct ChainLayout {
    std::vector<Layout::Per> per;            // stage 1
    std::vector<int32_t> geom1, geom2;       // ordinary descriptors, N x kGeomWords each
    Layout second;                           // the stage-2 plan
    int64_t items_h = 0, items_v = 0, words1 = 0, words = 0;
};

// Sizes of the chain plan of `geom` (validated here).  nullptr, or what is wrong.
inline const char* chain_layout_of(const int32_t* geom, int64_t N, int Ho, int Wo, ChainLayout& L) {
    if (const char* e = check_sizes(N, Ho, Wo)) return e;
    if (N > 0 && !geom) return "image_resample_chain: null geometry";
    L.per.resize((size_t)N);
    L.geom1.resize((size_t)(N * kGeomWords));
    L.geom2.resize((size_t)(N * kGeomWords));
    L.items_h = L.items_v = 0;
    int64_t words = kHeaderWords + N * kSampleWords;
    for (int64_t s = 0; s < N; ++s) {
        const int32_t* g = geom + s * kChainGeomWords;
        if (const char* e = check_chain_geom(g)) return e;
        int32_t* g1 = L.geom1.data() + s * kGeomWords;
        int32_t* g2 = L.geom2.data() + s * kGeomWords;
        chain_stage_geoms(g, Ho, Wo, g1, g2);
        if (const char* e = layout_sample(g1, g[kCGh], g[kCGw], L.per[(size_t)s], words, L.items_h, L.items_v)) return e;
    }
    words += 3 * (L.items_h + L.items_v);
    if (const char* e = layout_of(L.geom2.data(), N, Ho, Wo, L.second)) return e;
    L.words1 = words;
    L.words = kChainHeaderWords + words + L.second.words;
    if (L.words >= ((int64_t)1 << 31) / 4) return "image_resample_chain: the plan does not fit 2^31 bytes";
    return nullptr;
}

// Writes the chain plan of N samples into plan[0 .. plan_bytes); arguments as build_plan's, geom N x kChainGeomWords.  nullptr,
// or what is wrong (then the plan's magic is not set).
inline const char* build_chain_plan(const int32_t* geom, const int64_t* src_offset, int64_t N, int C, int Ho, int Wo, int64_t src_bytes,
                                    int32_t* plan, size_t plan_bytes) {
    if (!plan || plan_bytes < (size_t)kChainHeaderWords * 4) return "image_resample_chain: null or short plan memory";
    if ((uintptr_t)plan & 3) return "image_resample_chain: plan memory must be 4-byte aligned";
    plan[kCMagic] = 0;      // before every other refusal: what is left behind is never a plan
    if (C < 1 || C > 4) return "image_resample_chain: C must lie in 1 .. 4";
    if (src_bytes < 0) return "image_resample_chain: negative source size";
    ChainLayout L;
    if (const char* e = chain_layout_of(geom, N, Ho, Wo, L)) return e;
    if (N > 0 && !src_offset) return "image_resample_chain: null source offsets";
    if ((size_t)L.words * 4 > plan_bytes) return "image_resample_chain: plan memory too small (ask pleas_resample_chain_plan_bytes)";
    for (int64_t s = 0; s < N; ++s) {
        const int32_t* g = geom + s * kChainGeomWords;
        const int64_t bytes = (int64_t)g[kCGH] * g[kCGW] * C;
        if (src_offset[s] < 0 || src_offset[s] > src_bytes || bytes > src_bytes - src_offset[s])
            return "image_resample_chain: a sample does not lie inside the source buffer";
    }
    std::memset(plan, 0, (size_t)L.words * 4);
    int32_t* p1 = plan + kChainHeaderWords;      // the stage-1 section: offsets count from here
    int32_t* samples = p1 + kHeaderWords;
    int64_t at = kHeaderWords + N * kSampleWords;
    const int64_t off_items_h = at;
    at += 3 * L.items_h;
    const int64_t off_items_v = at;
    at += 3 * L.items_v;
    int32_t* ih = p1 + off_items_h;
    int32_t* iv = p1 + off_items_v;
    int64_t ws1 = 0, mid = 0;
    std::vector<double> w;
    std::vector<int64_t> mid_offset((size_t)N);
    for (int64_t s = 0; s < N; ++s) {
        const int32_t* g = geom + s * kChainGeomWords;
        int32_t* sm = samples + s * kSampleWords;
        set64(sm + kSSrcLo, src_offset[s]);
        sm[kSWo] = g[kCGw];
        set64(sm + kSMidLo, mid);
        mid_offset[(size_t)s] = mid;
        mid += (int64_t)g[kCGh] * g[kCGw] * C;
        fill_sample(p1, sm, s, L.geom1.data() + s * kGeomWords, L.per[(size_t)s], C, g[kCGh], g[kCGw], at, ws1, ih, iv, w);
    }
    p1[kHN] = (int32_t)N;
    p1[kHC] = C;
    set64(p1 + kHSrcLo, src_bytes);
    set64(p1 + kHWsLo, ws1);
    p1[kHWords] = (int32_t)L.words1;
    p1[kHItemsH] = (int32_t)L.items_h;
    p1[kHItemsV] = (int32_t)L.items_v;
    p1[kHOffItemsH] = (int32_t)off_items_h;
    p1[kHOffItemsV] = (int32_t)off_items_v;
    p1[kHOffSamples] = kHeaderWords;
    p1[kHMagic] = kStage1Magic;
    int32_t* p2 = p1 + L.words1;
    if (const char* e = build_plan(L.geom2.data(), mid_offset.data(), N, C, Ho, Wo, mid, p2, (size_t)L.second.words * 4)) return e;
    const int64_t mid_at = ws1, ws2_at = mid_at + (mid + 15) / 16 * 16;      // ws1 is a sum of multiples of 16
    plan[kCN] = (int32_t)N;
    plan[kCC] = C;
    plan[kCHo] = Ho;
    plan[kCWo] = Wo;
    set64(plan + kCSrcLo, src_bytes);
    set64(plan + kCWsLo, ws2_at + pair64(p2 + kHWsLo));
    plan[kCWords] = (int32_t)L.words;
    plan[kCOff1] = kChainHeaderWords;
    plan[kCOff2] = (int32_t)(kChainHeaderWords + L.words1);
    set64(plan + kCMidAtLo, mid_at);
    set64(plan + kCMidLo, mid);
    set64(plan + kCWs2AtLo, ws2_at);
    plan[kCMagic] = kChainMagic;
    return nullptr;
}

// The headers of a chain plan the caller hands back: what a launch checks on the host copy.
inline const char* check_chain_header(const int32_t* plan, size_t plan_bytes) {
    if (!plan || plan_bytes < (size_t)kChainHeaderWords * 4 || ((uintptr_t)plan & 3))
        return "image_resample_chain: null, short or unaligned plan";
    if (plan[kCMagic] != kChainMagic) return "image_resample_chain: not a chain plan (build it with pleas_resample_chain_plan)";
    const int64_t words = plan[kCWords], off1 = plan[kCOff1], off2 = plan[kCOff2];
    if (words < kChainHeaderWords + 2 * kHeaderWords || (size_t)words * 4 > plan_bytes)
        return "image_resample_chain: the plan is longer than plan_bytes";
    if (off1 != kChainHeaderWords || off2 < off1 + kHeaderWords || off2 > words - kHeaderWords)
        return "image_resample_chain: damaged plan header";
    const int32_t* p1 = plan + off1;
    const int32_t* p2 = plan + off2;
    if (check_header(p2, (size_t)(words - off2) * 4) || p2[kHWords] != words - off2) return "image_resample_chain: damaged stage-2 plan";
    const int64_t ws = pair64(plan + kCWsLo), mid_at = pair64(plan + kCMidAtLo), mid = pair64(plan + kCMidLo), ws2_at = pair64(plan + kCWs2AtLo);
    if (p1[kHMagic] != kStage1Magic || p1[kHWords] != off2 - off1 || p1[kHN] != plan[kCN] || p1[kHC] != plan[kCC] || p1[kHItemsH] < 0 ||
        p1[kHItemsV] < 0 || pair64(p1 + kHWsLo) != mid_at)
        return "image_resample_chain: damaged stage-1 section";
    if (plan[kCN] < 0 || plan[kCC] < 1 || plan[kCC] > 4 || p2[kHN] != plan[kCN] || p2[kHC] != plan[kCC] || p2[kHHo] != plan[kCHo] ||
        p2[kHWo] != plan[kCWo] || pair64(plan + kCSrcLo) < 0 || mid_at < 0 || mid < 0 || pair64(p2 + kHSrcLo) != mid || mid > ws2_at - mid_at ||
        pair64(p2 + kHWsLo) != ws - ws2_at)
        return "image_resample_chain: damaged plan header";
    return nullptr;
}

// The vertical pass of a chain's stage-1 section, item by item as resample_bytes_kernel does: a row of the intermediate is
// w_s * C bytes, each the same sum down its column of the scratch, whatever channel it belongs to.
inline void execute_bytes(const uint8_t* ws, const int32_t* p1, uint8_t* mid) {
    const int C = p1[kHC];
    const int32_t* samples = p1 + p1[kHOffSamples];
    const int32_t* items = p1 + p1[kHOffItemsV];
    for (int32_t it = 0; it < p1[kHItemsV]; ++it) {
        const int32_t* sm = samples + (int64_t)items[3 * it] * kSampleWords;
        const uint8_t* rows = ws + pair64(sm + kSWsLo);
        uint8_t* out = mid + pair64(sm + kSMidLo);
        const int32_t* vb = p1 + sm[kSOffVB];
        const int64_t rb = (int64_t)sm[kSWo] * C;
        for (int y = items[3 * it + 1]; y < items[3 * it + 1] + items[3 * it + 2]; ++y) {
            const int32_t* k = p1 + sm[kSOffVK] + (int64_t)y * sm[kSKsV];
            for (int64_t b = 0; b < rb; ++b) {
                int32_t acc = 1 << (kPrecisionBits - 1);
                for (int j = 0; j < vb[2 * y + 1]; ++j) acc += k[j] * (int32_t)rows[(int64_t)(vb[2 * y] + j) * rb + b];
                out[y * rb + b] = clip8(acc);
            }
        }
    }
}

// Executes a chain plan on the host, launch by launch and item by item as the four kernels do.  dst, dst_u8 as execute's;
// `ws`: at least the chain header's workspace bytes (the intermediate lies inside it, at kCMidAt, packed).
inline void execute_chain(const uint8_t* src, const int32_t* plan, const float* lut, const uint8_t* flip, float* dst, uint8_t* dst_u8,
                          uint8_t* ws) {
    const int32_t* p1 = plan + plan[kCOff1];
    uint8_t* mid = ws + pair64(plan + kCMidAtLo);
    execute_rows(src, p1, ws, true);
    execute_bytes(ws, p1, mid);
    execute(mid, plan + plan[kCOff2], lut, flip, dst, dst_u8, ws + pair64(plan + kCWs2AtLo));
}

}  // namespace resample
}  // namespace pleas
