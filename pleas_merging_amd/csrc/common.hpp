// Shared host-side helpers of libpleas_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pleas_hip.h"

namespace pleas {

extern thread_local char g_last_error[256];

inline int hip_fail(hipError_t e, const char* what) {
    std::snprintf(g_last_error, sizeof(g_last_error), "%s: %s", what, hipGetErrorString(e));
    return PLEAS_EHIP;
}

inline int bad_arg(const char* what) {
    std::snprintf(g_last_error, sizeof(g_last_error), "invalid argument: %s", what);
    return PLEAS_EINVAL;
}

#define PLEAS_HIP_CHECK(expr)                                  \
    do {                                                       \
        hipError_t e_ = (expr);                                \
        if (e_ != hipSuccess) return ::pleas::hip_fail(e_, #expr); \
    } while (0)

#define PLEAS_LAUNCH_CHECK(name)                                   \
    do {                                                           \
        hipError_t e_ = hipGetLastError();                         \
        if (e_ != hipSuccess) return ::pleas::hip_fail(e_, name);  \
    } while (0)

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
// every table of a plan starts on a 256-byte boundary of the caller's workspace
inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }

// PLEAS_ACT_RELU6 of every epilogue that carries an activation code: F.relu6 / torch.clamp(v, 0, 6) for every fp32 input -- both
// comparisons are false for a NaN, which stays; +inf -> 6, -inf -> 0.  No rounding: the result is 0, 6 or v itself.
__device__ __forceinline__ float relu6_keep_nan(float v) { return v < 0.f ? 0.f : (v > 6.f ? 6.f : v); }

// Pointers that reach a kernel through a device-side table are "generic" to hipcc, which then emits
// flat_load / flat_store: those count on lgkmcnt as well as vmcnt, so every LDS wait in the MFMA loop
// also waits for the global prefetch.  Casting to the global address space gives global_load / global_store.
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) const float cgfloat;
typedef __attribute__((address_space(1))) const int gcint;
#define PLEAS_GLOBAL(p) ((::pleas::cgfloat*)(p))
#define PLEAS_GLOBAL_W(p) ((::pleas::gfloat*)(p))
#define PLEAS_GLOBAL_I(p) ((::pleas::gcint*)(p))

// ---- alternative arithmetics of the contraction kernels (pleas_arith): an fp32 value as the EXACT sum of three bf16 values,
// v = h1 + h2 + h3 (8 + 8 + 8 significant bits, each the round-to-nearest bf16 of what the previous ones left; bf16 has
// fp32's exponent range), so that an fp32 product becomes bf16-MFMA products with fp32 accumulation.  Every bf16 x bf16
// product has at most 16 significant bits: it is exact in fp32, the only rounding is the accumulation.
//   six products (PLEAS_ARITH_SPLIT_BF16):  x * y = x1 y1 + (x1 y2 + x2 y1) + (x2 y2 + x1 y3 + x3 y1) + dropped terms
//     dropped: x2 y3 + x3 y2 + x3 y3, up to about 2^-25 .. 2^-24 |x y|: half to one fp32 ulp of the product
//   nine products (PLEAS_ARITH_SPLIT_BF16_EXACT): nothing dropped, every fp32 product is summed exactly as its nine parts
// Six (nine) v_mfma_f32_32x32x16_bf16 (32 cycles each, K = 16) replace eight v_mfma_f32_32x32x2_f32 (64 cycles each, K = 2):
// 2.67x (1.78x) less matrix-pipe time.  The split is done once per element when a K chunk goes from registers to LDS, the same
// way for both: the two differ only in the MFMA list.  Not for inf / NaN operands (inf - inf in the residual).
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
constexpr int kSplitRow = 104;   // bf16 per LDS row of a split image: 3 planes x 32 k + 8 pad = 208 B (13 16-byte slots: odd,
                                 // so the 16 rows of a ds_read_b128 lane group fall on 16 different slots)
__device__ __forceinline__ uint32_t split_bf16_pair(float a, float b) {
    const f32x2_t v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));      // a in the low half
}
// two values at a time: one v_cvt_pk_bf16_f32 per pair and plane, the bf16 values back as floats by a shift / a mask
__device__ __forceinline__ void split3_pair(float a, float b, uint32_t (&p)[3]) {
    p[0] = split_bf16_pair(a, b);
    const float ra = a - __builtin_bit_cast(float, p[0] << 16), rb = b - __builtin_bit_cast(float, p[0] & 0xffff0000u);
    p[1] = split_bf16_pair(ra, rb);
    p[2] = split_bf16_pair(ra - __builtin_bit_cast(float, p[1] << 16), rb - __builtin_bit_cast(float, p[1] & 0xffff0000u));
}
// Which row of a 32-row staging pass the 8-lane group g = tid / 8 (0 .. 31) writes under the split arithmetic.  Rows of a split
// image are kSplitRow = 208 bytes apart (the stride that keeps the 16-byte fragment READS conflict-free) and a lane writes 8 bytes
// per plane, so the four CONSECUTIVE rows of a half-wave overlap in 4 of 64 banks pairwise (a two-way conflict on every plane
// write: profiles/r05_pmc_split_*.txt); rows 4 apart start 16 banks apart and tile the 64 banks exactly.  Which lane group
// stages which row is free -- global rows are whole cache lines either way.
__device__ __forceinline__ int split_stage_row(int g) { return ((g & 3) << 2) | ((g >> 2) & 3) | (g & 16); }
// four consecutive k of one row -> the row's three planes of an LDS split image (`row` points at the row's plane 0, `col` = k)
__device__ __forceinline__ void split3_store4(__bf16* row, int col, float v0, float v1, float v2, float v3) {
    uint32_t lo[3], hi[3];
    split3_pair(v0, v1, lo);
    split3_pair(v2, v3, hi);
#pragma unroll
    for (int p = 0; p < 3; ++p) *reinterpret_cast<u32x2_t*>(row + p * 32 + col) = u32x2_t{lo[p], hi[p]};
}
// the products of one 16-deep k step, smallest terms first: NPROD = 6 (x2 y3, x3 y2, x3 y3 dropped) or all 9
typedef float f32x16_t __attribute__((ext_vector_type(16)));
template <int NPROD = 6>
__device__ __forceinline__ f32x16_t split3_mfma(const bf16x8_t (&a)[3], const bf16x8_t (&b)[3], f32x16_t c) {
    static_assert(NPROD == 6 || NPROD == 9, "six or nine of the nine bf16 products");
    if constexpr (NPROD == 9) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[2], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[2], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[1], c, 0, 0, 0);
    }
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], c, 0, 0, 0);
    return c;
}
// SPLIT (the kernels' template parameter = pleas_arith's mode: 0 exact, 1 six products, 2 nine) -> products per step
constexpr int split_products(int split) { return split == 2 ? 9 : 6; }
// process-wide arithmetic switch (pleas_arith): 0 = exact fp32 MFMA (default), 1 / 2 = split bf16 with six / nine products where
// a kernel has the form
int arith_mode();

// bn_train.hip, for the convolution that emits its output's batch statistics (conv_fwd.hip): `tile_part` [pixel tiles][2][channels][2]
// holds, per tile of `tile` pixels (of ptot, `per_batch` to a batch) and channel, the sums of y and y^2 over the tile's pixels of
// the first batch it touches (segment 0) and of the next one (segment 1).  Sums them per (batch, channel) into `sums`
// [batches][channels][2] (+ a moments tail of the same size) and folds them with bn_train_finalize_kernel (S = 1).
int bn_fold_tile_partials(const double* tile_part, int tile, uint32_t ptot, uint32_t per_batch, int channels, int batches, double* sums,
                          const float* gamma, const float* beta, double eps, double momentum, float* running_mean, float* running_var,
                          int64_t* num_batches_tracked, float* scale, float* shift, hipStream_t stream);

// ---- launch shape of a streaming kernel (elementwise.hip, bn_train.hip, target_residual in conv.hip): what the launcher
// computes its grid from AND what the host-only query pleas_stream_plan_info answers -- one function per kernel makes both.
struct StreamPlan {
    int vec = 1;          // floats per load / store: 4 (16-byte path) or 1
    int form = 0;         // where a launcher picks between two kernels (bn_act_maxpool: 0 general, 1 stem)
    unsigned blocks = 0;  // workgroups; 0: nothing to do, nothing is launched
    int threads = 256;    // per workgroup
    int lanes = 1;        // threads that share one work item (64: a wave per row)
    int64_t work = 0;     // work items the grid strides over (channel_sum / bn_train_fold: one thread's inner loop)
    int S = 0;            // bn_train_fold: sample slabs per channel
    int64_t sweeps() const {
        const int64_t per = (int64_t)blocks * threads / lanes;
        return per ? ceil_div(work, per) : 0;
    }
};
// the shape checks of the launches live in these too: a refused geometry is refused with one message from either side
int bn_train_stream_plan(int64_t n, int batches, int channels, int64_t inner, bool aligned, StreamPlan& p);    // bn_train.hip
int target_residual_stream_plan(int64_t N, int64_t C, int64_t Csrc, int64_t HW, bool aligned, StreamPlan& p);  // conv.hip

// ---- opt-in per-kernel timing with HIP events on the launch stream (pleas_prof_* in the C-ABI)
enum ProfKernel { kProfGramPartial = 0, kProfGramFinalize, kProfLsap, kProfMergeBlocks, kProfMaskedAdam, kProfSqerr,
                  kProfConvFwd, kProfConvWgrad, kProfNormalEq, kProfSolve, kProfBnAct, kProfConv2d, kProfCount };
extern bool g_prof_on;
extern unsigned g_prof_mask;   // bit k set: kernel id k is recorded while profiling is on
void prof_begin(int kernel, double flops, double bytes, hipStream_t stream);
void prof_end(hipStream_t stream);

struct ProfScope {
    hipStream_t s;
    bool on;
    ProfScope(int kernel, double flops, double bytes, hipStream_t stream) : s(stream), on(g_prof_on && ((g_prof_mask >> kernel) & 1u)) {
        if (on) prof_begin(kernel, flops, bytes, s);
    }
    ~ProfScope() {
        if (on) prof_end(s);
    }
};


// a caller's workspace holds fewer than the `need` bytes `what` asks for: the answer a caller sizes its workspace again on
inline int workspace_too_small(const char* what, size_t need) {
    std::snprintf(g_last_error, sizeof(g_last_error), "%s workspace too small: need %zu bytes", what, need);
    return PLEAS_ENOMEM;
}

// ---- a few plans per grouped launch (host side), and the ws / ws_fresh protocol of include/pleas_hip.h written once.
// A plan (work-item tables of one layer / node list; members `key`, `total` = workspace bytes, `uploaded`) is keyed by its
// geometry AND the address of the caller's workspace the tables are uploaded to (element WS of the key).  Keeping several lets
// callers that alternate inside one process -- two fitters, the per-group contractions of weight matching, matching next to
// PLeaS -- find their plan again instead of rebuilding and re-uploading it at every call.  Slots are recycled round robin.
// Guarded by the caller's mutex.  A launch entry point calls `get`, then `prepare`, then launches.
struct PlanTable {              // one static table of a plan: `bytes` from `host` to `offset` of the workspace
    size_t offset;
    const void* host;
    size_t bytes;
};
template <class T>
inline PlanTable plan_table(size_t offset, const std::vector<T>& v) { return PlanTable{offset, v.data(), v.size() * sizeof(T)}; }

template <class Plan, int WS, int N = 8>
struct PlanCache {
    Plan slots[N];
    unsigned turn = 0;
    Plan* last = nullptr;       // most recently used (diagnostics)
    Plan* find(const std::vector<int64_t>& key) {
        for (auto& p : slots)
            if (!p.key.empty() && p.key == key) return last = &p;
        return nullptr;
    }
    Plan& take() {              // slot for a new plan: the caller builds it, then sets its key
        Plan& p = slots[turn++ % N];
        p.key.clear();
        p.uploaded = false;
        return *(last = &p);
    }
    // p's tables are about to be written into its workspace: other plans that had theirs at that address lost them
    void claims_workspace(const Plan& p) {
        for (auto& o : slots)
            if (&o != &p && (int)o.key.size() > WS && (int)p.key.size() > WS && o.key[WS] == p.key[WS]) o.uploaded = false;
    }
    // The plan of `key` into `plan`: the cached one, or a recycled slot filled by `build(Plan&)`, whose error code is passed on
    // (the slot then stays without a key).  `key` is consumed.
    template <class Build>
    int get(std::vector<int64_t>& key, Plan*& plan, Build&& build) {
        if ((plan = find(key))) return PLEAS_OK;
        Plan& p = take();
        const int rc = build(p);
        if (rc != PLEAS_OK) return rc;
        p.key.swap(key);
        plan = &p;
        return PLEAS_OK;
    }
    // p's static tables into the caller's workspace, once per (plan, workspace).  `ws_fresh`: the caller says the tables inside
    // ws are not (or no longer) there.  A workspace below p.total drops the plan's key (the caller comes back with another
    // workspace, i.e. another key) and answers PLEAS_ENOMEM.  `tables()` lists what to upload and is called only when an upload
    // is due; what it points at must live until this returns (the stream is synchronised: once per plan).
    template <class Tables>
    int prepare(Plan& p, const char* what, void* ws, size_t ws_bytes, int ws_fresh, hipStream_t stream, Tables&& tables) {
        if (ws_fresh) p.uploaded = false;
        if (!ws || ws_bytes < p.total) {
            p.key.clear();
            return workspace_too_small(what, p.total);
        }
        if (p.uploaded) return PLEAS_OK;
        claims_workspace(p);
        for (const PlanTable& t : tables())
            if (t.bytes) PLEAS_HIP_CHECK(hipMemcpyAsync((char*)ws + t.offset, t.host, t.bytes, hipMemcpyHostToDevice, stream));
        PLEAS_HIP_CHECK(hipStreamSynchronize(stream));
        p.uploaded = true;
        return PLEAS_OK;
    }
};

// ---- N side streams of the library + the events to fork from / join into the caller's stream, one set per device (streams
// belong to the device that was current when they were created), created on first use and kept for the process; no device
// memory.  Every grouped launch that forks owns an instance, so two launches never wait on each other's events.  Guarded by
// the caller's mutex.
template <int N>
struct SideStreams {
    struct Set {
        hipStream_t streams[N];
        hipEvent_t forked, joined[N];
        bool ok = false;        // false: creation failed, everything goes back to back on the caller's stream
    };
    static constexpr int kMaxDev = 16;
    Set sets[kMaxDev], none;
    bool tried[kMaxDev] = {false};
    Set& current() {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) return none;
        Set& s = sets[dev];
        if (!tried[dev]) {
            tried[dev] = true;
            bool ok = hipEventCreateWithFlags(&s.forked, hipEventDisableTiming) == hipSuccess;
            for (int i = 0; ok && i < N; ++i)
                ok = hipStreamCreateWithFlags(&s.streams[i], hipStreamNonBlocking) == hipSuccess &&
                     hipEventCreateWithFlags(&s.joined[i], hipEventDisableTiming) == hipSuccess;
            s.ok = ok;
        }
        return s;
    }
};

// ---- XCD-aware work-item order for grouped launches (host side).
// Workgroup b of a grid runs on XCD b % 8, and every XCD has a private L2.  Items that read the same operand rows
// (same `key`) are therefore given grid positions of ONE residue class, so that their re-reads hit that L2 instead
// of crossing to the MALL / HBM once per XCD.  Groups go to the least-loaded of 8 queues (longest items first), the
// queues are interleaved (position 8 j + x = j-th item of queue x) and short queues are padded with `noop`.
// PLEAS_XCD_ORDER=0 in the environment keeps the plain longest-first order (A/B experiments).
template <class Item>
struct XcdWork {
    double w;       // relative duration of the item
    int64_t key;    // sharing key
    Item it;
};
template <class Item>
inline std::vector<Item> xcd_order_items(std::vector<XcdWork<Item>>& work, const Item& noop, bool by_default = true) {
    std::vector<Item> out;
    const char* env = std::getenv("PLEAS_XCD_ORDER");
    if (env ? env[0] == '0' : !by_default) {
        std::stable_sort(work.begin(), work.end(), [](const XcdWork<Item>& a, const XcdWork<Item>& b) { return a.w > b.w; });
        for (auto& x : work) out.push_back(x.it);
        return out;
    }
    struct Group { double total = 0, longest = 0; std::vector<size_t> idx; };
    std::vector<Group> groups;
    {
        std::vector<size_t> order(work.size());
        for (size_t i = 0; i < work.size(); ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return work[a].key < work[b].key; });
        int64_t last = 0;
        for (size_t n = 0; n < order.size(); ++n) {
            const size_t i = order[n];
            if (n == 0 || work[i].key != last) groups.emplace_back();
            last = work[i].key;
            Group& g = groups.back();
            g.total += work[i].w;
            g.longest = std::max(g.longest, work[i].w);
            g.idx.push_back(i);
        }
    }
    // balance first (largest groups placed first, each on the least-loaded queue), then run every queue longest items first
    std::stable_sort(groups.begin(), groups.end(), [](const Group& a, const Group& b) { return a.total > b.total; });
    constexpr int kXcds = 8;
    std::vector<size_t> qgroups[kXcds];
    double load[kXcds] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        int best = 0;
        for (int x = 1; x < kXcds; ++x)
            if (load[x] < load[best]) best = x;
        load[best] += groups[gi].total;
        qgroups[best].push_back(gi);
    }
    std::vector<size_t> queue[kXcds];
    for (int x = 0; x < kXcds; ++x) {
        std::stable_sort(qgroups[x].begin(), qgroups[x].end(),
                         [&](size_t a, size_t b) { return groups[a].longest > groups[b].longest; });
        for (size_t gi : qgroups[x])
            for (size_t i : groups[gi].idx) queue[x].push_back(i);
    }
    size_t rows = 0;
    for (int x = 0; x < kXcds; ++x) rows = std::max(rows, queue[x].size());
    out.assign(rows * kXcds, noop);
    for (int x = 0; x < kXcds; ++x)
        for (size_t j = 0; j < queue[x].size(); ++j) out[j * kXcds + x] = work[queue[x][j]].it;
    return out;
}

}  // namespace pleas
