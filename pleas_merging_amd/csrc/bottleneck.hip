// Batched lexicographic bottleneck assignment on gfx950 (include/pleas_hip.h, pleas_bottleneck_*).
//
// Replaces pleas/core/solvers.py:88-115 (scipy_solve_minimax_assignment: D2H copy, sort of all n^2 values, ~log2(n^2)
// CSR rebuilds, each followed by scipy's Hopcroft-Karp).  Three launches per batch, all on the caller's stream:
//   1. bottleneck_t_kernel, one workgroup per problem (largest first): the bottleneck value t* = max over permutations p
//      of min_i A[i, p(i)], by bisection on order-preserving uint32 keys of the fp32 entries.  Each probe t asks for a
//      perfect matching of the dense bipartite graph {A_ij >= t}; adjacency is evaluated on the fly from coalesced row
//      reads.  The matching is warm-started from the previous probe (filtered to the edges still present) and augmented
//      by level-synchronous multi-source BFS phases (Hopcroft-Karp style: a phase stops at the first level that reaches
//      a free column and augments a set of vertex-disjoint shortest paths, one per BFS root).  All matching state is in
//      LDS: 6 n ints + 2 n bits (96 KiB + 1 KiB at n = 4096).
//   2. bottleneck_mask_kernel: A_hat = A with every entry below t* replaced by L32 (bn_floor_bound), in the workspace.
//   3. pleas_lsap_batched (lsap.hip, unchanged) on the A_hat copies, maximize = 1: the largest sum among the
//      bottleneck-optimal permutations, scipy's tie rule for what is left.
//   4. bottleneck_final_kernel: t_out, and col_ind = -1 for a problem whose status word is not 0.
// Every loop has a hard cap; hitting one writes a status word (workspace head) instead of hanging.
// maximize = 0 is the same call on -A (negation is exact).
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "common.hpp"

namespace pleas {

constexpr int kBnThreads = 1024;
constexpr int kBnWaves = kBnThreads / 64;
constexpr int kBnBatch = 64;
constexpr int kBnMaskThreads = 256;

enum BnStatus { kBnOk = 0, kBnNonFinite = 1, kBnCap = 2, kBnBound = 3 };

struct BnBatch {
    const float* cost[kBnBatch];
    float* masked[kBnBatch];
    int64_t* out[kBnBatch];
    int n[kBnBatch];
    int id[kBnBatch];      // index of the problem in the caller's arrays (status, stats, t_out)
    float sign;            // +1: maximize, -1: the same call on -A
    int* status;           // [nprob]
    uint32_t* stats;       // [nprob][3]: key of t*, of the largest entry, of the smallest entry (of sign * A)
    float* t_out;          // [nprob] or null
};

// Order-preserving keys: a < b  <=>  key(a) < key(b) for finite values, with -0 folded onto +0 (the reference's B >= t
// compares fp32 values, where -0 == +0).
__host__ __device__ inline uint32_t bn_key(float f) {
    const uint32_t b = f == 0.0f ? 0u : __builtin_bit_cast(uint32_t, f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__host__ __device__ inline float bn_unkey(uint32_t k) {
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
inline uint64_t bn_key(double f) {
    const uint64_t b = f == 0.0 ? 0u : __builtin_bit_cast(uint64_t, f);
    return (b >> 63) ? ~b : (b | (uint64_t(1) << 63));
}
inline double bn_unkey(uint64_t k) {
    return __builtin_bit_cast(double, (k >> 63) ? (k & ~(uint64_t(1) << 63)) : ~k);
}

// The value that replaces every entry below t*: L = t* - (n (M - m) + max(1, |t*|)) in fp64, rounded toward -inf to fp32.
// Any permutation that uses a replaced entry then sums below any permutation that stays at or above t*.  Written without
// FMA contraction so that host and device round identically.
__host__ __device__ inline float bn_floor_bound(double t, double M, double m, int n) {
#pragma clang fp contract(off)
    const double span = (double)n * (M - m);
    const double L = t - (span + fmax(1.0, fabs(t)));
    float f = (float)L;
    if ((double)f > L) f = nextafterf(f, -INFINITY);
    return f;
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t x) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x = max(x, (uint32_t)__shfl_xor((int)x, s));
    return x;
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t x) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x = min(x, (uint32_t)__shfl_xor((int)x, s));
    return x;
}

struct BnShared {
    int* rowmate;   // column matched to a row, -1: free
    int* colmate;   // row matched to a column, -1: free
    int* parent;    // BFS: row that reached a column in the current phase
    int* front[2];  // BFS frontier rows, current / next level
    int* found;     // free columns reached by the last level; -1 once their path lost its root to another path
    uint32_t* vis;  // column visited in the current phase (bits)
    uint32_t* claim;  // BFS root taken by an augmenting path (bits)
    int* cnt;       // [0]: free columns found, [1..3]: next-frontier counters rotating over levels, [4]: error
};

// Perfect matching of {sign * A_ij >= tf}?  1: yes, 0: no, -1: an iteration cap was hit.  Uniform over the workgroup.
__device__ int bn_match(const BnShared sh, const float* __restrict__ A, const int n, const float sg, const float tf) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int words = (n + 31) >> 5;
    for (int r = tid; r < n; r += kBnThreads) {   // warm start: keep the edges of the previous matching still present
        const int j = sh.rowmate[r];
        if (j >= 0 && !(sg * A[(size_t)r * n + j] >= tf)) {
            sh.rowmate[r] = -1;
            sh.colmate[j] = -1;
        }
    }
    for (int phase = 0;; ++phase) {     // each phase augments at least one path, or returns
        __syncthreads();
        if (phase > n) return -1;
        for (int w = tid; w < words; w += kBnThreads) sh.vis[w] = 0u, sh.claim[w] = 0u;
        if (tid < 4) sh.cnt[tid] = 0;
        __syncthreads();
        for (int r = tid; r < n; r += kBnThreads)
            if (sh.rowmate[r] < 0) sh.front[0][atomicAdd(&sh.cnt[1], 1)] = r;
        __syncthreads();
        int fsize = sh.cnt[1];
        if (fsize == 0) return 1;
        int cur = 0;
        for (int level = 0;; ++level) {
            if (level > n) return -1;
            __syncthreads();
            const int* fr = cur ? sh.front[1] : sh.front[0];      // selects: no dynamic index into a private array
            int* nx = cur ? sh.front[0] : sh.front[1];
            int* ncnt = &sh.cnt[1 + (level + 1) % 3];         // written by this level
            if (tid == 0) sh.cnt[1 + (level + 2) % 3] = 0;     // next level's counter: last read two barriers ago
            for (int idx = wave; idx < fsize; idx += kBnWaves) {
                const int r = fr[idx];
                const float* __restrict__ row = A + (size_t)r * n;
                constexpr int U = 4;
                for (int j0 = 0; j0 < n; j0 += 64 * U) {
                    float v[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int j = j0 + u * 64 + lane;
                        v[u] = j < n ? row[j] : 0.f;
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int j = j0 + u * 64 + lane;
                        const uint32_t bit = 1u << (j & 31);
                        if (j < n && sg * v[u] >= tf && !(sh.vis[j >> 5] & bit)) {
                            if (!(atomicOr(&sh.vis[j >> 5], bit) & bit)) {
                                sh.parent[j] = r;
                                const int c = sh.colmate[j];
                                if (c < 0) sh.found[atomicAdd(&sh.cnt[0], 1)] = j;
                                else nx[atomicAdd(ncnt, 1)] = c;
                            }
                        }
                    }
                }
            }
            __syncthreads();
            if (sh.cnt[0] > 0) break;
            fsize = *ncnt;
            if (fsize == 0) return 0;     // no augmenting path: the matching is maximum and not perfect
            cur ^= 1;
        }
        // augment: trace every found column back to its BFS root (reads only); one path per root wins
        const int nfound = sh.cnt[0];
        for (int i = tid; i < nfound; i += kBnThreads) {
            int j = sh.found[i], root = -1;
            for (int s = 0; s <= n; ++s) {
                const int r = sh.parent[j];
                const int nj = sh.rowmate[r];
                if (nj < 0) {
                    root = r;
                    break;
                }
                j = nj;
            }
            if (root < 0) {
                sh.cnt[4] = 1;
                sh.found[i] = -1;
            } else {
                const uint32_t bit = 1u << (root & 31);
                if (atomicOr(&sh.claim[root >> 5], bit) & bit) sh.found[i] = -1;
            }
        }
        __syncthreads();
        if (sh.cnt[4]) return -1;
        for (int i = tid; i < nfound; i += kBnThreads) {   // the winners' paths are vertex-disjoint
            int j = sh.found[i];
            if (j < 0) continue;
            for (int s = 0; s <= n; ++s) {
                const int r = sh.parent[j];
                const int nj = sh.rowmate[r];
                sh.rowmate[r] = j;
                sh.colmate[j] = r;
                if (nj < 0) break;
                j = nj;
            }
        }
    }
}

__global__ __launch_bounds__(kBnThreads) void bottleneck_t_kernel(const BnBatch b) {
    extern __shared__ __attribute__((aligned(16))) int bn_smem[];
    __shared__ uint32_t s_lo, s_hi, s_max, s_bad;
    __shared__ int s_cnt[5];
    const int q = blockIdx.x, n = b.n[q], id = b.id[q];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* __restrict__ A = b.cost[q];
    const float sg = b.sign;
    BnShared sh;
    sh.rowmate = bn_smem;
    sh.colmate = sh.rowmate + n;
    sh.parent = sh.colmate + n;
    sh.front[0] = sh.parent + n;
    sh.front[1] = sh.front[0] + n;
    sh.found = sh.front[1] + n;
    sh.vis = reinterpret_cast<uint32_t*>(sh.found + n);
    sh.claim = sh.vis + ((n + 31) >> 5);
    sh.cnt = s_cnt;
    if (tid == 0) s_lo = 0xffffffffu, s_hi = 0xffffffffu, s_max = 0u, s_bad = 0u, s_cnt[4] = 0;
    for (int r = tid; r < n; r += kBnThreads) sh.rowmate[r] = -1, sh.colmate[r] = -1;
    __syncthreads();
    // bounds: lo = smallest entry (always feasible), hi = min(min over rows of the row max, min over columns of the column max)
    uint32_t lmin = 0xffffffffu, lmax = 0u;
    bool bad = false;
    for (int r = wave; r < n; r += kBnWaves) {
        uint32_t rmax = 0u;
        for (int j = lane; j < n; j += 64) {
            const float v = sg * A[(size_t)r * n + j];
            bad |= !isfinite(v);
            const uint32_t k = bn_key(v);
            rmax = max(rmax, k);
            lmin = min(lmin, k);
        }
        rmax = wave_max_u32(rmax);
        lmax = max(lmax, rmax);
        if (lane == 0) atomicMin(&s_hi, rmax);
    }
    for (int j = tid; j < n; j += kBnThreads) {
        uint32_t cmax = 0u;
        for (int r = 0; r < n; ++r) cmax = max(cmax, bn_key(sg * A[(size_t)r * n + j]));
        atomicMin(&s_hi, cmax);
    }
    lmin = wave_min_u32(lmin);
    lmax = wave_max_u32(lmax);
    if (lane == 0) {
        atomicMin(&s_lo, lmin);
        atomicMax(&s_max, lmax);
    }
    if (bad) atomicOr(&s_bad, 1u);
    __syncthreads();
    int status = s_bad ? kBnNonFinite : kBnOk;
    uint32_t lo = s_lo, hi = s_hi;
    if (status == kBnOk) {
        // largest key whose graph has a perfect matching; at most 32 probes (the key range halves every probe)
        for (int step = 0; lo < hi; ++step) {
            if (step >= 33) {
                status = kBnCap;
                break;
            }
            const uint32_t mid = lo + (hi - lo) / 2 + ((hi - lo) & 1u);
            const int ok = bn_match(sh, A, n, sg, bn_unkey(mid));
            if (ok < 0) {
                status = kBnCap;
                break;
            }
            if (ok) lo = mid;
            else hi = mid - 1;
        }
    }
    if (tid == 0) {
        b.status[id] = status;
        b.stats[3 * id + 0] = lo;
        b.stats[3 * id + 1] = s_max;
        b.stats[3 * id + 2] = s_lo;
    }
}

__global__ __launch_bounds__(kBnMaskThreads) void bottleneck_mask_kernel(const BnBatch b) {
    const int q = blockIdx.y, n = b.n[q], id = b.id[q];
    const int status = b.status[id];
    const float t = bn_unkey(b.stats[3 * id + 0]);
    const float L32 = bn_floor_bound(t, bn_unkey(b.stats[3 * id + 1]), bn_unkey(b.stats[3 * id + 2]), n);
    const bool ok = status == kBnOk && isfinite(L32);
    if (status == kBnOk && !ok && blockIdx.x == 0 && threadIdx.x == 0) b.status[id] = kBnBound;
    const float* __restrict__ A = b.cost[q];
    float* __restrict__ out = b.masked[q];
    const float sg = b.sign;
    const size_t total = (size_t)n * n;
    // a problem that failed gets a finite all-zero matrix: the LAP that follows runs on defined data
    for (size_t i = (size_t)blockIdx.x * kBnMaskThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kBnMaskThreads) {
        const float v = sg * A[i];
        out[i] = ok ? (v >= t ? v : L32) : 0.f;
    }
}

__global__ __launch_bounds__(256) void bottleneck_final_kernel(const BnBatch b) {
    const int q = blockIdx.x, n = b.n[q], id = b.id[q];
    const int status = b.status[id];
    if (status != kBnOk) {
        for (int i = threadIdx.x; i < n; i += 256) b.out[q][i] = -1;
        if (b.t_out && threadIdx.x == 0) b.t_out[id] = NAN;
    } else if (b.t_out && threadIdx.x == 0) {
        const float t = b.sign * bn_unkey(b.stats[3 * id]);
        b.t_out[id] = t == 0.f ? 0.f : t;
    }
}

// ---- workspace: int32 status[nprob] | uint32 stats[nprob][3] | A_hat of every problem (256-byte aligned each)
inline size_t bn_align(size_t x) { return (x + 255) & ~size_t(255); }

static bool bn_sizes_ok(const int* n, int nprob) {
    if (nprob < 0 || (nprob > 0 && !n)) return false;
    for (int p = 0; p < nprob; ++p)
        if (n[p] < 1 || n[p] > PLEAS_LSAP_MAX_N) return false;
    return true;
}

static size_t bn_ws_layout(const int* n, int nprob, std::vector<size_t>* mat_off) {
    size_t off = bn_align(sizeof(int) * (size_t)nprob) + bn_align(3 * sizeof(uint32_t) * (size_t)nprob);
    for (int p = 0; p < nprob; ++p) {
        if (mat_off) mat_off->push_back(off);
        off += bn_align(sizeof(float) * (size_t)n[p] * n[p]);
    }
    return off;
}

// ---- host: the same contract on a host matrix (fp32 or fp64), one problem, synchronous
template <class T>
struct BnHost {
    const T* A;
    int n;
    T sg;
    std::vector<int> rowmate, colmate, parent, front, next, found;
    std::vector<char> vis, claim;

    bool edge(int r, int j, T t) const { return sg * A[(size_t)r * n + j] >= t; }

    // the device algorithm, sequentially: 1 perfect, 0 not, -1 cap
    int match(T t) {
        for (int r = 0; r < n; ++r)
            if (rowmate[r] >= 0 && !edge(r, rowmate[r], t)) colmate[rowmate[r]] = -1, rowmate[r] = -1;
        for (int phase = 0; phase <= n; ++phase) {
            std::fill(vis.begin(), vis.end(), 0);
            std::fill(claim.begin(), claim.end(), 0);
            front.clear();
            found.clear();
            for (int r = 0; r < n; ++r)
                if (rowmate[r] < 0) front.push_back(r);
            if (front.empty()) return 1;
            for (int level = 0; found.empty(); ++level) {
                if (level > n) return -1;
                next.clear();
                for (int r : front)
                    for (int j = 0; j < n; ++j)
                        if (!vis[j] && edge(r, j, t)) {
                            vis[j] = 1;
                            parent[j] = r;
                            if (colmate[j] < 0) found.push_back(j);
                            else next.push_back(colmate[j]);
                        }
                if (found.empty() && next.empty()) return 0;
                front.swap(next);
            }
            for (int& f : found) {
                int j = f, root = -1;
                for (int s = 0; s <= n && root < 0; ++s) {
                    const int r = parent[j];
                    if (rowmate[r] < 0) root = r;
                    else j = rowmate[r];
                }
                if (root < 0) return -1;
                if (claim[root]) f = -1;
                claim[root] = 1;
            }
            for (int f : found) {
                for (int j = f, s = 0; j >= 0 && s <= n; ++s) {
                    const int r = parent[j];
                    const int nj = rowmate[r];
                    rowmate[r] = j;
                    colmate[j] = r;
                    j = nj;
                }
            }
        }
        return -1;
    }
};

template <class T>
static int bn_host_solve(const T* A, int n, int maximize, int64_t* col_ind, double* t_out) {
    const T sg = maximize ? T(1) : T(-1);
    using K = decltype(bn_key(T(0)));
    K kmin = std::numeric_limits<K>::max(), hi = kmin, kmax = 0;
    std::vector<K> colmax(n, 0);
    for (int r = 0; r < n; ++r) {
        K rmax = 0;
        for (int j = 0; j < n; ++j) {
            const T v = sg * A[(size_t)r * n + j];
            if (!std::isfinite(v)) return bad_arg("non-finite cost entry");
            const K k = bn_key(v);
            rmax = std::max(rmax, k);
            colmax[j] = std::max(colmax[j], k);
            kmin = std::min(kmin, k);
        }
        hi = std::min(hi, rmax);
        kmax = std::max(kmax, rmax);
    }
    for (int j = 0; j < n; ++j) hi = std::min(hi, colmax[j]);
    BnHost<T> m{A, n, sg};
    m.rowmate.assign(n, -1);
    m.colmate.assign(n, -1);
    m.parent.assign(n, -1);
    m.vis.assign(n, 0);
    m.claim.assign(n, 0);
    K lo = kmin;
    for (int step = 0; lo < hi; ++step) {
        if (step > (int)(8 * sizeof(K))) return bad_arg("bisection iteration cap");
        const K mid = lo + (hi - lo) / 2 + ((hi - lo) & 1u);
        const int ok = m.match(bn_unkey(mid));
        if (ok < 0) return bad_arg("matching iteration cap");
        if (ok) lo = mid;
        else hi = mid - 1;
    }
    const T t = bn_unkey(lo);
    const float L32 = bn_floor_bound((double)t, (double)bn_unkey(kmax), (double)bn_unkey(kmin), n);
    if (!std::isfinite(L32)) return bad_arg("the replacement value L32 is not finite (entries too large)");
    std::vector<T> hat((size_t)n * n);
    for (size_t i = 0; i < hat.size(); ++i) {
        const T v = sg * A[i];
        hat[i] = v >= t ? v : (T)L32;
    }
    if (t_out) {
        const double tv = (double)(sg * t);
        *t_out = tv == 0.0 ? 0.0 : tv;
    }
    return pleas_lsap_host(hat.data(), sizeof(T) == sizeof(double), n, 1, col_ind);
}

}  // namespace pleas

using namespace pleas;

extern "C" size_t pleas_bottleneck_ws_bytes(const int* n, int nprob) {
    if (!bn_sizes_ok(n, nprob)) return 0;
    return bn_ws_layout(n, nprob, nullptr);
}

extern "C" int pleas_bottleneck_host(const void* cost, int is_double, int n, int maximize, int64_t* col_ind,
                                     double* t_out) {
    if (!cost || !col_ind) return bad_arg("null pointer");
    if (n < 1 || n > PLEAS_LSAP_MAX_N) return bad_arg("n out of range [1, PLEAS_LSAP_MAX_N]");
    return is_double ? bn_host_solve((const double*)cost, n, maximize, col_ind, t_out)
                     : bn_host_solve((const float*)cost, n, maximize, col_ind, t_out);
}

extern "C" int pleas_bottleneck_batched(const float* const* cost, const int* n, int nprob, int maximize,
                                        int64_t* const* col_ind, float* t_out, void* ws, size_t ws_bytes, void* stream_) {
    if (nprob < 0) return bad_arg("nprob");
    if (nprob == 0) return PLEAS_OK;
    if (!cost || !n || !col_ind) return bad_arg("null array");
    if (!bn_sizes_ok(n, nprob)) return bad_arg("n out of range [1, PLEAS_LSAP_MAX_N]");
    for (int p = 0; p < nprob; ++p)
        if (!cost[p] || !col_ind[p]) return bad_arg("null problem pointer");
    std::vector<size_t> mat_off;
    const size_t need = bn_ws_layout(n, nprob, &mat_off);
    if (!ws) return bad_arg("null workspace");
    if (ws_bytes < need) return bad_arg("workspace smaller than pleas_bottleneck_ws_bytes");
    hipStream_t stream = (hipStream_t)stream_;
    unsigned char* base = static_cast<unsigned char*>(ws);
    int* status = reinterpret_cast<int*>(base);
    uint32_t* stats = reinterpret_cast<uint32_t*>(base + bn_align(sizeof(int) * (size_t)nprob));
    std::vector<const float*> masked(nprob);
    for (int p = 0; p < nprob; ++p) masked[p] = reinterpret_cast<const float*>(base + mat_off[p]);
    PLEAS_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int) * (size_t)nprob, stream));
    // largest problems first: they are the tail of the launch
    std::vector<int> order(nprob);
    for (int p = 0; p < nprob; ++p) order[p] = p;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return n[a] > n[b]; });
    std::vector<BnBatch> batches;
    std::vector<int> nmaxes;
    for (int start = 0; start < nprob; start += kBnBatch) {
        BnBatch b;
        b.sign = maximize ? 1.f : -1.f;
        b.status = status;
        b.stats = stats;
        b.t_out = t_out;
        const int cnt = std::min(kBnBatch, nprob - start);
        int nmax = 0;
        for (int q = 0; q < kBnBatch; ++q) {
            const int p = q < cnt ? order[start + q] : order[start];
            b.cost[q] = cost[p];
            b.masked[q] = const_cast<float*>(masked[p]);
            b.out[q] = col_ind[p];
            b.n[q] = n[p];
            b.id[q] = p;
            nmax = std::max(nmax, n[p]);
        }
        batches.push_back(b);
        nmaxes.push_back(nmax);
    }
    for (size_t c = 0; c < batches.size(); ++c) {
        const int cnt = std::min(kBnBatch, nprob - (int)c * kBnBatch);
        const int nmax = nmaxes[c];
        const size_t lds = sizeof(int) * 6 * (size_t)nmax + sizeof(uint32_t) * 2 * (size_t)((nmax + 31) / 32);
        hipLaunchKernelGGL(bottleneck_t_kernel, dim3(cnt), dim3(kBnThreads), lds, stream, batches[c]);
        PLEAS_LAUNCH_CHECK("bottleneck_t_kernel");
        const size_t tiles = ((size_t)nmax * nmax + 4 * kBnMaskThreads - 1) / (4 * kBnMaskThreads);
        const int gx = (int)std::min<size_t>(std::max<size_t>(tiles, 1), 256);
        hipLaunchKernelGGL(bottleneck_mask_kernel, dim3(gx, cnt), dim3(kBnMaskThreads), 0, stream, batches[c]);
        PLEAS_LAUNCH_CHECK("bottleneck_mask_kernel");
    }
    const int rc = pleas_lsap_batched(masked.data(), n, nprob, 1, col_ind, stream);
    if (rc != PLEAS_OK) return rc;
    for (size_t c = 0; c < batches.size(); ++c) {
        const int cnt = std::min(kBnBatch, nprob - (int)c * kBnBatch);
        hipLaunchKernelGGL(bottleneck_final_kernel, dim3(cnt), dim3(256), 0, stream, batches[c]);
        PLEAS_LAUNCH_CHECK("bottleneck_final_kernel");
    }
    return PLEAS_OK;
}
