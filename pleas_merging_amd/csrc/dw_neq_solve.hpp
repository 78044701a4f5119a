// One channel of the closed-form fit of a depthwise layer: the routine both pleas_dw_normal_eq_solve (a wave per channel) and
// pleas_dw_normal_eq_solve_host (one caller, nlanes = 1) run.
//
//   S   double[D][D], D = K*K + 2, LOWER triangle: rows / columns 0 .. K*K-1 the taps, K*K the bias column (column sums of U and
//       the count M on the diagonal), K*K + 1 the target (h = sum u * t, sum t, sum t^2)
//   T = K*K + has_bias unknowns:  (G_T + ridge * mean(diag G_T) I) x = h_T,  G_T = S[0..T)[0..T),  h_T = S[K*K + 1][0..T)
//
// Column (left-looking) Cholesky in fp64 on a packed lower triangle `a` (T (T + 1) / 2 doubles, row i at i (i + 1) / 2): per column
// j every lane forms the pivot d = a[j][j] - sum_{k<j} L[j][k]^2 (k ascending) for itself, then the lanes deal the rows below,
// L[i][j] = (a[i][j] - sum_{k<j} L[i][k] L[j][k]) / sqrt(d) (k ascending); `sync` separates the columns.  Lane 0 substitutes
// forwards and backwards (k ascending in both).  Every entry has ONE summation order whatever nlanes is.  A pivot that is not
// positive (NaN included) ends the factorisation: the answer is false and x is not to be used.
#pragma once
#include <cmath>

namespace pleas {

#if defined(__HIPCC__)
#define PLEAS_HD __host__ __device__
#else
#define PLEAS_HD
#endif

constexpr int kDwNeqMaxT = 50;                                       // 7 x 7 taps and a bias
constexpr int kDwNeqTri = kDwNeqMaxT * (kDwNeqMaxT + 1) / 2;         // doubles of the packed triangle

PLEAS_HD inline int dw_neq_tri(int i, int j) { return i * (i + 1) / 2 + j; }      // j <= i

// `a`: kDwNeqTri doubles, `x`: kDwNeqMaxT doubles, both shared by the nlanes callers of one channel.  Returns whether x holds the
// solution (the same answer on every lane).
template <class Sync>
PLEAS_HD inline bool dw_neq_solve_channel(const double* S, int K, int has_bias, double ridge, double* a, double* x, int lane, int nlanes,
                                          Sync&& sync) {
    const int KK = K * K, D = KK + 2, T = KK + (has_bias ? 1 : 0);
    double tr = 0.0;
    for (int i = 0; i < T; ++i) tr += S[i * D + i];
    const double shift = ridge * (tr / T);
    for (int i = lane; i < T; i += nlanes) {
        for (int j = 0; j < i; ++j) a[dw_neq_tri(i, j)] = S[i * D + j];
        a[dw_neq_tri(i, i)] = S[i * D + i] + shift;
        x[i] = S[(KK + 1) * D + i];
    }
    sync();
    bool ok = true;
    for (int j = 0; j < T; ++j) {
        double d = a[dw_neq_tri(j, j)];
        for (int k = 0; k < j; ++k) d -= a[dw_neq_tri(j, k)] * a[dw_neq_tri(j, k)];
        if (!(d > 0.0)) ok = false;              // the same value on every lane: no lane leaves the barriers behind
        const double piv = ok ? sqrt(d) : 1.0;
        sync();                                  // every lane has read a[j][j]
        if (lane == 0) a[dw_neq_tri(j, j)] = piv;
        for (int i = j + 1 + lane; i < T; i += nlanes) {
            double s = a[dw_neq_tri(i, j)];
            for (int k = 0; k < j; ++k) s -= a[dw_neq_tri(i, k)] * a[dw_neq_tri(j, k)];
            a[dw_neq_tri(i, j)] = s / piv;
        }
        sync();
    }
    if (lane == 0 && ok) {
        for (int i = 0; i < T; ++i) {            // L y = h
            double s = x[i];
            for (int k = 0; k < i; ++k) s -= a[dw_neq_tri(i, k)] * x[k];
            x[i] = s / a[dw_neq_tri(i, i)];
        }
        for (int i = T - 1; i >= 0; --i) {       // L^T x = y
            double s = x[i];
            for (int k = i + 1; k < T; ++k) s -= a[dw_neq_tri(k, i)] * x[k];
            x[i] = s / a[dw_neq_tri(i, i)];
        }
    }
    sync();
    return ok;
}

}  // namespace pleas
