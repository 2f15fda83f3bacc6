// qm_picks.hpp -- phase picks on the device: what the reference's GaussianPicker does to every onset row of a
// located event (quakemigrate/signal/pickers/gaussian.py:319-560): a noise threshold from the median and MAD of the
// row outside the station's pick windows, the run of samples above it that holds the window's maximum, and a 1-D
// Gaussian fitted to that run.
//
// One workgroup of four wavefronts per onset row, one launch for all rows of a call.  LDS holds the row (f64), one
// 64-bit key per sample, the reductions' slots and the median's histogram -- 16 T + 768 + 1040 bytes (picks_lds_bytes),
// all of it dynamic: T <= kPicksLdsSamples.  The workgroup's sums, maxima and the median: qm_block.hpp.
//   noise set  key[t] = order_key(row[t]) where t lies in no window of the row's group and row[t] > 1, all ones (no
//              finite value's key) elsewhere.
//   medians    block_median over the keys, then over order_key(|row[t] - med|) formed on the fly where key[t] is a
//              value's: eight radix passes each, exact, ties and all.  (a + b) / 2, |x - med|, 1.4826 mad,
//              med + mad * multiplier follow in NumPy's order without contraction -- the threshold has NumPy's bits.
//   peak       three reductions over [lo, hi): the maximum, its first index, the nearest samples not above the
//              threshold on either side of it.
//   fit        Levenberg-Marquardt on the 3x3 normal equations, analytic Jacobian, More's scaling (D = running
//              maximum of the column norms), gain-ratio test, Nielsen's update of the damping.  Every thread carries
//              the same parameters; the ten sums behind J'J, J'r, r'r (and the trial point's r'r) are strided over the
//              workgroup's 256 threads and added in a fixed order (lane butterfly, then wavefront 0..3): the same bits
//              in every thread and every run.
#pragma once
#include "qm_block.hpp"

namespace qm {

constexpr int kPicksLdsSamples = 10112;         // 16 bytes per sample + slots + histogram <= 160 KB: 240 bytes to spare
constexpr int kPicksThreads = 256;
constexpr int kPicksSlots = 12;                 // values per reduction, at most
constexpr int kPicksMaxIter = 200;
constexpr int kPicksColumns = 8;

enum PickStatus : int {
    kPicked = 0, kPickNothingAbove = 1, kPickOneSample = 2, kPickLeavesTrace = 3, kPickNotConverged = 4,
    kPickMeanOutside = 5, kPickNonFinite = 6,
};

struct PickArgs {
    const double *onsets;           // [n_rows][T]
    const int32_t *windows;         // [n_rows][3]: lo, arrival, hi
    const int32_t *row_group;       // [n_rows]
    const double *halfwidth;        // [n_rows], samples
    const double *thresholds_in;    // [n_rows] (mode 1)
    double *picks;                  // [n_rows][8]
    int32_t *status;                // [n_rows]
    int n_rows, T, mode;
    double rate, mad_multiplier;
};

using PickReduce = BlockReduce<kPicksSlots, kPicksThreads / 64>;
constexpr unsigned long long kPickNoKey = ~0ull;

// all of the workgroup's LDS (the kernel declares none of its own): row, keys, slots, histogram
constexpr size_t picks_lds_bytes(int T) {
    return (size_t)T * 16 + (size_t)PickReduce::kWords * 8 + sizeof(MedianLds);
}
static_assert(picks_lds_bytes(kPicksLdsSamples) <= 160 * 1024, "the longest row must fit a workgroup's 160 KB of LDS");

__device__ __forceinline__ bool pick_solve3(const double (&s)[6], const double (&rhs)[3], double (&q)[3]) {
    // Cholesky of the symmetric s = [s00 s10 s11 s20 s21 s22]
    if (!(s[0] > 0.0)) return false;
    const double l00 = sqrt(s[0]);
    const double l10 = s[1] / l00, l20 = s[3] / l00;
    const double d11 = s[2] - l10 * l10;
    if (!(d11 > 0.0)) return false;
    const double l11 = sqrt(d11);
    const double l21 = (s[4] - l20 * l10) / l11;
    const double d22 = s[5] - l20 * l20 - l21 * l21;
    if (!(d22 > 0.0)) return false;
    const double l22 = sqrt(d22);
    const double z0 = rhs[0] / l00;
    const double z1 = (rhs[1] - l10 * z0) / l11;
    const double z2 = (rhs[2] - l20 * z0 - l21 * z1) / l22;
    q[2] = z2 / l22;
    q[1] = (z1 - l21 * q[2]) / l11;
    q[0] = (z0 - l10 * q[1] - l20 * q[2]) / l00;
    return isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]);
}

// sum over the fit range of (a exp(-(x - b)^2 / (2 c^2)) - y)^2
__device__ __forceinline__ double pick_cost(const double *row, int f0, int f1, double rate, const double (&p)[3],
                                            PickReduce &red) {
    double f[1] = {0.0};
    for (int k = f0 + (int)threadIdx.x; k < f1; k += kPicksThreads) {
        const double d = (double)k / rate - p[1];
        const double r = p[0] * exp(-(d * d) / (2.0 * (p[2] * p[2]))) - row[k];
        f[0] += r * r;
    }
    red.run(f, BlockAdd());
    return f[0];
}

#ifdef QM_TU_PICKS
__global__ __launch_bounds__(kPicksThreads) void pick_phases_kernel(PickArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pick_lds[];
    const int T = a.T, row_id = blockIdx.x, tid = threadIdx.x;
    double *row = reinterpret_cast<double *>(pick_lds);
    unsigned long long *key = reinterpret_cast<unsigned long long *>(pick_lds) + T;
    PickReduce red{key + T, kPicksThreads / 64, 0};
    MedianLds &hist = *reinterpret_cast<MedianLds *>(red.slots + PickReduce::kWords);

    const double *x = a.onsets + (int64_t)row_id * T;
    const int lo = a.windows[3 * row_id], hi = a.windows[3 * row_id + 2];
    double out[kPicksColumns] = {0.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0, 0.0};
    int status = kPicked;

    long long bad[1] = {0};
    for (int t = tid; t < T; t += kPicksThreads) {
        const double v = x[t];
        row[t] = v;
        bad[0] += isfinite(v) ? 0 : 1;
    }
    red.run(bad, BlockAdd());                            // (its barrier: the row is in LDS)
    double thr = __builtin_nan("");
    if (bad[0] > 0) {
        status = kPickNonFinite;
    } else if (a.mode == 1) {
        thr = a.thresholds_in[row_id];
    } else {
#pragma clang fp contract(off)
        for (int t = tid; t < T; t += kPicksThreads) {
            const double v = row[t];
            key[t] = v > 1.0 ? order_key(v) : kPickNoKey;
        }
        __syncthreads();
        const int group = a.row_group[row_id];
        for (int r = 0; r < a.n_rows; ++r) {            // (uniform: every window of the station masks the row)
            if (a.row_group[r] != group) continue;
            const int w1 = a.windows[3 * r + 2];
            for (int t = a.windows[3 * r] + tid; t < w1; t += kPicksThreads) key[t] = kPickNoKey;
        }
        __syncthreads();
        long long n[1] = {0};
        for (int t = tid; t < T; t += kPicksThreads) n[0] += key[t] != kPickNoKey ? 1 : 0;
        red.run(n, BlockAdd());
        if (n[0] > 0) {
            const double med = block_median(T, (unsigned)n[0], [&](int t, unsigned long long &q) {
                q = key[t];
                return q != kPickNoKey;
            }, hist, red);
            const double mad = 1.4826 * block_median(T, (unsigned)n[0], [&](int t, unsigned long long &q) {
                q = order_key(fabs(row[t] - med));
                return key[t] != kPickNoKey;
            }, hist, red);
            thr = med + mad * a.mad_multiplier;
        }
    }
    out[0] = thr;

    // the peak: first maximum of [lo, hi), the run above the threshold around it
    int f0 = 0, f1 = 0;
    if (status == kPicked) {
        double top[1] = {-__builtin_inf()};
        for (int t = lo + tid; t < hi; t += kPicksThreads) top[0] = row[t] > top[0] ? row[t] : top[0];
        red.run(top, BlockMax());
        if (!(top[0] > thr)) {                          // (an empty window, a NaN threshold: nothing above it)
            status = kPickNothingAbove;
        } else {
            long long first[1] = {hi};
            for (int t = lo + tid; t < hi; t += kPicksThreads)
                if (row[t] == top[0] && t < first[0]) first[0] = t;
            red.run(first, BlockMin());
            const int imax = (int)first[0];
            long long left[1] = {lo - 1}, right[1] = {hi};      // nearest samples not above the threshold
            for (int t = lo + tid; t < hi; t += kPicksThreads) {
                if (row[t] > thr) continue;
                if (t < imax && t > left[0]) left[0] = t;
                if (t > imax && t < right[0]) right[0] = t;
            }
            red.run(left, BlockMax());
            red.run(right, BlockMin());
            const int run0 = (int)left[0] + 1, run1 = (int)right[0];
            if (run1 - run0 < 2) {
                status = kPickOneSample;
            } else {
                f0 = run0 - 1;
                f1 = run1 + 1;
                out[5] = (double)f0;
                out[6] = (double)f1;
                if (f0 < 0 || f1 > T) status = kPickLeavesTrace;
            }
        }
    }

    if (status == kPicked) {
        // p0 = [max y, time of its first sample, halfwidth]: the run holds the window's first maximum, and the two
        // samples of padding do not exceed the threshold (or lie outside the window: then they may)
        double top[1] = {-__builtin_inf()};
        for (int k = f0 + tid; k < f1; k += kPicksThreads) top[0] = row[k] > top[0] ? row[k] : top[0];
        red.run(top, BlockMax());
        long long first[1] = {f1};
        for (int k = f0 + tid; k < f1; k += kPicksThreads)
            if (row[k] == top[0] && k < first[0]) first[0] = k;
        red.run(first, BlockMin());
        const double rate = a.rate;
        double p[3] = {top[0], (double)first[0] / rate, a.halfwidth[row_id] / rate};
        double dmax[3] = {0.0, 0.0, 0.0};
        double mu = 1e-3, nu = 2.0;
        double f = pick_cost(row, f0, f1, rate, p, red);
        int it = 0;
        bool converged = false;
        while (it < kPicksMaxIter && !converged) {
            ++it;
            // J'J (6), J'r (3) at p
            double s[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            const double c2 = p[2] * p[2], c3 = c2 * p[2];
            for (int k = f0 + tid; k < f1; k += kPicksThreads) {
                const double d = (double)k / rate - p[1];
                const double e = exp(-(d * d) / (2.0 * c2));
                const double ja = e, jb = p[0] * e * d / c2, jc = p[0] * e * d * d / c3;
                const double r = p[0] * e - row[k];
                s[0] += ja * ja; s[1] += jb * ja; s[2] += jb * jb;
                s[3] += jc * ja; s[4] += jc * jb; s[5] += jc * jc;
                s[6] += ja * r; s[7] += jb * r; s[8] += jc * r;
            }
            red.run(s, BlockAdd());
            const double n0 = sqrt(s[0]), n1 = sqrt(s[2]), n2 = sqrt(s[5]);
            dmax[0] = n0 > dmax[0] ? n0 : dmax[0];
            dmax[1] = n1 > dmax[1] ? n1 : dmax[1];
            dmax[2] = n2 > dmax[2] ? n2 : dmax[2];
            const double m[6] = {s[0] / (dmax[0] * dmax[0]) + mu, s[1] / (dmax[1] * dmax[0]),
                                 s[2] / (dmax[1] * dmax[1]) + mu, s[3] / (dmax[2] * dmax[0]),
                                 s[4] / (dmax[2] * dmax[1]), s[5] / (dmax[2] * dmax[2]) + mu};
            const double rhs[3] = {-s[6] / dmax[0], -s[7] / dmax[1], -s[8] / dmax[2]};
            bool finite = true;
            for (int k = 0; k < 6; ++k) finite = finite && isfinite(m[k]);
            for (int k = 0; k < 3; ++k) finite = finite && isfinite(rhs[k]);
            double q[3] = {0.0, 0.0, 0.0};
            const bool solved = finite && pick_solve3(m, rhs, q);   // (uniform: every thread holds the same sums)
            double rho = -1.0, f_new = f;
            double dp[3] = {0.0, 0.0, 0.0}, p_new[3] = {p[0], p[1], p[2]};
            if (solved) {
                for (int k = 0; k < 3; ++k) {
                    dp[k] = q[k] / dmax[k];
                    p_new[k] = p[k] + dp[k];
                }
                f_new = pick_cost(row, f0, f1, rate, p_new, red);
                const double pred = q[0] * (mu * q[0] + rhs[0]) + q[1] * (mu * q[1] + rhs[1]) +
                                    q[2] * (mu * q[2] + rhs[2]);
                if (isfinite(f_new) && pred > 0.0) rho = (f - f_new) / pred;
            }
            bool small = solved;
            for (int k = 0; k < 3; ++k) small = small && fabs(dp[k]) <= 1e-13 * (fabs(p[k]) + 1e-13);
            if (rho > 1e-4) {
                for (int k = 0; k < 3; ++k) p[k] = p_new[k];
                f = f_new;
                const double t = 2.0 * rho - 1.0;
                const double shrink = 1.0 - t * t * t;
                mu *= shrink > 1.0 / 3.0 ? shrink : 1.0 / 3.0;
                nu = 2.0;
            } else {
                mu *= nu;
                nu *= 2.0;
            }
            converged = small;
        }
        out[7] = (double)it;
        if (!converged) {
            status = kPickNotConverged;
        } else {
            const double at = p[1] * rate;
            if (!((double)lo < at && at < (double)hi)) {
                status = kPickMeanOutside;
            } else {
                out[1] = p[0];
                out[2] = p[1];
                out[3] = fabs(p[2]);
                out[4] = p[2];
            }
        }
    }
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < kPicksColumns; ++k) a.picks[(int64_t)row_id * kPicksColumns + k] = out[k];
        a.status[row_id] = status;
    }
}
#endif  // QM_TU_PICKS

}  // namespace qm
