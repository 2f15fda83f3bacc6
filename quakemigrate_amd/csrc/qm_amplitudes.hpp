// qm_amplitudes.hpp -- local-magnitude amplitudes on the device: what the reference's Amplitude.get_amplitudes does to
// every component trace of a located event (quakemigrate/signal/local_mag/amplitude.py:174-371): an optional causal
// Butterworth filter behind a detrend and a taper (_filter_trace, :413-539), then per time window (noise, P, S) a cut,
// a linear detrend, scipy.signal.find_peaks on the window and on its negative, the peak/trough pairing rules of
// _peak_to_trough_amplitude (:858-901) and an RMS / STD average (:994-997).
//
// Two kernels, two launches per call.
//   stage A  amp_filter_kernel, one workgroup of four wavefronts per trace that has a filter, on qm_condition.hpp's
//            steps: the least-squares line subtracted (line only: the reference calls detrend("linear") alone,
//            amplitude.py:478, :529), the taper's ramps, ONE forward pass from a zero state (zerophase=False) --
//            scipy.signal.sosfilt's bits.  The trace lives in LDS up to kPreprocLdsSamples samples (all 160 KB, so the
//            kernel holds no other LDS), else it is worked on in place in the engine's working copy: the same
//            arithmetic in the same order.
//   stage B  amp_window_kernel, ONE WAVEFRONT per window record: nothing crosses wavefronts, every reduction is a
//            lane-strided sum closed by a fixed butterfly (wave_sum and its kin, qm_block.hpp) and the ordered compaction of
//            the extrema is a ballot and a prefix count per tile of 64 samples -- no atomics, the same bits in every
//            run.  LDS holds the window (f64) and the two extremum lists (int32, at most n / 2 + 1 entries each):
//            12 n + 8 bytes, n <= kAmpLdsSamples; a longer window has the same three arrays in its slice of scratch.
//   extrema  SciPy's _local_maxima_1d: lane i owns the plateau that STARTS at sample i (y[i - 1] < y[i]), walks to its
//            end and records (left + right) / 2 where the sample behind it is lower; a plateau that reaches the
//            window's last sample is no peak.  Plateaus are ordered like their starts, so the compaction by start
//            gives SciPy's order.  Troughs: the same on -y (negation is exact).
//   prominence (multiplier > 0)  SciPy's _peak_prominences without wlen, by the owner lane at once: to each side walk
//            while the sample is not HIGHER than the peak, take the minimum over the walk; the peak minus the larger
//            of the two minima.  The walks are serial per extremum; the tall ones are few.
//   pairing  amplitude.py:862-901 on the two lists: the four slicings a, b, c, d are offsets into them.
#pragma once
#include "qm_preproc.hpp"

namespace qm {

constexpr int kAmpLdsSamples = 13312;           // 12 bytes per sample + 8 <= 160 KB
constexpr int kAmpWindowThreads = 64;
constexpr int kAmpTraceFields = 4;              // offset, n, filter (-1: none), taper (-1: none)
constexpr int kAmpWindowFields = 5;             // trace offset + lo, n, kind, lo, scratch offset in doubles (-1: LDS)
constexpr int kAmpColumns = 4;

enum AmpStatus : int {
    kAmpMeasured = 0, kAmpEmptyOrFlat = 1, kAmpNoExtremum = 2, kAmpConsecutive = 3, kAmpEqualPair = 4,
    kAmpNonFinite = 5,
};

struct AmpArgs {
    double *work;               // packed traces: stage A filters in place, stage B reads
    const int64_t *traces;      // [n_traces][kAmpTraceFields]
    const int64_t *tapers;      // [n_tapers][2]: offset into taper_w, ramp length m (left ramp, then right ramp)
    const double *sos;          // [n_filters][n_sections][6], a0 == 1
    const double *taper_w;
    const int64_t *windows;     // [n_windows][kAmpWindowFields]
    double *scratch;            // windows above the LDS limit: samples, then the two lists
    double *values;             // [n_windows][4]
    int32_t *index;             // [n_windows][4]
    int n_sections, skew, detrend_windows, method;
    double multiplier;
};

inline size_t amp_lds_bytes(int64_t n) { return (size_t)n * 8 + 2 * ((size_t)n / 2 + 1) * 4; }
inline size_t amp_scratch_doubles(int64_t n) { return (amp_lds_bytes(n) + 7) / 8; }

// ---- stage A ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ void amp_filter_trace(const AmpArgs &a, const int64_t *r, double *buf) {
#pragma clang fp contract(off)
    const int n = (int)r[1];
    detrend_line(buf, n, false);                        // (the line only)
    if (r[3] >= 0) {                                    // (2 m <= n)
        const int64_t *tp = a.tapers + 2 * r[3];
        const double *w = a.taper_w + tp[0];
        const int m = (int)tp[1];
        taper_ends(buf, n, w, m, w + m, m);
    }
    sos_passes(buf, n, a.sos + r[2] * a.n_sections * 6, a.n_sections, 1, a.skew);
}

// ---- stage B ----------------------------------------------------------------------------------------------------
// The local maxima of sign * y in SciPy's order into list[0..count), those below the prominence `need` left out
// (need <= 0: nothing is computed); returns count.
__device__ __forceinline__ int amp_extrema(const double *y, int n, double sign, double need, int32_t *list) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    int count = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        int at = -1;
        if (i >= 1 && i < n - 1 && sign * y[i - 1] < sign * y[i]) {
            const double v = sign * y[i];
            int ahead = i + 1;
            while (ahead < n - 1 && sign * y[ahead] == v) ++ahead;
            if (sign * y[ahead] < v) {
                at = (i + ahead - 1) / 2;
                if (need > 0.0) {
                    double left = v, right = v;
                    for (int k = at; k >= 0 && sign * y[k] <= v; --k) left = sign * y[k] < left ? sign * y[k] : left;
                    for (int k = at; k < n && sign * y[k] <= v; ++k) right = sign * y[k] < right ? sign * y[k] : right;
                    const double prominence = v - (left > right ? left : right);
                    if (!(prominence >= need)) at = -1;
                }
            }
        }
        const unsigned long long found = __ballot(at >= 0);
        if (at >= 0) list[count + __popcll(found & ((1ull << lane) - 1ull))] = at;
        count += __popcll(found);
    }
    return count;
}

// max over k < m of |y[pa[k]] - y[pb[k]]| and the first k that has it
__device__ __forceinline__ double amp_best_pair(const double *y, const int32_t *pa, const int32_t *pb, int m,
                                                int *pos) {
#pragma clang fp contract(off)
    const double top = wave_max(m, [&](int k) { return fabs(y[pa[k]] - y[pb[k]]); });
    *pos = wave_first(m, [&](int k) { return fabs(y[pa[k]] - y[pb[k]]) == top; });
    return top;
}

__device__ __forceinline__ void amp_window(const AmpArgs &a, const int64_t *r, double *y, int32_t *peaks,
                                           int32_t *troughs) {
#pragma clang fp contract(off)
    const int n = (int)r[1], kind = (int)r[2];
    const double *x = a.work + r[0];
    double out[kAmpColumns] = {0.0, 0.0, 0.0, 0.0};
    int status = kAmpMeasured, peak = -1, trough = -1, kept = 0;
    if (n < 1) {
        status = kAmpEmptyOrFlat;
    } else {
        for (int i = threadIdx.x; i < n; i += kAmpWindowThreads) y[i] = x[i];
        __syncthreads();
        const double bad = wave_max(n, [&](int i) { return isfinite(y[i]) ? 0.0 : 1.0; });
        if (bad > 0.0) status = kAmpNonFinite;
    }
    bool flat = false;
    if (status == kAmpMeasured && kind == 0)            // noise: flat is tested BEFORE the detrend (amplitude.py:955)
        flat = wave_max(n, [&](int i) { return y[i]; }) == -wave_max(n, [&](int i) { return -y[i]; });
    if (status == kAmpMeasured && !flat && a.detrend_windows) detrend_line(y, n, false);
    if (status == kAmpMeasured && kind == 1)            // signal: ... AFTER it (:765-771)
        flat = wave_max(n, [&](int i) { return y[i]; }) == -wave_max(n, [&](int i) { return -y[i]; });
    if (flat) status = kAmpEmptyOrFlat;
    if (status == kAmpMeasured) {
        out[2] = wave_max(n, [&](int i) { return fabs(y[i]); });
        if (a.method == 0) {
            out[1] = sqrt(wave_sum(n, [&](int i) { return y[i] * y[i]; }) / (double)n);
        } else {
            const double m = wave_sum(n, [&](int i) { return y[i]; }) / (double)n;
            out[1] = sqrt(wave_sum(n, [&](int i) { const double d = fabs(y[i] - m); return d * d; }) / (double)n);
        }
    }
    if (status == kAmpMeasured && kind == 1) {
        const double need = a.multiplier > 0.0 ? a.multiplier * out[2] : 0.0;
        const int np = amp_extrema(y, n, 1.0, need, peaks);
        const int nt = amp_extrema(y, n, -1.0, need, troughs);
        __syncthreads();
        kept = np;
        // amplitude.py:862-901 in its order: a, b, c, d are slices of the two lists
        const int32_t *pa = peaks, *pb = troughs, *pc = peaks, *pd = troughs;
        int m1 = 0, m2 = 0;
        if (np == 0 || nt == 0) {
            status = kAmpNoExtremum;
        } else if (np == 1 && nt == 1) {
            out[0] = fabs(y[peaks[0]] - y[troughs[0]]);
            peak = peaks[0];
            trough = troughs[0];
            // (`if not full_amp`: the reference's unbound names; a guard -- include/qmhip.h shows that finite samples
            // never give one peak and one trough of equal value)
            if (!(out[0] != 0.0)) status = kAmpEqualPair;
        } else if (np == nt) {
            m1 = np; m2 = np - 1;
            if (peaks[0] < troughs[0]) pc = peaks + 1;
            else pd = troughs + 1;
        } else if (np - nt != 1 && nt - np != 1) {
            status = kAmpConsecutive;
        } else if (np > nt) {
            if (!(peaks[0] < troughs[0])) status = kAmpConsecutive;
            m1 = m2 = nt;
            pc = peaks + 1;
        } else {
            if (!(peaks[0] > troughs[0])) status = kAmpConsecutive;
            m1 = m2 = np;
            pb = troughs + 1;
        }
        if (status == kAmpMeasured && m1 > 0) {
            int pos1 = 0, pos2 = 0;
            const double f1 = amp_best_pair(y, pa, pb, m1, &pos1);
            const double f2 = amp_best_pair(y, pc, pd, m2, &pos2);
            if (f1 >= f2) {                                     // (fp1 wins ties; the FIRST argmax inside the winner)
                out[0] = f1; peak = pa[pos1]; trough = pb[pos1];
            } else {
                out[0] = f2; peak = pc[pos2]; trough = pd[pos2];
            }
        }
        if (status != kAmpMeasured && status != kAmpEqualPair) {
            out[0] = 0.0;
            peak = trough = -1;
        }
        if (status == kAmpEqualPair) peak = trough = -1;
    }
    if (threadIdx.x == 0) {
        const int64_t w = blockIdx.x;
        const int lo = (int)r[3];
#pragma unroll
        for (int k = 0; k < kAmpColumns; ++k) a.values[w * kAmpColumns + k] = out[k];
        a.index[w * 4] = status;
        a.index[w * 4 + 1] = peak >= 0 ? lo + peak : -1;
        a.index[w * 4 + 2] = trough >= 0 ? lo + trough : -1;
        a.index[w * 4 + 3] = kept;
    }
}

#ifdef QM_TU_AMPLITUDES
__global__ __launch_bounds__(256) void amp_filter_kernel(AmpArgs a) {
    extern __shared__ double amp_trace[];
    const int64_t *r = a.traces + (int64_t)blockIdx.x * kAmpTraceFields;
    if (r[2] < 0) return;                               // no filter: measured as given
    double *row = a.work + r[0];
    const int n = (int)r[1];
    if (n <= kPreprocLdsSamples) {
        for (int i = threadIdx.x; i < n; i += blockDim.x) amp_trace[i] = row[i];
        __syncthreads();
        amp_filter_trace(a, r, amp_trace);
        for (int i = threadIdx.x; i < n; i += blockDim.x) row[i] = amp_trace[i];
    } else {
        amp_filter_trace(a, r, row);
    }
}

__global__ __launch_bounds__(kAmpWindowThreads) void amp_window_kernel(AmpArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char amp_lds[];
    const int64_t *r = a.windows + (int64_t)blockIdx.x * kAmpWindowFields;
    const int64_t n = r[1], cap = n / 2 + 1;
    if (r[4] < 0) {
        double *y = reinterpret_cast<double *>(amp_lds);
        int32_t *lists = reinterpret_cast<int32_t *>(y + n);
        amp_window(a, r, y, lists, lists + cap);
    } else {
        double *y = a.scratch + r[4];
        int32_t *lists = reinterpret_cast<int32_t *>(y + n);
        amp_window(a, r, y, lists, lists + cap);
    }
}
#endif  // QM_TU_AMPLITUDES

}  // namespace qm
