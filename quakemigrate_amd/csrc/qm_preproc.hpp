// qm_preproc.hpp -- waveform pre-processing on the device: what the reference's calculate_onsets does to
// every component trace before the STA/LTA (quakemigrate/signal/onsets/stalta.py:137-211, :353-489):
// linear detrend, demean, taper, zero-phase Butterworth band-pass (sosfilt forward, then backward).
//
// One workgroup of four wavefronts per trace.  The trace is staged in LDS (up to kPreprocLdsSamples samples: all
// 160 KB of a CU -- so the kernel holds NO other LDS; longer traces are worked on in place in the output row).
// The conditioning steps themselves -- fixed-order sums, detrend, taper, the skewed filter passes -- are
// qm_condition.hpp's; this file stages the trace and calls them.
#pragma once
#include "qm_condition.hpp"

namespace qm {

constexpr int kPreprocLdsSamples = 20480;       // 160 KB of float64: the onset stage's limit as well

struct PreprocArgs {
    const double *in;           // [n][T] resampled component traces
    double *out;                // [n][T] (may be `in`)
    const int32_t *trace_filter;   // [n] filter of each trace
    const double *sos;          // [n_filters][n_sections][6]: b0 b1 b2 a0 a1 a2, a0 == 1
    const double *taper_left;   // [n_left] weights of the first samples
    const double *taper_right;  // [n_right] weights of the last samples
    int T, n_sections, n_left, n_right;
    int detrend, zero_phase, skew;
};

template <bool IN_LDS>
__device__ __forceinline__ void preproc_trace(const PreprocArgs &a, double *buf) {
#pragma clang fp contract(off)
    const int n = a.T;
    const int64_t tr = blockIdx.x;
    const double *x = a.in + tr * n;
    double *out = a.out + tr * n;
    if (IN_LDS || x != out)
        for (int i = threadIdx.x; i < n; i += blockDim.x) buf[i] = x[i];
    __syncthreads();
    if (a.detrend) detrend_line(buf, n, true);
    taper_ends(buf, n, a.taper_left, a.n_left, a.taper_right, a.n_right);
    const double *c = a.sos + (int64_t)a.trace_filter[tr] * a.n_sections * 6;
    sos_passes(buf, n, c, a.n_sections, a.zero_phase ? 2 : 1, a.skew);
    if (IN_LDS)
        for (int i = threadIdx.x; i < n; i += blockDim.x) out[i] = buf[i];
}

// The segmented form: gappy traces (the reference's allow_gaps = True / full_timespan = False, stalta.py:137-211,
// :442-461).  A trace is a row of T samples in window layout of which one or more SEGMENTS hold data; every segment is
// conditioned on its own -- detrend, taper, filter, and a second taper that takes the filter's transients off -- and
// what lies between the segments and at the window's ends is filled with one value (the reference's
// sqrt(finfo(float).tiny)).  One workgroup per segment RECORD: the segments of a trace condition in parallel, no
// workgroup waits on another, nothing is atomic -- a record's workgroup writes its segment and its share of the fill,
// and the host has checked that the records of a trace tile the row exactly once.  Samples outside every segment are
// never read.  A segment lives in LDS up to kPreprocLdsSamples, above that in place in the output row.
constexpr int kSegmentFields = 8;
enum SegmentField : int {
    kSegTrace = 0,          // row of the (step's) traces
    kSegFirst = 1,          // the segment is samples [first, first + n) of the row
    kSegN = 2,              // 0: the record is padding, nothing is done
    kSegFillBefore = 3,     // out[first - fill_before .. first) = fill_value
    kSegFillAfter = 4,      // out[first + n .. first + n + fill_after) = fill_value
    kSegWOffset = 5,        // its taper: weights w = taper_w + w_offset, w[0..m) for the first m samples,
    kSegM = 6,              // ... w[m..2m) for the last m
};

struct SegmentArgs {
    const double *in;           // step k's traces [n_traces][T] at in + k * in_step
    double *out;                // ... at out + k * out_step (may be `in`)
    const int32_t *trace_filter;   // [n_traces] filter of each trace
    const double *sos;          // [n_filters][n_sections][6]
    const int64_t *rec;         // step k's records [n_records][kSegmentFields] at rec + k * rec_step
    const double *taper_w;      // step k's weights at taper_w + k * w_step
    int64_t in_step, out_step, rec_step, w_step;
    int T, n_records, n_sections;
    int detrend, zero_phase, skew, second_taper;
    double fill_value;
};

template <bool IN_LDS>
__device__ __forceinline__ void preproc_segment(const SegmentArgs &a, const double *x, double *y, double *buf, int n,
                                                const double *w, int m, const double *c) {
#pragma clang fp contract(off)
    if (IN_LDS || x != y)
        for (int i = threadIdx.x; i < n; i += blockDim.x) buf[i] = x[i];
    __syncthreads();
    if (a.detrend) detrend_line(buf, n, true);
    taper_ends(buf, n, w, m, w + m, m);
    sos_passes(buf, n, c, a.n_sections, a.zero_phase ? 2 : 1, a.skew);
    if (a.second_taper) taper_ends(buf, n, w, m, w + m, m);
    if (IN_LDS)
        for (int i = threadIdx.x; i < n; i += blockDim.x) y[i] = buf[i];
}

#ifdef QM_TU_PREPROC
__global__ __launch_bounds__(256) void preproc_kernel(PreprocArgs a, int in_lds) {
    extern __shared__ double trace[];
    if (in_lds) preproc_trace<true>(a, trace);
    else preproc_trace<false>(a, a.out + (int64_t)blockIdx.x * a.T);
}

// grid: n_steps x n_records workgroups; dynamic LDS: the longest segment that fits, in doubles
__global__ __launch_bounds__(256) void segments_kernel(SegmentArgs a) {
    extern __shared__ double trace[];
    const int64_t step = blockIdx.x / (unsigned)a.n_records;
    const int64_t *r = a.rec + step * a.rec_step + (int64_t)(blockIdx.x % (unsigned)a.n_records) * kSegmentFields;
    const int n = (int)r[kSegN];
    if (n == 0) return;                                 // (the whole workgroup: a stream's padding)
    const int64_t tr = r[kSegTrace], first = r[kSegFirst];
    const double *x = a.in + step * a.in_step + tr * a.T + first;
    double *row = a.out + step * a.out_step + tr * a.T;
    double *y = row + first;
    const double *w = a.taper_w + step * a.w_step + r[kSegWOffset];
    const double *c = a.sos + (int64_t)a.trace_filter[tr] * a.n_sections * 6;
    const int m = (int)r[kSegM];
    if (n <= kPreprocLdsSamples) preproc_segment<true>(a, x, y, trace, n, w, m, c);
    else preproc_segment<false>(a, x, y, y, n, w, m, c);
    // the record's share of the fill: samples no segment holds, so nobody reads or writes them but this workgroup
    const int before = (int)r[kSegFillBefore], after = (int)r[kSegFillAfter];
    for (int i = threadIdx.x; i < before; i += blockDim.x) row[first - before + i] = a.fill_value;
    for (int i = threadIdx.x; i < after; i += blockDim.x) row[first + n + i] = a.fill_value;
}
#endif  // QM_TU_PREPROC

}  // namespace qm
