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

#ifdef QM_TU_PREPROC
__global__ __launch_bounds__(256) void preproc_kernel(PreprocArgs a, int in_lds) {
    extern __shared__ double trace[];
    if (in_lds) preproc_trace<true>(a, trace);
    else preproc_trace<false>(a, a.out + (int64_t)blockIdx.x * a.T);
}
#endif  // QM_TU_PREPROC

}  // namespace qm
