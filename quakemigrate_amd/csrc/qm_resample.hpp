// qm_resample.hpp -- raw component traces to the scan rate on the device: what the reference's util.resample does to
// every trace of a timestep before anything else (quakemigrate/util.py:404-604, called from stalta.py:191):
// linear-interpolation upsampling by an integer factor with constant padding at the window's ends, then decimation
// behind a detrend, a cosine taper and a zero-phase Butterworth low-pass.
//
// One workgroup of four wavefronts per trace; detrend, taper and filter passes are qm_condition.hpp's, the ones the
// pre-processing stage runs: the low-pass is SciPy's sosfilt bit for bit.
// A trace's record (ResampleField) says which raw samples it reads and which of the steps it takes; the host plans
// the records (quakemigrate_amd/preprocess.py: ResampleStage) and checks them (qm_resample.hip: check_resample), the
// kernel trusts them.
//   kept series  the padded, upsampled series cut to [up_first, up_first + n_up): in LDS up to kPreprocLdsSamples
//                samples (all 160 KB -- so, as in qm_preproc.hpp, the kernel holds NO other LDS), else in the trace's
//                row of scratch in global memory.  Both paths run the same arithmetic in the same order.
//   filter       the reference's low-pass has ONE section, so the skewed pipeline has one busy lane and the critical
//                path is 2 n_up dependent steps on wavefront 0 -- inherent to sosfilt's bits; what the skewed form
//                still buys is the blocked LDS traffic (64 samples per read and per write).
#pragma once
#include "qm_preproc.hpp"

namespace qm {

// a trace's record: kResampleFields int64 each
enum ResampleField : int {
    kRsRawOffset = 0,   // first raw sample of the trace in the packed raw buffer (elements)
    kRsNRaw,            // raw samples, >= 1
    kRsUp,              // u >= 1: upsampling factor
    kRsPadLeft,         // copies of the first raw sample in front of the upsampled series (u > 1 only)
    kRsPadRight,        // copies of the last one behind it
    kRsUpFirst,         // the kept slice of the padded, upsampled series: first sample ...
    kRsNUp,             // ... and length
    kRsDec,             // d >= 1: decimation factor
    kRsLowpass,         // d > 1: index into sos [n_lowpass][n_sections][6]
    kRsTaper,           // d > 1: index into the taper table
    kRsOutFirst,        // first decimated sample of the output row
    kResampleFields
};

enum ResampleDtype : int { kRawInt32 = 0, kRawFloat64 = 1 };

struct ResampleArgs {
    const void *raw;            // packed raw samples of every trace, int32 or float64
    const int64_t *rec;         // [n][kResampleFields]
    const int64_t *tapers;      // [n_tapers][2]: offset into taper_w, ramp length m (left ramp, then right ramp)
    const double *sos;          // [n_lowpass][n_sections][6], a0 == 1
    const double *taper_w;
    double *out;                // [n][T]
    double *scratch;            // [n][scratch_stride]: the kept series of traces above the LDS limit
    int64_t scratch_stride;
    int T, n_sections, raw_dtype, detrend, skew;
};

template <bool RAW_INT32>
__device__ __forceinline__ void resample_trace(const ResampleArgs &a, const int64_t *r, double *buf) {
#pragma clang fp contract(off)
    const int64_t n_raw = r[kRsNRaw], u = r[kRsUp], pad_left = r[kRsPadLeft], first = r[kRsUpFirst];
    const int n = (int)r[kRsNUp], d = (int)r[kRsDec];
    const int64_t len = (n_raw - 1) * u + 1;            // the upsampled series, before the pads
    auto x = [&](int64_t j) {
        const int64_t at = r[kRsRawOffset] + j;
        return RAW_INT32 ? (double)static_cast<const int32_t *>(a.raw)[at] : static_cast<const double *>(a.raw)[at];
    };
    // upsampled sample j u + i: (i / u) x[j + 1] + ((u - i) / u) x[j] -- the two quotients first, then two products,
    // one sum: NumPy's bits for the reference's expression (util.py:548-551)
    for (int k = threadIdx.x; k < n; k += blockDim.x) {
        const int64_t q = first + k - pad_left;
        double v;
        if (q <= 0) v = x(0);
        else if (q >= len - 1) v = x(n_raw - 1);
        else {
            const int64_t j = q / u, i = q - j * u;
            if (i == 0) v = x(j);
            else {
                const double wa = (double)i / (double)u, wb = (double)(u - i) / (double)u;
                const double pa = wa * x(j + 1), pb = wb * x(j);
                v = pa + pb;
            }
        }
        buf[k] = v;
    }
    __syncthreads();
    if (d > 1) {
        if (a.detrend) detrend_line(buf, n, true);
        const int64_t *tp = a.tapers + 2 * r[kRsTaper];     // (2 m <= n_up)
        const double *w = a.taper_w + tp[0];
        const int m = (int)tp[1];
        taper_ends(buf, n, w, m, w + m, m);
        sos_passes(buf, n, a.sos + r[kRsLowpass] * a.n_sections * 6, a.n_sections, 2, a.skew);
    }
    // every d-th sample from out_first on (obspy's decimate without its own filter: data[::d])
    double *out = a.out + (int64_t)blockIdx.x * a.T;
    const int64_t o0 = r[kRsOutFirst];
    for (int k = threadIdx.x; k < a.T; k += blockDim.x) out[k] = buf[(o0 + k) * d];
}

#ifdef QM_TU_RESAMPLE
__global__ __launch_bounds__(256) void resample_kernel(ResampleArgs a) {
    extern __shared__ double kept[];
    const int64_t *r = a.rec + (int64_t)blockIdx.x * kResampleFields;
    const bool in_lds = r[kRsNUp] <= kPreprocLdsSamples;
    double *row = a.scratch + (int64_t)blockIdx.x * a.scratch_stride;
    // (four copies: the buffer's address space and the raw type are known in each)
    if (a.raw_dtype == kRawInt32) {
        if (in_lds) resample_trace<true>(a, r, kept);
        else resample_trace<true>(a, r, row);
    } else {
        if (in_lds) resample_trace<false>(a, r, kept);
        else resample_trace<false>(a, r, row);
    }
}
#endif  // QM_TU_RESAMPLE

}  // namespace qm
