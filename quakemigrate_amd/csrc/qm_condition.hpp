// qm_condition.hpp -- what the trace stages do to a trace before their own work, written once: the least-squares line
// out (detrend_line), the taper's two ramps (taper_ends), a cascade of second-order sections as SciPy's sosfilt
// computes it (sos_passes).  qm_preproc.hpp, qm_resample.hpp and qm_amplitudes.hpp call them on a trace that the whole
// workgroup sees -- in LDS or in global memory: the address space is the call site's -- and keep what is theirs:
// staging, records, upsampling, the window measurement.
//   sums       every wavefront computes each sum for itself (qm_block.hpp: wave_sum): lane l adds samples l, l + 64, ...
//              in that order, a fixed butterfly adds the 64 partials.  All wavefronts get the same bits, the result
//              does not depend on the run, and nothing has to cross wavefronts (the trace kernels have no LDS left
//              for that).
//   detrend,   elementwise, all threads of the workgroup (256 in the trace kernels, 64 in amp_window_kernel)
//   taper
//   filter     the recurrence is the serial part.  A cascade of S second-order sections over T samples is
//              T x S dependent steps on one lane; here section s runs on lane s of wavefront 0 at sample
//              n - s (a software pipeline across lanes): lane s hands its output to lane s + 1 with a DPP
//              row shift, lane 0 takes the next sample, lane S - 1 delivers.  Every (section, sample)
//              operation is the one SciPy's _sosfilt does, in its order, without contraction -- the bits are
//              SciPy's -- and the critical path is T + S steps.  Samples enter and leave in blocks of 64: one
//              LDS read, one LDS write per block, v_readlane in between.
//              "preproc_skew" = 0 keeps the plain form (lane 0 walks sample by sample, section by section):
//              the in-device cross-check.
// Every function here switches contraction off in its own body: the pragma is lexical and device code is otherwise
// compiled with contraction allowed, so a function without it would gain FMAs and lose the pinned bits
// (tests/preprocess_ref.py: detrend_device_order, sosfilt).
#pragma once
#include "qm_block.hpp"

namespace qm {

constexpr int kPreprocMaxSections = 8;

__device__ __forceinline__ double lane_below(double v) {       // lane l <- lane l - 1 within a row of 16
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x111, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x111, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double from_lane(double v, int lane) {      // `lane` is uniform
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane),
                            __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// One pass of the cascade over buf[0..T), logical sample i at buf[rev ? T - 1 - i : i], in place.
// Called by the whole of wavefront 0.  c: this filter's [S][6].
__device__ __forceinline__ void sos_pass_skewed(double *buf, int T, bool rev, const double *c, int S) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    double b0 = 0.0, b1 = 0.0, b2 = 0.0, a1 = 0.0, a2 = 0.0;
    if (lane < S) {
        b0 = c[6 * lane]; b1 = c[6 * lane + 1]; b2 = c[6 * lane + 2];
        a1 = c[6 * lane + 4]; a2 = c[6 * lane + 5];
    }
    double z0 = 0.0, z1 = 0.0, xn = 0.0;
    const int steps = T + S - 1;                        // step k: lane s works on sample k - s
    for (int base = 0; base < steps; base += 64) {
        const int i = base + lane;
        const double xv = i < T ? buf[rev ? T - 1 - i : i] : 0.0;
        double yv = 0.0;
        const int jn = min(64, steps - base);
        // (the step loop below starts 4 bytes past an 8-byte boundary wherever this function is inlined: its time
        // depends on where its 8-byte instructions fall, by some 4 % between the two phases)
        asm volatile(".p2align 3\n\ts_nop 0");
        for (int j = 0; j < jn; ++j) {
            const double handed = lane_below(xn);       // the section below, one step ago: its sample k - s
            const double xc = lane == 0 ? from_lane(xv, j) : handed;
            const double t = b0 * xc + z0;
            const double n0 = b1 * xc - a1 * t + z1;
            const double n1 = b2 * xc - a2 * t;
            if (base + j >= lane) {                     // (before its first sample a section keeps its zero state)
                xn = t;
                z0 = n0;
                z1 = n1;
            }
            const double y = from_lane(xn, S - 1);
            if (lane == j) yv = y;
        }
        const int o = i - (S - 1);                      // lane j holds step base + j's delivery: sample k - (S - 1)
        if (lane < jn && o >= 0 && o < T) buf[rev ? T - 1 - o : o] = yv;
    }
}

// the same pass on lane 0 alone
__device__ __forceinline__ void sos_pass_plain(double *buf, int T, bool rev, const double *c, int S) {
#pragma clang fp contract(off)
    double z[kPreprocMaxSections][2];
    for (int s = 0; s < S; ++s) z[s][0] = z[s][1] = 0.0;
    for (int i = 0; i < T; ++i) {
        double *p = buf + (rev ? T - 1 - i : i);
        double xc = *p;
        for (int s = 0; s < S; ++s) {
            const double *k = c + 6 * s;
            const double xn = k[0] * xc + z[s][0];
            z[s][0] = k[1] * xc - k[4] * xn + z[s][1];
            z[s][1] = k[2] * xc - k[5] * xn;
            xc = xn;
        }
        *p = xc;
    }
}

// The least-squares line over i = 0..n-1 out of buf[0..n) in its centred form and, with also_mean, the mean of what
// is left (the reference's detrend("linear"), then detrend("constant"), stalta.py:447-448).  Called by the whole
// workgroup behind a barrier; ends on one.
__device__ __forceinline__ void detrend_line(double *buf, int n, bool also_mean) {
#pragma clang fp contract(off)
    const double mean = wave_sum(n, [&](int i) { return buf[i]; }) / (double)n;
    const double tbar = 0.5 * (double)(n - 1);
    const double sxx = wave_sum(n, [&](int i) { const double d = (double)i - tbar; return d * d; });
    const double sxy = wave_sum(n, [&](int i) { return ((double)i - tbar) * (buf[i] - mean); });
    const double slope = sxx > 0.0 ? sxy / sxx : 0.0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) buf[i] = buf[i] - (mean + slope * ((double)i - tbar));
    __syncthreads();
    if (also_mean) {
        const double rest = wave_sum(n, [&](int i) { return buf[i]; }) / (double)n;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += blockDim.x) buf[i] = buf[i] - rest;
        __syncthreads();
    }
}

// The first n_left samples times `left`, the last n_right times `right`; n_left + n_right <= n, so no sample has two
// weights.  A taper-table entry [offset, m] is (w, m, w + m, m).  Whole workgroup; ends on a barrier.
__device__ __forceinline__ void taper_ends(double *buf, int n, const double *left, int n_left, const double *right,
                                           int n_right) {
#pragma clang fp contract(off)
    for (int k = threadIdx.x; k < n_left; k += blockDim.x) buf[k] *= left[k];
    for (int k = threadIdx.x; k < n_right; k += blockDim.x) buf[n - n_right + k] *= right[k];
    __syncthreads();
}

// n_passes (1: forward, 2: then backward) of the cascade c [n_sections][6] over buf[0..n) on wavefront 0 from a zero
// state each, skewed or plain.  Whole workgroup behind a barrier; ends on one.
__device__ __forceinline__ void sos_passes(double *buf, int n, const double *c, int n_sections, int n_passes,
                                           int skew) {
#pragma clang fp contract(off)
    if (threadIdx.x < 64) {                             // wavefront 0
        for (int pass = 0; pass < n_passes; ++pass) {
            if (pass) __threadfence_block();            // (the backward pass reads what other lanes delivered)
            if (skew) sos_pass_skewed(buf, n, pass == 1, c, n_sections);
            else if (threadIdx.x == 0) sos_pass_plain(buf, n, pass == 1, c, n_sections);
        }
    }
    __syncthreads();
}

}  // namespace qm
