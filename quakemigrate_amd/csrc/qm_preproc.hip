// qm_preproc.hip -- the pre-processing stage's host side: argument checks, staging, the launch (kernel and its
// notes: qm_preproc.hpp).  qm_engine_preprocess is the staged call; the pipeline (qm_stream.hip) launches the same
// kernel over the (step, trace)s of a slot through launch_preproc_stage.
#define QM_TU_PREPROC 1
#include "qm_engine.hpp"

int check_preproc(const char *what, int32_t n_traces, int32_t t_samples, const int32_t *trace_filter,
                  const double *sos, int32_t n_filters, int32_t n_sections, const double *taper_left, int32_t n_left,
                  const double *taper_right, int32_t n_right) {
    if (!trace_filter || !sos) return fail("%s: NULL argument", what);
    if (n_traces < 1 || t_samples < 1) return fail("%s: empty input", what);
    if (n_filters < 1) return fail("%s: at least one filter is needed (got %d)", what, n_filters);
    if (n_sections < 1 || n_sections > qm::kPreprocMaxSections)
        return fail("%s: n_sections must be in 1..%d (got %d)", what, qm::kPreprocMaxSections, n_sections);
    if (n_left < 0 || n_right < 0 || (n_left > 0 && !taper_left) || (n_right > 0 && !taper_right))
        return fail("%s: taper of %d + %d samples without weights", what, n_left, n_right);
    if ((int64_t)n_left + n_right > t_samples)
        return fail("%s: the tapers cover %d + %d samples, the traces hold %d", what, n_left, n_right, t_samples);
    for (int i = 0; i < n_traces; ++i)
        if (trace_filter[i] < 0 || trace_filter[i] >= n_filters)
            return fail("%s: trace %d: filter %d out of range (%d filters)", what, i, trace_filter[i], n_filters);
    for (int k = 0; k < n_filters * n_sections; ++k)
        if (sos[6 * k + 3] != 1.0)
            return fail("%s: filter %d, section %d: a0 = %.17g, sections must be normalised to a0 == 1", what,
                        k / n_sections, k % n_sections, sos[6 * k + 3]);
    return 0;
}

int launch_preproc_stage(qm_engine *e, const qm::PreprocArgs &a, int64_t n_traces) {
    // one workgroup per trace; the trace lives in LDS if it fits (20 480 samples), else in its output row
    const size_t lds = (size_t)a.T * sizeof(double);
    const int in_lds = a.T <= qm::kPreprocLdsSamples ? 1 : 0;
    if (in_lds)
        QM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&qm::preproc_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(qm::preproc_kernel, dim3((unsigned)n_traces), dim3(256), in_lds ? lds : 0, e->stream, a,
                       in_lds);
    QM_HIP(hipGetLastError());
    return 0;
}

extern "C" {

int qm_engine_preprocess(qm_engine *e, const double *signals, int signals_on_device, int32_t n_traces,
                         int32_t t_samples, const int32_t *trace_filter, const double *sos, int32_t n_filters,
                         int32_t n_sections, int detrend, const double *taper_left, int32_t n_left,
                         const double *taper_right, int32_t n_right, int zero_phase, double *filtered,
                         int out_on_device) {
    if (!e || !signals || !filtered) return fail("qm_engine_preprocess: NULL argument");
    if (check_preproc("qm_engine_preprocess", n_traces, t_samples, trace_filter, sos, n_filters, n_sections,
                      taper_left, n_left, taper_right, n_right))
        return 1;
    DeviceGuard guard(e->device);
    const size_t sig = (size_t)n_traces * t_samples;
    const size_t n_coef = (size_t)n_filters * n_sections * 6, n_w = n_coef + n_left + n_right;
    if (e->d_pre_coef.ensure(n_w) || e->d_pre_meta.ensure((size_t)n_traces)) return 1;
    std::vector<double> w(sos, sos + n_coef);
    w.insert(w.end(), taper_left, taper_left + n_left);
    w.insert(w.end(), taper_right, taper_right + n_right);
    QM_HIP(copy_in(e->d_pre_coef.p, w.data(), n_w * sizeof(double), e->stream));
    QM_HIP(copy_in(e->d_pre_meta.p, trace_filter, (size_t)n_traces * sizeof(int32_t), e->stream));
    const double *d_sig = signals;
    if (!signals_on_device) {
        if (e->d_sig.ensure(sig)) return 1;
        QM_HIP(copy_in(e->d_sig.p, signals, sig * sizeof(double), e->stream));
        d_sig = e->d_sig.p;
    }
    double *d_out = filtered;
    if (!out_on_device) {
        if (e->d_pre_out.ensure(sig)) return 1;
        d_out = e->d_pre_out.p;
    }
    qm::PreprocArgs a{};
    a.in = d_sig;
    a.out = d_out;
    a.trace_filter = e->d_pre_meta.p;
    a.sos = e->d_pre_coef.p;
    a.taper_left = e->d_pre_coef.p + n_coef;
    a.taper_right = e->d_pre_coef.p + n_coef + n_left;
    a.T = t_samples; a.n_sections = n_sections; a.n_left = n_left; a.n_right = n_right;
    a.detrend = detrend ? 1 : 0; a.zero_phase = zero_phase ? 1 : 0; a.skew = e->cfg_preproc_skew;
    if (launch_preproc_stage(e, a, n_traces)) return 1;
    if (!out_on_device) {
        QM_HIP(copy_back(filtered, d_out, sig * sizeof(double), e->stream));
        QM_HIP(hipStreamSynchronize(e->stream));
    }
    return 0;
}

}  // extern "C"
