// qm_preproc.hip -- the pre-processing stage's host side (kernel and its notes: qm_preproc.hpp).  PreprocStage
// (qm_engine.hpp) is the stage: build checks the caller's arrays and puts them on the device, launch runs the kernel over
// the (step, trace)s of a launch.  qm_engine_preprocess is the staged call on the engine's record; the pipeline
// (qm_stream.hip) holds a record of its own.
#define QM_TU_PREPROC 1
#include "qm_engine.hpp"

namespace {

int check_preproc(const char *what, int32_t n_traces, int32_t t_samples, const int32_t *trace_filter,
                  const double *sos, int32_t n_filters, int32_t n_sections, const double *taper_left, int32_t n_left,
                  const double *taper_right, int32_t n_right) {
    if (!trace_filter || !sos) return fail("%s: NULL argument", what);
    if (n_traces < 1 || t_samples < 1) return fail("%s: empty input", what);
    if (n_filters < 1) return fail("%s: at least one filter is needed (got %d)", what, n_filters);
    if (check_sections(what, "filter", "n_sections", sos, n_filters, n_sections)) return 1;
    if (n_left < 0 || n_right < 0 || (n_left > 0 && !taper_left) || (n_right > 0 && !taper_right))
        return fail("%s: taper of %d + %d samples without weights", what, n_left, n_right);
    if ((int64_t)n_left + n_right > t_samples)
        return fail("%s: the tapers cover %d + %d samples, the traces hold %d", what, n_left, n_right, t_samples);
    for (int i = 0; i < n_traces; ++i)
        if (trace_filter[i] < 0 || trace_filter[i] >= n_filters)
            return fail("%s: trace %d: filter %d out of range (%d filters)", what, i, trace_filter[i], n_filters);
    return 0;
}

}  // namespace

int PreprocStage::build(qm_engine *e, const char *what, int repeat, int32_t n_traces_, int32_t t_samples,
                        const int32_t *trace_filter, const double *sos, int32_t n_filters, int32_t n_sections,
                        int detrend, const double *taper_left, int32_t n_left, const double *taper_right,
                        int32_t n_right, int zero_phase) {
    if (check_preproc(what, n_traces_, t_samples, trace_filter, sos, n_filters, n_sections, taper_left, n_left,
                      taper_right, n_right))
        return 1;
    const size_t n_coef = (size_t)n_filters * n_sections * 6;
    std::vector<double> w(sos, sos + n_coef);
    w.insert(w.end(), taper_left, taper_left + n_left);
    w.insert(w.end(), taper_right, taper_right + n_right);
    std::vector<int32_t> filters;
    for (int k = 0; k < repeat; ++k) filters.insert(filters.end(), trace_filter, trace_filter + n_traces_);
    if (coef.ensure(w.size()) || meta.ensure(filters.size())) return 1;
    QM_HIP(copy_in(coef.p, w.data(), w.size() * sizeof(double), e->stream));
    QM_HIP(copy_in(meta.p, filters.data(), filters.size() * sizeof(int32_t), e->stream));
    n_traces = n_traces_;
    args = qm::PreprocArgs{};
    args.trace_filter = meta.p;
    args.sos = coef.p;
    args.taper_left = coef.p + n_coef;
    args.taper_right = coef.p + n_coef + n_left;
    args.T = t_samples; args.n_sections = n_sections; args.n_left = n_left; args.n_right = n_right;
    args.detrend = detrend ? 1 : 0; args.zero_phase = zero_phase ? 1 : 0;
    return 0;
}

int PreprocStage::launch(qm_engine *e, const double *in, double *out, int n_steps) const {
    qm::PreprocArgs a = args;
    a.in = in;
    a.out = out;
    a.skew = e->cfg.preproc_skew;
    // one workgroup per trace; the trace lives in LDS if it fits (20 480 samples), else in its output row
    const int in_lds = a.T <= qm::kPreprocLdsSamples ? 1 : 0;
    const size_t lds = in_lds ? (size_t)a.T * sizeof(double) : 0;
    return launch_with_lds(e, qm::preproc_kernel, (unsigned)((int64_t)n_steps * n_traces), 256, lds, a, in_lds);
}

extern "C" {

int qm_engine_preprocess(qm_engine *e, const double *signals, int signals_on_device, int32_t n_traces,
                         int32_t t_samples, const int32_t *trace_filter, const double *sos, int32_t n_filters,
                         int32_t n_sections, int detrend, const double *taper_left, int32_t n_left,
                         const double *taper_right, int32_t n_right, int zero_phase, double *filtered,
                         int out_on_device) {
    if (!e || !signals || !filtered) return fail("qm_engine_preprocess: NULL argument");
    DeviceGuard guard(e->device);
    if (e->pre_stage.build(e, "qm_engine_preprocess", 1, n_traces, t_samples, trace_filter, sos, n_filters, n_sections,
                           detrend, taper_left, n_left, taper_right, n_right, zero_phase))
        return 1;
    const size_t sig = (size_t)n_traces * t_samples;
    const double *d_sig = stage_in(e, e->staging.sig, signals, signals_on_device, sig);
    if (!d_sig) return 1;
    const StagedOut<double> out = stage_host_out(e->staging.pre_out, filtered, out_on_device, sig);
    if (!out.d || e->pre_stage.launch(e, d_sig, out.d, 1) || out.fetch(e)) return 1;
    if (!out_on_device) QM_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

}  // extern "C"
