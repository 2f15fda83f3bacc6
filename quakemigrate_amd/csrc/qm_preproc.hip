// qm_preproc.hip -- the pre-processing stage's host side (kernel and its notes: qm_preproc.hpp).  PreprocStage
// (qm_engine.hpp) is the stage: build checks the caller's arrays and puts them on the device, launch runs the kernel over
// the (step, trace)s of a launch.  qm_engine_preprocess is the staged call on the engine's record; the pipeline
// (qm_stream.hip) holds a record of its own.  SegmentStage is the same for gappy traces -- one workgroup per segment
// record -- with qm_engine_preprocess_segments beside it and, for the stream, the layout of a pushed step (adopt, pack,
// the slot form of launch); check_segment_records is what both refuse in a timestep's records.
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

// ---- the segmented form: gappy traces ---------------------------------------------------------------------------

int check_segment_records(const char *what, int32_t n_traces, int32_t t_samples, const int64_t *records,
                          int32_t n_segments, int64_t n_taper_weights) {
    using namespace qm;
    if (!records) return fail("%s: NULL argument", what);
    if (n_segments < 1) return fail("%s: at least one segment is needed (got %d)", what, n_segments);
    const int64_t T = t_samples;
    std::vector<std::pair<int64_t, int64_t>> spans;     // (trace, start of segment + fill), then their ends by index
    std::vector<int64_t> ends((size_t)n_segments);
    for (int i = 0; i < n_segments; ++i) {
        const int64_t *r = records + (size_t)i * kSegmentFields;
        const int64_t first = r[kSegFirst], n = r[kSegN], fb = r[kSegFillBefore], fa = r[kSegFillAfter];
        const int64_t off = r[kSegWOffset], m = r[kSegM];
        if (r[kSegTrace] < 0 || r[kSegTrace] >= n_traces)
            return fail("%s: segment %d: trace %lld out of range (%d traces)", what, i, (long long)r[kSegTrace], n_traces);
        if (n < 1) return fail("%s: segment %d: n = %lld, at least one sample is needed", what, i, (long long)n);
        if (fb < 0 || fa < 0)
            return fail("%s: segment %d: a fill of %lld + %lld samples (fills are >= 0)", what, i, (long long)fb,
                        (long long)fa);
        if (first < 0 || first > T || n > T || fb > T || fa > T || first - fb < 0 || first + n + fa > T)
            return fail("%s: segment %d: samples [%lld, %lld) with their fill leave the window of %d", what, i,
                        (long long)(first - fb), (long long)(first + n + fa), t_samples);
        if (off < 0 || m < 0 || m > T || off + 2 * m > n_taper_weights)
            return fail("%s: segment %d: 2 x %lld weights from %lld on, %lld weights given", what, i, (long long)m,
                        (long long)off, (long long)n_taper_weights);
        if (2 * m > n)
            return fail("%s: segment %d: its taper's ramps cover 2 x %lld samples, the segment holds %lld", what, i,
                        (long long)m, (long long)n);
        if (r[7] != 0) return fail("%s: segment %d: field 7 is %lld, it must be 0", what, i, (long long)r[7]);
        spans.push_back({r[kSegTrace] * (T + 1) + (first - fb), i});
        ends[(size_t)i] = first + n + fa;
    }
    // every trace's [first - fill_before, first + n + fill_after) tile [0, T) exactly once: what makes one workgroup per
    // record safe -- no sample has two writers, none is left unwritten
    std::sort(spans.begin(), spans.end());
    size_t k = 0;
    for (int64_t tr = 0; tr < n_traces; ++tr) {
        int64_t at = 0;
        for (; k < spans.size() && spans[k].first / (T + 1) == tr; ++k) {
            const int64_t start = spans[k].first % (T + 1);
            if (start != at)
                return fail("%s: trace %d: its segments and fills do not tile the window [0, %d) exactly once (%s at "
                            "sample %lld)", what, (int)tr, t_samples, start < at ? "an overlap" : "a hole",
                            (long long)std::min(start, at));
            at = ends[(size_t)spans[k].second];
        }
        if (at != T)
            return fail("%s: trace %d: its segments and fills do not tile the window [0, %d) exactly once (%s at "
                        "sample %lld)", what, (int)tr, t_samples, at == 0 ? "no segment" : "a hole", (long long)at);
    }
    return 0;
}

int SegmentStage::build(qm_engine *e, const char *what, int32_t n_traces_, int32_t t_samples,
                        const int32_t *trace_filter, const double *sos, int32_t n_filters, int32_t n_sections,
                        int detrend, int zero_phase, const int64_t *records, int32_t n_segments,
                        const double *taper_weights, int64_t n_taper_weights, int second_taper, double fill_value) {
    if (check_preproc(what, n_traces_, t_samples, trace_filter, sos, n_filters, n_sections, nullptr, 0, nullptr, 0))
        return 1;
    if (n_taper_weights < 0 || (n_taper_weights > 0 && !taper_weights))
        return fail("%s: %lld taper weights without their array", what, (long long)n_taper_weights);
    if (!std::isfinite(fill_value)) return fail("%s: fill_value %g is not finite", what, fill_value);
    if (check_segment_records(what, n_traces_, t_samples, records, n_segments, n_taper_weights)) return 1;
    const size_t n_coef = (size_t)n_filters * n_sections * 6, n_rec = (size_t)n_segments * qm::kSegmentFields;
    std::vector<double> w(sos, sos + n_coef);
    if (n_taper_weights > 0) w.insert(w.end(), taper_weights, taper_weights + n_taper_weights);
    if (coef.ensure(w.size()) || meta.ensure((size_t)n_traces_) || rec.ensure(n_rec)) return 1;
    QM_HIP(copy_in(coef.p, w.data(), w.size() * sizeof(double), e->stream));
    QM_HIP(copy_in(meta.p, trace_filter, (size_t)n_traces_ * sizeof(int32_t), e->stream));
    QM_HIP(copy_in(rec.p, records, n_rec * sizeof(int64_t), e->stream));
    n_traces = n_traces_;
    max_n = 0;
    for (int i = 0; i < n_segments; ++i)
        max_n = std::max(max_n, (int)records[(size_t)i * qm::kSegmentFields + qm::kSegN]);
    args = qm::SegmentArgs{};
    args.trace_filter = meta.p;
    args.sos = coef.p;
    args.T = t_samples; args.n_records = n_segments; args.n_sections = n_sections;
    args.detrend = detrend ? 1 : 0; args.zero_phase = zero_phase ? 1 : 0;
    args.second_taper = second_taper ? 1 : 0;
    args.fill_value = fill_value;
    return 0;
}

int SegmentStage::adopt(const char *what, int repeat, const PreprocStage &pre, int32_t max_segments_,
                        int64_t max_taper_weights, int second_taper, double fill_value) {
    const double words = (double)pre.n_traces * pre.args.T + (double)qm::kSegmentFields * max_segments_ +
                         (double)max_taper_weights;
    if ((double)repeat * words * 8.0 >= 0x1p40 || (int64_t)repeat * max_segments_ >= INT32_MAX)
        return fail("%s: too many segments or taper weights per launch", what);
    sig_words = (size_t)pre.n_traces * pre.args.T;
    max_segments = max_segments_;
    max_weights = max_taper_weights;
    n_traces = pre.n_traces;
    max_n = pre.args.T;                                 // (a step's layout is not known before it is pushed)
    args = qm::SegmentArgs{};
    args.trace_filter = pre.args.trace_filter;          // (step 0's image: every step's traces have the same filters)
    args.sos = pre.args.sos;
    args.T = pre.args.T; args.n_records = max_segments; args.n_sections = pre.args.n_sections;
    args.detrend = pre.args.detrend; args.zero_phase = pre.args.zero_phase;
    args.second_taper = second_taper ? 1 : 0;
    args.fill_value = fill_value;
    return 0;
}

void SegmentStage::pack(double *dst, const double *signals, const int64_t *records, int32_t n_segments,
                        const double *weights, int64_t n_weights) const {
    host_copy(dst, signals, sig_words * sizeof(double));
    int64_t *rec_dst = reinterpret_cast<int64_t *>(dst + sig_words);
    const size_t used = (size_t)n_segments * qm::kSegmentFields, room = (size_t)max_segments * qm::kSegmentFields;
    std::memcpy(rec_dst, records, used * sizeof(int64_t));
    std::memset(rec_dst + used, 0, (room - used) * sizeof(int64_t));
    if (n_weights > 0) std::memcpy(dst + sig_words + room, weights, (size_t)n_weights * sizeof(double));
}

int SegmentStage::launch(qm_engine *e, const double *d_steps, double *d_signals, int n_steps) const {
    const int64_t step = (int64_t)step_words();
    const double *d_rec = d_steps + sig_words;
    return launch(e, d_steps, step, reinterpret_cast<const int64_t *>(d_rec), step,
                  d_rec + (size_t)max_segments * qm::kSegmentFields, step, d_signals, (int64_t)sig_words, n_steps);
}

int SegmentStage::launch(qm_engine *e, const double *in, int64_t in_step, const int64_t *records, int64_t rec_step,
                         const double *w, int64_t w_step, double *out, int64_t out_step, int n_steps) const {
    qm::SegmentArgs a = args;
    a.in = in; a.in_step = in_step;
    a.rec = records; a.rec_step = rec_step;
    a.taper_w = w; a.w_step = w_step;
    a.out = out; a.out_step = out_step;
    a.skew = e->cfg.preproc_skew;
    // one workgroup per record; LDS for the longest segment that fits (longer ones are worked on in their output rows)
    const size_t lds = (size_t)std::min(max_n, qm::kPreprocLdsSamples) * sizeof(double);
    return launch_with_lds(e, qm::segments_kernel, (unsigned)((int64_t)n_steps * a.n_records), 256, lds, a);
}

extern "C" {

int qm_engine_preprocess_segments(qm_engine *e, const double *signals, int signals_on_device, int32_t n_traces,
                                  int32_t t_samples, const int32_t *trace_filter, const double *sos,
                                  int32_t n_filters, int32_t n_sections, int detrend, int zero_phase,
                                  const int64_t *records, int32_t n_segments, const double *taper_weights,
                                  int64_t n_taper_weights, int second_taper, double fill_value, double *filtered,
                                  int out_on_device) {
    const char *what = "qm_engine_preprocess_segments";
    if (!e || !signals || !filtered) return fail("%s: NULL argument", what);
    DeviceGuard guard(e->device);
    SegmentStage &seg = e->seg_stage;
    if (seg.build(e, what, n_traces, t_samples, trace_filter, sos, n_filters, n_sections, detrend, zero_phase, records,
                  n_segments, taper_weights, n_taper_weights, second_taper, fill_value))
        return 1;
    const size_t sig = (size_t)n_traces * t_samples;
    const double *d_sig = stage_in(e, e->staging.sig, signals, signals_on_device, sig);
    if (!d_sig) return 1;
    const StagedOut<double> out = stage_host_out(e->staging.pre_out, filtered, out_on_device, sig);
    const double *d_w = seg.coef.p + (size_t)n_filters * n_sections * 6;
    if (!out.d || timed_launches(e, [&] { return seg.launch(e, d_sig, 0, seg.rec.p, 0, d_w, 0, out.d, 0, 1); }) ||
        out.fetch(e))
        return 1;
    if (!out_on_device) QM_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

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
