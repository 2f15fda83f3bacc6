// qm_amplitudes.hip -- the amplitude stage's host side: argument checks, staging, the two launches (kernels and their
// notes: qm_amplitudes.hpp).  Records, filters, tapers and outputs are host arrays; the packed traces are the caller's,
// on the host or on the device.  The engine works on a copy of them (amps.work) whenever a trace is filtered or the
// traces come from the host; device traces without any filter are read where they are.
#define QM_TU_AMPLITUDES 1
#include "qm_engine.hpp"

extern "C" {

int qm_engine_measure_amplitudes(qm_engine *e, const double *traces, int traces_on_device, int64_t total_samples,
                                 int32_t n_traces, const int64_t *trace_records, const double *sos, int32_t n_filters,
                                 int32_t n_sections, const int32_t *taper_table, int32_t n_tapers,
                                 const double *taper_weights, int64_t n_taper_weights, int32_t n_windows,
                                 const int64_t *window_records, int detrend_windows, int average_method,
                                 double prominence_multiplier, double *values, int32_t *index, double *filtered_out) {
    using namespace qm;
    const char *what = "qm_engine_measure_amplitudes";
    if (!e || !traces || !trace_records || !window_records || !values || !index) return fail("%s: NULL argument", what);
    if (n_traces < 1 || n_windows < 1 || total_samples < 1)
        return fail("%s: empty input (%d traces, %d windows, %lld samples)", what, n_traces, n_windows,
                    (long long)total_samples);
    if (n_filters < 0 || n_tapers < 0 || n_taper_weights < 0 || (n_filters > 0 && !sos) ||
        (n_tapers > 0 && !taper_table) || (n_taper_weights > 0 && !taper_weights))
        return fail("%s: %d filters, %d tapers, %lld taper weights without their arrays", what, n_filters, n_tapers,
                    (long long)n_taper_weights);
    if (check_sections(what, "filter", "n_sections", sos, n_filters, n_sections) ||
        check_taper_table(what, taper_table, n_tapers, n_taper_weights))
        return 1;
    if (detrend_windows != 0 && detrend_windows != 1)
        return fail("%s: detrend_windows must be 0 or 1 (got %d)", what, detrend_windows);
    if (average_method != 0 && average_method != 1)
        return fail("%s: average_method must be 0 (RMS) or 1 (STD), got %d", what, average_method);
    if (!(prominence_multiplier >= 0.0) || !std::isfinite(prominence_multiplier))
        return fail("%s: prominence_multiplier must be finite and >= 0 (got %g)", what, prominence_multiplier);
    bool any_filter = false;
    int64_t longest_filtered = 0;
    for (int i = 0; i < n_traces; ++i) {
        const int64_t *r = trace_records + (size_t)i * kAmpTraceFields;
        if (r[1] < 1 || r[1] > INT32_MAX)
            return fail("%s: trace %d: %lld samples (1 .. 2^31 - 1)", what, i, (long long)r[1]);
        if (r[0] < 0 || r[0] > total_samples - r[1])
            return fail("%s: trace %d: samples [%lld, %lld) leave the buffer of %lld", what, i, (long long)r[0],
                        (long long)(r[0] + r[1]), (long long)total_samples);
        if (r[2] < -1 || r[2] >= n_filters)
            return fail("%s: trace %d: filter %lld out of range (%d filters, -1: none)", what, i, (long long)r[2],
                        n_filters);
        if (r[3] < -1 || r[3] >= n_tapers)
            return fail("%s: trace %d: taper %lld out of range (%d tapers, -1: none)", what, i, (long long)r[3],
                        n_tapers);
        if (r[2] >= 0) {
            any_filter = true;
            longest_filtered = std::max(longest_filtered, r[1]);
            if (r[3] >= 0 && 2 * (int64_t)taper_table[2 * r[3] + 1] > r[1])
                return fail("%s: trace %d: its taper's ramps cover 2 x %d samples, the trace holds %lld", what, i,
                            taper_table[2 * r[3] + 1], (long long)r[1]);
        }
    }
    if (any_filter) {
        // stage A filters in place: a filtered trace shares no sample with any other trace
        std::vector<int> order(n_traces);
        for (int i = 0; i < n_traces; ++i) order[i] = i;
        std::sort(order.begin(), order.end(), [&](int a, int b) {
            return trace_records[(size_t)a * kAmpTraceFields] < trace_records[(size_t)b * kAmpTraceFields];
        });
        int64_t reach = 0, reach_filtered = 0;          // ends of the traces so far, of the filtered ones among them
        for (int i : order) {
            const int64_t *r = trace_records + (size_t)i * kAmpTraceFields;
            if (r[0] < reach_filtered || (r[2] >= 0 && r[0] < reach))
                return fail("%s: trace %d: samples [%lld, %lld) overlap another trace and one of the two is filtered",
                            what, i, (long long)r[0], (long long)(r[0] + r[1]));
            reach = std::max(reach, r[0] + r[1]);
            if (r[2] >= 0) reach_filtered = std::max(reach_filtered, r[0] + r[1]);
        }
    }
    // the windows as the kernel reads them: first sample in the packed buffer, length, kind, lo, scratch slice
    std::vector<int64_t> wrec((size_t)n_windows * kAmpWindowFields);
    int64_t longest_lds = 0, scratch_doubles = 0;
    for (int w = 0; w < n_windows; ++w) {
        const int64_t *r = window_records + (size_t)w * 4;
        if (r[0] < 0 || r[0] >= n_traces) return fail("%s: window %d: trace %lld of %d", what, w, (long long)r[0], n_traces);
        const int64_t *tr = trace_records + (size_t)r[0] * kAmpTraceFields;
        if (r[1] < 0 || r[2] > tr[1] || r[1] > r[2])
            return fail("%s: window %d: samples [%lld, %lld) do not lie in trace %lld's %lld", what, w, (long long)r[1],
                        (long long)r[2], (long long)r[0], (long long)tr[1]);
        if (r[3] != 0 && r[3] != 1) return fail("%s: window %d: kind %lld: 0 (noise) or 1 (signal)", what, w, (long long)r[3]);
        const int64_t n = r[2] - r[1];
        int64_t *o = wrec.data() + (size_t)w * kAmpWindowFields;
        o[0] = tr[0] + r[1]; o[1] = n; o[2] = r[3]; o[3] = r[1]; o[4] = -1;
        if (n > kAmpLdsSamples) {
            o[4] = scratch_doubles;
            scratch_doubles += (int64_t)amp_scratch_doubles(n);
        } else {
            longest_lds = std::max(longest_lds, n);
        }
    }

    DeviceGuard guard(e->device);
    const size_t n_trec = (size_t)n_traces * kAmpTraceFields;
    std::vector<int64_t> meta(trace_records, trace_records + n_trec);
    for (int t = 0; t < 2 * n_tapers; ++t) meta.push_back(taper_table[t]);
    const size_t n_wrec0 = meta.size();
    meta.insert(meta.end(), wrec.begin(), wrec.end());
    const size_t n_coef = (size_t)n_filters * n_sections * 6;
    std::vector<double> coef;
    if (n_coef) coef.assign(sos, sos + n_coef);
    if (n_taper_weights) coef.insert(coef.end(), taper_weights, taper_weights + n_taper_weights);
    const size_t nw = (size_t)n_windows;
    const bool copy = any_filter || !traces_on_device;
    if (e->amps.meta.ensure(meta.size()) || e->amps.coef.ensure(std::max<size_t>(coef.size(), 1)) ||
        e->amps.val.ensure(nw * kAmpColumns) || e->amps.idx.ensure(nw * 4))
        return 1;
    if (copy && e->amps.work.ensure((size_t)total_samples)) return 1;
    if (scratch_doubles && e->amps.scratch.ensure((size_t)scratch_doubles)) return 1;
    QM_HIP(copy_in(e->amps.meta.p, meta.data(), meta.size() * sizeof(int64_t), e->stream));
    if (!coef.empty()) QM_HIP(copy_in(e->amps.coef.p, coef.data(), coef.size() * sizeof(double), e->stream));
    if (copy) {
        if (traces_on_device)
            QM_HIP(hipMemcpyAsync(e->amps.work.p, traces, (size_t)total_samples * sizeof(double),
                                  hipMemcpyDeviceToDevice, e->stream));
        else
            QM_HIP(copy_in(e->amps.work.p, traces, (size_t)total_samples * sizeof(double), e->stream));
    }
    AmpArgs a{};
    a.work = copy ? e->amps.work.p : const_cast<double *>(traces);     // (read only where nothing is filtered)
    a.traces = e->amps.meta.p;
    a.tapers = e->amps.meta.p + n_trec;
    a.windows = e->amps.meta.p + n_wrec0;
    a.sos = e->amps.coef.p;
    a.taper_w = e->amps.coef.p + n_coef;
    a.scratch = e->amps.scratch.p;
    a.values = e->amps.val.p;
    a.index = e->amps.idx.p;
    a.n_sections = n_sections; a.skew = e->cfg.preproc_skew;
    a.detrend_windows = detrend_windows; a.method = average_method; a.multiplier = prominence_multiplier;
    if (timed_launches(e, [&]() -> int {
            const size_t lds = (size_t)std::min<int64_t>(longest_filtered, kPreprocLdsSamples) * sizeof(double);
            if (any_filter && launch_with_lds(e, amp_filter_kernel, (unsigned)n_traces, 256, lds, a)) return 1;
            return launch_with_lds(e, amp_window_kernel, (unsigned)n_windows, kAmpWindowThreads,
                                   amp_lds_bytes(longest_lds), a);
        }))
        return 1;
    QM_HIP(copy_back(values, a.values, nw * kAmpColumns * sizeof(double), e->stream));
    QM_HIP(copy_back(index, a.index, nw * 4 * sizeof(int32_t), e->stream));
    if (filtered_out) QM_HIP(copy_back(filtered_out, a.work, (size_t)total_samples * sizeof(double), e->stream));
    QM_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

}  // extern "C"
