// qm_trigger.hip -- the trigger stage's host side: argument checks, staging, the launch sequence (kernels and their
// notes: qm_trigger.hpp).  The candidate count comes back to the host before the per-candidate buffers are sized, the
// event count before the events are copied: two small read-backs inside the call.
#define QM_TU_TRIGGER 1
#include "qm_engine.hpp"

// the two public calls: `resident` -- the series are on the engine's GPU already (device to device on the stream)
static int trigger_run(qm_engine *e, const char *what, bool resident, const double *coa, const double *coa_n, int64_t n,
                       const qm_trigger_params *p, int64_t max_events, int64_t *n_candidates, int64_t *n_events,
                       int64_t *events_i, double *events_f, double *thresholds, double *smoothed, int64_t *candidates,
                       int64_t max_candidates) {
    if (!e || !coa || !coa_n || !p || !n_candidates || !n_events || !events_i || !events_f)
        return fail("%s: NULL argument", what);
    if (n < 1) return fail("%s: empty input (%lld samples)", what, (long long)n);
    if (n > qm::kTrigMaxSamples)
        return fail("%s: %lld samples, at most %lld are taken", what, (long long)n, (long long)qm::kTrigMaxSamples);
    if (p->trigger_on != 0 && p->trigger_on != 1)
        return fail("%s: trigger_on must be 0 (COA) or 1 (COA_N), got %d", what, p->trigger_on);
    if (p->threshold_method < 0 || p->threshold_method > 2)
        return fail("%s: threshold_method must be 0 (static), 1 (MAD) or 2 (median ratio), got %d", what,
                    p->threshold_method);
    if (p->threshold_method != 0 && p->chunk_samples < 1)
        return fail("%s: chunk_samples must be at least 1 under a dynamic threshold (got %lld)", what,
                    (long long)p->chunk_samples);
    const bool smooth = p->smooth_weights != nullptr;
    if (smooth && (p->smooth_radius < 0 || p->smooth_radius > qm::kTrigMaxRadius))
        return fail("%s: smoothing radius %d outside 0..%d (\"trigger_max_radius\")", what, p->smooth_radius,
                    qm::kTrigMaxRadius);
    if (p->period_ns < 1) return fail("%s: period_ns must be positive (got %lld)", what, (long long)p->period_ns);
    if (p->mw_ns < 0 || p->mei_ns < 2 * p->mw_ns)
        return fail("%s: mei_ns (%lld) must be at least 2 mw_ns (mw_ns = %lld, not negative)", what,
                    (long long)p->mei_ns, (long long)p->mw_ns);
    if (max_events < 0 || (candidates && max_candidates < 0))
        return fail("%s: negative capacity (max_events %lld, max_candidates %lld)", what, (long long)max_events,
                    (long long)max_candidates);

    DeviceGuard guard(e->device);
    const size_t N = (size_t)n;
    const int r = smooth ? p->smooth_radius : 0;
    const bool dynamic = p->threshold_method != 0;
    // (a chunk longer than the series is the series: one chunk)
    const int chunk = dynamic ? (int)std::min<int64_t>(p->chunk_samples, n) : (int)n;
    const size_t n_chunks = (N + chunk - 1) / chunk;
    const int nblocks = (int)((N + qm::kTrigRunBlock - 1) / qm::kTrigRunBlock);
    if (e->trig.x.ensure(smooth ? 4 * N : 2 * N) || e->trig.par.ensure((size_t)r + 1 + n_chunks) ||
        e->trig.cnt.ensure(5 * (size_t)nblocks) || e->trig.tot.ensure(4))
        return 1;
    double *d_raw = e->trig.x.p, *d_w = e->trig.par.p, *d_thr = e->trig.par.p + r + 1;
    if (resident) {
        QM_HIP(hipMemcpyAsync(d_raw, coa, N * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
        QM_HIP(hipMemcpyAsync(d_raw + N, coa_n, N * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    } else {
        QM_HIP(copy_in(d_raw, coa, N * sizeof(double), e->stream));
        QM_HIP(copy_in(d_raw + N, coa_n, N * sizeof(double), e->stream));
    }
    if (smooth) QM_HIP(copy_in(d_w, p->smooth_weights, ((size_t)r + 1) * sizeof(double), e->stream));
    if (!dynamic) QM_HIP(copy_in(d_thr, &p->threshold_value, sizeof(double), e->stream));

    // the stage clock runs under "trigger_timing" only, and its times read 0 from here on: a call that fails below
    // leaves zeros, not the call before's times
    auto &clock = e->trig.clock;
    clock.begin(e->cfg.trigger_timing != 0, true);
    hipStream_t s = e->stream;
    int64_t nc = 0, ne = 0;
    const auto sequence = [&]() -> int {
        const double *d_series = d_raw;
        if (smooth) {
            qm::TrigSmoothArgs a{d_raw, d_w, d_raw + 2 * N, (int)n, r};
            const size_t lds = qm::trig_smooth_lds_bytes(r);
            QM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&qm::trig_smooth_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            const unsigned tiles = (unsigned)((N + qm::kTrigSmoothTile - 1) / qm::kTrigSmoothTile);
            if (clock.launch(s, qm::kTrigSmooth, qm::trig_smooth_kernel, dim3(tiles, 2), dim3(qm::kTrigSmoothThreads), lds, a))
                return 1;
            d_series = d_raw + 2 * N;
        }
        const double *d_coa = d_series, *d_coa_n = d_series + N;
        const double *d_trig = p->trigger_on ? d_coa_n : d_coa;
        if (dynamic) {
            qm::TrigStatArgs a{d_trig, d_thr, (int)n, chunk, p->threshold_method, p->threshold_value};
            const int threads = chunk <= qm::kTrigStatSmall ? 256 : qm::kTrigStatThreads;
            if (clock.launch(s, qm::kTrigStats, qm::trig_stat_kernel, dim3((unsigned)n_chunks), dim3(threads), 0, a)) return 1;
        }
        qm::TrigRunArgs ra{};
        ra.raw = d_raw; ra.trig = d_trig; ra.thr = d_thr;
        ra.n = (int)n; ra.chunk = chunk; ra.nblocks = nblocks;
        ra.counts = e->trig.cnt.p; ra.offsets = e->trig.cnt.p + 3 * (size_t)nblocks; ra.totals = e->trig.tot.p;
        const dim3 run_blocks((unsigned)nblocks), run_threads(qm::kTrigRunThreads);
        if (clock.stage(s, qm::kTrigRuns, [&] {
                hipLaunchKernelGGL(qm::trig_count_kernel, run_blocks, run_threads, 0, s, ra);
                hipLaunchKernelGGL(qm::trig_scan_kernel, dim3(1), run_threads, 0, s, ra);
            }))
            return 1;
        int64_t totals[4] = {0, 0, 0, 0};
        QM_HIP(copy_back(totals, e->trig.tot.p, sizeof(totals), s));
        if (totals[2] > 0)
            return fail("%s: %lld non-finite samples in the two series (the reference would trigger nothing on NaN "
                        "thresholds)", what, (long long)totals[2]);
        if (totals[0] != totals[1])
            return fail("%s: %lld run starts, %lld run ends", what, (long long)totals[0], (long long)totals[1]);
        nc = totals[0];
        if (candidates && nc > max_candidates)
            return fail("%s: %lld candidates, the candidate table has room for %lld", what, (long long)nc,
                        (long long)max_candidates);
        if (nc == 0) return 0;
        const size_t C = (size_t)nc;
        if (e->trig.run.ensure(2 * C) || e->trig.cand.ensure((qm::kTrigCandColumns + qm::kTrigEventInts) * C) ||
            e->trig.val.ensure((1 + qm::kTrigEventValues) * C))
            return 1;
        ra.first = e->trig.run.p;
        ra.last = e->trig.run.p + C;
        if (clock.launch(s, qm::kTrigCompact, qm::trig_compact_kernel, run_blocks, run_threads, 0, ra)) return 1;
        qm::TrigPeakArgs pa{};
        pa.coa = d_coa; pa.coa_n = d_coa_n; pa.trig = d_trig;
        pa.first = ra.first; pa.last = ra.last;
        pa.cand = e->trig.cand.p; pa.ev_i = e->trig.cand.p + qm::kTrigCandColumns * C;
        pa.cval = e->trig.val.p; pa.ev_f = e->trig.val.p + C;
        pa.totals = e->trig.tot.p;
        pa.nc = (int)nc; pa.period = p->period_ns; pa.mw = p->mw_ns; pa.mei = p->mei_ns;
        if (clock.launch(s, qm::kTrigPeaks, qm::trig_peak_kernel, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, pa) ||
            clock.launch(s, qm::kTrigMerge, qm::trig_merge_kernel, dim3(1), dim3(qm::kTrigMergeThreads), 0, pa))
            return 1;
        QM_HIP(copy_back(&ne, e->trig.tot.p + 3, sizeof(ne), s));
        return 0;
    };
    if (timed_launches(e, sequence)) return 1;
    if (ne > max_events)
        return fail("%s: %lld events, the event tables have room for %lld (max_events)", what, (long long)ne,
                    (long long)max_events);
    if (ne > 0) {
        const size_t C = (size_t)nc;
        QM_HIP(copy_back(events_i, e->trig.cand.p + qm::kTrigCandColumns * C,
                         (size_t)ne * qm::kTrigEventInts * sizeof(int64_t), s));
        QM_HIP(copy_back(events_f, e->trig.val.p + C, (size_t)ne * qm::kTrigEventValues * sizeof(double), s));
    }
    if (candidates && nc > 0)
        QM_HIP(copy_back(candidates, e->trig.cand.p, (size_t)nc * qm::kTrigCandColumns * sizeof(int64_t), s));
    if (thresholds) QM_HIP(copy_back(thresholds, d_thr, n_chunks * sizeof(double), s));
    if (smoothed && smooth) QM_HIP(copy_back(smoothed, d_raw + 2 * N, 2 * N * sizeof(double), s));
    QM_HIP(hipStreamSynchronize(s));
    if (clock.collect()) return 1;
    *n_candidates = nc;
    *n_events = ne;
    return 0;
}

extern "C" {

int qm_engine_trigger(qm_engine *e, const double *coa, const double *coa_n, int64_t n, const qm_trigger_params *p,
                      int64_t max_events, int64_t *n_candidates, int64_t *n_events, int64_t *events_i,
                      double *events_f, double *thresholds, double *smoothed, int64_t *candidates,
                      int64_t max_candidates) {
    return trigger_run(e, "qm_engine_trigger", false, coa, coa_n, n, p, max_events, n_candidates, n_events, events_i,
                       events_f, thresholds, smoothed, candidates, max_candidates);
}

int qm_engine_trigger_resident(qm_engine *e, const double *coa, const double *coa_n, int64_t n,
                               const qm_trigger_params *p, int64_t max_events, int64_t *n_candidates,
                               int64_t *n_events, int64_t *events_i, double *events_f, double *thresholds,
                               double *smoothed, int64_t *candidates, int64_t max_candidates) {
    return trigger_run(e, "qm_engine_trigger_resident", true, coa, coa_n, n, p, max_events, n_candidates, n_events,
                       events_i, events_f, thresholds, smoothed, candidates, max_candidates);
}

}  // extern "C"
