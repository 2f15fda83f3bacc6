// qm_trigger.hip -- the trigger stage's host side: argument checks, staging, the launch sequence (kernels and their
// notes: qm_trigger.hpp).  The candidate count comes back to the host before the per-candidate buffers are sized, the
// event count before the events are copied: two small read-backs inside the call.
#define QM_TU_TRIGGER 1
#include "qm_engine.hpp"

// "trigger_timing": an event before (side 0) and after (side 1) a stage of the sequence
static int trig_mark(qm_engine *e, int stage, int side, bool (&ran)[qm::kTrigStages]) {
    if (!e->cfg.trigger_timing) return 0;
    while (e->trg_ev.size() < 2 * (size_t)qm::kTrigStages) {
        Event ev;
        QM_HIP(ev.create());
        e->trg_ev.push_back(std::move(ev));
    }
    QM_HIP(hipEventRecord(e->trg_ev[2 * stage + side], e->stream));
    if (side) ran[stage] = true;
    return 0;
}
#define QM_TRIG_STAGE(stage, ...)                              \
    do {                                                       \
        if (trig_mark(e, stage, 0, ran)) return 1;             \
        __VA_ARGS__;                                           \
        QM_HIP(hipGetLastError());                             \
        if (trig_mark(e, stage, 1, ran)) return 1;             \
    } while (0)

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
    if (e->d_trg_x.ensure(smooth ? 4 * N : 2 * N) || e->d_trg_par.ensure((size_t)r + 1 + n_chunks) ||
        e->d_trg_cnt.ensure(5 * (size_t)nblocks) || e->d_trg_tot.ensure(4))
        return 1;
    double *d_raw = e->d_trg_x.p, *d_w = e->d_trg_par.p, *d_thr = e->d_trg_par.p + r + 1;
    if (resident) {
        QM_HIP(hipMemcpyAsync(d_raw, coa, N * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
        QM_HIP(hipMemcpyAsync(d_raw + N, coa_n, N * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    } else {
        QM_HIP(copy_in(d_raw, coa, N * sizeof(double), e->stream));
        QM_HIP(copy_in(d_raw + N, coa_n, N * sizeof(double), e->stream));
    }
    if (smooth) QM_HIP(copy_in(d_w, p->smooth_weights, ((size_t)r + 1) * sizeof(double), e->stream));
    if (!dynamic) QM_HIP(copy_in(d_thr, &p->threshold_value, sizeof(double), e->stream));

    bool ran[qm::kTrigStages] = {};
    for (int64_t &ns : e->trg_ns) ns = 0;
    QM_HIP(hipEventRecord(e->ev0, e->stream));
    const double *d_series = d_raw;
    if (smooth) {
        qm::TrigSmoothArgs a{d_raw, d_w, d_raw + 2 * N, (int)n, r};
        const size_t lds = qm::trig_smooth_lds_bytes(r);
        QM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&qm::trig_smooth_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        const unsigned tiles = (unsigned)((N + qm::kTrigSmoothTile - 1) / qm::kTrigSmoothTile);
        QM_TRIG_STAGE(qm::kTrigSmooth, hipLaunchKernelGGL(qm::trig_smooth_kernel, dim3(tiles, 2),
                                                           dim3(qm::kTrigSmoothThreads), lds, e->stream, a));
        d_series = d_raw + 2 * N;
    }
    const double *d_coa = d_series, *d_coa_n = d_series + N;
    const double *d_trig = p->trigger_on ? d_coa_n : d_coa;
    if (dynamic) {
        qm::TrigStatArgs a{d_trig, d_thr, (int)n, chunk, p->threshold_method, p->threshold_value};
        const int threads = chunk <= qm::kTrigStatSmall ? 256 : qm::kTrigStatThreads;
        QM_TRIG_STAGE(qm::kTrigStats, hipLaunchKernelGGL(qm::trig_stat_kernel, dim3((unsigned)n_chunks), dim3(threads),
                                                          0, e->stream, a));
    }
    qm::TrigRunArgs ra{};
    ra.raw = d_raw; ra.trig = d_trig; ra.thr = d_thr;
    ra.n = (int)n; ra.chunk = chunk; ra.nblocks = nblocks;
    ra.counts = e->d_trg_cnt.p; ra.offsets = e->d_trg_cnt.p + 3 * (size_t)nblocks; ra.totals = e->d_trg_tot.p;
    QM_TRIG_STAGE(qm::kTrigRuns,
                  hipLaunchKernelGGL(qm::trig_count_kernel, dim3((unsigned)nblocks), dim3(qm::kTrigRunThreads), 0,
                                     e->stream, ra);
                  hipLaunchKernelGGL(qm::trig_scan_kernel, dim3(1), dim3(qm::kTrigRunThreads), 0, e->stream, ra));
    int64_t totals[4] = {0, 0, 0, 0};
    QM_HIP(copy_back(totals, e->d_trg_tot.p, sizeof(totals), e->stream));
    if (totals[2] > 0)
        return fail("%s: %lld non-finite samples in the two series (the reference would trigger nothing on NaN "
                    "thresholds)", what, (long long)totals[2]);
    if (totals[0] != totals[1])
        return fail("%s: %lld run starts, %lld run ends", what, (long long)totals[0], (long long)totals[1]);
    const int64_t nc = totals[0];
    if (candidates && nc > max_candidates)
        return fail("%s: %lld candidates, the candidate table has room for %lld", what, (long long)nc,
                    (long long)max_candidates);
    int64_t ne = 0;
    if (nc > 0) {
        const size_t C = (size_t)nc;
        if (e->d_trg_run.ensure(2 * C) || e->d_trg_cand.ensure((qm::kTrigCandColumns + qm::kTrigEventInts) * C) ||
            e->d_trg_val.ensure((1 + qm::kTrigEventValues) * C))
            return 1;
        ra.first = e->d_trg_run.p;
        ra.last = e->d_trg_run.p + C;
        QM_TRIG_STAGE(qm::kTrigCompact, hipLaunchKernelGGL(qm::trig_compact_kernel, dim3((unsigned)nblocks),
                                                            dim3(qm::kTrigRunThreads), 0, e->stream, ra));
        qm::TrigPeakArgs pa{};
        pa.coa = d_coa; pa.coa_n = d_coa_n; pa.trig = d_trig;
        pa.first = ra.first; pa.last = ra.last;
        pa.cand = e->d_trg_cand.p; pa.ev_i = e->d_trg_cand.p + qm::kTrigCandColumns * C;
        pa.cval = e->d_trg_val.p; pa.ev_f = e->d_trg_val.p + C;
        pa.totals = e->d_trg_tot.p;
        pa.nc = (int)nc; pa.period = p->period_ns; pa.mw = p->mw_ns; pa.mei = p->mei_ns;
        QM_TRIG_STAGE(qm::kTrigPeaks, hipLaunchKernelGGL(qm::trig_peak_kernel, dim3((unsigned)((nc + 3) / 4)), dim3(256),
                                                          0, e->stream, pa));
        QM_TRIG_STAGE(qm::kTrigMerge, hipLaunchKernelGGL(qm::trig_merge_kernel, dim3(1), dim3(qm::kTrigMergeThreads), 0,
                                                          e->stream, pa));
        QM_HIP(copy_back(&ne, e->d_trg_tot.p + 3, sizeof(ne), e->stream));
    }
    QM_HIP(hipEventRecord(e->ev1, e->stream));
    e->timed = true;
    if (ne > max_events)
        return fail("%s: %lld events, the event tables have room for %lld (max_events)", what, (long long)ne,
                    (long long)max_events);
    if (ne > 0) {
        const size_t C = (size_t)nc;
        QM_HIP(copy_back(events_i, e->d_trg_cand.p + qm::kTrigCandColumns * C,
                         (size_t)ne * qm::kTrigEventInts * sizeof(int64_t), e->stream));
        QM_HIP(copy_back(events_f, e->d_trg_val.p + C, (size_t)ne * qm::kTrigEventValues * sizeof(double),
                         e->stream));
    }
    if (candidates && nc > 0)
        QM_HIP(copy_back(candidates, e->d_trg_cand.p, (size_t)nc * qm::kTrigCandColumns * sizeof(int64_t),
                         e->stream));
    if (thresholds) QM_HIP(copy_back(thresholds, d_thr, n_chunks * sizeof(double), e->stream));
    if (smoothed && smooth) QM_HIP(copy_back(smoothed, d_raw + 2 * N, 2 * N * sizeof(double), e->stream));
    QM_HIP(hipStreamSynchronize(e->stream));
    for (int st = 0; st < qm::kTrigStages; ++st) {
        if (!ran[st]) continue;
        float ms = 0.0f;
        QM_HIP(hipEventElapsedTime(&ms, e->trg_ev[2 * st], e->trg_ev[2 * st + 1]));
        e->trg_ns[st] = (int64_t)((double)ms * 1e6);
    }
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
