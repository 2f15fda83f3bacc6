// qm_picks.hip -- the phase-pick stage's host side: argument checks, staging, the launch (kernel and its notes:
// qm_picks.hpp).  Windows, groups, half-widths and thresholds are host arrays; the onset rows are the caller's, on
// the host or left on the device by qm_engine_onsets.
#define QM_TU_PICKS 1
#include "qm_engine.hpp"

extern "C" {

int qm_engine_pick_phases(qm_engine *e, const double *onsets, int onsets_on_device, int32_t n_rows,
                          int32_t t_samples, const int32_t *windows, const int32_t *row_group, double sampling_rate,
                          const double *halfwidth, int threshold_mode, double mad_multiplier,
                          const double *thresholds_in, double *picks, int32_t *status) {
    const char *what = "qm_engine_pick_phases";
    if (!e || !onsets || !windows || !row_group || !halfwidth || !picks || !status)
        return fail("%s: NULL argument", what);
    if (n_rows < 1 || t_samples < 1) return fail("%s: empty input (%d rows of %d samples)", what, n_rows, t_samples);
    if (t_samples > qm::kPicksLdsSamples)
        return fail("%s: rows of %d samples, a workgroup's LDS holds %d (\"pick_lds_samples\")", what, t_samples,
                    qm::kPicksLdsSamples);
    if (!(sampling_rate > 0.0)) return fail("%s: sampling_rate must be positive (got %g)", what, sampling_rate);
    if (threshold_mode != 0 && threshold_mode != 1)
        return fail("%s: threshold_mode must be 0 (MAD) or 1 (given thresholds), got %d", what, threshold_mode);
    if (threshold_mode == 1 && !thresholds_in) return fail("%s: threshold_mode 1 without thresholds_in", what);
    for (int r = 0; r < n_rows; ++r) {
        const int32_t lo = windows[3 * r], hi = windows[3 * r + 2];
        if (lo < 0 || hi > t_samples || lo > hi)
            return fail("%s: row %d: window [%d, %d) does not lie in the row's %d samples", what, r, lo, hi,
                        t_samples);
    }
    DeviceGuard guard(e->device);
    const size_t n = (size_t)n_rows, sig = n * t_samples;
    // one buffer of doubles (half-widths, thresholds, then the picks), one of integers (windows, groups, status)
    std::vector<double> val(halfwidth, halfwidth + n);
    if (threshold_mode == 1) val.insert(val.end(), thresholds_in, thresholds_in + n);
    std::vector<int32_t> meta(windows, windows + 3 * n);
    meta.insert(meta.end(), row_group, row_group + n);
    if (!stage_in(e, e->picks.val, val.data(), 0, n * (2 + qm::kPicksColumns), val.size() * sizeof(double)) ||
        !stage_in(e, e->picks.meta, meta.data(), 0, n * 5, meta.size() * sizeof(int32_t)))
        return 1;
    const double *d_on = stage_in(e, e->staging.sig, onsets, onsets_on_device, sig);
    if (!d_on) return 1;
    qm::PickArgs a{};
    a.onsets = d_on;
    a.windows = e->picks.meta.p;
    a.row_group = e->picks.meta.p + 3 * n;
    a.status = e->picks.meta.p + 4 * n;
    a.halfwidth = e->picks.val.p;
    a.thresholds_in = threshold_mode == 1 ? e->picks.val.p + n : nullptr;
    a.picks = e->picks.val.p + 2 * n;
    a.n_rows = n_rows; a.T = t_samples; a.mode = threshold_mode;
    a.rate = sampling_rate; a.mad_multiplier = mad_multiplier;
    const size_t lds = qm::picks_lds_bytes(t_samples);
    if (timed_launches(e, [&] {
            return launch_with_lds(e, qm::pick_phases_kernel, (unsigned)n_rows, qm::kPicksThreads, lds, a);
        }))
        return 1;
    QM_HIP(copy_back(picks, a.picks, n * qm::kPicksColumns * sizeof(double), e->stream));
    QM_HIP(copy_back(status, a.status, n * sizeof(int32_t), e->stream));
    QM_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

}  // extern "C"
