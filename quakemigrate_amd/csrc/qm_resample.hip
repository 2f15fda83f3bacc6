// qm_resample.hip -- the resampling stage's host side (kernel and its notes: qm_resample.hpp).  ResampleStage
// (qm_engine.hpp) is the stage: build checks the records and puts them on the device, launch runs the kernel over the
// (step, trace)s of a launch.  qm_engine_resample is the staged call on the engine's record; the pipeline
// (qm_stream.hip) holds a record of its own.
#define QM_TU_RESAMPLE 1
#include "qm_engine.hpp"

namespace {

// what build refuses; *max_kept: the longest kept series
int check_resample(const char *what, int raw_dtype, int64_t total_raw_samples, int32_t n_traces, int32_t t_samples,
                   const int64_t *records, const double *sos_lp, int32_t n_lowpass, int32_t n_sections_lp,
                   const int32_t *taper_table, int32_t n_tapers, const double *taper_weights, int64_t n_taper_weights,
                   int64_t *max_kept) {
    using namespace qm;
    if (!records) return fail("%s: NULL argument", what);
    if (raw_dtype != kRawInt32 && raw_dtype != kRawFloat64)
        return fail("%s: raw_dtype %d: 0 (int32) or 1 (float64)", what, raw_dtype);
    if (n_traces < 1 || t_samples < 1 || total_raw_samples < 1) return fail("%s: empty input", what);
    if (n_lowpass < 0 || n_tapers < 0 || n_taper_weights < 0 || (n_lowpass > 0 && !sos_lp) ||
        (n_tapers > 0 && !taper_table) || (n_taper_weights > 0 && !taper_weights))
        return fail("%s: %d low-passes, %d tapers, %lld taper weights without their arrays", what, n_lowpass, n_tapers,
                    (long long)n_taper_weights);
    if (check_sections(what, "low-pass", "n_sections_lp", sos_lp, n_lowpass, n_sections_lp) ||
        check_taper_table(what, taper_table, n_tapers, n_taper_weights))
        return 1;
    int64_t kept = 0;
    for (int i = 0; i < n_traces; ++i) {
        const int64_t *r = records + (size_t)i * kResampleFields;
        const int64_t n_raw = r[kRsNRaw], u = r[kRsUp], d = r[kRsDec], n_up = r[kRsNUp];
        if (n_raw < 1) return fail("%s: trace %d: n_raw = %lld, at least one raw sample is needed", what, i, (long long)n_raw);
        if (r[kRsRawOffset] < 0 || r[kRsRawOffset] + n_raw > total_raw_samples)
            return fail("%s: trace %d: raw samples [%lld, %lld) leave the raw buffer of %lld", what, i,
                        (long long)r[kRsRawOffset], (long long)(r[kRsRawOffset] + n_raw), (long long)total_raw_samples);
        if (u < 1 || u > INT32_MAX || d < 1 || d > INT32_MAX)
            return fail("%s: trace %d: up = %lld, dec = %lld: factors of at least 1", what, i, (long long)u, (long long)d);
        if (r[kRsPadLeft] < 0 || r[kRsPadRight] < 0 || r[kRsPadLeft] > INT32_MAX || r[kRsPadRight] > INT32_MAX ||
            (u == 1 && (r[kRsPadLeft] || r[kRsPadRight])))
            return fail("%s: trace %d: pads of %lld + %lld samples with up = %lld (pads go with an upsampling, >= 0)",
                        what, i, (long long)r[kRsPadLeft], (long long)r[kRsPadRight], (long long)u);
        const int64_t padded = r[kRsPadLeft] + (n_raw - 1) * u + 1 + r[kRsPadRight];
        if (n_raw > INT32_MAX || padded > INT32_MAX || n_up > INT32_MAX)     // (the kernel counts them in int)
            return fail("%s: trace %d: too many samples", what, i);
        if (r[kRsUpFirst] < 0 || n_up < 1 || r[kRsUpFirst] + n_up > padded)
            return fail("%s: trace %d: the kept slice [%lld, %lld) leaves the padded series of %lld samples", what, i,
                        (long long)r[kRsUpFirst], (long long)(r[kRsUpFirst] + n_up), (long long)padded);
        if (r[kRsOutFirst] < 0 || r[kRsOutFirst] + t_samples > (n_up + d - 1) / d)
            return fail("%s: trace %d: output samples [%lld, %lld) of %lld decimated ones (n_up = %lld, dec = %lld)",
                        what, i, (long long)r[kRsOutFirst], (long long)(r[kRsOutFirst] + t_samples),
                        (long long)((n_up + d - 1) / d), (long long)n_up, (long long)d);
        if (d > 1) {
            if (r[kRsLowpass] < 0 || r[kRsLowpass] >= n_lowpass)
                return fail("%s: trace %d: low-pass %lld out of range (%d low-passes)", what, i, (long long)r[kRsLowpass],
                            n_lowpass);
            if (r[kRsTaper] < 0 || r[kRsTaper] >= n_tapers)
                return fail("%s: trace %d: taper %lld out of range (%d tapers)", what, i, (long long)r[kRsTaper], n_tapers);
            const int64_t m = taper_table[2 * r[kRsTaper] + 1];
            if (2 * m > n_up)
                return fail("%s: trace %d: its taper's ramps cover 2 x %lld samples, the kept series holds %lld", what, i,
                            (long long)m, (long long)n_up);
        }
        kept = std::max(kept, n_up);
    }
    *max_kept = kept;
    return 0;
}

}  // namespace

int ResampleStage::build(qm_engine *e, const char *what, int repeat, int raw_dtype, int64_t total_raw_samples,
                         int32_t n_traces_, int32_t t_samples, const int64_t *records, const double *sos_lp,
                         int32_t n_lowpass, int32_t n_sections_lp, int detrend, const int32_t *taper_table,
                         int32_t n_tapers, const double *taper_weights, int64_t n_taper_weights) {
    int64_t kept = 0;
    if (check_resample(what, raw_dtype, total_raw_samples, n_traces_, t_samples, records, sos_lp, n_lowpass,
                       n_sections_lp, taper_table, n_tapers, taper_weights, n_taper_weights, &kept))
        return 1;
    const size_t width = raw_dtype == qm::kRawInt32 ? 4 : 8;
    const size_t bytes = (size_t)total_raw_samples * width, step = step_doubles(raw_dtype, total_raw_samples);
    // the records `repeat` times, step k reading k raw steps further on
    const size_t n_rec = (size_t)n_traces_ * qm::kResampleFields;
    std::vector<int64_t> image;
    for (int k = 0; k < repeat; ++k) {
        image.insert(image.end(), records, records + n_rec);
        for (int i = 0; i < n_traces_; ++i)
            image[((size_t)k * n_traces_ + i) * qm::kResampleFields + qm::kRsRawOffset] +=
                (int64_t)k * (int64_t)(step * 8 / width);
    }
    const size_t n_rec_all = image.size();
    image.insert(image.end(), taper_table, taper_table + 2 * (size_t)n_tapers);
    const size_t n_coef = (size_t)n_lowpass * n_sections_lp * 6;
    std::vector<double> w(sos_lp, sos_lp + n_coef);
    w.insert(w.end(), taper_weights, taper_weights + n_taper_weights);
    const bool spill = kept > qm::kPreprocLdsSamples;
    if (meta.ensure(image.size()) || coef.ensure(std::max<size_t>(w.size(), 1))) return 1;
    if (spill && scratch.ensure((size_t)repeat * n_traces_ * kept)) return 1;
    QM_HIP(copy_in(meta.p, image.data(), image.size() * sizeof(int64_t), e->stream));
    if (!w.empty()) QM_HIP(copy_in(coef.p, w.data(), w.size() * sizeof(double), e->stream));
    max_kept = kept;
    n_traces = n_traces_;
    raw_bytes = bytes;
    raw_step = step;
    args = qm::ResampleArgs{};
    args.rec = meta.p;
    args.tapers = meta.p + n_rec_all;
    args.sos = coef.p;
    args.taper_w = coef.p + n_coef;
    args.scratch = spill ? scratch.p : nullptr;
    args.scratch_stride = spill ? kept : 0;
    args.T = t_samples; args.n_sections = n_sections_lp; args.raw_dtype = raw_dtype;
    args.detrend = detrend ? 1 : 0;
    return 0;
}

int ResampleStage::launch(qm_engine *e, const void *raw, double *out, int n_steps) const {
    qm::ResampleArgs a = args;
    a.raw = raw;
    a.out = out;
    a.skew = e->cfg.preproc_skew;
    // one workgroup per trace; LDS for the longest kept series that fits (longer ones live in their scratch rows)
    const size_t lds = (size_t)std::min<int64_t>(max_kept, qm::kPreprocLdsSamples) * sizeof(double);
    return launch_with_lds(e, qm::resample_kernel, (unsigned)((int64_t)n_steps * n_traces), 256, lds, a);
}

extern "C" {

int qm_engine_resample(qm_engine *e, const void *raw, int raw_dtype, int raw_on_device, int64_t total_raw_samples,
                       int32_t n_traces, const int64_t *records, const double *sos_lp, int32_t n_lowpass,
                       int32_t n_sections_lp, int detrend, const int32_t *taper_table, int32_t n_tapers,
                       const double *taper_weights, int64_t n_taper_weights, int32_t t_samples, double *out,
                       int out_on_device) {
    if (!e || !raw || !out) return fail("qm_engine_resample: NULL argument");
    DeviceGuard guard(e->device);
    ResampleStage &rs = e->rs_stage;
    if (rs.build(e, "qm_engine_resample", 1, raw_dtype, total_raw_samples, n_traces, t_samples, records, sos_lp,
                 n_lowpass, n_sections_lp, detrend, taper_table, n_tapers, taper_weights, n_taper_weights))
        return 1;
    const size_t sig = (size_t)n_traces * t_samples;
    const void *d_raw = stage_in(e, e->staging.rs_raw, raw, raw_on_device, rs.raw_step, rs.raw_bytes);
    if (!d_raw) return 1;
    // (the resampled traces leave through the pre-processing call's output buffer: CallStaging)
    const StagedOut<double> res = stage_host_out(e->staging.pre_out, out, out_on_device, sig);
    if (!res.d || timed_launches(e, [&] { return rs.launch(e, d_raw, res.d, 1); }) || res.fetch(e)) return 1;
    if (!out_on_device) QM_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

}  // extern "C"
