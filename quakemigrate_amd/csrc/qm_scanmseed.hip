// qm_scanmseed.hip -- the .scanmseed codec's host side: argument checks, staging, the launch sequences (kernels and
// their notes: qm_scanmseed.hpp).  Encode reads the channels' word and record counts and the refusals back before the
// output is sized, as the trigger does with its candidate count; decode reads its one error slot back after the launch.
#define QM_TU_SCANMSEED 1
#include "qm_engine.hpp"

// an event before (side 0) and after (side 1) a stage: "scanmseed_ns_<stage>"
static int sms_mark(qm_engine *e, int stage, int side, bool (&ran)[qm::kSmsStages]) {
    while (e->sms_ev.size() < 2 * (size_t)qm::kSmsStages) {
        Event ev;
        QM_HIP(ev.create());
        e->sms_ev.push_back(std::move(ev));
    }
    QM_HIP(hipEventRecord(e->sms_ev[2 * stage + side], e->stream));
    if (side) ran[stage] = true;
    return 0;
}
#define QM_SMS_STAGE(stage, ...)                               \
    do {                                                       \
        if (sms_mark(e, stage, 0, ran)) return 1;              \
        __VA_ARGS__;                                           \
        QM_HIP(hipGetLastError());                             \
        if (sms_mark(e, stage, 1, ran)) return 1;              \
    } while (0)

static int sms_times(qm_engine *e, const bool (&ran)[qm::kSmsStages]) {
    for (int st = 0; st < qm::kSmsStages; ++st) {
        e->sms_ns[st] = 0;
        if (!ran[st]) continue;
        float ms = 0.0f;
        QM_HIP(hipEventElapsedTime(&ms, e->sms_ev[2 * st], e->sms_ev[2 * st + 1]));
        e->sms_ns[st] = (int64_t)((double)ms * 1e6);
    }
    return 0;
}

static const char *const kSmsChannelNames[qm::kSmsChannels] = {"COA", "COA_N", "X", "Y", "Z"};
constexpr unsigned long long kSmsNone = ~0ull;

extern "C" {

int qm_engine_scanmseed_encode(qm_engine *e, const void *series, int series_dtype, int series_on_device, int64_t n,
                               const double *factors, const double *clips, int64_t max_records, int64_t *n_records,
                               uint8_t *records, int32_t *rec_first, int32_t *rec_count) {
    const char *what = "qm_engine_scanmseed_encode";
    if (!e || !series || !n_records || !records || !rec_first || !rec_count) return fail("%s: NULL argument", what);
    if (series_dtype != 0 && series_dtype != 1)
        return fail("%s: series_dtype must be 0 (int32) or 1 (float64), got %d", what, series_dtype);
    if (series_dtype == 1 && (!factors || !clips))
        return fail("%s: NULL argument (float64 series need factors and clips)", what);
    if (n < 1) return fail("%s: empty input (%lld samples)", what, (long long)n);
    if (n > qm::kSmsMaxSamples)
        return fail("%s: %lld samples per channel, at most %lld are taken", what, (long long)n,
                    (long long)qm::kSmsMaxSamples);
    if (max_records < 0) return fail("%s: negative capacity (max_records %lld)", what, (long long)max_records);
    if (series_dtype == 1)
        for (int c = 0; c < qm::kSmsChannels; ++c)
            if (!std::isfinite(factors[c]) || clips[c] != clips[c])
                return fail("%s: channel %s: factor %.17g, clip %.17g (a finite factor and a clip or +infinity "
                            "expected)", what, kSmsChannelNames[c], factors[c], clips[c]);

    DeviceGuard guard(e->device);
    const size_t N = (size_t)n, all = qm::kSmsChannels * N;
    const int tiles = (int)((N + qm::kSmsTile - 1) / qm::kSmsTile);
    const size_t all_tiles = (size_t)qm::kSmsChannels * tiles;
    if (e->d_sms_bytes.ensure(2 * all) || e->d_sms_map.ensure(all_tiles * qm::kSmsMaxCount) ||
        e->d_sms_tile.ensure(2 * all_tiles) || e->d_sms_tot.ensure(2 * qm::kSmsChannels + qm::kSmsErrSlots))
        return 1;
    unsigned long long *d_tot = e->d_sms_tot.p, *d_err = d_tot + 2 * qm::kSmsChannels;
    QM_HIP(hipMemsetAsync(d_err, 0xff, qm::kSmsErrSlots * sizeof(unsigned long long), e->stream));

    bool ran[qm::kSmsStages] = {};
    const int32_t *d_x = nullptr;
    const bool is_float = series_dtype == 1;
    if (is_float) {
        const double *d_in = static_cast<const double *>(series);
        if (!series_on_device) {
            if (e->d_sms_f.ensure(all)) return 1;
            QM_HIP(copy_in(e->d_sms_f.p, series, all * sizeof(double), e->stream));
            d_in = e->d_sms_f.p;
        }
        if (e->d_sms_x.ensure(all)) return 1;
        QM_HIP(hipEventRecord(e->ev0, e->stream));
        qm::SmsQuantArgs q{};
        q.in = d_in; q.out = e->d_sms_x.p; q.n = (int)n; q.err = d_err;
        for (int c = 0; c < qm::kSmsChannels; ++c) {
            q.factor[c] = factors[c];
            q.clip[c] = clips[c];
        }
        const unsigned blocks = (unsigned)std::min<size_t>((N + qm::kSmsThreads - 1) / qm::kSmsThreads, 4096);
        QM_SMS_STAGE(qm::kSmsQuantise, hipLaunchKernelGGL(qm::sms_quantise_kernel, dim3(blocks, qm::kSmsChannels),
                                                           dim3(qm::kSmsThreads), 0, e->stream, q));
        d_x = e->d_sms_x.p;
    } else if (series_on_device) {
        d_x = static_cast<const int32_t *>(series);
        QM_HIP(hipEventRecord(e->ev0, e->stream));
    } else {
        if (e->d_sms_x.ensure(all)) return 1;
        QM_HIP(copy_in(e->d_sms_x.p, series, all * sizeof(int32_t), e->stream));
        d_x = e->d_sms_x.p;
        QM_HIP(hipEventRecord(e->ev0, e->stream));
    }

    qm::SmsEncodeArgs a{};
    a.x = d_x; a.n = (int)n; a.tiles = tiles;
    a.count = e->d_sms_bytes.p; a.codes = e->d_sms_bytes.p + all;
    a.map = e->d_sms_map.p;
    a.entry = e->d_sms_tile.p; a.word0 = e->d_sms_tile.p + all_tiles;
    a.totals = d_tot; a.err = d_err;
    QM_SMS_STAGE(qm::kSmsScan, hipLaunchKernelGGL(qm::sms_scan_kernel, dim3((unsigned)tiles, qm::kSmsChannels),
                                                   dim3(qm::kSmsThreads), 0, e->stream, a));
    QM_SMS_STAGE(qm::kSmsCompose, hipLaunchKernelGGL(qm::sms_compose_kernel, dim3(qm::kSmsChannels),
                                                      dim3(qm::kSmsThreads), 0, e->stream, a));
    unsigned long long h[2 * qm::kSmsChannels + qm::kSmsErrSlots];
    QM_HIP(copy_back(h, d_tot, sizeof(h), e->stream));
    const unsigned long long *h_err = h + 2 * qm::kSmsChannels;
    auto where = [&](unsigned long long at, const char **ch, long long *pos) {
        *ch = kSmsChannelNames[at / N];
        *pos = (long long)(at % N);
    };
    const char *ch;
    long long pos;
    if (h_err[qm::kSmsErrNaN] != kSmsNone) {
        where(h_err[qm::kSmsErrNaN], &ch, &pos);
        return fail("%s: channel %s, sample %lld is NaN: not quantised (NumPy's cast to int32 is platform-defined there)",
                    what, ch, pos);
    }
    if (h_err[qm::kSmsErrRange] != kSmsNone) {
        where(h_err[qm::kSmsErrRange], &ch, &pos);
        return fail("%s: channel %s, sample %lld: the scaled value is outside int32: not quantised (NumPy's cast to "
                    "int32 is platform-defined there)", what, ch, pos);
    }
    if (h_err[qm::kSmsErrDiff] != kSmsNone) {
        where(h_err[qm::kSmsErrDiff], &ch, &pos);
        return fail("%s: channel %s, sample %lld: difference does not fit 30 bits: not STEIM2-encodable", what, ch,
                    pos);
    }
    int64_t total = 0;
    for (int c = 0; c < qm::kSmsChannels; ++c) {
        a.rec_off[c] = (int)total;
        a.words[c] = (int)h[c];
        total += (int64_t)h[qm::kSmsChannels + c];
    }
    a.rec_off[qm::kSmsChannels] = (int)total;
    if (total > max_records)
        return fail("%s: %lld records, the output has room for %lld (max_records)", what, (long long)total,
                    (long long)max_records);
    const size_t R = (size_t)total;
    if (e->d_sms_out.ensure(R * qm::kSmsRecU32) || e->d_sms_rec.ensure(2 * R)) return 1;
    a.out = e->d_sms_out.p;
    a.rec_first = e->d_sms_rec.p;
    a.rec_count = e->d_sms_rec.p + R;
    QM_HIP(hipMemsetAsync(a.out, 0, R * qm::kSmsRecLen, e->stream));
    QM_SMS_STAGE(qm::kSmsPack, hipLaunchKernelGGL(qm::sms_pack_kernel, dim3((unsigned)tiles, qm::kSmsChannels),
                                                   dim3(qm::kSmsThreads), 0, e->stream, a));
    QM_SMS_STAGE(qm::kSmsFrame, hipLaunchKernelGGL(qm::sms_frame_kernel, dim3((unsigned)R), dim3(64), 0, e->stream, a));
    QM_HIP(hipEventRecord(e->ev1, e->stream));
    e->timed = true;
    QM_HIP(copy_back(records, a.out, R * qm::kSmsRecLen, e->stream));
    QM_HIP(copy_back(rec_first, a.rec_first, R * sizeof(int32_t), e->stream));
    QM_HIP(copy_back(rec_count, a.rec_count, R * sizeof(int32_t), e->stream));
    QM_HIP(hipStreamSynchronize(e->stream));
    if (sms_times(e, ran)) return 1;
    for (int c = 0; c < qm::kSmsChannels; ++c) n_records[c] = (int64_t)h[qm::kSmsChannels + c];
    return 0;
}

int qm_engine_scanmseed_decode(qm_engine *e, const uint8_t *records, int64_t n_records, const int32_t *rec_samples,
                               const int64_t *rec_offset, const double *rec_factor, int64_t n_total, int32_t *out,
                               double *out_f64, int out_on_device) {
    const char *what = "qm_engine_scanmseed_decode";
    if (!e || !records || !rec_samples || !rec_offset || !out) return fail("%s: NULL argument", what);
    if (out_f64 && !rec_factor) return fail("%s: NULL argument (out_f64 needs rec_factor)", what);
    if (n_records < 1 || n_records > INT32_MAX)
        return fail("%s: %lld records (1 .. 2^31 - 1 are taken)", what, (long long)n_records);
    if (n_total < 1) return fail("%s: empty output (n_total %lld)", what, (long long)n_total);
    for (int64_t r = 0; r < n_records; ++r) {
        if (rec_samples[r] < 1)
            return fail("%s: record %lld: %d samples", what, (long long)r, rec_samples[r]);
        if (rec_samples[r] > qm::kSmsRecMaxSamples)
            return fail("%s: record %lld holds fewer differences than samples (%d samples, a record holds at most %d)",
                        what, (long long)r, rec_samples[r], qm::kSmsRecMaxSamples);
        if (rec_offset[r] < 0 || rec_offset[r] > n_total - rec_samples[r])
            return fail("%s: record %lld: %d samples from %lld on leave the output of %lld", what, (long long)r,
                        rec_samples[r], (long long)rec_offset[r], (long long)n_total);
        if (out_f64 && !(rec_factor[r] == rec_factor[r]) )
            return fail("%s: record %lld: factor is NaN", what, (long long)r);
    }

    DeviceGuard guard(e->device);
    const size_t R = (size_t)n_records, NT = (size_t)n_total;
    const bool want_f = out_f64 != nullptr;
    if (e->d_sms_out.ensure(R * qm::kSmsRecU32) || e->d_sms_rec.ensure(R) || e->d_sms_off.ensure(R) ||
        e->d_sms_tot.ensure(2 * qm::kSmsChannels + qm::kSmsErrSlots))
        return 1;
    if (want_f && e->d_sms_fac.ensure(R)) return 1;
    if (!out_on_device && (e->d_sms_x.ensure(NT) || (want_f && e->d_sms_f.ensure(NT)))) return 1;
    unsigned long long *d_err = e->d_sms_tot.p + 2 * qm::kSmsChannels;
    QM_HIP(hipMemsetAsync(d_err, 0xff, qm::kSmsErrSlots * sizeof(unsigned long long), e->stream));
    QM_HIP(copy_in(e->d_sms_out.p, records, R * qm::kSmsRecLen, e->stream));
    QM_HIP(copy_in(e->d_sms_rec.p, rec_samples, R * sizeof(int32_t), e->stream));
    QM_HIP(copy_in(e->d_sms_off.p, rec_offset, R * sizeof(int64_t), e->stream));
    if (want_f) QM_HIP(copy_in(e->d_sms_fac.p, rec_factor, R * sizeof(double), e->stream));

    qm::SmsDecodeArgs a{};
    a.rec = e->d_sms_out.p; a.rec_n = e->d_sms_rec.p; a.rec_out = e->d_sms_off.p;
    a.rec_factor = want_f ? e->d_sms_fac.p : nullptr;
    a.out = out_on_device ? out : e->d_sms_x.p;
    a.outf = !want_f ? nullptr : out_on_device ? out_f64 : e->d_sms_f.p;
    a.err = d_err;
    bool ran[qm::kSmsStages] = {};
    QM_HIP(hipEventRecord(e->ev0, e->stream));
    QM_SMS_STAGE(qm::kSmsDecode, hipLaunchKernelGGL(qm::sms_decode_kernel, dim3((unsigned)R), dim3(qm::kSmsThreads), 0,
                                                     e->stream, a));
    QM_HIP(hipEventRecord(e->ev1, e->stream));
    e->timed = true;
    unsigned long long h_err[qm::kSmsErrSlots];
    QM_HIP(copy_back(h_err, d_err, sizeof(h_err), e->stream));
    if (sms_times(e, ran)) return 1;
    const unsigned long long bad = h_err[qm::kSmsErrDecode];
    if (bad != kSmsNone) {
        const long long r = (long long)(bad / 4);
        switch ((int)(bad % 4)) {
            case qm::kSmsBadCode: return fail("%s: record %lld: invalid STEIM2 code / dnib pair", what, r);
            case qm::kSmsShort: return fail("%s: record %lld holds fewer differences than samples", what, r);
            default: return fail("%s: record %lld: STEIM2 reverse integration constant mismatch", what, r);
        }
    }
    if (!out_on_device) {
        QM_HIP(copy_back(out, e->d_sms_x.p, NT * sizeof(int32_t), e->stream));
        if (want_f) QM_HIP(copy_back(out_f64, e->d_sms_f.p, NT * sizeof(double), e->stream));
        QM_HIP(hipStreamSynchronize(e->stream));
    }
    return 0;
}

}  // extern "C"
