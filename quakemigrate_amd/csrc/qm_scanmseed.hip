// qm_scanmseed.hip -- the .scanmseed codec's host side: argument checks, staging, the launch sequences (kernels and
// their notes: qm_scanmseed.hpp).  Encode reads the channels' word and record counts and the refusals back before the
// output is sized, as the trigger does with its candidate count; decode reads its one error slot back after the launch.
#define QM_TU_SCANMSEED 1
#include "qm_engine.hpp"

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
    if (e->sms.bytes.ensure(2 * all) || e->sms.map.ensure(all_tiles * qm::kSmsMaxCount) ||
        e->sms.tile.ensure(2 * all_tiles) || e->sms.tot.ensure(2 * qm::kSmsChannels + qm::kSmsErrSlots))
        return 1;
    unsigned long long *d_tot = e->sms.tot.p, *d_err = d_tot + 2 * qm::kSmsChannels;
    QM_HIP(hipMemsetAsync(d_err, 0xff, qm::kSmsErrSlots * sizeof(unsigned long long), e->stream));

    // the stage clock always runs, and it rewrites its six times only at the end of a call that gets as far as
    // collect(): a refused call leaves the times of the call before
    auto &clock = e->sms.clock;
    clock.begin(true, false);
    hipStream_t s = e->stream;
    const bool is_float = series_dtype == 1;
    const double *d_in = nullptr;                       // float64: the series to quantise into sms.x
    const int32_t *d_x = nullptr;
    if (is_float) {
        d_in = stage_in(e, e->sms.f, static_cast<const double *>(series), series_on_device, all);
        d_x = d_in && !e->sms.x.ensure(all) ? e->sms.x.p : nullptr;
    } else {
        d_x = stage_in(e, e->sms.x, static_cast<const int32_t *>(series), series_on_device, all);
    }
    if (!d_x) return 1;

    qm::SmsEncodeArgs a{};
    a.x = d_x; a.n = (int)n; a.tiles = tiles;
    a.count = e->sms.bytes.p; a.codes = e->sms.bytes.p + all;
    a.map = e->sms.map.p;
    a.entry = e->sms.tile.p; a.word0 = e->sms.tile.p + all_tiles;
    a.totals = d_tot; a.err = d_err;
    unsigned long long h[2 * qm::kSmsChannels + qm::kSmsErrSlots];
    size_t R = 0;
    const dim3 per_tile((unsigned)tiles, qm::kSmsChannels), threads(qm::kSmsThreads);
    const auto sequence = [&]() -> int {
        if (is_float) {
            qm::SmsQuantArgs q{};
            q.in = d_in; q.out = e->sms.x.p; q.n = (int)n; q.err = d_err;
            for (int c = 0; c < qm::kSmsChannels; ++c) {
                q.factor[c] = factors[c];
                q.clip[c] = clips[c];
            }
            const unsigned blocks = (unsigned)std::min<size_t>((N + qm::kSmsThreads - 1) / qm::kSmsThreads, 4096);
            if (clock.launch(s, qm::kSmsQuantise, qm::sms_quantise_kernel, dim3(blocks, qm::kSmsChannels), threads, 0, q))
                return 1;
        }
        if (clock.launch(s, qm::kSmsScan, qm::sms_scan_kernel, per_tile, threads, 0, a) ||
            clock.launch(s, qm::kSmsCompose, qm::sms_compose_kernel, dim3(qm::kSmsChannels), threads, 0, a))
            return 1;
        QM_HIP(copy_back(h, d_tot, sizeof(h), s));
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
        R = (size_t)total;
        if (e->sms.out.ensure(R * qm::kSmsRecU32) || e->sms.rec.ensure(2 * R)) return 1;
        a.out = e->sms.out.p;
        a.rec_first = e->sms.rec.p;
        a.rec_count = e->sms.rec.p + R;
        QM_HIP(hipMemsetAsync(a.out, 0, R * qm::kSmsRecLen, s));
        return clock.launch(s, qm::kSmsPack, qm::sms_pack_kernel, per_tile, threads, 0, a) ||
               clock.launch(s, qm::kSmsFrame, qm::sms_frame_kernel, dim3((unsigned)R), dim3(64), 0, a);
    };
    if (timed_launches(e, sequence)) return 1;
    QM_HIP(copy_back(records, a.out, R * qm::kSmsRecLen, e->stream));
    QM_HIP(copy_back(rec_first, a.rec_first, R * sizeof(int32_t), e->stream));
    QM_HIP(copy_back(rec_count, a.rec_count, R * sizeof(int32_t), e->stream));
    QM_HIP(hipStreamSynchronize(e->stream));
    if (clock.collect()) return 1;
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
    if (e->sms.out.ensure(R * qm::kSmsRecU32) || e->sms.rec.ensure(R) || e->sms.off.ensure(R) ||
        e->sms.tot.ensure(2 * qm::kSmsChannels + qm::kSmsErrSlots))
        return 1;
    if (want_f && e->sms.fac.ensure(R)) return 1;
    const StagedOut<int32_t> ints = stage_host_out(e->sms.x, out, out_on_device, NT);
    StagedOut<double> floats;                           // (no out_f64: nothing staged, floats.d stays NULL)
    if (!ints.d || (want_f && !(floats = stage_host_out(e->sms.f, out_f64, out_on_device, NT)).d)) return 1;
    unsigned long long *d_err = e->sms.tot.p + 2 * qm::kSmsChannels;
    QM_HIP(hipMemsetAsync(d_err, 0xff, qm::kSmsErrSlots * sizeof(unsigned long long), e->stream));
    QM_HIP(copy_in(e->sms.out.p, records, R * qm::kSmsRecLen, e->stream));
    QM_HIP(copy_in(e->sms.rec.p, rec_samples, R * sizeof(int32_t), e->stream));
    QM_HIP(copy_in(e->sms.off.p, rec_offset, R * sizeof(int64_t), e->stream));
    if (want_f) QM_HIP(copy_in(e->sms.fac.p, rec_factor, R * sizeof(double), e->stream));

    qm::SmsDecodeArgs a{};
    a.rec = e->sms.out.p; a.rec_n = e->sms.rec.p; a.rec_out = e->sms.off.p;
    a.rec_factor = want_f ? e->sms.fac.p : nullptr;
    a.out = ints.d;
    a.outf = floats.d;
    a.err = d_err;
    auto &clock = e->sms.clock;
    clock.begin(true, false);                           // (as in encode: always on, times rewritten by collect() only)
    if (timed_launches(e, [&] {
            return clock.launch(e->stream, qm::kSmsDecode, qm::sms_decode_kernel, dim3((unsigned)R), dim3(qm::kSmsThreads), 0, a);
        }))
        return 1;
    unsigned long long h_err[qm::kSmsErrSlots];
    QM_HIP(copy_back(h_err, d_err, sizeof(h_err), e->stream));
    if (clock.collect()) return 1;
    const unsigned long long bad = h_err[qm::kSmsErrDecode];
    if (bad != kSmsNone) {
        const long long r = (long long)(bad / 4);
        switch ((int)(bad % 4)) {
            case qm::kSmsBadCode: return fail("%s: record %lld: invalid STEIM2 code / dnib pair", what, r);
            case qm::kSmsShort: return fail("%s: record %lld holds fewer differences than samples", what, r);
            default: return fail("%s: record %lld: STEIM2 reverse integration constant mismatch", what, r);
        }
    }
    if (ints.fetch(e) || floats.fetch(e)) return 1;
    if (!out_on_device) QM_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

}  // extern "C"
