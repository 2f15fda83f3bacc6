// stage_build_check.cpp -- the three front-end stage records' build() on the CPU, under the sanitizers: their
// refusals and the images they put on the "device" for repeat = 1 and 3; then the two checks the trace stages share
// (check_sections, check_taper_table: qm_engine.hpp), every refusal with its whole message; then the step a stream's
// segment feed holds -- SegmentStage::adopt, step_words and pack into a malloc of exactly that size.  A stand-alone host program: the runtime's
// pool and copies are replaced below by malloc and memcpy, so no device is needed and every image lands in an
// allocation of exactly the size build() asked for (an overrun is an AddressSanitizer report).  No kernel is launched.
// The records own their device arrays: once they and the engine are gone, no block of the pool is out.
//
//   cd quakemigrate_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined qm_preproc.hip qm_resample.hip qm_widen.hip \
//         ../../tools/stage_build_check.cpp -o /tmp/stage_build_check && /tmp/stage_build_check
//
// Prints one line per stage and "stage_build_check: ok"; any mismatch or sanitizer report ends it with a non-zero status.
#include "../quakemigrate_amd/csrc/qm_engine.hpp"

static std::string g_error;
int fail(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_error = buf;
    return 1;
}
static long g_blocks_out = 0;
hipError_t pool_alloc(void **out, size_t bytes) {
    *out = std::malloc(bytes);
    if (*out) ++g_blocks_out;
    return *out ? hipSuccess : hipErrorOutOfMemory;
}
void pool_free(void *p) {
    --g_blocks_out;
    std::free(p);
}
// (the engine's pinned ring and events are never made here: nothing to give back)
hipError_t pinned_alloc(void **, size_t, unsigned) { return hipErrorNotSupported; }
void pinned_free(void *) {}
hipError_t event_create(hipEvent_t *, unsigned) { return hipErrorNotSupported; }
void event_destroy(hipEvent_t) {}
hipError_t copy_in(void *dst, const void *src, size_t bytes, hipStream_t) {
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t copy_back(void *dst, const void *src, size_t bytes, hipStream_t) {
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
void host_copy(void *dst, const void *src, size_t n) { std::memcpy(dst, src, n); }
PoolReleaseScope::PoolReleaseScope() {}
PoolReleaseScope::~PoolReleaseScope() {}

#define CHECK(cond)                                                                         \
    do {                                                                                    \
        if (!(cond)) {                                                                      \
            std::fprintf(stderr, "stage_build_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                   \
        }                                                                                   \
    } while (0)
#define REFUSED(call, text)                                        \
    do {                                                           \
        g_error.clear();                                           \
        CHECK((call) != 0);                                        \
        CHECK(g_error.find(text) != std::string::npos);            \
    } while (0)

static void stages() {
    std::unique_ptr<qm_engine> engine(new qm_engine());
    qm_engine *e = engine.get();
    const int T = 100, n_traces = 5, n_rows = 3;

    // -- pre-processing ------------------------------------------------------------------------------------------
    const int32_t filter[n_traces] = {0, 1, 0, 1, 0};
    std::vector<double> sos(2 * 2 * 6, 0.5), left(7, 0.25), right(4, 0.75);
    for (int k = 0; k < 4; ++k) sos[6 * k + 3] = 1.0;
    PreprocStage pre;
    auto pre_build = [&](int repeat, const int32_t *f, const double *s, int n_sections, int n_left) {
        return pre.build(e, "pre", repeat, n_traces, T, f, s, 2, n_sections, 1, left.data(), n_left, right.data(),
                         (int)right.size(), 1);
    };
    REFUSED(pre_build(3, filter, sos.data(), 9, 7), "n_sections");
    const int32_t bad_filter[n_traces] = {0, 1, 2, 1, 0};
    REFUSED(pre_build(3, bad_filter, sos.data(), 2, 7), "out of range");
    REFUSED(pre_build(3, filter, sos.data(), 2, T), "tapers cover");
    std::vector<double> bad_sos = sos;
    bad_sos[6 + 3] = 2.0;
    REFUSED(pre_build(3, filter, bad_sos.data(), 2, 7), "a0");
    REFUSED(pre_build(3, nullptr, sos.data(), 2, 7), "NULL");
    for (int repeat : {3, 1, 3}) {                              // (grown, reused, reused)
        CHECK(pre_build(repeat, filter, sos.data(), 2, 7) == 0);
        for (int k = 0; k < repeat; ++k)
            for (int i = 0; i < n_traces; ++i) CHECK(pre.args.trace_filter[k * n_traces + i] == filter[i]);
        CHECK(std::equal(sos.begin(), sos.end(), pre.args.sos));
        CHECK(std::equal(left.begin(), left.end(), pre.args.taper_left));
        CHECK(std::equal(right.begin(), right.end(), pre.args.taper_right));
        CHECK(pre.n_traces == n_traces && pre.args.T == T && pre.args.n_left == 7 && pre.args.n_right == 4);
    }
    std::printf("pre-processing: 5 refusals, images for repeat = 3, 1, 3\n");

    // -- onsets --------------------------------------------------------------------------------------------------
    const int32_t row[n_traces] = {0, 0, 1, 2, 2}, nsta[n_rows] = {4, 6, 5}, nlta[n_rows] = {17, 23, 20};
    OnsetStage on;
    auto on_build = [&](int repeat, const int32_t *r, int transform, int position) {
        return on.build(e, "on", repeat, n_traces, T, r, n_rows, nsta, nlta, transform, position, 3, 0.3);
    };
    const int32_t orphan[n_traces] = {0, 0, 1, 1, 1}, outside[n_traces] = {0, 0, 1, 2, 3};
    REFUSED(on_build(3, orphan, 0, 0), "row 2 has no trace");
    REFUSED(on_build(3, outside, 0, 0), "trace 4: row out of range");
    REFUSED(on_build(3, row, 2, 0), "transform");
    REFUSED(on_build(3, row, 0, 3), "position");
    REFUSED(on_build(3, nullptr, 0, 0), "NULL");
    REFUSED(on.build(e, "on", 3, 0, T, row, n_rows, nsta, nlta, 0, 0, 3, 0.3), "empty input");
    for (int repeat : {3, 1, 3}) {
        CHECK(on_build(repeat, row, 1, 2) == 0);
        for (int k = 0; k < repeat; ++k) {
            for (int i = 0; i < n_traces; ++i) CHECK(on.args.trace_row[k * n_traces + i] == k * n_rows + row[i]);
            for (int r = 0; r < n_rows; ++r)
                CHECK(on.args.nsta[k * n_rows + r] == nsta[r] && on.args.nlta[k * n_rows + r] == nlta[r]);
        }
        CHECK(on.args.nsta == on.args.trace_row + repeat * n_traces && on.args.nlta == on.args.nsta + repeat * n_rows);
        CHECK(on.sta.n >= (size_t)repeat * n_traces * T && on.lta.n >= (size_t)repeat * n_traces * T);
        std::memset(on.args.sta, 0, (size_t)repeat * n_traces * T * sizeof(double));   // (all of it is the record's)
        std::memset(on.args.lta, 0, (size_t)repeat * n_traces * T * sizeof(double));
        CHECK(on.n_traces == n_traces && on.n_rows == n_rows && on.args.transform == 1 && on.args.position == 2);
    }
    std::printf("onsets: 6 refusals, images for repeat = 3, 1, 3\n");

    // -- resampling: two traces, a pass-through slice and a decimation by 2; 251 raw samples (an odd count: an int32
    //    step is rounded up to whole doubles)
    using namespace qm;
    const int n_rs = 2, total = 251;
    int64_t rec[n_rs * kResampleFields] = {};
    auto field = [&](int64_t *records, int i, int f) -> int64_t & { return records[i * kResampleFields + f]; };
    for (int i = 0; i < n_rs; ++i) field(rec, i, kRsUp) = field(rec, i, kRsDec) = 1;
    field(rec, 0, kRsRawOffset) = 0; field(rec, 0, kRsNRaw) = 50; field(rec, 0, kRsNUp) = 50;
    field(rec, 1, kRsRawOffset) = 50; field(rec, 1, kRsNRaw) = 201; field(rec, 1, kRsNUp) = 201;
    field(rec, 1, kRsDec) = 2;
    const int32_t tapers[2] = {0, 10};
    std::vector<double> lp(6, 0.5), weights(20, 0.5);
    lp[3] = 1.0;
    ResampleStage rs;
    auto rs_build = [&](int repeat, int dtype, const int64_t *records, int t_samples) {
        return rs.build(e, "rs", repeat, dtype, total, n_rs, t_samples, records, lp.data(), 1, 1, 1, tapers, 1,
                        weights.data(), (int64_t)weights.size());
    };
    int64_t bad[n_rs * kResampleFields];
    std::copy(std::begin(rec), std::end(rec), bad);
    field(bad, 1, kRsDec) = 0;
    REFUSED(rs_build(3, kRawInt32, bad, 50), "factors of at least 1");
    std::copy(std::begin(rec), std::end(rec), bad);
    field(bad, 1, kRsNRaw) = 202;
    REFUSED(rs_build(3, kRawInt32, bad, 50), "leave the raw buffer");
    REFUSED(rs_build(3, 2, rec, 50), "raw_dtype 2");
    REFUSED(rs_build(3, kRawInt32, rec, 0), "empty input");
    REFUSED(rs_build(3, kRawInt32, rec, 51), "decimated ones");
    REFUSED(rs_build(3, kRawInt32, nullptr, 50), "NULL");
    for (int dtype : {(int)kRawInt32, (int)kRawFloat64})
        for (int repeat : {3, 1, 3}) {
            CHECK(rs_build(repeat, dtype, rec, 50) == 0);
            const int64_t step = dtype == kRawInt32 ? 252 : 251;        // raw elements between two steps
            CHECK(rs.raw_bytes == (size_t)total * (dtype == kRawInt32 ? 4 : 8) && rs.raw_step == (rs.raw_bytes + 7) / 8);
            for (int k = 0; k < repeat; ++k)
                for (int i = 0; i < n_rs; ++i)
                    for (int f = 0; f < kResampleFields; ++f)
                        CHECK(rs.args.rec[(k * n_rs + i) * kResampleFields + f] ==
                              field(rec, i, f) + (f == kRsRawOffset ? k * step : 0));
            CHECK(rs.args.tapers == rs.args.rec + repeat * n_rs * kResampleFields);
            CHECK(rs.args.tapers[0] == 0 && rs.args.tapers[1] == 10);
            CHECK(std::equal(lp.begin(), lp.end(), rs.args.sos) && std::equal(weights.begin(), weights.end(), rs.args.taper_w));
            CHECK(rs.max_kept == 201 && rs.args.scratch == nullptr && rs.args.scratch_stride == 0 && rs.n_traces == n_rs);
        }
    // no low-pass, no taper, no weights: the coefficient buffer is never empty
    field(rec, 1, kRsDec) = 1;
    CHECK(rs.build(e, "rs", 2, kRawFloat64, total, n_rs, 50, rec, nullptr, 0, 1, 0, nullptr, 0, nullptr, 0) == 0);
    CHECK(rs.coef.n >= 1);
    std::printf("resampling: 6 refusals, images for int32 and float64, repeat = 3, 1, 3\n");

    // -- the checks the trace stages share (the amplitude entry point calls them as well): every refusal, whole message
    auto refused_with = [&](int rc, const char *text) { return rc != 0 && g_error == text; };
    CHECK(refused_with(check_sections("amp", "filter", "n_sections", sos.data(), 2, 0),
                       "amp: n_sections must be in 1..8 (got 0)"));
    CHECK(refused_with(check_sections("rs", "low-pass", "n_sections_lp", sos.data(), 2, 9),
                       "rs: n_sections_lp must be in 1..8 (got 9)"));
    CHECK(refused_with(check_sections("amp", "filter", "n_sections", bad_sos.data(), 2, 2),
                       "amp: filter 0, section 1: a0 = 2, sections must be normalised to a0 == 1"));
    CHECK(refused_with(check_sections("rs", "low-pass", "n_sections_lp", bad_sos.data(), 4, 1),
                       "rs: low-pass 1, section 0: a0 = 2, sections must be normalised to a0 == 1"));
    CHECK(check_sections("amp", "filter", "n_sections", nullptr, 0, 1) == 0);      // (no filter: nothing is read)
    CHECK(check_sections("pre", "filter", "n_sections", sos.data(), 2, 2) == 0);
    const int32_t table[6] = {0, 10, 20, 0, 4, 8};
    CHECK(check_taper_table("amp", table, 3, 20) == 0);
    CHECK(refused_with(check_taper_table("amp", table, 3, 19), "amp: taper 0: 2 x 10 weights from 0 on, 19 weights given"));
    const int32_t negative[4] = {-1, 2, 0, -3};
    CHECK(refused_with(check_taper_table("rs", negative, 2, 20), "rs: taper 0: 2 x 2 weights from -1 on, 20 weights given"));
    CHECK(refused_with(check_taper_table("rs", negative + 2, 1, 20), "rs: taper 0: 2 x -3 weights from 0 on, 20 weights given"));
    CHECK(check_taper_table("rs", nullptr, 0, 0) == 0);
    std::printf("shared checks: 7 refusals, whole messages\n");

    // -- the segment feed's step: adopt() from the pre-processing stage built above, pack() into exactly step_words()
    //    words pre-filled with a marker -- an overrun is a sanitizer report
    const size_t sig = (size_t)n_traces * T;
    std::vector<double> signals(sig), w_in(6);
    for (size_t i = 0; i < sig; ++i) signals[i] = 1.0 + (double)i;
    for (size_t i = 0; i < w_in.size(); ++i) w_in[i] = 0.125 * (double)(i + 1);
    const int max_seg = 3;
    int64_t seg_rec[max_seg * kSegmentFields];
    for (int i = 0; i < max_seg * kSegmentFields; ++i) seg_rec[i] = 100 + i;
    double marker;
    std::memset(&marker, 0xA5, sizeof(marker));
    auto same_bits = [](double a, double b) { return std::memcmp(&a, &b, sizeof(a)) == 0; };
    SegmentStage seg;
    REFUSED(seg.adopt("seg", 3, pre, max_seg, (int64_t)1 << 40, 1, 0.5), "too many segments or taper weights per launch");
    REFUSED(seg.adopt("seg", 2, pre, INT32_MAX / 2 + 1, 0, 1, 0.5), "too many segments or taper weights per launch");
    // (a) every record and every weight; (b) one segment, no weights; (c) as (b), a feed without room for weights
    struct { int64_t max_w; int32_t n_seg; int64_t n_w; } const cases[3] = {{6, max_seg, 6}, {6, 1, 0}, {0, 1, 0}};
    for (const auto &c : cases) {
        CHECK(seg.adopt("seg", 3, pre, max_seg, c.max_w, 1, 0.5) == 0);
        CHECK(seg.sig_words == sig && seg.max_segments == max_seg && seg.max_weights == c.max_w);
        CHECK(seg.step_words() == sig + (size_t)max_seg * kSegmentFields + (size_t)c.max_w);
        CHECK(seg.step_bytes() == seg.step_words() * 8 && seg.args.n_records == max_seg && seg.args.T == T);
        CHECK(seg.args.trace_filter == pre.args.trace_filter && seg.args.sos == pre.args.sos && seg.n_traces == n_traces);
        double *dst = static_cast<double *>(std::malloc(seg.step_words() * 8));
        CHECK(dst != nullptr);
        for (size_t i = 0; i < seg.step_words(); ++i) dst[i] = marker;
        seg.pack(dst, signals.data(), seg_rec, c.n_seg, c.n_w > 0 ? w_in.data() : nullptr, c.n_w);
        CHECK(std::equal(signals.begin(), signals.end(), dst));
        int64_t got[max_seg * kSegmentFields];
        std::memcpy(got, dst + sig, sizeof(got));
        for (int i = 0; i < max_seg * kSegmentFields; ++i) CHECK(got[i] == (i < c.n_seg * kSegmentFields ? seg_rec[i] : 0));
        const double *w_out = dst + sig + max_seg * kSegmentFields;
        for (int64_t i = 0; i < c.max_w; ++i) CHECK(same_bits(w_out[i], i < c.n_w ? w_in[(size_t)i] : marker));
        std::free(dst);
    }
    std::printf("segment feed: 2 refusals, adopt, step_words and pack for 3 + 6, 1 + 0 of 6, 1 + 0 of 0\n");

    CHECK(g_blocks_out > 0);
}

int main() {
    stages();
    CHECK(g_blocks_out == 0);                           // (the records and the engine went out of scope)
    std::printf("stage_build_check: ok\n");
    return 0;
}
