// qm_engine.hpp -- internal header of the engine's host side (not installed; the C ABI is
// include/qmhip.h).  The host runtime is split by what it deals with:
//   qm_runtime.hip   error text, pooled streams, the pinned bounce buffers, the device-memory pool
//   qm_config.hip    the tunables: one record, one table with a row per key, config_set / config_get (qm_config.hpp;
//                    plain host C++)
//   qm_tables.hip    everything derived from ONE travel-time table: load, layout search, the kernels'
//                    derived tables (round-2 offsets, paired, shift-reuse, screening), parked tables,
//                    on-device serving
//   qm_engine.hip    engine handle, tunables, read-outs (one table: kReadouts), the stacking launch (run_stack:
//                    plan_stack decides into a StackPlan, issue_stack enqueues it, e->last keeps it), one core per launch
//                    kind and the step entry points around them (detect / detect_batch / partial / finalize / migrate /
//                    marginal / find_max_coa)
//   qm_screen.hip    the opt-in screened detect's launch sequence
//   qm_stream.hip    the continuous detect pipeline: one lane per engine (StreamLane: pinned ring, copies overlapped
//                    with compute), launches round-robin over the lanes; a stream on one engine is the one-lane case
//   qm_widen.hip     the rows next to the path: onset stage (OnsetStage), locate fits, RBF peak
//   qm_preproc.hip   the row before the onset stage: detrend, taper, zero-phase band-pass of the component traces
//                    (PreprocStage), and its segmented form for gappy traces (SegmentStage)
//   qm_resample.hip  the row before that: raw traces, each at its own rate and length, upsampled and decimated to the
//                    scan rate (ResampleStage)
//                    -- each of the three: the stage's record below (checks, device arrays, launch), shared by the
//                    engine's staged call, which lives beside it, and the pipeline
//   qm_picks.hip     the row after the location: phase picks, a Gaussian fitted to every onset row of an event
//   qm_trigger.hip   the row after the detect sweep: coalescence series in, triggered events out
//   qm_scanmseed.hip the file between the detect sweep and the trigger: the day's five series to and from the STEIM2
//                    records of a .scanmseed file (encode, decode)
//   qm_amplitudes.hip  the row after the picks: local-magnitude amplitudes, filtered traces and time windows in,
//                    peak-to-trough measurements out
//   qm_traveltimes.hip  the table the engine is built around: travel-time grids for a homogeneous medium, eikonal
//                    sections of 1-D models and their sweep round the stations
//   qm_compat.hip    the five reference-signature symbols (qmlib.h:28-44)
//   qm_group.hip     engine groups: one process driving the boxes of a column partition on several devices
// Whose scratch is whose: the stacking scratch and the serving grids are the engine's own members (folds, ties, streams
// and groups read them); every other call family has a record below (the front-end stages', PickStage ... CallStaging)
// whose comments name what is shared.  Host arrays pass through stage_in / stage_host_out, timed launches through
// timed_launches, a sequence's per-stage times through StageClock.
// Who frees what: nobody by name.  Device buffers, pinned host buffers and events are the owning handles below
// (DevBuf, PinnedBuf, Event); the structs here hold them as members and have no release lists.  What a teardown
// still does itself -- one wait, the right device, the order -- stands with the handles.
// Everything declared here lives in the library only (hidden visibility).
#pragma once
#include "../../include/qmhip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <variant>
#include <vector>

#include "qm_config.hpp"
#include "qm_kernels.hpp"
#include "qm_launch.hpp"
#include "qm_screen.hpp"
#include "qm_pair.hpp"
#include "qm_shift.hpp"
#include "qm_ties.hpp"
#include "qm_preproc.hpp"
#include "qm_resample.hpp"
#include "qm_picks.hpp"
#include "qm_trigger.hpp"
#include "qm_amplitudes.hpp"
#include "qm_scanmseed.hpp"
#include "qm_traveltimes.hpp"

#pragma GCC visibility push(hidden)

// ---- qm_runtime.hip ---------------------------------------------------------------------------
int fail(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
void clear_error();
const char *error_text();

#define QM_HIP(call)                                                                         \
    do {                                                                                     \
        hipError_t err__ = (call);                                                           \
        if (err__ != hipSuccess)                                                             \
            return fail("%s failed: %s (%s:%d)", #call, hipGetErrorString(err__), __FILE__,   \
                        __LINE__);                                                           \
    } while (0)
// HIP status of a launcher of qm_launch.hpp -> the same error convention
#define QM_TABLE(call) QM_HIP(call)

hipError_t acquire_stream(int device, hipStream_t *out);
void park_stream(int device, hipStream_t s);
hipError_t copy_back(void *dst, const void *src, size_t bytes, hipStream_t s);
hipError_t copy_in(void *dst, const void *src, size_t bytes, hipStream_t s);
// `pieces` consecutive device pieces of `bytes` each to `pieces` separate host destinations: one DMA
// where they fit a half together
hipError_t copy_back_pieces(void *const *dst, const void *src, int pieces, size_t bytes, hipStream_t s);
hipError_t copy_back_2d(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width,
                        size_t height, hipStream_t s);
hipError_t copy_in_2d(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width,
                      size_t height, hipStream_t s);
void host_copy(void *dst, const void *src, size_t n);
hipError_t pool_alloc(void **out, size_t bytes);
void pool_free(void *p);
void pool_release_all_idle();
size_t pool_live_bytes(int device);     // handed out on `device` and not yet parked or freed (whole process)
// buffers released inside a scope are parked behind ONE device-wide wait when the outermost ends
struct PoolReleaseScope {
    PoolReleaseScope();
    ~PoolReleaseScope();
    PoolReleaseScope(const PoolReleaseScope &) = delete;
    PoolReleaseScope &operator=(const PoolReleaseScope &) = delete;
};
// pinned host memory and HIP events as the handles below take and return them: hipHostMalloc / hipHostFree,
// hipEventCreateWithFlags / hipEventDestroy
hipError_t pinned_alloc(void **out, size_t bytes, unsigned flags);
void pinned_free(void *p);
hipError_t event_create(hipEvent_t *out, unsigned flags);
void event_destroy(hipEvent_t ev);

// ---- owning handles ---------------------------------------------------------------------------------------------
// Device buffers (DevBuf), pinned host buffers (PinnedBuf) and events (Event) belong to the handle that holds them:
// move-only, a move leaves the source empty, the destructor gives back what is held.  A struct made of them (a layout,
// a TableState, a stage record, a stream's slot, the engine) needs no list of what to free: dropping it -- delete,
// `x = X{}` -- frees all of it, once.  What a teardown still sees to itself:
//   one wait    pool_free outside a PoolReleaseScope waits for the whole device, once per block.  Whoever drops an
//               owner opens a scope AROUND the delete or the assignment (member destructors run after a destructor's
//               body: a scope inside the owner's own destructor ends too early).  Engine destroy, a table's eviction or
//               un-keyed replacement, a stream's release, a stage's undo, a group's parts and its lead: one wait each.
//   the device  the scope's end and pool_free wait for the CURRENT device: every owner is torn down under a DeviceGuard
//               of its device (a group: each part under its own, the lead's buffers under the lead's).
//   the order   an engine's stream lanes are orphaned -- they release what they hold and forget the engine -- before
//               the engine's own buffers go; a qm_stream destroyed later finds such a lane empty and frees nothing.
// release() is for giving something up EARLY, on purpose, while its owner lives on.
struct PoolMem {
    static hipError_t get(void **out, size_t bytes, unsigned) { return pool_alloc(out, bytes); }
    static void put(void *p) { pool_free(p); }
};
struct PinnedMem {                                      // (flags: hipHostMallocDefault, hipHostMallocPortable)
    static hipError_t get(void **out, size_t bytes, unsigned flags) { return pinned_alloc(out, bytes, flags); }
    static void put(void *p) { pinned_free(p); }
};
template <typename T, typename Mem>
struct OwnedBuf {
    T *p = nullptr;
    size_t n = 0;
    OwnedBuf() = default;
    OwnedBuf(OwnedBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }      // (declared moves: no copies)
    OwnedBuf &operator=(OwnedBuf &&o) noexcept {
        if (this != &o) {
            release();
            p = o.p; n = o.n;
            o.p = nullptr; o.n = 0;
        }
        return *this;
    }
    ~OwnedBuf() { release(); }
    hipError_t alloc(size_t count, unsigned flags = 0) {    // room for `count` elements: grows, never shrinks
        if (count <= n) return hipSuccess;
        release();
        const hipError_t r = Mem::get(reinterpret_cast<void **>(&p), count * sizeof(T), flags);
        if (r == hipSuccess) n = count;
        return r;
    }
    int ensure(size_t count, unsigned flags = 0) {          // ... in the error convention
        QM_HIP(alloc(count, flags));
        return 0;
    }
    void release() {
        if (p) Mem::put(p);
        p = nullptr;
        n = 0;
    }
};
template <typename T> using DevBuf = OwnedBuf<T, PoolMem>;
template <typename T> using PinnedBuf = OwnedBuf<T, PinnedMem>;

// a HIP event; converts to hipEvent_t where one is recorded, waited for or timed
struct Event {
    struct Destroy { void operator()(hipEvent_t ev) const { event_destroy(ev); } };
    std::unique_ptr<ihipEvent_t, Destroy> ev;
    hipError_t create(unsigned flags = hipEventDefault) {   // (hipEventDisableTiming: an event that only orders)
        hipEvent_t made = nullptr;
        const hipError_t r = event_create(&made, flags);
        ev.reset(made);
        return r;
    }
    void release() { ev.reset(); }
    operator hipEvent_t() const { return ev.get(); }
};

// The bricks of one kernel family over a table: brick grid, per-(brick, row) window records (`raw`: before the
// prefix pass, where the family keeps them), the bricks' totals, the bricks whose windows do NOT fit the family's LDS
// budget (the direct kernel takes them) and the 16-bit window offsets.  What a layout was built for -- its key --
// stands beside it in the family's struct, with an invalidate() that voids the key and keeps grid and buffers.
// invalidate() voids the RESIDENT table's layout only: a table parked at that moment (qm_engine_table_select) keeps
// the layout it built under the former configuration and runs on it when it is selected back.
struct BrickLayout {
    qm::GridDesc g{};
    DevBuf<int32_t> raw, meta, total, list;
    DevBuf<uint16_t> rel;
    int n_list = 0;
    size_t device_bytes() const { return (raw.n + meta.n + total.n + list.n) * 4 + rel.n * 2; }
};
struct Round2Layout : BrickLayout {     // the round-2 kernels' (chunked, exact-row-count), on the table's own grid
    bool rel_built = false;             // `rel` holds this table's offsets (built on first use)
    std::vector<int32_t> h_total;       // the totals on the host: `list` is planned from them ...
    int plan_j = -1, plan_cap = -1;     // ... for these samples per lane and this LDS budget (plan_wide)
    void invalidate() { plan_j = -1; }
};
struct PairLayout : BrickLayout {       // the paired (16-byte operand) float64 kernel's (qm_pair.hpp): own brick grid
    int kt = 0;                         // tile length the paired tables were built for
    bool ok = false;                    // ... and whether (almost) every brick fits
    void invalidate() { kt = 0; }
};
struct ScreenLayout : BrickLayout {     // the float32 screening sweep's (qm_screen.hpp): own brick grid,
    int kt = 0, wb = 0;                 // staggered-copy offset table; what the screening table was built for
    void invalidate() { kt = 0; }
};

// One shift-reuse layout of a table (qm_shift.hpp): brick grid with even brick dimensions, the row-window
// records of every brick, which bricks fit, the record stream dealt over the workgroup's wavefronts.  A table
// has up to two: `sh`, what rounds 3-5 built (256-sample tiles; any launch kind), and -- round 6 -- `shw` for
// the fused detect where WIDE tiles fit: the 8-wave shape on its own brick grid, with a second set of records
// and a second stream for the 384-sample tiles beside those of the 256-sample and tail tiles behind them.
struct ShiftLayout : BrickLayout {          // (list: the bricks that do not fit -- direct kernel; rel stays empty)
    int nw = 0;                             // workgroup shape the tables were built for
    DevBuf<int32_t> fit;
    DevBuf<uint32_t> stream;
    int rows2 = 0;
    int nblk = 1, sb = 0;                   // row blocks (tables of more than 64 rows): blocks, rows per block
    int stage_slots = 0, stage_reach = 0;   // ... largest row window (slots), furthest sample it holds
    bool direct = false;                    // ... staged by LDS-direct loads (stack_shift_rows2_kernel)
    bool quad = false;                      // ... by two 4-wave workgroups per CU (stack_shift_rows4_kernel)
    bool built = false, ok = false;
    int64_t quads = 0, group_rows = 0;      // register-window quads fetched / (group, row)s
    // wide tiles (shw only)
    bool wide = false;
    DevBuf<int32_t> wmeta, wtotal;
    DevBuf<uint32_t> wstream;
    int64_t wquads = 0;                     // quads fetched by the wide tiles' windows (per 48 adds, not 32)

    // this layout's kernel has tail tiles, a step axis and per-brick maxima: neither row blocks nor the 12-wave shape
    // (`sh` is never wide, so the test means the same on it as where only `shw` can be at hand)
    bool plain() const { return nblk == 1 && nw != qm::kShiftWaves3 && !(wide && direct); }
    void invalidate() { built = false; }
    // early, on purpose (ensure_shift_tables: the table does not qualify, its step runs on the other kernels): the
    // buffers go back now, grid and read-outs stay
    void release() {
        PoolReleaseScope one_wait;
        raw.release(); meta.release(); total.release(); list.release(); rel.release();
        fit.release(); stream.release(); wmeta.release(); wtotal.release(); wstream.release();
    }
    size_t device_bytes() const {
        return BrickLayout::device_bytes() + (fit.n + stream.n + wmeta.n + wtotal.n + wstream.n) * 4;
    }
};

// Everything that is derived from ONE travel-time table: the table itself, its brick records and
// window offsets, the layouts of the paired / screened / shift-reuse kernels built from it on first
// use, and the launch shape the table's layout search picked.  The engine works on the state it
// inherits; qm_engine_table_select parks it in a slot and brings another one in (a swap of pointers:
// no device work), so that a change of station availability -- a different served table,
// lut.py:529-537 -- costs a rebuild only the first time that table is seen.
// (The round-2 layout is a base, not a member like the others: its grid is the table's shape as well and is read
// all over the engine as e->g.  Where the layout is meant, r2() says so.)
struct TableState : Round2Layout {
    bool have_lut = false;
    uint64_t serial = 0;            // identity of the loaded table (process-unique; travels with the state
                                    // through qm_engine_table_select): what a qm_stream checks before a launch
    uint64_t digest = 0;            // qm_engine_table_digest of this table, valid while digest_serial == serial
    uint64_t digest_serial = 0;     // (computed once per table; travels with the state like the serial)
    int64_t n_nodes = 0;
    int64_t node_offset = 0;
    int32_t lut_max = 0;
    int n_rows_hint = 0;            // row count the automatic choice is based on
    int auto_j = 0;                 // samples per lane picked by the table's layout search (> 64 rows)
    int tab_waves = 0, tab_lds_bytes = 0;   // workgroup shape the layout search picked (0: none yet)
    DevBuf<int32_t> d_lut;

    Round2Layout &r2() { return *this; }
    const Round2Layout &r2() const { return *this; }
    PairLayout pair;
    ScreenLayout screen;
    // shift-reuse layouts (qm_shift.hpp): own brick grids, row-window slots, record streams
    ShiftLayout sh, shw;

    // another table's values are coming in: every layout's key is void, and the shift-reuse layouts' read-outs
    // report nothing until they are rebuilt.  Grids and buffers stay (qm_engine_load_lut reuses the allocations).
    void invalidate_derived() {
        r2().invalidate(); screen.invalidate(); pair.invalidate(); sh.invalidate(); shw.invalidate();
        sh.ok = shw.ok = false;
    }
    size_t device_bytes() const {
        return d_lut.n * 4 + r2().device_bytes() + pair.device_bytes() + screen.device_bytes() +
               sh.device_bytes() + shw.device_bytes();
    }
};

struct TableSlot {
    TableState state;
    uint64_t key = 0;
    uint64_t stamp = 0;             // last use (the engine's table clock): the oldest slot is evicted
    bool used = false;
};

// The stages in front of the fused detect -- resampling, pre-processing, onsets -- one record each.  A record is the
// stage's small arrays on the device, `repeat` times over (a stream's launch holds that many timesteps: (step, trace)
// is the kernels' trace, (step, row) their row), and the kernel's arguments as far as they do not change from launch
// to launch.  An engine holds one of each for its staged calls (repeat = 1), a qm_stream its own (repeat = its steps
// per launch): neither sees the other's.
//   build    checks the caller's host arrays, makes their images, grows the buffers, copies in on e->stream (the
//            images are consumed when it returns) and fills `args`.  It may be called again, after a failure as well.
//   launch   n_steps timesteps of `in` to `out` on e->stream: enqueue only
// Each is defined where its kernel is compiled: qm_preproc.hip, qm_widen.hip, qm_resample.hip.
struct PreprocStage {
    DevBuf<double> coef;                // sos, taper_left, taper_right
    DevBuf<int32_t> meta;               // trace_filter [repeat][n_traces]
    qm::PreprocArgs args{};
    int n_traces = 0;                   // of one timestep
    int build(qm_engine *e, const char *what, int repeat, int32_t n_traces, int32_t t_samples,
              const int32_t *trace_filter, const double *sos, int32_t n_filters, int32_t n_sections, int detrend,
              const double *taper_left, int32_t n_left, const double *taper_right, int32_t n_right, int zero_phase);
    int launch(qm_engine *e, const double *in, double *out, int n_steps) const;
};
// The pre-processing of gappy traces (qm_preproc.hpp: segments_kernel): what PreprocStage holds, and the segment
// records and taper weights of ONE call.  A stream's records travel with its pushes, so its stage holds neither:
// adopt() borrows the filters of the stream's PreprocStage -- which outlives it, both are the lane's -- and lays out
// the STEP the stream's slots hold, `repeat` of them per launch: [sig_words] signals, [max_segments][8] records,
// [max_weights] taper weights, all 8-byte words.  pack() writes one on the host, the slot form of launch reads them.
struct SegmentStage {
    DevBuf<double> coef;                // sos, then the call's taper weights
    DevBuf<int32_t> meta;               // trace_filter [n_traces]
    DevBuf<int64_t> rec;                // the call's records [n_segments][8]
    qm::SegmentArgs args{};
    int n_traces = 0;                   // of one timestep
    int max_n = 0;                      // the longest segment a launch may meet: sizes the LDS
    size_t sig_words = 0;               // a stream's step (adopt): its signals ...
    int32_t max_segments = 0;           // ... the records it has room for ...
    int64_t max_weights = 0;            // ... and the taper weights
    size_t step_words() const { return sig_words + (size_t)max_segments * qm::kSegmentFields + (size_t)max_weights; }
    size_t step_bytes() const { return step_words() * sizeof(double); }
    int build(qm_engine *e, const char *what, int32_t n_traces, int32_t t_samples, const int32_t *trace_filter,
              const double *sos, int32_t n_filters, int32_t n_sections, int detrend, int zero_phase,
              const int64_t *records, int32_t n_segments, const double *taper_weights, int64_t n_taper_weights,
              int second_taper, double fill_value);
    // refuses a step too large for a launch of `repeat` of them; max_segments >= 1, max_taper_weights >= 0
    int adopt(const char *what, int repeat, const PreprocStage &pre, int32_t max_segments, int64_t max_taper_weights,
              int second_taper, double fill_value);
    // one step into dst [step_words()], on the host: n_segments <= max_segments records, the unused ones padded with
    // n = 0; n_weights <= max_weights weights, the words behind them left alone (no record reads them)
    void pack(double *dst, const double *signals, const int64_t *records, int32_t n_segments, const double *weights,
              int64_t n_weights) const;
    // n_steps packed steps on the device -> their signals [n_steps][sig_words]
    int launch(qm_engine *e, const double *d_steps, double *d_signals, int n_steps) const;
    // step k reads in + k in_step, its records at rec + k rec_step, its weights at w + k w_step, writes out + k out_step
    int launch(qm_engine *e, const double *in, int64_t in_step, const int64_t *rec, int64_t rec_step, const double *w,
               int64_t w_step, double *out, int64_t out_step, int n_steps) const;
};
// What the segment calls refuse in a timestep's records [n_segments][8] (include/qmhip.h: qm_engine_preprocess_segments),
// on the caller's thread; defined in qm_preproc.hip.
int check_segment_records(const char *what, int32_t n_traces, int32_t t_samples, const int64_t *records,
                          int32_t n_segments, int64_t n_taper_weights);
struct OnsetStage {
    DevBuf<int32_t> meta;               // trace_row [repeat][n_traces] (step k's rows k * n_rows on), nsta, nlta [repeat][n_rows]
    DevBuf<double> sta, lta;            // [repeat][n_traces][T] scratch of the two kernels
    qm::OnsetArgs args{};
    int n_traces = 0, n_rows = 0;       // of one timestep
    int build(qm_engine *e, const char *what, int repeat, int32_t n_traces, int32_t t_samples, const int32_t *trace_row,
              int32_t n_rows, const int32_t *nsta, const int32_t *nlta, int transform, int position, int32_t taper_pad,
              double min_onset_value);
    // raw_onsets: [n_steps][n_rows][T] or nullptr
    int launch(qm_engine *e, const double *signals, double *raw_onsets, double *log_onsets, int n_steps) const;
};
struct ResampleStage {
    DevBuf<int64_t> meta;               // records [repeat][n_traces][kResampleFields] (step k's raw offsets k raw steps on), taper table
    DevBuf<double> coef, scratch;       // low-pass sections and taper weights; [repeat][n_traces][max_kept] where a
    qm::ResampleArgs args{};            // ... kept series is above the LDS limit
    int64_t max_kept = 0;               // the longest kept series
    int n_traces = 0;                   // of one timestep
    size_t raw_bytes = 0, raw_step = 0; // a timestep's raw samples in bytes; in doubles (step_doubles): what lies between two steps
    static size_t step_doubles(int raw_dtype, int64_t total_raw_samples) {
        return ((size_t)total_raw_samples * (raw_dtype == qm::kRawInt32 ? 4 : 8) + 7) / 8;
    }
    size_t step_words() const { return raw_step; }      // a stream's step, under the names SegmentStage answers to
    size_t step_bytes() const { return raw_bytes; }
    int build(qm_engine *e, const char *what, int repeat, int raw_dtype, int64_t total_raw_samples, int32_t n_traces,
              int32_t t_samples, const int64_t *records, const double *sos_lp, int32_t n_lowpass, int32_t n_sections_lp,
              int detrend, const int32_t *taper_table, int32_t n_tapers, const double *taper_weights,
              int64_t n_taper_weights);
    int launch(qm_engine *e, const void *raw, double *out, int n_steps) const;
};

// The clock of a launch sequence of N stages: a pair of HIP events around each stage's launches, the elapsed times
// once the call has synchronised.  `names`: the stages as the read-outs "<prefix>_ns_<name>" call them, defined beside
// the stage enum.  A call goes begin, stage ..., its synchronise, collect.
template <int N>
struct StageClock {
    const char *const (&names)[N];
    std::vector<Event> ev;              // 2 per stage, made on first use
    int64_t ns[N] = {};                 // the last collected call's stage times, 0: the stage did not run
    bool ran[N] = {};                   // the stages bracketed since begin
    bool on = true;
    explicit StageClock(const char *const (&names_)[N]) : names(names_) {}
    int ensure_events() {
        while (ev.size() < 2 * (size_t)N) {
            Event made;
            QM_HIP(made.create());
            ev.push_back(std::move(made));
        }
        return 0;
    }
    // on_ = false: nothing is recorded, every stage reads 0 after collect.  zero_now: the times read 0 from here on -- a
    // call that fails before collect leaves zeros, not the previous call's times.
    void begin(bool on_, bool zero_now) {
        on = on_;
        for (bool &r : ran) r = false;
        if (zero_now) for (int64_t &t : ns) t = 0;
    }
    // `launches` (enqueue only) between the stage's two events on `stream`
    template <typename F>
    int stage(hipStream_t stream, int st, F &&launches) {
        if (on) {
            if (ensure_events()) return 1;
            QM_HIP(hipEventRecord(ev[2 * st], stream));
        }
        launches();
        QM_HIP(hipGetLastError());
        if (on) {
            QM_HIP(hipEventRecord(ev[2 * st + 1], stream));
            ran[st] = true;
        }
        return 0;
    }
    // ... one kernel
    template <typename... P, typename... A>
    int launch(hipStream_t stream, int st, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, A... args) {
        return stage(stream, st, [&] { hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...); });
    }
    // after the synchronise: every stage's time, 0 where it did not run
    int collect() {
        for (int st = 0; st < N; ++st) {
            ns[st] = 0;
            if (!ran[st]) continue;
            float ms = 0.0f;
            QM_HIP(hipEventElapsedTime(&ms, ev[2 * st], ev[2 * st + 1]));
            ns[st] = (int64_t)((double)ms * 1e6);
        }
        return 0;
    }
};

// The scratch of the stages behind the detect and of the engine's own sweeps, one record per call family: device
// buffers that grow with the largest call seen, the family's counters and clocks.  Plain data -- the calls that fill
// them are named with each record -- and nothing outside a family touches its record, except where a comment says so.
struct PickStage {                      // qm_engine_pick_phases (qm_picks.hip)
    DevBuf<double> val;                 // half-widths, thresholds, then the picks
    DevBuf<int32_t> meta;               // windows, groups, then the status
};
struct AmplitudeStage {                 // qm_engine_measure_amplitudes (qm_amplitudes.hip)
    DevBuf<double> work, scratch;       // the working copy of the packed traces, windows above the LDS limit
    DevBuf<double> coef, val;           // sections and taper weights; the value table
    DevBuf<int64_t> meta;               // trace records, taper table and window records
    DevBuf<int32_t> idx;                // the index table
};
struct TriggerStage {                   // qm_engine_trigger / _trigger_resident (qm_trigger.hip)
    DevBuf<double> x, par;              // the two series (raw, then smoothed), weights and thresholds
    DevBuf<int32_t> cnt;                // the run kernels' counts ...
    DevBuf<int64_t> tot;                // ... and totals
    DevBuf<int32_t> run;                // sized once the candidate count is known: run starts and ends,
    DevBuf<int64_t> cand;               // ... candidate and event tables,
    DevBuf<double> val;                 // ... their values
    StageClock<qm::kTrigStages> clock{qm::kTrigStageNames};     // "trigger_ns_<stage>": runs under cfg.trigger_timing
};
struct ScanmseedCodec {                 // qm_engine_scanmseed_encode / _decode (qm_scanmseed.hip)
    DevBuf<int32_t> x;                  // the int32 series: quantised, copied in or decoded
    DevBuf<double> f, fac;              // float64 series in or descaled out; decode's factors
    DevBuf<uint8_t> bytes;              // count(p) and the words' codes
    DevBuf<uint32_t> map, out;          // the tiles' maps; the records
    DevBuf<int32_t> tile, rec;          // the tiles' entries and first words; first samples and counts (decode: sample counts)
    DevBuf<unsigned long long> tot;     // totals and error slots
    DevBuf<int64_t> off;                // decode's offsets
    StageClock<qm::kSmsStages> clock{qm::kSmsStageNames};       // "scanmseed_ns_<stage>": always runs
};
struct TravelTimeStage {                // qm_engine_tt_homogeneous / _tt_sections / _tt_sweep / _tt_eikonal3d (qm_traveltimes.hip)
    // (every call fills what it uses before it launches and reads it back before it returns: nothing here is carried
    // from one call to the next, whichever of the four it is -- only the sizes grow)
    DevBuf<double> par;                 // row parameters; the sections' slowness rows and sources
    DevBuf<double> sec, out;            // a host caller's sections (eikonal3d: slowness volumes) on their way in; grids or
                                        // sections on their way out (eikonal3d: a host caller's tau lives here, in place)
    DevBuf<double> tau;                 // the solver's tau of sections above the LDS limit: [n_sections][nr * nz]
    DevBuf<int32_t> meta;               // the sweep's row -> section; the solver's rounds and status; eikonal3d: row ->
                                        // model, the sources' cells [n_rows][3], two sets of row flags
    DevBuf<unsigned long long> bad;     // the sweep's first node outside its section, per row; eikonal3d: slot 0, the first
                                        // slowness that is not finite and positive
    StageClock<qm::kTtStages> clock{qm::kTtStageNames};         // "tt_ns_<stage>": always runs
};
struct TieScratch {                     // the near-tie refinement (refine_ties, qm_engine_tie_partial; qm_ties.hpp)
    DevBuf<double> zext, zgrid, z;      // the largest z per sample left by the combine of the own sets; the GRID's (sharded)
    DevBuf<int32_t> pairs, imin, count, cands;
    DevBuf<unsigned long long> emax, keys;
    int64_t refined_steps = 0, overflow_last = 0, pairs_last = 0;
    bool counts_pending = false;        // the last refinement's counters are still on the device
};
struct ScreenScratch {                  // the screened detect's sweep (run_screen, drain_flags; qm_screen.hpp)
    DevBuf<int32_t> counts, cells, work, flags;     // (work: also ensure_shift_tables' per-brick fit flags of a wide
    DevBuf<int32_t> onq, cell, gmax, pm, sparams;   // layout, qm_tables.hip)
    DevBuf<double> rowmax, ssum, cand_z;
    DevBuf<int64_t> cand_idx;
    int64_t screened_steps = 0, fallback_steps = 0, last_candidates = 0;
    int last_plan_jp = 0, last_plan_big = 0;
    PinnedBuf<int32_t> h_flags;             // pinned ring of per-step (flags, candidates) pairs
    int flags_pending = 0, flags_head = 0;  // not yet folded into the counters
};
struct FitScratch {                     // qm_engine_locate_fits, _rbf_peak (qm_widen.hip): three map-sized work buffers,
    DevBuf<double> a, b, c;             // ... (a, b: also qm_engine_exp_correctly_rounded's input and output)
    DevBuf<double> part, val, win;      // reduction partials (also qm_engine_exp2f_max_error's), device-side scalars, windows
    DevBuf<int64_t> pidx;
};
// Where the staged calls put host arrays on their way in and out.  Shared on purpose: a call is over when it returns.
struct CallStaging {
    DevBuf<double> sig;                 // in: qm_engine_preprocess', _preprocess_segments' and _onsets' signals,
                                        // qm_engine_pick_phases' onset rows
    DevBuf<double> raw;                 // out: qm_engine_onsets' raw onsets
    DevBuf<double> pre_out;             // out: qm_engine_preprocess' and _preprocess_segments' filtered and
                                        // qm_engine_resample's resampled traces
    DevBuf<double> rs_raw;              // in: qm_engine_resample's raw samples (bytes, in doubles)
};

struct StreamLane;                   // a continuous-detect pipeline's ring on one engine (qm_stream.hip)

// One stacking launch (StackLaunch below) as plan_stack decides it and issue_stack enqueues it (qm_engine.hip).
// qm_engine::last is the plan of the last launch enqueued, assigned whole by run_stack: the only description of
// that launch, for the refinement, the folds and the read-outs of qm_engine_get alike.
enum StackFamily : int { kFamilyChunked = 0, kFamilyExact = 1, kFamilyPair = 2, kFamilyShift = 3 };   // "last_kernel"
struct StackPlan {
    StackFamily family = kFamilyChunked;    // the LDS launch's kernel and its samples per lane (a launch of the
    int j = 0;                              // ... direct kernel alone: 0 and 0)
    const BrickLayout *layout = nullptr;    // the layout whose bricks the launch runs on ...
    const ShiftLayout *shift = nullptr;     // ... the same, where it is a shift-reuse launch
    int shift_mode = 0, lazy = 0;           // shift-reuse: detect / volume / marginal, the detect loop's flavour,
    int tail_spl = 0, wide_tiles = 0;       // ... samples per lane of the tail tile (0: none), wide tiles in front
    int ntiles = 0, cap_doubles = 0;        // the LDS launch's time tiles, its LDS window capacity
    int steps = 1;                          // timesteps in the launch
    bool use_lds = false, use_direct = false;
    int groups_lds = 0, groups_direct = 0;
    int direct_j = 0, direct_threads = 0;   // the direct launch: samples per lane, workgroup, publish area
    size_t direct_publish = 0;
    int brick_rows = 0;                     // rows of maxima per brick in d_bmax (StackArgs::brick_max), 0: none
    int marg_tiles = 0;                     // time tiles of a marginal-map launch (rows of d_marg)
    bool batched = true;                    // false: the kernel cannot hold the launch's n_steps -- not launched
    // which bricks the partial sets in d_pmax stand for (qm_ties.hpp): the grid, the direct launch's bricks,
    qm::GridDesc g{};
    const int32_t *list = nullptr;
    int n_list = 0;
    int sets = 0, scan_n = 0;               // ... their number, the samples each one spans
    bool sets_own = false;                  // ... left by a float64 detect_partial (detect_core, the group's launches)
};

struct qm_engine : TableState {
    int device = 0;
    std::vector<StreamLane *> streams;  // pipelines' lanes alive on this engine: orphaned when it is destroyed
    int n_cu = 256;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    Event ev0, ev1;
    bool timed = false;
    // optional per-call timing log (cfg.log_timing; bench): pairs of events around every stacking launch
    std::vector<Event> ev_log;          // 2 events per recorded call
    size_t ev_used = 0;

    // parked tables (qm_engine_table_select) and the key of the one being worked on
    std::vector<TableSlot> slots;
    uint64_t cur_key = 0, table_clock = 0;
    bool cur_keyed = false;
    int64_t table_hits = 0, table_misses = 0, table_evictions = 0;
    int64_t table_digests = 0;          // digest kernels run (qm_engine_table_digest: once per table)
    DevBuf<unsigned long long> d_digest;    // ... their sum

    EngineConfig cfg;                   // the tunables (qm_config.hpp): written by config_set only

    DevBuf<int32_t> d_scalar;           // a few device-side counters of the table builds (qm_tables.hip)
    int last_batched = 1;               // timesteps the last detect_batch put into one launch
    StackPlan last;                     // the last stacking launch (run_stack)

    // float64 travel-time grids in seconds (optional; on-device table serving)
    DevBuf<double> d_grids;
    DevBuf<int32_t> d_rows, d_served;
    int gx = 0, gy = 0, gz = 0, g_rows = 0;

    // the stacking scratch, read by folds, ties, streams and groups alike: log-onsets staged from the host (and
    // qm_engine_onsets' output on its way there), the launch's partial sets and its row of maxima per brick (StackPlan::
    // brick_rows), the packed three series and a host volume's chunk on their way out, the marginal map's tile sums, the map
    DevBuf<double> d_onsets, d_pmax, d_psum, d_bmax, d_out_a, d_chunk, d_marg, d_marg_out;
    DevBuf<int64_t> d_pidx;

    // the stages in front of the detect as the staged calls (qm_engine_resample / _preprocess / _preprocess_segments /
    // _onsets) last built them
    ResampleStage rs_stage;
    PreprocStage pre_stage;
    SegmentStage seg_stage;
    OnsetStage on_stage;
    // the scratch records above, one per call family
    CallStaging staging;
    PickStage picks;
    AmplitudeStage amps;
    TriggerStage trig;
    ScanmseedCodec sms;
    TravelTimeStage tt;
    TieScratch tie;
    ScreenScratch sweep;
    FitScratch fit;
};

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// What the trace stages (pre-processing, resampling, amplitudes) all refuse in their sections and taper tables.
// sos: [n_filters][n_sections][6]; `noun` is what the stage calls a filter ("filter", "low-pass"), `name` its
// section-count argument.
inline int check_sections(const char *what, const char *noun, const char *name, const double *sos, int32_t n_filters,
                          int32_t n_sections) {
    if (n_sections < 1 || n_sections > qm::kPreprocMaxSections)
        return fail("%s: %s must be in 1..%d (got %d)", what, name, qm::kPreprocMaxSections, n_sections);
    for (int k = 0; k < n_filters * n_sections; ++k)
        if (sos[6 * k + 3] != 1.0)
            return fail("%s: %s %d, section %d: a0 = %.17g, sections must be normalised to a0 == 1", what, noun,
                        k / n_sections, k % n_sections, sos[6 * k + 3]);
    return 0;
}
// table: [n_tapers][2], offset into the weights and ramp length m: 2 m weights from there on
inline int check_taper_table(const char *what, const int32_t *table, int32_t n_tapers, int64_t n_weights) {
    for (int t = 0; t < n_tapers; ++t) {
        const int64_t off = table[2 * t], m = table[2 * t + 1];
        if (off < 0 || m < 0 || off + 2 * m > n_weights)
            return fail("%s: taper %d: 2 x %lld weights from %lld on, %lld weights given", what, t, (long long)m,
                        (long long)off, (long long)n_weights);
    }
    return 0;
}

// `kernel` over blocks x threads on e->stream with `lds` bytes of dynamic LDS, its limit raised to that (lds == 0:
// the kernel's limit is left alone)
template <typename... P, typename... A>
int launch_with_lds(qm_engine *e, void (*kernel)(P...), unsigned blocks, unsigned threads, size_t lds, A... args) {
    if (lds)
        QM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), lds, e->stream, args...);
    QM_HIP(hipGetLastError());
    return 0;
}

// Staging of a call's arrays.  In: the device pointer to read `n` elements of `src` from -- `src` itself where it is
// on the device, else `buf`, grown and filled on e->stream; nullptr: that failed.
// (bytes: what to copy where that is not n elements -- raw samples of either width in a buffer of doubles)
template <typename T, typename U>
const U *stage_in(qm_engine *e, DevBuf<T> &buf, const U *src, int on_device, size_t n, size_t bytes = 0) {
    if (on_device) return src;
    const auto fill = [&]() -> int {
        if (buf.ensure(n)) return 1;
        QM_HIP(copy_in(buf.p, src, bytes ? bytes : n * sizeof(T), e->stream));
        return 0;
    };
    return fill() ? nullptr : reinterpret_cast<const U *>(buf.p);
}
// Out: where the kernels write the caller's `n` elements -- `user` itself on the device, else `buf` (d == nullptr:
// growing it failed); fetch enqueues the copy back, the synchronise that follows stays with the call.
template <typename T>
struct StagedOut {
    T *d = nullptr, *user = nullptr;    // user: the host destination, nullptr where there is none
    size_t n = 0;
    int fetch(qm_engine *e) const {
        if (user) QM_HIP(copy_back(user, d, n * sizeof(T), e->stream));
        return 0;
    }
};
template <typename T>
StagedOut<T> stage_host_out(DevBuf<T> &buf, T *user, int on_device, size_t n) {
    if (on_device) return {user, nullptr, n};
    return {buf.ensure(n) ? nullptr : buf.p, user, n};
}
// The engine's own event pair (qm_engine_last_kernel_ms) around `launches`, a callable in the error convention: the
// call counts as timed only once the end event is recorded -- one that fails in between leaves e->timed as it was.
template <typename F>
int timed_launches(qm_engine *e, F &&launches) {
    QM_HIP(hipEventRecord(e->ev0, e->stream));
    if (launches()) return 1;
    QM_HIP(hipEventRecord(e->ev1, e->stream));
    e->timed = true;
    return 0;
}

// pairs of samples per lane: time tile = 128 * JP; 0 = this table is not screened
// How the sweep is launched: JP pairs of samples per lane (time tile 128*JP) and either two
// 8-wave workgroups per CU with 80 KB of LDS each, or ("big") one 16-wave workgroup with all
// 160 KB -- twice the tile for the same rows, so fewer address / epilogue instructions per sample.
struct ScreenPlan {
    int jp = 0;                     // 0 = this table is not screened
    bool big = false;
    int kt() const { return 128 * jp; }
    int lds_bytes(const qm_engine *e) const {
        return big ? 160 * 1024 : (e->cfg.user_lds ? e->cfg.lds_bytes : 80 * 1024);
    }
    int window_bytes(const qm_engine *e) const {       // minus the cell-maximum row
        return (lds_bytes(e) - kt() * 4) / 16 * 16;
    }
    int threads() const { return big ? 1024 : 512; }
};

// combine_kernel's modes (qm_kernels.hpp)
enum CombineMode : int {
    kCombinePartial = 0,            // one combined partial: log2-domain maximum, sum, index + node offset
    kCombineFinal = 1,              // the final series from log2-domain partials
    kCombineValues = 2,             // the final series from partials that hold coalescence values (volume scan)
};

// The three series a combine writes, in this order everywhere: maxima, second (max_norm for the final
// series, the sum for a partial), indices.  at(k): the same series from sample k on.
struct OutSeries {
    double *max = nullptr, *second = nullptr;
    int64_t *idx = nullptr;
    OutSeries at(int64_t k) const { return {max + k, second + k, idx + k}; }
};

// Partial sets as combine reads them: n samples per set, set s from element s * stride of each array
struct SetView {
    const double *max = nullptr;
    const int64_t *idx = nullptr;
    const double *sum = nullptr;
    int n_sets = 0, n = 0;
    int64_t stride = 0;
};

// One stacking launch (run_stack): samples [sample0, sample0 + n_chunk) of a scan of n_samples over the
// onsets (rows of T samples, fsmp before the scan), and what it leaves besides the partial sets.
struct StackLaunch {
    struct Detect {};
    struct Volume {                         // [n_nodes][stride] rows of the launch's samples
        double *p = nullptr;
        int64_t stride = 0;
        int accumulate = 0;                 // 1: added to (the reference's +=), 0: overwritten
    };
    struct Marginal {                       // per node, the sum over the scan's samples [first, end)
        int first = 0, end = 0;
        double *map = nullptr;
    };
    const double *onsets = nullptr;
    int T = 0, fsmp = 0, n_samples = 0, available = 0;
    int sample0 = 0, n_chunk = 0;
    std::variant<Detect, Volume, Marginal> kind;
    bool want_scan = true;                  // partial sets for the three series
    const int32_t *run_if = nullptr;        // returns at once unless *run_if (the screened step's fallback)
    int n_steps = 1;                        // that many timesteps in ONE launch (fused detect only), their
    int64_t step_stride = 0;                // ... onsets step_stride doubles apart

    // a detect of the whole scan, one timestep
    StackLaunch(const double *on, int T_, int fsmp_, int ns, int avail)
        : onsets(on), T(T_), fsmp(fsmp_), n_samples(ns), available(avail), n_chunk(ns) {}
};

// What run_stack reports.  rc != 0: it failed (qm_last_error).  batched = false: the launch cannot hold
// its n_steps timesteps (row blocks, the 12-wave shape) -- nothing was launched, the caller goes step by step.
struct StackResult {
    int rc = 0;
    int sets = 0;                           // partial sets in d_pmax / d_pidx / d_psum: [sets][n_steps * n_chunk]
    bool batched = true;
    StackResult(int rc_ = 0) : rc(rc_) {}   // (from an int: `return fail(...)` as everywhere else)
};

// ---- qm_tables.hip ------------------------------------------------------------------------------
// the workgroup shape of the round-2 launches: the user's value if they set one, else the resident table's layout
// search's choice, else the default (8 waves, 80 KiB)
int run_waves(const qm_engine *e);
int run_lds_bytes(const qm_engine *e);
inline int lds_cap_doubles(int lds_bytes) { return lds_bytes / 8; }
inline int lds_cap_doubles(const qm_engine *e) { return lds_cap_doubles(run_lds_bytes(e)); }
int ensure_rel(qm_engine *e);
int eff_j(const qm_engine *e, int lds_bytes);          // ... under a trial LDS budget (the layout search)
inline int eff_j(const qm_engine *e) { return eff_j(e, run_lds_bytes(e)); }
int run_j(const qm_engine *e, int n_chunk);
int plan_wide(qm_engine *e, int J);
int pair_jp(const qm_engine *e, int n_chunk, bool volume);
void table_set_key(qm_engine *e, uint64_t key);     // the resident table is known under `key` (engine groups)
int ensure_pair_tables(qm_engine *e, int jp);
int ensure_shift_tables(qm_engine *e, ShiftLayout &L);
bool screen_plan_feasible(const qm_engine *e, int S, const ScreenPlan &p);
ScreenPlan screen_plan(const qm_engine *e, int S, int n_samples);
int ensure_screen_tables(qm_engine *e, const ScreenPlan &plan);

// ---- qm_engine.hip ------------------------------------------------------------------------------
int auto_groups(const qm_engine *e, int ntiles, int units, int blocks_per_cu, int rounds = 0);
// the two events around a timed launch (the timing log's next pair, or the engine's own)
int timing_events(qm_engine *e, hipEvent_t *begin, hipEvent_t *end);
StackResult run_stack(qm_engine *e, const StackLaunch &s);
// the sets the last stacking launch or volume scan left: [n_sets][n] in d_pmax / d_pidx / d_psum
SetView engine_sets(const qm_engine *e, int n_sets, int n);
// n_sets packed sets [n_sets][3][n]: rows maxima, index bits, sums (the layout of the exchange across devices)
SetView packed_sets(const double *d_packed, int n_sets, int n);
OutSeries packed_set(double *d_packed, int n);      // ... one of them, as a combine in partial mode writes it
int combine(qm_engine *e, const SetView &in, CombineMode mode, int64_t node_offset, int64_t n_nodes_total,
            const OutSeries &out, const int32_t *run_if);
int refine_ties(qm_engine *e, const StackLaunch &s, int64_t *o_idx, const double *zext,
                unsigned long long *o_key);
// The cores of the step calls: device in, device out, nothing waits.  The public calls wrap them in the
// argument checks and the staging of host arrays; the engine group (qm_group.hip) calls them in partial mode.
//   stack_fold:  one stacking launch, the marginal map (a marginal launch), the combine of its sets into `out`
//                from s.sample0 on (want_scan) and, final series only, the near-tie refinement
//   scan_fold:   find_max_coa's scan of the n_nodes rows [node0, node0 + n_nodes) of a volume, combined
//   detect_core: a detect step, screened or float64
StackResult stack_fold(qm_engine *e, const StackLaunch &s, CombineMode mode, int64_t n_nodes_total,
                       const OutSeries &out);
int scan_fold(qm_engine *e, const double *vol, int64_t stride, int ns, int64_t n_nodes, int64_t node0,
              CombineMode mode, const OutSeries &out);
int detect_core(qm_engine *e, const double *d_on, int T, int fsmp, int ns, int available, CombineMode mode,
                int64_t n_nodes_total, const OutSeries &out);
int check_step(qm_engine *e, int T, int fsmp, int lsmp, int available, int *n_samples);
// the log-onsets of n_steps timesteps on the device: the caller's pointer or their copy in d_onsets; nullptr: failed
inline const double *stage_onsets(qm_engine *e, const double *onsets, int on_device, int T, int n_steps = 1) {
    return stage_in(e, e->d_onsets, onsets, on_device, (size_t)e->g.n_rows * T * n_steps);
}
// where the kernels write the caller's three series (on host: the engine's packed [3][n] buffer) ...
int stage_out(qm_engine *e, int n, int out_on_device, const OutSeries &user, OutSeries *st);
// ... and their copy back to the caller
int fetch_out(qm_engine *e, int n, int out_on_device, const OutSeries &st, const OutSeries &user);

// ---- qm_stream.hip ------------------------------------------------------------------------------
// the engine is going away: its pipelines give their buffers back and refuse further calls
void streams_orphan(qm_engine *e);

// ---- qm_screen.hip ------------------------------------------------------------------------------
constexpr int kFlagRing = 1024;
int drain_flags(qm_engine *e);
int run_screen(qm_engine *e, const double *d_onsets, int T, int fsmp, int ns, int available,
               int *n_sets, bool *screened);

#pragma GCC visibility pop
