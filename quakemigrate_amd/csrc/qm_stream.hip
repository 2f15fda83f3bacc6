// qm_stream.hip -- the continuous detect sweep as a native pipeline (C ABI part 3, include/qmhip.h).
//
// The reference's QuakeScan._continuous_compute (quakemigrate/signal/scan.py:407-470; the loop
// itself :434-448) walks the timesteps serially: read -> onsets -> migrate -> find_max_coa -> append.
// Timesteps are independent given their onsets, so the hot-path part of that loop is a pipeline over
// a ring of `depth` slots, each holding `steps_per_launch` timesteps:
//
//   caller's thread : a push            CPU copy of a step's input into the slot's PINNED input
//   copy stream     : H2D of the slot's inputs                 (overlaps the previous launch's kernel)
//                     -- or, for slots of up to kPullBytes (the example-sized grids, one timestep per launch: a
//                     step is a fraction of a millisecond and the wait for another stream's copy costs a quarter
//                     of it), NO copy command at all: a small kernel on the engine's stream PULLS the pinned
//                     input over the bus into the slot's device buffer, in order before the detect launch
//   engine's stream : whatever makes signals, conditioning, onsets -- as far as the stream's kind of input needs
//                     them, see below -- then ONE fused-detect launch for the slot's K steps
//                     (qm_engine_detect_batch); its combine kernel writes the results, packed as
//                     [3][K x n_samples] float64, STRAIGHT into the slot's pinned host buffer (a few KB per
//                     timestep; no D2H command)
//   caller's thread : qm_stream_pop    waits for the launch's event, CPU copy of a step's three series
//
// What crosses the bus is one kind of input per stream (kFeedTable: a row per kind), and a slot's launch is the part
// of ONE chain that kind still needs (launch_slot), every kernel writing straight into the slot's next buffer:
//
//   input over the bus  ->  signals made here  ->  conditioning  ->  onsets  ->  detect
//   log-onsets   qm_stream_push            [n_rows][T]:  detect
//   signals      qm_stream_push_signals    resampled component traces [n_traces][T]:  pre-processing in place (detrend,
//                                          taper, zero-phase band-pass; qm_preproc.hpp), the two onset kernels over the
//                                          slot's (step, trace)s and (step, row)s, detect
//   raw traces   qm_stream_push_raw        packed raw samples, each trace at its own rate and length, int32 as miniSEED
//                                          holds them or float64:  the resampling kernel (qm_resample.hpp) makes the
//                                          signals, then as for signals
//   gappy traces qm_stream_push_segments   traces with their layout, which changes from timestep to timestep and so
//                                          travels with the push -- traces, records, taper weights in ONE pinned step
//                                          (SegmentStage::pack; one move over the bus: bits):  the segment kernel
//                                          (qm_preproc.hpp) over the slot's (step, record)s makes the signals,
//                                          conditioned segment by segment, then onsets and detect
//
// Round 4 drove a pipeline like this from Python (three D2H copies, three events and NumPy staging per
// launch): with the copies inside the clock the example-sized grids lost 30-40 % of their kernel
// rate and K steps per launch bought nothing (profiles/r04_bench_{C1,E1,E2}_k*.json).  Here a launch
// costs the host one memcpy per pushed step and a handful of enqueues; ordering is HIP events, the
// host blocks only in qm_stream_pop, and only for the oldest launch: 8 timesteps per launch run at
// x1.00 of the resident step on those grids.  The caller's pointers are never handed to the HIP
// runtime.
//
// The stages in front of the detect are the records of qm_engine.hpp (ResampleStage, SegmentStage, PreprocStage,
// OnsetStage): the stream builds its own, steps_per_launch times over, where the stage is set, launches them slot by
// slot and releases them with its slots.  Nothing here checks a stage's arrays, fills a kernel's arguments or lays out
// a step of more than one array.
//
// Two records: a StreamLane is one engine's ring and does what it is told (fill, launch, pop, build or undo a stage,
// release); a qm_stream, the C ABI's handle, owns one lane per engine and keeps what belongs to the whole stream --
// the launches in push order, the kind of input, which stages are set.  Launch j goes to lane j mod n; a stream on
// one engine (qm_stream_create) is the one-lane case of a stream over replicas (qm_stream_create_replicas).
#include "qm_engine.hpp"

#include <deque>

// what the pushes carry, one kind per stream (kFeedTable below says what each kind is called, needs and makes)
enum Feed { kNothingYet = 0, kLogOnsets = 1, kSignals = 2, kRaw = 3, kSegments = 4, kFeeds = 5 };

struct StreamLane {
    qm_engine *e = nullptr;             // (nullptr: orphaned by qm_engine_destroy -- the lane holds nothing any more)
    int n_rows = 0, T = 0, fsmp = 0, lsmp = 0, available = 0, ns = 0, K = 1, depth = 2;
    int64_t n_nodes_total = 0;
    uint64_t table_serial = 0;          // the table the stream was made on (TableState::serial)
    hipStream_t copy_stream = nullptr;
    struct Slot {
        struct In {
            PinnedBuf<double> h;        // pinned [K][step_words[feed]] (the signals': given up at the first step of a
                                        // feed that makes them on the device)
            DevBuf<double> d;           // device, the same (the signals': filtered in place)
        } in[kFeeds];                   // by Feed: log-onsets from create on, signals and raw samples from their stage on
        PinnedBuf<double> h_out;        // pinned [3][K * ns]: max_coa, max_norm_coa, indices (int64 bits) --
                                        // written by the kernels themselves
        Event copied;                   // the inputs are on the device
        Event done;                     // the launch has finished: the results are in h_out
        int n = 0;                      // steps launched from this slot
        int taken = 0;                  // ... of which popped
        bool in_flight = false;
    };
    std::vector<Slot> slots;
    std::deque<int> order;              // slots in flight, oldest first
    int fill_slot = 0, fill_n = 0;      // slot being filled, steps pushed into it so far
    int64_t launched_steps = 0, launches = 0;
    PinnedBuf<unsigned long long> h_stamp;   // ("stream_stamps") pinned [2][4096]
    bool pulled = false;                // the last launch's inputs were pulled by a kernel (no copy command)
    size_t step_words[kFeeds] = {};     // a timestep of each kind in doubles, as a slot holds it (raw bytes: rounded up)
    size_t step_bytes[kFeeds] = {};     // ... in bytes, as it is pushed
    // the stages (qm_engine.hpp), K times over: qm_stream_set_onset_stage builds `pre` and `on`,
    // qm_stream_set_resample_stage `rs`; qm_stream_set_segment_feed has `seg` adopt `pre`'s filters
    PreprocStage pre;
    OnsetStage on;
    ResampleStage rs;
    SegmentStage seg;
};

// One row per kind of input: its names in the refusals, what its stage stands on, what its stage is on a lane.  The
// refusals (may_set, may_push), the pinned buffers (alloc_inputs, fill) and a stage's undoing read it; only the
// launch chain (launch_slot) names kinds.
struct FeedRow {
    const char *push;                   // the entry point that pushes this kind
    const char *set;                    // ... that sets its stage (nullptr: none -- log-onsets are taken from creation)
    const char *takes;                  // "this stream takes <takes>"
    const char *noun;                   // the stage in "has no <noun>", "has its <noun> already"
    const char *word;                   // "the <word> is set before the first push"
    int after;                          // the kind whose stage must be set first (kNothingYet: none)
    bool makes_signals;                 // ... on the device: the signals' pinned buffers go at its first push, its own
                                        // start zeroed (an int32 step's last bytes, weights a step does not bring)
    void (*drop)(StreamLane *);         // the lane's stage records go back to empty
};
constexpr FeedRow kFeedTable[kFeeds] = {
    {},
    {"qm_stream_push", nullptr, "log-onsets", nullptr, nullptr, kNothingYet, false, nullptr},
    {"qm_stream_push_signals", "qm_stream_set_onset_stage", "signals", "onset stage", "stage", kNothingYet, false,
     [](StreamLane *l) { l->pre = PreprocStage{}; l->on = OnsetStage{}; }},
    {"qm_stream_push_raw", "qm_stream_set_resample_stage", "raw traces", "resampling stage", "stage", kSignals, true,
     [](StreamLane *l) { l->rs = ResampleStage{}; }},
    {"qm_stream_push_segments", "qm_stream_set_segment_feed", "gappy traces", "segment feed", "feed", kSignals, true,
     [](StreamLane *l) { l->seg = SegmentStage{}; }},
};

struct qm_stream {
    std::vector<std::unique_ptr<StreamLane>> lanes;    // one per engine, at least one (registered on that engine)
    struct Launch {
        int lane = 0;
        int left = 0;                   // steps not yet popped
    };
    std::deque<Launch> launched;        // every lane's launches in push order, oldest first
    int cur = 0;                        // the lane being filled
    int feed = kNothingYet;             // the kind of the steps pushed so far
    bool set[kFeeds] = {false, true};   // by Feed: its stage is set, on every lane or on none (log-onsets need none)
};

namespace {

// Slots this small are pulled by a kernel instead of copied by a command on another stream (round 6).  One
// timestep per launch on the example-sized grids ran at x1.27-1.30 of the resident step with the copy command --
// back to back under the tracer, so not the copy's duration: the dependency across two streams (a signal the
// runtime's host thread has to forward) -- profiles/r06_trace_stream_k1.json.  A kernel that reads pinned host
// memory moves ~170 KB (C1) in a few microseconds and needs no event: the engine's stream orders it.  Large
// slots (C3: 1.5 MB per timestep, 41 ms of kernel to hide the copy behind) keep the copy stream.
constexpr size_t kPullBytes = 1u << 20;

using pull2 = double __attribute__((ext_vector_type(2)));
__global__ __launch_bounds__(256) void pull_kernel(const pull2 *__restrict__ src, pull2 *__restrict__ dst,
                                                   size_t n2, const double *__restrict__ src1, double *__restrict__ dst1,
                                                   size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride)
        dst[i] = __builtin_nontemporal_load(src + i);
    if (blockIdx.x == 0 && threadIdx.x == 0 && (n & 1)) dst1[n - 1] = src1[n - 1];
}

// ("stream_stamps": the GPU's own clock before and behind every launch of a stream, digested at its destruction)
__global__ void stamp_kernel(unsigned long long *slot) { *slot = wall_clock64(); }

// ---- a lane: one engine's ring.  The engine's device is current in all of these. ------------------------------

// every slot's buffers for one kind of input, K timesteps of `step_words` doubles each, `step_bytes` of them pushed
int alloc_inputs(StreamLane *s, int feed, size_t step_words, size_t step_bytes, const char *what) {
    s->step_words[feed] = step_words;
    s->step_bytes[feed] = step_bytes;
    const size_t words = (size_t)s->K * step_words;
    hipError_t r = hipSuccess;
    for (StreamLane::Slot &sl : s->slots) {
        StreamLane::Slot::In &in = sl.in[feed];
        if (r == hipSuccess) r = in.h.alloc(words, hipHostMallocDefault);
        if (r == hipSuccess) r = in.d.alloc(words);
        if (r == hipSuccess && kFeedTable[feed].makes_signals) std::memset(in.h.p, 0, words * sizeof(double));
    }
    if (r != hipSuccess)
        return fail("%s: %s (%d steps of %zu bytes per slot, %d slots)", what, hipGetErrorString(r), s->K,
                    s->step_bytes[feed], s->depth);
    return 0;
}

// everything the lane holds on its engine's device goes back
void release_lane(StreamLane *s) {
    (void)hipStreamSynchronize(s->e->stream);
    if (s->h_stamp.p) {
        // launch i: [begin_i, end_i]; gap_i = begin_i - end_(i-1)   (wall_clock64: 100 MHz)
        const int n = (int)std::min<int64_t>(s->launches, 4096);
        const unsigned long long *stamp = s->h_stamp.p;
        std::vector<double> busy, gap;
        for (int i = 8; i < n; ++i) {
            busy.push_back((double)(stamp[4096 + i] - stamp[i]) * 0.01);
            gap.push_back((double)(stamp[i] - stamp[4096 + i - 1]) * 0.01);
        }
        for (int i = 0; i < (int)gap.size(); ++i)
            if (gap[i] > 200.0) std::fprintf(stderr, "qm_stream stamps: gap of %.1f us before launch %d\n", gap[i], i + 8);
        std::sort(busy.begin(), busy.end());
        std::sort(gap.begin(), gap.end());
        if (!busy.empty())
            std::fprintf(stderr, "qm_stream stamps: %d launches; launch busy us median %.1f p90 %.1f; gap between launches "
                         "us median %.1f p90 %.1f max %.1f\n", n, busy[busy.size() / 2], busy[busy.size() * 9 / 10],
                         gap[gap.size() / 2], gap[gap.size() * 9 / 10], gap.back());
        s->h_stamp.release();
    }
    if (s->copy_stream) (void)hipStreamSynchronize(s->copy_stream);
    {
        PoolReleaseScope one_wait;
        for (StreamLane::Slot &sl : s->slots) sl = StreamLane::Slot{};
        for (const FeedRow &row : kFeedTable)
            if (row.drop) row.drop(s);
    }
    if (s->copy_stream) park_stream(s->e->device, s->copy_stream);
    s->copy_stream = nullptr;
    s->order.clear();
}

// A timestep of the stream's kind into the slot being filled, which has room (fill_n < K): `write(dst)` puts the step
// into its pinned words.  0, or 2: that slot is the lane's oldest launch and holds results that have not been popped.
template <typename Write>
int fill(StreamLane *s, int feed, const char *what, Write write) {
    StreamLane::Slot &sl = s->slots[s->fill_slot];
    if (s->fill_n == 0 && sl.in_flight) {
        (void)fail("%s: all %d slots hold results that have not been popped", what, s->depth);
        return 2;
    }
    // (the slot's previous H2D has finished: its launch's results were popped)
    if (kFeedTable[feed].makes_signals && sl.in[kSignals].h.p)     // its first step: the ring's pinned slots hold this
        for (StreamLane::Slot &other : s->slots)                    // kind from here on, the signals' pinned buffers
            other.in[kSignals].h.release();                         // are given up
    write(sl.in[feed].h.p + (size_t)s->fill_n * s->step_words[feed]);
    ++s->fill_n;
    return 0;
}

// H2D, the launch and D2H of the slot being filled, which holds steps of kind `feed`: enqueue only
int launch_slot(StreamLane *s, int feed) {
    qm_engine *e = s->e;
    StreamLane::Slot &sl = s->slots[s->fill_slot];
    const int n = s->fill_n;
    // (not the row count alone -- another table of the same shape, e.g. a table_select switch or a
    // foreign load on the shared default engine, would be stacked and normalised as if it were the stream's)
    if (!e->have_lut || e->serial != s->table_serial || e->g.n_rows != s->n_rows)
        return fail("qm_stream: the engine's resident table changed under the stream (table #%llu with %d rows, "
                    "the stream was made on #%llu with %d): select the stream's table again, then push or flush",
                    (unsigned long long)(e->have_lut ? e->serial : 0), e->have_lut ? e->g.n_rows : 0,
                    (unsigned long long)s->table_serial, s->n_rows);
    const size_t kns = (size_t)s->K * s->ns;
    const size_t words = (size_t)n * s->step_words[feed];
    const double *h_in = sl.in[feed].h.p;
    double *d_in = sl.in[feed].d.p;
    const bool pull = e->cfg.stream_pull > 0 || (e->cfg.stream_pull < 0 && words * sizeof(double) <= kPullBytes);
    // ("stream_stamps" = 1, measurement: the GPU's clock before and behind every launch -- two one-thread kernels;
    // the digest goes to stderr when the stream is destroyed.  What found round 6's one-off stall: tools/diag_stream.py)
    constexpr int kStamps = 4096;
    const bool stamps = e->cfg.stream_stamps != 0 && s->launches < kStamps;   // (the first 4096 launches of a stream)
    if (stamps && !s->h_stamp.p) {
        if (s->h_stamp.ensure(2 * kStamps, hipHostMallocDefault)) return 1;
        std::memset(s->h_stamp.p, 0, 2 * kStamps * sizeof(unsigned long long));
    }
    if (stamps) hipLaunchKernelGGL(stamp_kernel, dim3(1), dim3(1), 0, e->stream, s->h_stamp.p + (s->launches % kStamps));
    if (pull) {
        const unsigned blocks = (unsigned)std::min<size_t>(4 * (size_t)e->n_cu, (words / 2 + 255) / 256 + 1);
        hipLaunchKernelGGL(pull_kernel, dim3(blocks), dim3(256), 0, e->stream,
                           reinterpret_cast<const pull2 *>(h_in), reinterpret_cast<pull2 *>(d_in),
                           words / 2, h_in, d_in, words);
        QM_HIP(hipGetLastError());
    } else {
        if (!s->copy_stream && acquire_stream(e->device, &s->copy_stream) != hipSuccess)
            return fail("qm_stream: no HIP stream for the input copies");
        QM_HIP(hipMemcpyAsync(d_in, h_in, words * sizeof(double), hipMemcpyHostToDevice, s->copy_stream));
        QM_HIP(hipEventRecord(sl.copied, s->copy_stream));
        QM_HIP(hipStreamWaitEvent(e->stream, sl.copied, 0));
    }
    s->pulled = pull;
    // The chain, all on the engine's stream, every kernel straight into the slot's next buffer.  What makes the n
    // steps' signals on the device: raw samples resampled to the scan rate, or every record's segment conditioned and
    // the gaps filled ...
    double *d_sig = sl.in[kSignals].d.p, *d_on = sl.in[kLogOnsets].d.p;
    if (feed == kRaw && s->rs.launch(e, d_in, d_sig, n)) return 1;
    if (feed == kSegments && s->seg.launch(e, d_in, d_sig, n)) return 1;
    // ... signals that are not conditioned yet -- pushed, or resampled here -- are filtered in place ...
    if ((feed == kSignals || feed == kRaw) && s->pre.launch(e, d_sig, d_sig, n)) return 1;
    // ... and the onset kernels make the slot's log-onsets of them.
    if (feed != kLogOnsets && s->on.launch(e, d_sig, nullptr, d_on, n)) return 1;
    // The results are a few KB per timestep: the combine kernel writes them STRAIGHT into the slot's
    // pinned host buffer (pinned memory is device-accessible under one address; the event behind the
    // launch makes them visible to the host) -- no D2H copy command, no third stream.  (With a copy on a
    // download stream of its own, 8 timesteps per launch ran at x1.03-1.09 of the resident step on the
    // example-sized grids; now x1.00, profiles/r05_ab_runs.txt.)
    double *out = sl.h_out.p;
    if (qm_engine_detect_batch(e, d_on, 1, n, s->T, s->fsmp, s->lsmp, s->available, s->n_nodes_total,
                               out, out + kns, reinterpret_cast<int64_t *>(out + 2 * kns), 1))
        return 1;
    if (stamps)
        hipLaunchKernelGGL(stamp_kernel, dim3(1), dim3(1), 0, e->stream, s->h_stamp.p + kStamps + (s->launches % kStamps));
    QM_HIP(hipEventRecord(sl.done, e->stream));
    sl.n = n;
    sl.taken = 0;
    sl.in_flight = true;
    s->order.push_back(s->fill_slot);
    s->launched_steps += n;
    ++s->launches;
    s->fill_slot = (s->fill_slot + 1) % s->depth;
    s->fill_n = 0;
    return 0;
}

// the next `take` timesteps of the lane's oldest launch, which has that many left; waits for the launch
int pop_oldest(StreamLane *s, int take, double *max_coa, double *max_norm_coa, int64_t *max_coa_idx) {
    StreamLane::Slot &sl = s->slots[s->order.front()];
    QM_HIP(hipEventSynchronize(sl.done));
    const size_t ns = (size_t)s->ns, kns = (size_t)s->K * ns;
    const double *src = sl.h_out.p + (size_t)sl.taken * ns;
    std::memcpy(max_coa, src, (size_t)take * ns * sizeof(double));
    std::memcpy(max_norm_coa, src + kns, (size_t)take * ns * sizeof(double));
    std::memcpy(max_coa_idx, src + 2 * kns, (size_t)take * ns * sizeof(int64_t));
    sl.taken += take;
    if (sl.taken == sl.n) {
        sl.in_flight = false;
        s->order.pop_front();
    }
    return 0;
}

// A stage that did not come about, on this lane or on a later one: what it took goes back and the lane is what it
// was before (the error text stays).
void stage_undo(StreamLane *s, int feed) {
    PoolReleaseScope one_wait;
    for (StreamLane::Slot &sl : s->slots) sl.in[feed] = {};
    kFeedTable[feed].drop(s);
}

// ---- the stream: one pipeline over its lanes ------------------------------------------------------------------
// Launches go round the lanes in push order, so a lane's next slot is in flight only when all n x depth launches
// are un-popped -- and then the oldest launch is on that lane: "pop the oldest launch, push again" still frees it.

int alive(const qm_stream *s, const char *what) {
    if (!s) return fail("%s: NULL argument", what);
    for (const auto &lane : s->lanes)
        if (!lane->e) return fail("%s: the stream's engine has been destroyed", what);
    return 0;
}

// launched and not yet popped, over all lanes
int64_t waiting(const qm_stream *s) {
    int64_t n = 0;
    for (const qm_stream::Launch &l : s->launched) n += l.left;
    return n;
}

// "before the first push" is over: something has been pushed into or launched from a lane
bool pushed_to(const qm_stream *s) {
    return std::any_of(s->lanes.begin(), s->lanes.end(),
                       [](const auto &lane) { return lane->fill_n > 0 || lane->launched_steps > 0; });
}

// ---- what a stream refuses by its kind of input: every text comes from kFeedTable ----------------------------------
// "has no ... (...)": the kind's own stage is not set
int has_stage(const qm_stream *s, int feed, const char *what) {
    return s->set[feed] ? 0 : fail("%s: the stream has no %s (%s)", what, kFeedTable[feed].noun, kFeedTable[feed].set);
}

// "this stream takes ... (...)": `by` names the taker's set call in a set call, its push in a push
int taken(const char *what, int taker, const char *by) {
    return fail("%s: this stream takes %s (%s): one stream, one kind of input", what, kFeedTable[taker].takes, by);
}

// May the stage of `feed` be set now?  In this order: the stage it stands on is there, it is not set yet, no other
// stage stands on the same one, nothing has been pushed, the engines live.
int may_set(const qm_stream *s, int feed, const char *what) {
    const FeedRow &row = kFeedTable[feed], &base = kFeedTable[row.after];
    if (row.after != kNothingYet && !s->set[row.after])
        return fail("%s: the stream has no %s (%s comes first)", what, base.noun, base.set);
    if (s->set[feed]) return fail("%s: the stream has its %s already (it is set once)", what, row.noun);
    for (int other = kLogOnsets; row.after != kNothingYet && other < kFeeds; ++other)
        if (other != feed && s->set[other] && kFeedTable[other].after == row.after)
            return taken(what, other, kFeedTable[other].set);
    if (pushed_to(s)) return fail("%s: the %s is set before the first push", what, row.word);
    return alive(s, what);
}

// May a step of `feed` be pushed now?  In this order: its stage is set, no stage stands on it (that one's kind is
// what crosses the bus then), and the stream has not taken another kind already.
int may_push(const qm_stream *s, int feed, const char *what) {
    if (has_stage(s, feed, what)) return 1;
    for (int above = kLogOnsets; above < kFeeds; ++above)
        if (s->set[above] && kFeedTable[above].after == feed) return taken(what, above, kFeedTable[above].push);
    if (s->feed != kNothingYet && s->feed != feed) return taken(what, s->feed, kFeedTable[s->feed].push);
    return 0;
}

// the lane being filled sends what its slot holds (its device is current); the next lane is filled from here on
int send(qm_stream *s) {
    StreamLane *lane = s->lanes[s->cur].get();
    const int n = lane->fill_n;
    if (launch_slot(lane, s->feed)) return 1;
    s->launched.push_back({s->cur, n});
    s->cur = (s->cur + 1) % (int)s->lanes.size();
    return 0;
}

// ... the same from outside a lane's device; nothing to send is fine
int flush(qm_stream *s) {
    StreamLane *lane = s->lanes[s->cur].get();
    if (lane->fill_n == 0) return 0;
    DeviceGuard guard(lane->e->device);
    return send(s);
}

// a stage on every lane or on none: where a lane refuses, it and the lanes before it give back what they took
template <typename Build>
int stage_every_lane(qm_stream *s, int feed, Build build) {
    for (size_t i = 0; i < s->lanes.size(); ++i) {
        DeviceGuard guard(s->lanes[i]->e->device);
        if (!build(s->lanes[i].get())) continue;
        for (size_t j = 0; j <= i; ++j) {
            DeviceGuard undo(s->lanes[j]->e->device);
            stage_undo(s->lanes[j].get(), feed);
        }
        return 1;
    }
    s->set[feed] = true;
    return 0;
}

// A timestep of kind `feed` into the lane being filled; `write(lane, dst)` puts it into the slot's pinned words.
template <typename Write>
int push_step(qm_stream *s, int feed, Write write) {
    const char *what = kFeedTable[feed].push;
    if (alive(s, what) || may_push(s, feed, what)) return 1;
    // A full slot whose launch FAILED (the table changed under the stream, no memory, a refused step) is still
    // waiting to go out: it goes first, or this call fails as that one did -- never a copy past the slot's
    // K timesteps (the next push used to write one timestep behind the pinned buffer and launch
    // K + 1 of them).  This timestep then goes to the next lane, not behind it on the same one.
    if (s->lanes[s->cur]->fill_n >= s->lanes[s->cur]->K && flush(s)) return 1;
    StreamLane *lane = s->lanes[s->cur].get();
    DeviceGuard guard(lane->e->device);
    if (const int rc = fill(lane, feed, what, [&](double *dst) { write(lane, dst); })) return rc;
    s->feed = feed;
    return lane->fill_n < lane->K ? 0 : send(s);
}

// ... of the kinds whose step is one array: a plain copy of the bytes a step of that kind has
int push_array(qm_stream *s, const void *step, int feed) {
    if (!step || !s) return fail("%s: NULL argument", kFeedTable[feed].push);
    return push_step(s, feed, [&](const StreamLane *lane, double *dst) { host_copy(dst, step, lane->step_bytes[feed]); });
}

// One lane per engine, on tables the caller has found equal; `what` is the entry point's name.
int create(qm_engine *const *engines, int n_engines, const char *what, int32_t t_samples, int32_t fsmp, int32_t lsmp,
           int32_t available, int64_t n_nodes_total, int32_t steps_per_launch, int32_t depth, qm_stream **out) {
    if (steps_per_launch < 1 || steps_per_launch > 4096)
        return fail("%s: steps_per_launch must be in 1..4096 (got %d)", what, steps_per_launch);
    if (depth < 2 || depth > 64) return fail("%s: depth must be in 2..64 (got %d)", what, depth);
    // (destroyed as any stream is if a step below fails: a lane not yet on its engine's list, which destroy does not mind)
    std::unique_ptr<qm_stream, decltype(&qm_stream_destroy)> s(new qm_stream(), qm_stream_destroy);
    for (int r = 0; r < n_engines; ++r) {
        qm_engine *e = engines[r];
        int ns = 0;
        if (check_step(e, t_samples, fsmp, lsmp, available, &ns)) return 1;
        if ((int64_t)steps_per_launch * ns >= INT32_MAX) return fail("%s: too many samples per launch", what);
        DeviceGuard guard(e->device);
        s->lanes.emplace_back(new StreamLane());
        StreamLane *lane = s->lanes.back().get();
        lane->e = e;
        lane->n_rows = e->g.n_rows;
        lane->table_serial = e->serial;
        lane->T = t_samples; lane->fsmp = fsmp; lane->lsmp = lsmp; lane->available = available; lane->ns = ns;
        lane->K = steps_per_launch; lane->depth = depth;
        lane->n_nodes_total = n_nodes_total > 0 ? n_nodes_total : e->n_nodes;
        // (the copy stream is taken at the first launch that copies: slots that are pulled never need one)
        lane->slots.resize((size_t)depth);
        const size_t out_bytes = 3 * (size_t)lane->K * ns * sizeof(double);
        for (StreamLane::Slot &sl : lane->slots) {
            hipError_t err = sl.h_out.alloc(out_bytes / sizeof(double), hipHostMallocDefault);
            for (Event *ev : {&sl.copied, &sl.done})
                if (err == hipSuccess) err = ev->create(hipEventDisableTiming);
            if (err != hipSuccess)
                return fail("%s: %s (%d steps of %zu bytes of results per slot, %d slots)", what,
                            hipGetErrorString(err), lane->K, out_bytes / lane->K, depth);
        }
        const size_t words = (size_t)lane->n_rows * lane->T;
        if (alloc_inputs(lane, kLogOnsets, words, words * sizeof(double), what)) return 1;
        e->streams.push_back(lane);
    }
    *out = s.release();
    return 0;
}

}  // namespace

void streams_orphan(qm_engine *e) {
    for (StreamLane *lane : e->streams) {
        release_lane(lane);
        lane->e = nullptr;
    }
    e->streams.clear();
}

extern "C" {

int qm_stream_create(qm_engine *e, int32_t t_samples, int32_t fsmp, int32_t lsmp, int32_t available,
                     int64_t n_nodes_total, int32_t steps_per_launch, int32_t depth, qm_stream **out) {
    if (!e || !out) return fail("qm_stream_create: NULL argument");
    *out = nullptr;
    return create(&e, 1, "qm_stream_create", t_samples, fsmp, lsmp, available, n_nodes_total, steps_per_launch, depth,
                  out);
}

int qm_stream_create_replicas(qm_engine *const *engines, int32_t n_engines, int32_t t_samples, int32_t fsmp,
                              int32_t lsmp, int32_t available, int64_t n_nodes_total, int32_t steps_per_launch,
                              int32_t depth, qm_stream **out) {
    if (!engines || !out) return fail("qm_stream_create_replicas: NULL argument");
    *out = nullptr;
    if (n_engines < 1) return fail("qm_stream_create_replicas: at least one engine is needed (got %d)", n_engines);
    for (int r = 0; r < n_engines; ++r) {
        if (!engines[r]) return fail("qm_stream_create_replicas: replica %d is NULL", r);
        for (int q = 0; q < r; ++q)
            if (engines[q] == engines[r])
                return fail("qm_stream_create_replicas: replicas %d and %d are the same engine (two engines on one "
                            "device are fine, one engine twice is not)", q, r);
        if (!engines[r]->have_lut) return fail("qm_stream_create_replicas: replica %d holds no travel-time table", r);
    }
    const qm_engine *lead = engines[0];
    uint64_t d0 = 0;
    if (qm_engine_table_digest(engines[0], &d0)) return 1;
    for (int r = 1; r < n_engines; ++r) {
        const qm_engine *e = engines[r];
        if (e->g.n_rows != lead->g.n_rows || e->g.nx != lead->g.nx || e->g.ny != lead->g.ny || e->g.nz != lead->g.nz ||
            e->node_offset != lead->node_offset)
            return fail("qm_stream_create_replicas: replica %d holds a table of another shape (%d x %d x %d nodes, "
                        "%d rows, node offset %lld) than replica 0 (%d x %d x %d, %d rows, node offset %lld)", r,
                        e->g.nx, e->g.ny, e->g.nz, e->g.n_rows, (long long)e->node_offset, lead->g.nx, lead->g.ny,
                        lead->g.nz, lead->g.n_rows, (long long)lead->node_offset);
        uint64_t d = 0;
        if (qm_engine_table_digest(engines[r], &d)) return 1;
        if (d != d0) return fail("qm_stream_create_replicas: replica %d holds another table than replica 0", r);
    }
    return create(engines, n_engines, "qm_stream_create_replicas", t_samples, fsmp, lsmp, available, n_nodes_total,
                  steps_per_launch, depth, out);
}

void qm_stream_destroy(qm_stream *s) {
    if (!s) return;
    for (const auto &lane : s->lanes) {
        if (!lane->e) continue;                         // (orphaned by qm_engine_destroy: released there)
        DeviceGuard guard(lane->e->device);
        release_lane(lane.get());
        auto &list = lane->e->streams;
        list.erase(std::remove(list.begin(), list.end(), lane.get()), list.end());
    }
    delete s;
}

int qm_stream_push(qm_stream *s, const double *log_onsets) { return push_array(s, log_onsets, kLogOnsets); }
int qm_stream_push_signals(qm_stream *s, const double *signals) { return push_array(s, signals, kSignals); }
int qm_stream_push_raw(qm_stream *s, const void *raw) { return push_array(s, raw, kRaw); }

int qm_stream_set_resample_stage(qm_stream *s, int32_t n_traces, const int64_t *records, const double *sos_lp,
                                 int32_t n_lowpass, int32_t n_sections_lp, int detrend, const int32_t *taper_table,
                                 int32_t n_tapers, const double *taper_weights, int64_t n_taper_weights,
                                 int32_t t_samples, int raw_dtype, int64_t total_raw_samples) {
    const char *what = kFeedTable[kRaw].set;
    if (!s) return fail("%s: NULL argument", what);
    if (may_set(s, kRaw, what)) return 1;
    const StreamLane *lead = s->lanes[0].get();
    if (t_samples != lead->T || n_traces != lead->pre.n_traces)
        return fail("%s: %d traces of %d samples, the onset stage takes %d of %d", what, n_traces, t_samples,
                    lead->pre.n_traces, lead->T);
    if (total_raw_samples > 0 &&
        (double)lead->K * (double)ResampleStage::step_doubles(raw_dtype, total_raw_samples) * 8.0 >= 0x1p40)
        return fail("%s: too many raw samples per launch", what);
    return stage_every_lane(s, kRaw, [&](StreamLane *lane) {
        // (the signals' pinned buffers are given up at the first qm_stream_push_raw: until then nothing is lost)
        return lane->rs.build(lane->e, what, lane->K, raw_dtype, total_raw_samples, n_traces, t_samples, records, sos_lp,
                              n_lowpass, n_sections_lp, detrend, taper_table, n_tapers, taper_weights, n_taper_weights) ||
               alloc_inputs(lane, kRaw, lane->rs.step_words(), lane->rs.step_bytes(), what);
    });
}

int qm_stream_set_onset_stage(qm_stream *s, int32_t n_traces, const int32_t *trace_row, const int32_t *trace_filter,
                              const double *sos, int32_t n_filters, int32_t n_sections, int detrend,
                              const double *taper_left, int32_t n_left, const double *taper_right, int32_t n_right,
                              const int32_t *nsta, const int32_t *nlta, int transform, int position,
                              int32_t taper_pad, double min_onset_value) {
    const char *what = kFeedTable[kSignals].set;
    if (!s) return fail("%s: NULL argument", what);
    if (may_set(s, kSignals, what)) return 1;
    const StreamLane *lead = s->lanes[0].get();
    if ((int64_t)lead->K * n_traces * lead->T >= INT32_MAX || (int64_t)lead->K * lead->n_rows * lead->T >= INT32_MAX)
        return fail("%s: too many samples per launch", what);
    return stage_every_lane(s, kSignals, [&](StreamLane *lane) {
        const size_t words = (size_t)n_traces * lane->T;
        return lane->pre.build(lane->e, what, lane->K, n_traces, lane->T, trace_filter, sos, n_filters, n_sections,
                               detrend, taper_left, n_left, taper_right, n_right, /*zero_phase=*/1) ||
               lane->on.build(lane->e, what, lane->K, n_traces, lane->T, trace_row, lane->n_rows, nsta, nlta, transform,
                              position, taper_pad, min_onset_value) ||
               alloc_inputs(lane, kSignals, words, words * sizeof(double), what);
    });
}

int qm_stream_set_segment_feed(qm_stream *s, int32_t max_segments, int64_t max_taper_weights, int second_taper,
                               double fill_value) {
    const char *what = kFeedTable[kSegments].set;
    if (!s) return fail("%s: NULL argument", what);
    if (may_set(s, kSegments, what)) return 1;
    if (max_segments < 1) return fail("%s: max_segments must be at least 1 (got %d)", what, max_segments);
    if (max_taper_weights < 0)
        return fail("%s: max_taper_weights must be at least 0 (got %lld)", what, (long long)max_taper_weights);
    if (!std::isfinite(fill_value)) return fail("%s: fill_value %g is not finite", what, fill_value);
    return stage_every_lane(s, kSegments, [&](StreamLane *lane) {
        return lane->seg.adopt(what, lane->K, lane->pre, max_segments, max_taper_weights, second_taper, fill_value) ||
               alloc_inputs(lane, kSegments, lane->seg.step_words(), lane->seg.step_bytes(), what);
    });
}

int qm_stream_push_segments(qm_stream *s, const double *signals, const int64_t *records, int32_t n_segments,
                            const double *taper_weights, int64_t n_taper_weights) {
    const char *what = kFeedTable[kSegments].push;
    if (!s || !signals || !records) return fail("%s: NULL argument", what);
    if (has_stage(s, kSegments, what) || alive(s, what)) return 1;
    // the records, on the caller's thread: the kernel takes them as they are
    const StreamLane *lead = s->lanes[0].get();
    if (n_taper_weights < 0 || (n_taper_weights > 0 && !taper_weights))
        return fail("%s: %lld taper weights without their array", what, (long long)n_taper_weights);
    if (n_segments > lead->seg.max_segments)
        return fail("%s: %d segments, the feed was set for up to %d (max_segments)", what, n_segments,
                    lead->seg.max_segments);
    if (n_taper_weights > lead->seg.max_weights)
        return fail("%s: %lld taper weights, the feed was set for up to %lld (max_taper_weights)", what,
                    (long long)n_taper_weights, (long long)lead->seg.max_weights);
    if (check_segment_records(what, lead->pre.n_traces, lead->T, records, n_segments, n_taper_weights)) return 1;
    return push_step(s, kSegments, [&](const StreamLane *lane, double *dst) {
        lane->seg.pack(dst, signals, records, n_segments, taper_weights, n_taper_weights);
    });
}

int qm_stream_flush(qm_stream *s) {
    if (alive(s, "qm_stream_flush")) return 1;
    return flush(s);
}

int qm_stream_pending(qm_stream *s, int32_t *launched_not_popped, int32_t *pushed_not_launched) {
    if (alive(s, "qm_stream_pending")) return 1;
    if (launched_not_popped) *launched_not_popped = (int32_t)waiting(s);
    if (pushed_not_launched) *pushed_not_launched = s->lanes[s->cur]->fill_n;
    return 0;
}

int qm_stream_pop(qm_stream *s, int32_t n_steps, double *max_coa, double *max_norm_coa,
                  int64_t *max_coa_idx) {
    if (!max_coa || !max_norm_coa || !max_coa_idx) return fail("qm_stream_pop: NULL argument");
    if (alive(s, "qm_stream_pop")) return 1;
    if (n_steps < 0 || n_steps > waiting(s))
        return fail("qm_stream_pop: %d steps asked for, %lld launched and not yet popped (%d pushed into "
                    "a launch that has not gone out: qm_stream_flush)", n_steps, (long long)waiting(s),
                    s->lanes[s->cur]->fill_n);
    const size_t ns = (size_t)s->lanes[0]->ns;
    for (int k = 0; k < n_steps;) {
        qm_stream::Launch &l = s->launched.front();
        StreamLane *lane = s->lanes[l.lane].get();
        const int take = std::min(n_steps - k, l.left);
        DeviceGuard guard(lane->e->device);
        if (pop_oldest(lane, take, max_coa + k * ns, max_norm_coa + k * ns, max_coa_idx + k * ns)) return 1;
        k += take;
        l.left -= take;
        if (l.left == 0) s->launched.pop_front();
    }
    return 0;
}

}  // extern "C"
