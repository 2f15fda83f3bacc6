// ownership_check.cpp -- the owning handles of csrc/qm_engine.hpp (DevBuf, PinnedBuf, Event) and the structs made of
// them, on the CPU under the sanitizers: every block is freed exactly once, a dropped owner leaves nothing behind,
// device_bytes() counts every buffer, and a teardown inside one PoolReleaseScope is one device-wide wait.  A stand-alone
// host program: the pool, pinned memory and events are replaced below by malloc and counters that end the program on a
// block freed twice or never handed out; LeakSanitizer (part of AddressSanitizer here) fails the run on a leak.
//
//   cd quakemigrate_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined ../../tools/ownership_check.cpp -o /tmp/ownership_check \
//         && /tmp/ownership_check
//
// Prints one line per group and "ownership_check: ok"; any mismatch or sanitizer report ends it with a non-zero status.
#include "../quakemigrate_amd/csrc/qm_engine.hpp"

#include <map>
#include <type_traits>

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            std::fprintf(stderr, "ownership_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                  \
        }                                                                                  \
    } while (0)

int fail(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vfprintf(stderr, fmt, ap);
    va_end(ap);
    std::fputc('\n', stderr);
    return 1;
}

// one kind of resource: what is out (address -> bytes), how much was handed out and taken back so far
struct Ledger {
    const char *what;
    std::map<void *, size_t> live;
    size_t live_bytes = 0, handed_out = 0, taken_back = 0;
    void *give(size_t bytes) {
        void *p = std::malloc(bytes ? bytes : 1);
        CHECK(p != nullptr);
        live[p] = bytes;
        live_bytes += bytes;
        ++handed_out;
        return p;
    }
    void take(void *p) {
        auto it = live.find(p);
        if (it == live.end()) {
            std::fprintf(stderr, "ownership_check: %s %p freed twice or never handed out\n", what, p);
            std::abort();
        }
        live_bytes -= it->second;
        live.erase(it);
        ++taken_back;
        std::free(p);
    }
};
static Ledger g_pool{"pool block"}, g_pinned{"pinned block"}, g_events{"event"};
// waits: a pool_free outside a scope, or an outermost scope that ends with something deferred
static int g_depth = 0, g_deferred = 0, g_waits = 0;

hipError_t pool_alloc(void **out, size_t bytes) {
    *out = g_pool.give(bytes);
    return hipSuccess;
}
void pool_free(void *p) {
    g_pool.take(p);
    if (g_depth > 0) ++g_deferred;
    else ++g_waits;
}
PoolReleaseScope::PoolReleaseScope() { ++g_depth; }
PoolReleaseScope::~PoolReleaseScope() {
    if (--g_depth > 0 || g_deferred == 0) return;
    ++g_waits;
    g_deferred = 0;
}
hipError_t pinned_alloc(void **out, size_t bytes, unsigned) {
    *out = g_pinned.give(bytes);
    return hipSuccess;
}
void pinned_free(void *p) { g_pinned.take(p); }
hipError_t event_create(hipEvent_t *out, unsigned) {
    *out = static_cast<hipEvent_t>(g_events.give(1));
    return hipSuccess;
}
void event_destroy(hipEvent_t ev) { g_events.take(ev); }

static bool nothing_out() { return g_pool.live.empty() && g_pinned.live.empty() && g_events.live.empty(); }

template <typename H>
constexpr bool move_only = !std::is_copy_constructible<H>::value && !std::is_copy_assignable<H>::value &&
                           std::is_nothrow_move_constructible<H>::value && std::is_nothrow_move_assignable<H>::value;
static_assert(move_only<DevBuf<int32_t>> && move_only<DevBuf<double>>, "DevBuf is move-only");
static_assert(move_only<PinnedBuf<double>>, "PinnedBuf is move-only");
static_assert(move_only<Event>, "Event is move-only");
// (std::vector<TableSlot> grows by moving its slots only if the move cannot throw; else it would need copies)
static_assert(move_only<TableState> && move_only<TableSlot>, "a parked table moves, never copies");

// construct, fill, move-construct, move-assign onto a non-empty target, self-move-assign, release, scope exit
template <typename H, typename Fill, typename Held>
static void handle_checks(Ledger &ledger, Fill fill, Held held) {
    const size_t out0 = ledger.handed_out, back0 = ledger.taken_back;
    {
        H a;
        CHECK(held(a) == nullptr);
        fill(a, 10);
        const void *first = held(a);
        CHECK(first != nullptr && ledger.live.size() == 1);
        H b(std::move(a));
        CHECK(held(a) == nullptr && held(b) == first && ledger.live.size() == 1);
        H c;
        fill(c, 5);
        CHECK(ledger.live.size() == 2);
        c = std::move(b);                               // (what c held goes back)
        CHECK(held(b) == nullptr && held(c) == first && ledger.live.size() == 1);
        H &same = c;
        c = std::move(same);
        CHECK(held(c) == first && ledger.live.size() == 1);
        c.release();
        CHECK(held(c) == nullptr && ledger.live.empty());
        c.release();                                    // (an empty handle: nothing happens)
        H d;
        fill(d, 3);
        CHECK(ledger.live.size() == 1);
    }
    CHECK(ledger.live.empty() && ledger.live_bytes == 0);
    CHECK(ledger.handed_out - out0 == 3 && ledger.taken_back - back0 == 3);
}

// every buffer of a layout, each of another size
static void fill_bricks(BrickLayout &l, size_t &k) {
    CHECK(!l.raw.ensure(++k) && !l.meta.ensure(++k) && !l.total.ensure(++k) && !l.list.ensure(++k) && !l.rel.ensure(++k));
}
static void fill_shift(ShiftLayout &l, size_t &k) {
    fill_bricks(l, k);
    CHECK(!l.fit.ensure(++k) && !l.stream.ensure(++k) && !l.wmeta.ensure(++k) && !l.wtotal.ensure(++k) &&
          !l.wstream.ensure(++k));
}
static void fill_table(TableState &t, size_t k) {
    CHECK(!t.d_lut.ensure(++k));
    fill_bricks(t.r2(), k);
    fill_bricks(t.pair, k);
    fill_bricks(t.screen, k);
    fill_shift(t.sh, k);
    fill_shift(t.shw, k);
    t.have_lut = true;
}

static void stage_records(PreprocStage &pre, OnsetStage &on, ResampleStage &rs) {
    CHECK(!pre.coef.ensure(24) && !pre.meta.ensure(5));
    CHECK(!on.meta.ensure(11) && !on.sta.ensure(500) && !on.lta.ensure(500));
    CHECK(!rs.meta.ensure(22) && !rs.coef.ensure(26) && !rs.scratch.ensure(402));
}

// every buffer of every scratch record (58 pool blocks, the pinned flag ring) and the events of both stage clocks (24)
static void scratch_records(CallStaging &st, PickStage &pk, AmplitudeStage &am, TriggerStage &tr, ScanmseedCodec &sm,
                            TieScratch &ti, ScreenScratch &sw, FitScratch &fi) {
    size_t k = 300;
    CHECK(!st.sig.ensure(++k) && !st.raw.ensure(++k) && !st.pre_out.ensure(++k) && !st.rs_raw.ensure(++k));
    CHECK(!pk.val.ensure(++k) && !pk.meta.ensure(++k));
    CHECK(!am.work.ensure(++k) && !am.scratch.ensure(++k) && !am.coef.ensure(++k) && !am.val.ensure(++k) &&
          !am.meta.ensure(++k) && !am.idx.ensure(++k));
    CHECK(!tr.x.ensure(++k) && !tr.par.ensure(++k) && !tr.cnt.ensure(++k) && !tr.tot.ensure(++k) && !tr.run.ensure(++k) &&
          !tr.cand.ensure(++k) && !tr.val.ensure(++k));
    CHECK(!sm.x.ensure(++k) && !sm.f.ensure(++k) && !sm.fac.ensure(++k) && !sm.bytes.ensure(++k) && !sm.map.ensure(++k) &&
          !sm.out.ensure(++k) && !sm.tile.ensure(++k) && !sm.rec.ensure(++k) && !sm.tot.ensure(++k) && !sm.off.ensure(++k));
    CHECK(!ti.zext.ensure(++k) && !ti.zgrid.ensure(++k) && !ti.z.ensure(++k) && !ti.pairs.ensure(++k) &&
          !ti.imin.ensure(++k) && !ti.count.ensure(++k) && !ti.cands.ensure(++k) && !ti.emax.ensure(++k) &&
          !ti.keys.ensure(++k));
    CHECK(!sw.counts.ensure(++k) && !sw.cells.ensure(++k) && !sw.work.ensure(++k) && !sw.flags.ensure(++k) &&
          !sw.onq.ensure(++k) && !sw.cell.ensure(++k) && !sw.gmax.ensure(++k) && !sw.pm.ensure(++k) &&
          !sw.sparams.ensure(++k) && !sw.rowmax.ensure(++k) && !sw.ssum.ensure(++k) && !sw.cand_z.ensure(++k) &&
          !sw.cand_idx.ensure(++k));
    CHECK(!sw.h_flags.ensure(2 * kFlagRing, hipHostMallocDefault));
    CHECK(!fi.a.ensure(++k) && !fi.b.ensure(++k) && !fi.c.ensure(++k) && !fi.part.ensure(++k) && !fi.val.ensure(++k) &&
          !fi.win.ensure(++k) && !fi.pidx.ensure(++k));
    CHECK(k == 300 + 58);
    CHECK(!tr.clock.ensure_events() && !sm.clock.ensure_events());
    CHECK(tr.clock.ev.size() == 2 * qm::kTrigStages && sm.clock.ev.size() == 2 * qm::kSmsStages);
}

static void fill_engine(qm_engine *e) {
    fill_table(*e, 100);
    e->slots.emplace_back();
    fill_table(e->slots.back().state, 200);
    CHECK(!e->d_onsets.ensure(900) && !e->d_pmax.ensure(390) && !e->d_pidx.ensure(390) && !e->d_out_a.ensure(390) &&
          !e->d_digest.ensure(1));
    stage_records(e->pre_stage, e->on_stage, e->rs_stage);
    scratch_records(e->staging, e->picks, e->amps, e->trig, e->sms, e->tie, e->sweep, e->fit);
    CHECK(e->ev0.create() == hipSuccess && e->ev1.create() == hipSuccess);
    for (int i = 0; i < 2; ++i) {
        Event ev;
        CHECK(ev.create() == hipSuccess);
        e->ev_log.push_back(std::move(ev));
    }
    CHECK(g_pool.live.size() == 2 * 36 + 5 + 8 + 58 && g_pinned.live.size() == 1 && g_events.live.size() == 4 + 24);
}

// a create path that gives up half-way: what the engine holds by then goes back, behind one wait
static int early_return() {
    PoolReleaseScope one_wait;
    std::unique_ptr<qm_engine> e(new qm_engine());
    fill_engine(e.get());
    if (e->have_lut) return 1;
    return 0;
}

int main() {
    handle_checks<DevBuf<int32_t>>(g_pool, [](DevBuf<int32_t> &h, size_t n) { CHECK(!h.ensure(n) && h.n == n); },
                                   [](const DevBuf<int32_t> &h) -> const void * { CHECK((h.p == nullptr) == (h.n == 0)); return h.p; });
    handle_checks<PinnedBuf<double>>(g_pinned, [](PinnedBuf<double> &h, size_t n) { CHECK(!h.ensure(n, hipHostMallocDefault) && h.n == n); },
                                     [](const PinnedBuf<double> &h) -> const void * { CHECK((h.p == nullptr) == (h.n == 0)); return h.p; });
    handle_checks<Event>(g_events, [](Event &h, size_t) { CHECK(h.create(hipEventDisableTiming) == hipSuccess); },
                         [](const Event &h) -> const void * { return h.ev.get(); });
    CHECK(nothing_out() && g_waits == 3);               // (the three DevBufs went back outside any scope: a wait each)
    std::printf("handles: device, pinned, event -- each block freed once, moved-from handles empty\n");

    {
        TableState t, empty;
        fill_table(t, 0);
        CHECK(g_pool.live.size() == 36);
        CHECK(t.device_bytes() == g_pool.live_bytes);   // (a buffer missing from a sum shows here)
        const size_t bytes = g_pool.live_bytes, back = g_pool.taken_back;
        std::swap(t, empty);
        CHECK(g_pool.live_bytes == bytes && g_pool.taken_back == back);
        CHECK(t.device_bytes() == 0 && !t.have_lut && empty.device_bytes() == bytes && empty.have_lut);
        g_waits = 0;
        {
            PoolReleaseScope one_wait;
            empty = TableState{};
            CHECK(g_waits == 0);
        }
        CHECK(g_pool.live.empty() && g_pool.live_bytes == 0 && g_waits == 1);
        // parked tables: the vector grows from 1 to 5 slots, the state moves along
        std::vector<TableSlot> slots(1);
        fill_table(slots[0].state, 50);
        const size_t parked = g_pool.live_bytes, back2 = g_pool.taken_back;
        while (slots.size() < 5) {
            slots.emplace_back();
            slots.shrink_to_fit();                      // (every step reallocates)
        }
        CHECK(g_pool.live_bytes == parked && g_pool.taken_back == back2 && slots[0].state.device_bytes() == parked);
        std::swap(t, slots[0].state);
        CHECK(g_pool.live_bytes == parked && g_pool.taken_back == back2 && t.device_bytes() == parked);
        std::swap(t, slots[4].state);
        g_waits = 0;
        {
            PoolReleaseScope one_wait;
            slots[4].state = TableState{};
        }
        CHECK(g_pool.live.empty() && g_waits == 1);
    }
    std::printf("TableState: 36 buffers in device_bytes(), swaps move, an assignment in a scope is one wait\n");

    {
        qm_engine *e = new qm_engine();
        fill_engine(e);
        g_waits = 0;
        {
            PoolReleaseScope one_wait;
            delete e;
        }
        CHECK(nothing_out() && g_waits == 1);
        g_waits = 0;
        CHECK(early_return() == 1);
        CHECK(nothing_out() && g_waits == 1);
    }
    std::printf("qm_engine: deleted in a scope and dropped by a unique_ptr on an early return -- nothing out, one wait\n");

    {
        g_waits = 0;
        PoolReleaseScope one_wait;
        {
            PreprocStage pre;
            OnsetStage on;
            ResampleStage rs;
            stage_records(pre, on, rs);
            CHECK(g_pool.live.size() == 8);
            rs = ResampleStage{};                       // (a stage's undo)
            CHECK(g_pool.live.size() == 5 && rs.meta.p == nullptr);
        }
        CHECK(g_pool.live.empty() && g_waits == 0);
    }
    CHECK(nothing_out() && g_waits == 1);
    std::printf("stage records: out of scope with nothing out\n");

    {
        g_waits = 0;
        PoolReleaseScope one_wait;
        {
            CallStaging st;
            PickStage pk;
            AmplitudeStage am;
            TriggerStage tr;
            ScanmseedCodec sm;
            TieScratch ti;
            ScreenScratch sw;
            FitScratch fi;
            scratch_records(st, pk, am, tr, sm, ti, sw, fi);
            CHECK(g_pool.live.size() == 58 && g_pinned.live.size() == 1 && g_events.live.size() == 24);
        }
        CHECK(nothing_out() && g_waits == 0);
    }
    CHECK(nothing_out() && g_waits == 1);
    std::printf("scratch records: out of scope with nothing out\n");

    CHECK(g_pool.handed_out == g_pool.taken_back && g_pinned.handed_out == g_pinned.taken_back &&
          g_events.handed_out == g_events.taken_back);
    std::printf("ownership_check: ok\n");
    return 0;
}
