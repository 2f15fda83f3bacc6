// qm_config.hip -- the table of the engine's tunables and the two functions over it (qm_config.hpp).  Host code only.
#include "qm_config.hpp"

#include <cstring>

namespace {

using C = EngineConfig;

constexpr Tunable flag(const char *name, int C::*m, unsigned effects = 0) {
    return {name, m, nullptr, Tunable::kFlag, 0, 1, 0, {}, nullptr, effects};
}
constexpr Tunable range(const char *name, int C::*m, int64_t lo, int64_t hi, const char *refusal, unsigned effects = 0) {
    return {name, m, nullptr, Tunable::kRange, lo, hi, 0, {}, refusal, effects};
}
constexpr Tunable one_of(const char *name, int C::*m, int a, int b, int c, int d, const char *refusal,
                         unsigned effects = 0) {
    return {name, m, nullptr, Tunable::kSet, a, d, 4, {a, b, c, d}, refusal, effects};
}

}  // namespace

const Tunable kTunables[] = {
    range("brick_x", &C::brick_x, 0, 64, "brick_x must be in 0..64 (0 = automatic)"),      // (an explicit brick_x
    range("brick_y", &C::brick_y, 0, 64, "brick_y must be in 0..64 (0 = automatic)"),      // fills in the other two:
    range("brick_z", &C::brick_z, 0, 64, "brick_z must be in 0..64 (0 = automatic)"),      // config_set)
    one_of("samples_per_lane", &C::samples_per_lane, 0, 1, 2, 4, "samples_per_lane must be 0 (automatic), 1, 2 or 4"),
    range("waves", &C::waves, 1, 16, "waves must be 1..16", kUserWaves),
    {"groups", &C::groups, nullptr, Tunable::kAtLeast, 0, 0, 0, {}, "groups must be >= 0", 0},
    range("rounds", &C::rounds, 1, 1024, "rounds must be in 1..1024", kUserRounds),
    range("lds_bytes", &C::lds_bytes, 1024, 160 * 1024, "lds_bytes must be in 1 KiB..160 KiB", kUserLds),   // (stored
                                                                            // rounded down to 16: config_set)
    flag("force_direct", &C::force_direct),
    flag("generic", &C::generic),
    flag("exact", &C::exact),
    range("scan_waves", &C::scan_waves, 1, 4096, "scan_waves must be in 1..4096"),
    {"chunk_bytes", nullptr, &C::chunk_bytes, Tunable::kAtLeast, 1 << 20, 0, 0, {}, "chunk_bytes must be >= 1 MiB", 0},
    range("pair", &C::pair, 0, 2, "pair must be 0 (off), 1 (automatic) or 2 (any scan length)"),
    flag("screen", &C::screen),
    one_of("screen_pairs", &C::screen_pairs, 0, 1, 2, 4, "screen_pairs must be 0, 1, 2 or 4", kVoidScreen),
    flag("screen_brick16", &C::screen_brick16, kVoidScreen),
    range("screen_big", &C::screen_big, -1, 1, "screen_big must be -1 (automatic), 0 or 1", kVoidScreen),
    range("shift", &C::shift, -1, 1, "shift must be -1 (automatic), 0 (off) or 1"),
    one_of("shift_waves", &C::shift_waves, 0, 4, 8, 12, "shift_waves must be 0 (automatic), 4, 8 or 12", kVoidShift),
    range("shift_lazy", &C::shift_lazy, -1, 1, "shift_lazy must be -1 (automatic), 0 or 1"),
    flag("shift_tail", &C::shift_tail),
    range("shift_rows_direct", &C::shift_rows_direct, 0, 2, "shift_rows_direct must be 0, 1 or 2", kVoidShift),
    range("shift_wide", &C::shift_wide, -1, 1, "shift_wide must be -1 (automatic), 0 (off) or 1"),
    range("shift_wide_rows", &C::shift_wide_rows, 0, 2,
          "shift_wide_rows must be 0 (never), 1 (where all rows do not fit) or 2 (always)", kVoidShiftWide),
    range("stream_pull", &C::stream_pull, -1, 1, "stream_pull must be -1 (slots of <= 1 MB), 0 (never) or 1 (always)"),
    flag("stream_stamps", &C::stream_stamps),
    flag("preproc_skew", &C::preproc_skew),
    range("tie_rule", &C::tie_rule, 0, 1, "tie_rule must be 0 (largest sum) or 1 (the reference's exp rule)"),
    flag("tie_sets", &C::tie_sets),
    flag("trigger_timing", &C::trigger_timing),
    flag("log_timing", &C::log_timing, kResetTimingLog),
};
const int kNumTunables = (int)(sizeof(kTunables) / sizeof(kTunables[0]));

static const Tunable *find_tunable(const char *key) {
    for (const Tunable &t : kTunables)
        if (std::strcmp(t.name, key) == 0) return &t;
    return nullptr;
}

int config_set(EngineConfig &c, const char *key, int64_t v, unsigned *effects) {
    const Tunable *t = find_tunable(key);
    if (!t) return fail("unknown config key '%s'", key);
    bool ok = true;
    switch (t->check) {
    case Tunable::kFlag: v = v ? 1 : 0; break;
    case Tunable::kRange: ok = v >= t->lo && v <= t->hi; break;
    case Tunable::kAtLeast: ok = v >= t->lo; break;
    case Tunable::kSet:
        ok = false;
        for (int i = 0; i < t->n_allowed; ++i) ok = ok || v == t->allowed[i];
        break;
    }
    if (!ok) return fail("%s", t->refusal);
    if (t->wide) c.*t->wide = v;
    else c.*t->member = (int)v;
    // the specials
    if (t->member == &C::lds_bytes) c.lds_bytes = (int)(v / 16 * 16);
    if ((t->member == &C::brick_x || t->member == &C::brick_y || t->member == &C::brick_z) && c.brick_x > 0) {
        if (c.brick_y < 1) c.brick_y = 1;              // an explicit shape needs all three
        if (c.brick_z < 1) c.brick_z = 1;
    }
    if (t->effects & kUserWaves) c.user_waves = true;
    if (t->effects & kUserRounds) c.user_rounds = true;
    if (t->effects & kUserLds) c.user_lds = true;
    if (effects) *effects = t->effects;
    return 0;
}

bool config_get(const EngineConfig &c, const char *key, int64_t *v) {
    const Tunable *t = find_tunable(key);
    if (!t) return false;
    *v = t->wide ? c.*t->wide : (int64_t)(c.*t->member);
    return true;
}
