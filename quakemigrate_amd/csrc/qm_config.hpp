// qm_config.hpp -- the engine's tunables: one record (EngineConfig), one table with a row per key (kTunables: the
// check, the refusal text, what a change voids) and the two functions that are the only way in and out by name.
// Plain C++17, no HIP: qm_engine holds the record as `cfg`, qm_engine_config is config_set plus the effects,
// qm_engine_get falls back on config_get; tools/config_check.cpp walks the table on the CPU.
// The record is written by config_set only.  What the engine derives per table (the layout search's workgroup shape)
// lives with the table (TableState), not here.
#pragma once
#include <cstdint>

#pragma GCC visibility push(hidden)

int fail(const char *fmt, ...) __attribute__((format(printf, 1, 2)));     // qm_runtime.hip

struct EngineConfig {
    int brick_x = 0, brick_y = 0, brick_z = 0;   // 0 = choose the brick shape per table
    int samples_per_lane = 0;       // time tile = 64 x this; 0 = by table width
    int waves = 8;
    bool user_waves = false, user_lds = false;   // set explicitly: no automatic layout
    int groups = 0;
    int rounds = 12;                // automatic group count: grid = this many rounds over the slots
    bool user_rounds = false;       // ... set explicitly
    int lds_bytes = 80 * 1024;
    int force_direct = 0;
    int generic = 0;                // 1 = always the generic (any row count) LDS kernel
    int scan_waves = 32;            // find_max_coa of a volume: wavefronts per CU over the whole grid
    int exact = 1;                  // 1 = the exact-row-count kernel where one is built (see
                                    //     qm_launch.hpp), 0 = the chunked kernels only
    int64_t chunk_bytes = (int64_t)4 << 30;
    int pair = 1;                   // 1 = the 16-byte-operand kernel (qm_pair.hpp) where it applies
    int screen = 0;                 // 1 (opt-in): detect = float32 screening sweep + exact float64
                                    // refinement (qm_screen.hpp); 0: every node-sample in float64
    int screen_pairs = 0;           // pairs of samples per lane in the sweep (0 = automatic)
    int screen_brick16 = 0;         // also try 16x8x8 bricks for the sweep
    int screen_big = -1;            // 1: one 16-wave workgroup per CU with 160 KB of LDS; -1 = automatic
    int shift = -1;                         // -1: where the table qualifies, 0: never, 1: as -1 (explicit)
    int shift_waves = 0;                    // workgroup shape: 4 (two per CU), 12 (one per CU), 0 = automatic
    int shift_lazy = -1;                    // detect loop flavour: -1 automatic, 0 eager, 1 lazy arg-max
    int shift_tail = 1;                     // 1: a scan's remainder of <= 192 samples runs as one tail tile of
                                            // 64 / 128 / 192 samples; 0: whole tiles only (round 3)
    int shift_rows_direct = 1;
    int shift_wide = -1;                    // fused detect on WIDE tiles (384 samples, six per lane; round 6): -1 where
                                            // they fit and the scan holds at least one, 0 never, 1 as -1 (explicit)
    int shift_wide_rows = 1;                // ... on ROW BLOCKS where the windows of all rows do not fit (0: never,
                                            // 2: row blocks whatever fits -- tests)
    int stream_pull = -1;                   // qm_stream: a slot's pinned inputs pulled by a kernel on the engine's stream
                                            // instead of a copy command on another (-1: slots of <= 1 MB, 0, 1)
    int stream_stamps = 0;                  // qm_stream, measurement: GPU-clock stamps around every launch (stderr digest)
    int preproc_skew = 1;                   // pre-processing filter: 1 section s on lane s, one sample behind lane s - 1
                                            // (qm_preproc.hpp); 0: every section on one lane (the cross-check)
    int tie_rule = 0;                       // 0: largest float64 sum, lowest index among equal ones (default);
                                            // 1: the reference's rule on near-ties (qm_ties.hpp)
    int tie_sets = 1;                       // ... refined from a partial set PER BRICK where the stacking kernel has
                                            // that flavour (the shift-reuse fused detect); 0: round 5's sets of
                                            // four bricks everywhere (measurements)
    int trigger_timing = 0;                 // 1: HIP events around every stage of the trigger sequence (measurement)
    int log_timing = 0;                     // optional per-call timing log (bench): pairs of events around every
                                            // stacking launch
};

// What setting a key does besides storing the value: config_set reports it, its caller applies it.
enum ConfigEffect : unsigned {
    kVoidShift = 1u << 0,           // the resident table's 256-sample shift-reuse layout (sh) is rebuilt
    kVoidShiftWide = 1u << 1,       // ... its wide-tile layout (shw)
    kVoidScreen = 1u << 2,          // ... its screening layout
    kUserWaves = 1u << 3,           // user_waves / user_rounds / user_lds is set (config_set has done it)
    kUserRounds = 1u << 4,
    kUserLds = 1u << 5,
    kResetTimingLog = 1u << 6,      // the timing log starts over at its first event pair
};

struct Tunable {
    enum Check { kFlag, kRange, kAtLeast, kSet };
    const char *name;
    int EngineConfig::*member;      // where the value is stored, or ...
    int64_t EngineConfig::*wide;    // ... for a 64-bit key
    Check check;                    // kFlag: v ? 1 : 0, never refused; kRange: lo..hi; kAtLeast: >= lo; kSet: one of
    int64_t lo, hi;                 // ... the first n_allowed of `allowed`
    int n_allowed;
    int allowed[4];
    const char *refusal;            // the whole text of the refusal (no conversions)
    unsigned effects;
};
extern const Tunable kTunables[];
extern const int kNumTunables;

// `key` = v: 0, the value stored and *effects (may be nullptr) what else it does; or 1 with the refusal in fail(),
// nothing changed.
int config_set(EngineConfig &c, const char *key, int64_t v, unsigned *effects);
// the configured value of `key` as set; false: no such key
bool config_get(const EngineConfig &c, const char *key, int64_t *v);

#pragma GCC visibility pop
