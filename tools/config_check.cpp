// config_check.cpp -- the engine's tunables on the CPU, under the sanitizers: every row of kTunables
// (csrc/qm_config.hpp) through fixed probes on ONE record, in the table's order, then an explicit brick_x filling in
// the other two dimensions.  A stand-alone host program over qm_config.hip alone: no device, no engine.
//
//   c++ -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       tools/config_check.cpp quakemigrate_amd/csrc/qm_config.hip -o /tmp/config_check && /tmp/config_check
//
// Prints, one per line,
//   default <key> <value>                                          a fresh record
//   probe <key> <value> rc=<0|1> effects=<names|-> get=<value|-> msg=<refusal text>
//   step set <key> <value> rc=<0|1>  /  step get <key> <value>     the brick fill-in
// and "config_check: ok".  tests/test_host.py holds the lines against tests/tunables_cases.py, whose header states the
// probes' rule.  A sanitizer report ends the program with a non-zero status.
#include "../quakemigrate_amd/csrc/qm_config.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

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

static std::string effect_names(unsigned fx) {
    static const struct { unsigned bit; const char *name; } kNames[] = {
        {kVoidShift, "void_sh"}, {kVoidShiftWide, "void_shw"}, {kVoidScreen, "void_screen"},
        {kUserWaves, "user_waves"}, {kUserRounds, "user_rounds"}, {kUserLds, "user_lds"},
        {kResetTimingLog, "reset_log"}};
    std::string s;
    for (const auto &n : kNames)
        if (fx & n.bit) s += (s.empty() ? "" : "+") + std::string(n.name);
    return s.empty() ? "-" : s;
}

static bool same(const EngineConfig &a, const EngineConfig &b) {
    for (int i = 0; i < kNumTunables; ++i) {
        int64_t va = 0, vb = 0;
        if (!config_get(a, kTunables[i].name, &va) || !config_get(b, kTunables[i].name, &vb) || va != vb) return false;
    }
    return a.user_waves == b.user_waves && a.user_rounds == b.user_rounds && a.user_lds == b.user_lds;
}

static std::vector<int64_t> probes_of(const Tunable &t) {
    switch (t.check) {
    case Tunable::kFlag: return {0, 1, 7, -1};
    case Tunable::kRange:
        if (std::strcmp(t.name, "lds_bytes") == 0) return {t.lo - 1, t.hi + 1, t.hi, t.lo + 15, t.lo};   // (rounding)
        return {t.lo - 1, t.hi + 1, t.hi, t.lo};
    case Tunable::kAtLeast: return {t.lo - 1, t.lo, t.wide ? (int64_t)1 << 40 : 100000};
    case Tunable::kSet: {
        std::vector<int64_t> p = {t.allowed[0] - 1, t.allowed[t.n_allowed - 1] + 1};
        for (int i = 0; i + 1 < t.n_allowed; ++i)      // a value in the first gap
            if (t.allowed[i + 1] - t.allowed[i] > 1) { p.push_back(t.allowed[i + 1] - 1); break; }
        for (int i = t.n_allowed - 1; i >= 0; --i) p.push_back(t.allowed[i]);
        return p;
    }
    }
    return {};
}

int main() {
    const EngineConfig fresh;
    for (int i = 0; i < kNumTunables; ++i) {
        int64_t v = 0;
        if (!config_get(fresh, kTunables[i].name, &v)) return 1;
        std::printf("default %s %lld\n", kTunables[i].name, (long long)v);
    }
    EngineConfig c;
    for (int i = 0; i < kNumTunables; ++i) {
        const Tunable &t = kTunables[i];
        for (int64_t v : probes_of(t)) {
            const EngineConfig before = c;
            unsigned fx = 0;
            g_error.clear();
            const int rc = config_set(c, t.name, v, &fx);
            int64_t got = 0;
            if (!config_get(c, t.name, &got)) return 1;
            if (rc != 0 && !same(before, c)) {
                std::fprintf(stderr, "config_check: %s = %lld was refused and changed the record\n", t.name, (long long)v);
                return 1;
            }
            std::printf("probe %s %lld rc=%d effects=%s get=%s msg=%s\n", t.name, (long long)v, rc,
                        rc ? "-" : effect_names(fx).c_str(), rc ? "-" : std::to_string(got).c_str(), g_error.c_str());
        }
    }
    // unknown keys, and a set without an effects pointer
    int64_t v = 0;
    g_error.clear();
    if (config_set(c, "no_such_key", 1, nullptr) != 1 || config_get(c, "no_such_key", &v)) return 1;
    std::printf("unknown %s\n", g_error.c_str());
    // an explicit brick_x fills in the other two
    EngineConfig b;
    static const struct { const char *key; int64_t v; } kSteps[] = {
        {"brick_x", 4}, {"brick_z", 0}, {"brick_x", 0}, {"brick_y", 0}, {"brick_z", 0}};
    for (const auto &s : kSteps) {
        std::printf("step set %s %lld rc=%d\n", s.key, (long long)s.v, config_set(b, s.key, s.v, nullptr));
        for (const char *key : {"brick_x", "brick_y", "brick_z"}) {
            if (!config_get(b, key, &v)) return 1;
            std::printf("step get %s %lld\n", key, (long long)v);
        }
    }
    std::printf("config_check: ok\n");
    return 0;
}
