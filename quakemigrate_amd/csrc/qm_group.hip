// qm_group.hip -- engine groups (include/qmhip.h part 4): ONE host thread drives the column partition of a
// grid (quakemigrate_amd/distributed.py: shard_columns / column_boxes) on several devices, with no collective
// library.  A part is one entry of the device list (ids may repeat); below it sit up to three engines, one per
// box of its column range, each with its box's slice of the table and its node offset, all on the part's own
// stream.  Per step every box writes its partial [3][ns] into a packed buffer, the parts' buffers travel to the
// lead device (entry 0) by peer copies ordered with events, and the engines' own fold (combine_kernel, as
// qm_engine_finalize_packed) runs there over n_parts * 3 sets -- the exchange of ColumnShardedDetector with
// copies in place of the all-gather.  Every device's work is enqueued before the host waits once.
#include "qm_engine.hpp"

#include <array>
#include <limits>

#pragma GCC visibility push(hidden)

namespace {

constexpr int kMaxBoxes = 3;
constexpr int kBoxInts = 6;                  // (x0, x1, y0, y1, z0, z1)

// part `part` of n_parts: boxes of the column partition, or -- a flat (1, 1, N) table -- one balanced z-run
int plan_boxes(int64_t nx, int64_t ny, int64_t nz, int n_parts, int part, int32_t b[kMaxBoxes][kBoxInts]) {
    auto balanced = [](int64_t n, int64_t parts, int64_t p, int64_t *lo, int64_t *hi) {
        const int64_t base = n / parts, extra = n % parts;
        *lo = p * base + std::min(p, extra);
        *hi = *lo + base + (p < extra ? 1 : 0);
    };
    int n = 0;
    auto add = [&](int64_t x0, int64_t x1, int64_t y0, int64_t y1, int64_t z0, int64_t z1) {
        const int64_t v[kBoxInts] = {x0, x1, y0, y1, z0, z1};
        for (int k = 0; k < kBoxInts; ++k) b[n][k] = (int32_t)v[k];
        ++n;
    };
    int64_t lo = 0, hi = 0;
    if (nx == 1 && ny == 1) {                            // flat table: a contiguous z-run per part
        balanced(nz, n_parts, part, &lo, &hi);
        if (hi > lo) add(0, 1, 0, 1, lo, hi);
        return n;
    }
    balanced(nx * ny, n_parts, part, &lo, &hi);          // columns [c0, c1), as column_boxes
    if (hi <= lo) return 0;
    int64_t xa = lo / ny, ya = lo % ny, xb = hi / ny, yb = hi % ny;
    if (xa == xb) {
        add(xa, xa + 1, ya, yb, 0, nz);
        return n;
    }
    if (ya) {
        add(xa, xa + 1, ya, ny, 0, nz);
        ++xa;
    }
    if (xb > xa) add(xa, xb, 0, ny, 0, nz);
    if (yb) add(xb, xb + 1, 0, yb, 0, nz);
    return n;
}

int64_t box_offset(const int32_t *b, int64_t ny, int64_t nz) { return ((int64_t)b[0] * ny + b[2]) * nz + b[4]; }
int64_t box_nodes(const int32_t *b) { return (int64_t)(b[1] - b[0]) * (b[3] - b[2]) * (b[5] - b[4]); }

}  // namespace

struct GroupPart {
    int device = 0;
    bool on_lead = false;                    // same device as entry 0: writes straight into the lead's buffers
    hipStream_t stream = nullptr;
    qm_engine *eng[kMaxBoxes] = {nullptr, nullptr, nullptr};
    int n_boxes = 0;
    int32_t box[kMaxBoxes][kBoxInts] = {};
    int64_t node0 = 0, node1 = 0;            // flat node range of the boxes
    Event ev_done, ev_t0, ev_t1;
    bool timed = false;
    DevBuf<double> d_on, d_pack, d_gcopy, d_tie, d_map, d_vol, d_fpack;
    double *pack = nullptr, *tie = nullptr, *fpack = nullptr;   // where this part's partials go on its device
};

struct qm_group {
    std::vector<GroupPart> parts;
    qm_engine *lead = nullptr;               // fold engine on entry 0's device (no table)
    int lead_dev = 0;
    int64_t nx = 0, ny = 0, nz = 0;
    int32_t n_rows = 0;
    bool have_lut = false;
    std::vector<std::pair<uint64_t, std::array<int64_t, 4>>> shapes;   // key -> (nx, ny, nz, rows) of keyed tables
    uint64_t miss_key = 0;                   // a table_select miss: the next load is known under this key
    bool miss = false;
    Event ev_gathered;
    DevBuf<double> d_gather, d_tgather, d_fgather, d_out;
    int ready_ns = -1;                       // sample count the exchange buffers are laid out for
    PinnedBuf<double> h_on, h_out;
};

#pragma GCC visibility pop

namespace {

// n_sets packed sets of `rows` rows: neutral partials (maximum -inf, no index, sum 0) or, rows == 2, neutral
// tie outcomes (key 0, no index)
int fill_neutral(double *d, int n_sets, int rows, int ns, int device) {
    std::vector<double> h((size_t)n_sets * rows * ns, 0.0);
    const int64_t none = INT64_MAX;
    for (int s = 0; s < n_sets; ++s) {
        double *set = h.data() + (size_t)s * rows * ns;
        if (rows == 3) std::fill(set, set + ns, -std::numeric_limits<double>::infinity());
        for (int t = 0; t < ns; ++t) std::memcpy(set + (size_t)ns + t, &none, 8);
    }
    DeviceGuard guard(device);
    QM_HIP(hipMemcpy(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    return 0;
}

// the exchange buffers for scans of ns samples, every set neutral
int ready(qm_group *g, int ns) {
    if (g->ready_ns == ns) return 0;
    const int P = (int)g->parts.size(), sets = P * kMaxBoxes;
    {
        DeviceGuard guard(g->lead_dev);
        if (g->d_gather.ensure((size_t)sets * 3 * ns) || g->d_tgather.ensure((size_t)sets * 2 * ns) ||
            g->d_fgather.ensure((size_t)P * 3 * ns) || g->d_out.ensure(3 * (size_t)ns))
            return 1;
    }
    if (fill_neutral(g->d_gather.p, sets, 3, ns, g->lead_dev) || fill_neutral(g->d_tgather.p, sets, 2, ns, g->lead_dev) ||
        fill_neutral(g->d_fgather.p, P, 3, ns, g->lead_dev))
        return 1;
    for (int p = 0; p < P; ++p) {
        GroupPart &q = g->parts[p];
        if (q.on_lead) {
            q.pack = g->d_gather.p + (size_t)p * kMaxBoxes * 3 * ns;
            q.tie = g->d_tgather.p + (size_t)p * kMaxBoxes * 2 * ns;
            q.fpack = g->d_fgather.p + (size_t)p * 3 * ns;
            continue;
        }
        DeviceGuard guard(q.device);
        if (q.d_pack.ensure((size_t)kMaxBoxes * 3 * ns) || q.d_tie.ensure((size_t)kMaxBoxes * 2 * ns) ||
            q.d_fpack.ensure(3 * (size_t)ns) || q.d_gcopy.ensure((size_t)sets * 3 * ns))
            return 1;
        if (fill_neutral(q.d_pack.p, kMaxBoxes, 3, ns, q.device) || fill_neutral(q.d_tie.p, kMaxBoxes, 2, ns, q.device) ||
            fill_neutral(q.d_fpack.p, 1, 3, ns, q.device))
            return 1;
        q.pack = q.d_pack.p;
        q.tie = q.d_tie.p;
        q.fpack = q.d_fpack.p;
    }
    g->ready_ns = ns;
    return 0;
}

// after a failure: let whatever was enqueued finish before the pinned buffers are touched again
void drain(qm_group *g) {
    for (GroupPart &q : g->parts) {
        DeviceGuard guard(q.device);
        (void)hipStreamSynchronize(q.stream);
    }
    DeviceGuard guard(g->lead_dev);
    (void)hipStreamSynchronize(g->lead->stream);
}

int failed(qm_group *g) {
    const std::string msg = error_text();
    drain(g);
    return fail("%s", msg.c_str());
}

int check_group(qm_group *g, const char *what) {
    if (!g) return fail("%s: group is NULL", what);
    if (!g->have_lut) return fail("%s: no travel-time table resident: call qm_group_load_lut first", what);
    if (g->lead->cfg.screen || g->parts[0].eng[0]->cfg.screen)
        return fail("%s: the screened detect (screen = 1) has no partial form: groups run float64 only", what);
    return 0;
}

// The log-onsets staged once into pinned memory, one H2D per part on its stream
int stage_onsets_all(qm_group *g, const double *log_onsets, int T) {
    const size_t n = (size_t)g->n_rows * T;
    if (g->h_on.ensure(n, hipHostMallocPortable)) return 1;
    host_copy(g->h_on.p, log_onsets, n * sizeof(double));
    for (GroupPart &q : g->parts) {
        if (!q.n_boxes) continue;
        DeviceGuard guard(q.device);
        if (q.d_on.ensure(n)) return 1;
        QM_HIP(hipMemcpyAsync(q.d_on.p, g->h_on.p, n * sizeof(double), hipMemcpyHostToDevice, q.stream));
        QM_HIP(hipEventRecord(q.ev_t0, q.stream));
    }
    return 0;
}

// part p's `count` doubles at `src` (its device) to `dst` (the lead's), then the lead's stream waits for them
int to_lead(qm_group *g, GroupPart &q, double *dst, const double *src, size_t count) {
    DeviceGuard guard(q.device);
    if (!q.on_lead)
        QM_HIP(hipMemcpyPeerAsync(dst, g->lead_dev, src, q.device, count * sizeof(double), q.stream));
    QM_HIP(hipEventRecord(q.ev_done, q.stream));
    DeviceGuard lead(g->lead_dev);
    QM_HIP(hipStreamWaitEvent(g->lead->stream, q.ev_done, 0));
    return 0;
}

// The boxes' partials (in each part's `pack`) -> the lead, folded into d_out; with tie_rule = 1 the second
// exchange: gathered partials back to every device, each box's near-tie outcome, gathered, folded on the lead.
int exchange(qm_group *g, int T, int fsmp, int lsmp, int available, int ns) {
    const int P = (int)g->parts.size(), sets = P * kMaxBoxes;
    for (int p = 0; p < P; ++p) {
        GroupPart &q = g->parts[p];
        if (q.n_boxes) {
            DeviceGuard guard(q.device);
            QM_HIP(hipEventRecord(q.ev_t1, q.stream));
            q.timed = true;
        }
        if (to_lead(g, q, g->d_gather.p + (size_t)p * kMaxBoxes * 3 * ns, q.pack, (size_t)kMaxBoxes * 3 * ns))
            return 1;
    }
    double *o = g->d_out.p;
    if (qm_engine_finalize_packed(g->lead, g->d_gather.p, sets, ns, g->nx * g->ny * g->nz, o, o + ns,
                                  reinterpret_cast<int64_t *>(o + 2 * (size_t)ns), 1))
        return 1;
    if (!g->lead->cfg.tie_rule) return 0;
    {
        DeviceGuard lead(g->lead_dev);
        QM_HIP(hipEventRecord(g->ev_gathered, g->lead->stream));
    }
    for (int p = 0; p < P; ++p) {
        GroupPart &q = g->parts[p];
        if (!q.n_boxes) {
            if (to_lead(g, q, g->d_tgather.p + (size_t)p * kMaxBoxes * 2 * ns, q.tie, (size_t)kMaxBoxes * 2 * ns))
                return 1;
            continue;
        }
        const double *gathered = g->d_gather.p;
        {
            DeviceGuard guard(q.device);
            QM_HIP(hipStreamWaitEvent(q.stream, g->ev_gathered, 0));
            if (!q.on_lead) {
                QM_HIP(hipMemcpyPeerAsync(q.d_gcopy.p, q.device, g->d_gather.p, g->lead_dev,
                                          (size_t)sets * 3 * ns * sizeof(double), q.stream));
                gathered = q.d_gcopy.p;
            }
        }
        for (int k = 0; k < q.n_boxes; ++k)
            if (qm_engine_tie_partial(q.eng[k], q.d_on.p, 1, T, fsmp, lsmp, available, gathered, sets,
                                      q.tie + (size_t)k * 2 * ns))
                return 1;
        if (to_lead(g, q, g->d_tgather.p + (size_t)p * kMaxBoxes * 2 * ns, q.tie, (size_t)kMaxBoxes * 2 * ns))
            return 1;
    }
    return qm_engine_tie_fold(g->lead, g->d_tgather.p, sets, ns, reinterpret_cast<int64_t *>(o + 2 * (size_t)ns));
}

// d_out (the lead's [3][ns]) to the caller's three host series; the one wait of the step
int fetch_series(qm_group *g, int ns, double *max_coa, double *max_norm, int64_t *idx) {
    DeviceGuard lead(g->lead_dev);
    const size_t n = 3 * (size_t)ns;
    if (g->h_out.ensure(n, hipHostMallocPortable)) return 1;
    QM_HIP(hipMemcpyAsync(g->h_out.p, g->d_out.p, n * sizeof(double), hipMemcpyDeviceToHost, g->lead->stream));
    QM_HIP(hipStreamSynchronize(g->lead->stream));
    if (max_coa) {
        host_copy(max_coa, g->h_out.p, ns * sizeof(double));
        host_copy(max_norm, g->h_out.p + ns, ns * sizeof(double));
        host_copy(idx, g->h_out.p + 2 * (size_t)ns, ns * sizeof(double));
    }
    return 0;
}

int step_shape(qm_group *g, int T, int fsmp, int lsmp, int *ns) {
    if (fsmp < 0 || lsmp < 0) return fail("negative pad (fsmp=%d, lsmp=%d)", fsmp, lsmp);
    *ns = T - fsmp - lsmp;
    if (*ns <= 0) return fail("no samples to scan: T=%d fsmp=%d lsmp=%d", T, fsmp, lsmp);
    return ready(g, *ns);
}

void set_part_boxes(qm_group *g) {
    const int P = (int)g->parts.size();
    for (int p = 0; p < P; ++p) {
        GroupPart &q = g->parts[p];
        q.n_boxes = g->have_lut ? plan_boxes(g->nx, g->ny, g->nz, P, p, q.box) : 0;
        q.node0 = q.n_boxes ? box_offset(q.box[0], g->ny, g->nz) : 0;
        q.node1 = q.node0;
        for (int k = 0; k < q.n_boxes; ++k) q.node1 += box_nodes(q.box[k]);
    }
}

}  // namespace

extern "C" {

int qm_group_plan(int32_t nx, int32_t ny, int32_t nz, int32_t n_parts, int32_t part, int32_t *boxes,
                  int32_t *n_boxes) {
    if (!boxes || !n_boxes) return fail("qm_group_plan: NULL argument");
    if (nx < 1 || ny < 1 || nz < 1) return fail("qm_group_plan: empty grid (%d, %d, %d)", nx, ny, nz);
    if (n_parts < 1 || part < 0 || part >= n_parts)
        return fail("qm_group_plan: part %d of %d parts", part, n_parts);
    int32_t b[kMaxBoxes][kBoxInts] = {};
    *n_boxes = plan_boxes(nx, ny, nz, n_parts, part, b);
    std::memcpy(boxes, b, sizeof(b));
    return 0;
}

int qm_group_create(const int32_t *device_ids, int32_t n, qm_group **out) {
    if (!out) return fail("qm_group_create: out is NULL");
    *out = nullptr;
    if (!device_ids || n < 1) return fail("qm_group_create: an engine group needs at least one device (n = %d)", n);
    for (int i = 0; i < n; ++i)
        if (device_ids[i] < 0) return fail("qm_group_create: device id %d at entry %d is negative", device_ids[i], i);
    int count = 0;
    QM_HIP(hipGetDeviceCount(&count));
    for (int i = 0; i < n; ++i)
        if (device_ids[i] >= count)
            return fail("qm_group_create: device %d not available (%d HIP devices visible)", device_ids[i], count);
    // (destroyed as any group is if a step below fails)
    std::unique_ptr<qm_group, decltype(&qm_group_destroy)> g(new qm_group(), qm_group_destroy);
    g->lead_dev = device_ids[0];
    g->parts.resize(n);
    for (int i = 0; i < n; ++i) g->parts[i].device = device_ids[i];
    if (qm_engine_create(g->lead_dev, &g->lead)) return 1;
    {
        DeviceGuard lead(g->lead_dev);
        if (g->ev_gathered.create(hipEventDisableTiming) != hipSuccess)
            return fail("qm_group_create: hipEventCreate failed");
    }
    for (int i = 0; i < n; ++i) {
        GroupPart &q = g->parts[i];
        q.on_lead = q.device == g->lead_dev;
        DeviceGuard guard(q.device);
        if (acquire_stream(q.device, &q.stream) != hipSuccess || q.ev_t0.create() != hipSuccess ||
            q.ev_t1.create() != hipSuccess || q.ev_done.create(hipEventDisableTiming) != hipSuccess)
            return fail("qm_group_create: stream / events on device %d", q.device);
        for (int k = 0; k < kMaxBoxes; ++k)
            if (qm_engine_create(q.device, &q.eng[k]) || qm_engine_set_stream(q.eng[k], q.stream, 0)) return 1;
    }
    *out = g.release();
    return 0;
}

void qm_group_destroy(qm_group *g) {
    if (!g) return;
    for (GroupPart &q : g->parts) {
        DeviceGuard guard(q.device);
        if (q.stream) (void)hipStreamSynchronize(q.stream);
        for (qm_engine *e : q.eng) qm_engine_destroy(e);
        if (q.stream) park_stream(q.device, q.stream);
        PoolReleaseScope one_wait;
        q = GroupPart{};                                // (the part's buffers and events, on its device)
    }
    qm_engine *lead = g->lead;
    {
        DeviceGuard guard(g->lead_dev);
        if (lead) (void)hipStreamSynchronize(lead->stream);
        PoolReleaseScope one_wait;
        delete g;                                       // (the parts are empty by now: the lead's buffers, on its device)
    }
    qm_engine_destroy(lead);
}

int qm_group_config(qm_group *g, const char *key, int64_t value) {
    if (!g || !key) return fail("qm_group_config: NULL argument");
    if (std::strcmp(key, "screen") == 0 && value != 0)
        return fail("qm_group_config: screen = 1 is not available on an engine group (the screened detect has "
                    "no partial form)");
    if (qm_engine_config(g->lead, key, value)) return 1;
    for (GroupPart &q : g->parts)
        for (qm_engine *e : q.eng)
            if (qm_engine_config(e, key, value)) return 1;
    return 0;
}

int qm_group_get(qm_group *g, const char *key, int64_t *value) {
    if (!g || !key || !value) return fail("qm_group_get: NULL argument");
    const std::string k(key);
    if (k == "n_parts") { *value = (int64_t)g->parts.size(); return 0; }
    if (k == "n_nodes") { *value = g->have_lut ? g->nx * g->ny * g->nz : 0; return 0; }
    if (k == "n_rows") { *value = g->have_lut ? g->n_rows : 0; return 0; }
    if (k == "nx" || k == "ny" || k == "nz") {
        *value = !g->have_lut ? 0 : k == "nx" ? g->nx : k == "ny" ? g->ny : g->nz;
        return 0;
    }
    if (k == "lut_max") {
        if (!g->have_lut) return fail("qm_group_get: no travel-time table resident");
        int32_t most = 0;
        for (GroupPart &q : g->parts)
            for (int b = 0; b < q.n_boxes; ++b) {
                int32_t m = 0;
                if (qm_engine_lut_max(q.eng[b], &m)) return 1;
                most = std::max(most, m);
            }
        *value = most;
        return 0;
    }
    // anything else: every engine's word, which must agree (boxes only once a table is resident: the
    // read-outs of an engine without one are not comparable)
    bool have = false;
    int64_t first = 0;
    auto ask = [&](qm_engine *e) -> int {
        int64_t v = 0;
        if (qm_engine_get(e, key, &v)) return 1;
        if (have && v != first)
            return fail("qm_group_get: the group's engines disagree on '%s' (%lld, %lld)", key, (long long)first,
                        (long long)v);
        have = true;
        first = v;
        return 0;
    };
    for (GroupPart &q : g->parts)
        for (int b = 0; b < (g->have_lut ? q.n_boxes : kMaxBoxes); ++b)
            if (ask(q.eng[b])) return 1;
    if (!have && ask(g->lead)) return 1;
    *value = first;
    return 0;
}

int qm_group_load_lut(qm_group *g, const int32_t *host_table, int32_t nx, int32_t ny, int32_t nz, int32_t n_rows) {
    if (!g || !host_table) return fail("qm_group_load_lut: NULL argument");
    if (nx < 1 || ny < 1 || nz < 1 || n_rows < 1)
        return fail("qm_group_load_lut: bad shape (%d, %d, %d, %d)", nx, ny, nz, n_rows);
    const bool same_grid = g->nx == nx && g->ny == ny && g->nz == nz;
    const bool after_miss = g->miss;
    const uint64_t miss_key = g->miss_key;
    if (g->miss) {                                     // (loaded after a select miss: known under its key)
        g->miss = false;
        bool seen = false;
        for (auto &s : g->shapes)
            if (s.first == g->miss_key) {
                s.second = {nx, ny, nz, n_rows};
                seen = true;
            }
        if (!seen) g->shapes.push_back({g->miss_key, {nx, ny, nz, n_rows}});
        if (g->shapes.size() > 256) g->shapes.erase(g->shapes.begin());
    }
    g->nx = nx; g->ny = ny; g->nz = nz; g->n_rows = n_rows;
    g->have_lut = true;
    set_part_boxes(g);
    if (!same_grid) g->ready_ns = -1;                  // other boxes: the exchange buffers start neutral again
    for (GroupPart &q : g->parts)
        for (int k = 0; k < q.n_boxes; ++k) {
            const int32_t *b = q.box[k];
            const int64_t off = box_offset(b, ny, nz);
            if (qm_engine_load_lut(q.eng[k], host_table + off * n_rows, 0, b[1] - b[0], b[3] - b[2], b[5] - b[4],
                                   n_rows, off)) {
                g->have_lut = false;
                return 1;
            }
            // The GROUP's select missed as soon as one box engine had lost the table; an engine that still had its
            // box parked brought it back, and this load on top of it would take its key away (qm_engine_load_lut: a
            // load onto a resident table is a foreign one) -- that engine would never park the table again, and the
            // group would rebuild it at every later select although the cache has room.
            if (after_miss) table_set_key(q.eng[k], miss_key);
        }
    return 0;
}

int qm_group_table_select(qm_group *g, uint64_t key, int32_t capacity, int32_t *resident) {
    if (!g || !resident) return fail("qm_group_table_select: NULL argument");
    // the shape the current table had is remembered under its key (the engines park their own states)
    std::array<int64_t, 4> shape{0, 0, 0, 0};
    bool known = false;
    for (auto &s : g->shapes)
        if (s.first == key) {
            shape = s.second;
            known = true;
        }
    bool all = true;
    for (GroupPart &q : g->parts)
        for (qm_engine *e : q.eng) {
            int32_t r = 0;
            if (qm_engine_table_select(e, key, capacity, &r)) return 1;
            (void)r;
        }
    if (known) {
        const bool same_grid = g->nx == shape[0] && g->ny == shape[1] && g->nz == shape[2];
        g->nx = shape[0]; g->ny = shape[1]; g->nz = shape[2]; g->n_rows = (int32_t)shape[3];
        g->have_lut = true;
        set_part_boxes(g);
        if (!same_grid) g->ready_ns = -1;
        for (GroupPart &q : g->parts)
            for (int k = 0; k < q.n_boxes; ++k) all = all && q.eng[k]->have_lut;
    }
    *resident = known && all ? 1 : 0;
    g->miss = !*resident;
    g->miss_key = key;
    if (!*resident) g->have_lut = false;
    return 0;
}

int qm_group_detect(qm_group *g, const double *log_onsets, int32_t T, int32_t fsmp, int32_t lsmp,
                    int32_t available, double *max_coa, double *max_norm_coa, int64_t *max_coa_idx) {
    if (!log_onsets || !max_coa || !max_norm_coa || !max_coa_idx) return fail("qm_group_detect: NULL argument");
    if (check_group(g, "qm_group_detect")) return 1;
    int ns = 0;
    if (step_shape(g, T, fsmp, lsmp, &ns) || stage_onsets_all(g, log_onsets, T)) return failed(g);
    for (GroupPart &q : g->parts) {
        const int64_t three = 3 * (int64_t)ns;
        for (int k = 0; k < q.n_boxes; ++k) {
            double *pk = q.pack + k * three;
            if (qm_engine_detect_partial(q.eng[k], q.d_on.p, 1, T, fsmp, lsmp, available, pk,
                                         reinterpret_cast<int64_t *>(pk + ns), pk + 2 * ns))
                return failed(g);
        }
    }
    if (exchange(g, T, fsmp, lsmp, available, ns) ||
        fetch_series(g, ns, max_coa, max_norm_coa, max_coa_idx))
        return failed(g);
    return 0;
}

int qm_group_marginal(qm_group *g, const double *log_onsets, int32_t T, int32_t fsmp, int32_t lsmp,
                      int32_t available, int32_t first_sample, int32_t end_sample, double *coa_map, double *max_coa,
                      double *max_norm_coa, int64_t *max_coa_idx) {
    if (!log_onsets || !coa_map) return fail("qm_group_marginal: NULL argument");
    const bool want_scan = max_coa != nullptr;
    if (want_scan && (!max_norm_coa || !max_coa_idx)) return fail("qm_group_marginal: all three scan outputs or none");
    if (check_group(g, "qm_group_marginal")) return 1;
    int ns = 0;
    if (step_shape(g, T, fsmp, lsmp, &ns)) return failed(g);
    if (first_sample < 0 || end_sample > ns || first_sample >= end_sample)
        return fail("marginal window [%d, %d) outside the %d scanned samples", first_sample, end_sample, ns);
    if (stage_onsets_all(g, log_onsets, T)) return failed(g);
    for (GroupPart &q : g->parts) {
        if (!q.n_boxes) continue;
        {
            DeviceGuard guard(q.device);
            if (q.d_map.ensure((size_t)(q.node1 - q.node0))) return failed(g);
        }
        for (int k = 0; k < q.n_boxes; ++k) {
            qm_engine *e = q.eng[k];
            DeviceGuard guard(e->device);
            StackLaunch s(q.d_on.p, T, fsmp, ns, available);
            s.want_scan = want_scan;
            s.kind = StackLaunch::Marginal{first_sample, end_sample, q.d_map.p + (e->node_offset - q.node0)};
            int ns_k = 0;
            if (check_step(e, T, fsmp, lsmp, available, &ns_k) ||
                stack_fold(e, s, kCombinePartial, 0, packed_set(q.pack + k * 3 * (int64_t)ns, ns)).rc)
                return failed(g);
            e->last.sets_own = want_scan;
        }
    }
    if (want_scan && exchange(g, T, fsmp, lsmp, available, ns)) return failed(g);
    // every part's flat range to its node offset (the column partition keeps each one contiguous)
    for (GroupPart &q : g->parts) {
        if (!q.n_boxes) continue;
        DeviceGuard guard(q.device);
        if (copy_back(coa_map + q.node0, q.d_map.p, (size_t)(q.node1 - q.node0) * sizeof(double), q.stream) !=
            hipSuccess) {
            fail("qm_group_marginal: copy of part on device %d failed", q.device);
            return failed(g);
        }
    }
    if (want_scan && fetch_series(g, ns, max_coa, max_norm_coa, max_coa_idx)) return failed(g);
    return 0;
}

int qm_group_migrate(qm_group *g, const double *log_onsets, int32_t T, int32_t fsmp, int32_t lsmp,
                     int32_t available, double *map4d, int accumulate, double *max_coa, double *max_norm_coa,
                     int64_t *max_coa_idx) {
    if (!log_onsets || !map4d) return fail("qm_group_migrate: NULL argument");
    const bool want_scan = max_coa != nullptr;
    if (want_scan && (!max_norm_coa || !max_coa_idx)) return fail("qm_group_migrate: all three scan outputs or none");
    if (check_group(g, "qm_group_migrate")) return 1;
    int ns = 0;
    if (step_shape(g, T, fsmp, lsmp, &ns) || stage_onsets_all(g, log_onsets, T)) return failed(g);
    for (GroupPart &q : g->parts) {
        if (!q.n_boxes) continue;
        const size_t cells = (size_t)(q.node1 - q.node0) * ns;
        {
            DeviceGuard guard(q.device);
            if (q.d_vol.ensure(cells)) return failed(g);
            // (the reference's `+=`: the part's rows of the caller's volume first)
            if (accumulate && copy_in(q.d_vol.p, map4d + q.node0 * ns, cells * sizeof(double), q.stream) != hipSuccess) {
                fail("qm_group_migrate: upload of the volume to device %d failed", q.device);
                return failed(g);
            }
        }
        for (int k = 0; k < q.n_boxes; ++k) {
            qm_engine *e = q.eng[k];
            DeviceGuard guard(e->device);
            StackLaunch s(q.d_on.p, T, fsmp, ns, available);
            s.want_scan = want_scan;
            s.kind = StackLaunch::Volume{q.d_vol.p + (e->node_offset - q.node0) * ns, ns, accumulate};
            int ns_k = 0;
            if (check_step(e, T, fsmp, lsmp, available, &ns_k) ||
                stack_fold(e, s, kCombinePartial, 0, packed_set(q.pack + k * 3 * (int64_t)ns, ns)).rc)
                return failed(g);
            e->last.sets_own = want_scan;
        }
    }
    if (want_scan && exchange(g, T, fsmp, lsmp, available, ns)) return failed(g);
    for (GroupPart &q : g->parts) {
        if (!q.n_boxes) continue;
        DeviceGuard guard(q.device);
        if (copy_back(map4d + q.node0 * ns, q.d_vol.p, (size_t)(q.node1 - q.node0) * ns * sizeof(double),
                      q.stream) != hipSuccess) {
            fail("qm_group_migrate: copy of the volume from device %d failed", q.device);
            return failed(g);
        }
    }
    if (want_scan && fetch_series(g, ns, max_coa, max_norm_coa, max_coa_idx)) return failed(g);
    return 0;
}

int qm_group_find_max_coa(qm_group *g, const double *map4d, int32_t n_samples, int64_t n_nodes, double *max_coa,
                          double *max_norm_coa, int64_t *max_coa_idx) {
    if (!g || !map4d || !max_coa || !max_norm_coa || !max_coa_idx) return fail("qm_group_find_max_coa: NULL argument");
    if (n_samples < 1 || n_nodes < 1) return fail("qm_group_find_max_coa: empty volume");
    const int ns = n_samples, P = (int)g->parts.size();
    if (ready(g, ns)) return failed(g);
    for (int p = 0; p < P; ++p) {
        GroupPart &q = g->parts[p];
        // part p scans the balanced flat range of the volume's nodes
        const int64_t base = n_nodes / P, extra = n_nodes % P;
        const int64_t n0 = p * base + std::min<int64_t>(p, extra), n1 = n0 + base + (p < extra ? 1 : 0);
        if (n1 > n0) {
            const size_t cells = (size_t)(n1 - n0) * ns;
            DeviceGuard guard(q.device);
            if (q.d_vol.ensure(cells)) return failed(g);
            if (copy_in(q.d_vol.p, map4d + n0 * ns, cells * sizeof(double), q.stream) != hipSuccess) {
                fail("qm_group_find_max_coa: upload of the volume to device %d failed", q.device);
                return failed(g);
            }
            QM_HIP(hipEventRecord(q.ev_t0, q.stream));
            if (scan_fold(q.eng[0], q.d_vol.p, ns, ns, n1 - n0, n0, kCombinePartial, packed_set(q.fpack, ns)))
                return failed(g);
            QM_HIP(hipEventRecord(q.ev_t1, q.stream));
            q.timed = true;
        }
        if (to_lead(g, q, g->d_fgather.p + (size_t)p * 3 * ns, q.fpack, 3 * (size_t)ns)) return failed(g);
    }
    double *o = g->d_out.p;
    {
        DeviceGuard lead(g->lead_dev);
        if (combine(g->lead, packed_sets(g->d_fgather.p, P, ns), kCombineValues, 0, n_nodes,
                    OutSeries{o, o + ns, reinterpret_cast<int64_t *>(o + 2 * (size_t)ns)}, nullptr))
            return failed(g);
    }
    if (fetch_series(g, ns, max_coa, max_norm_coa, max_coa_idx)) return failed(g);
    return 0;
}

int qm_group_synchronize(qm_group *g) {
    if (!g) return fail("qm_group_synchronize: group is NULL");
    for (GroupPart &q : g->parts) {
        DeviceGuard guard(q.device);
        QM_HIP(hipStreamSynchronize(q.stream));
    }
    DeviceGuard lead(g->lead_dev);
    QM_HIP(hipStreamSynchronize(g->lead->stream));
    return 0;
}

int qm_group_n_parts(qm_group *g, int32_t *n_parts) {
    if (!g || !n_parts) return fail("qm_group_n_parts: NULL argument");
    *n_parts = (int32_t)g->parts.size();
    return 0;
}

int qm_group_part_info(qm_group *g, int32_t part, int32_t *device, int32_t *boxes, int32_t *n_boxes,
                       int64_t *node_range, double *last_ms) {
    if (!g) return fail("qm_group_part_info: group is NULL");
    if (part < 0 || part >= (int32_t)g->parts.size())
        return fail("qm_group_part_info: part %d of %d", part, (int)g->parts.size());
    GroupPart &q = g->parts[part];
    if (device) *device = q.device;
    if (boxes) std::memcpy(boxes, q.box, sizeof(q.box));
    if (n_boxes) *n_boxes = q.n_boxes;
    if (node_range) {
        node_range[0] = q.node0;
        node_range[1] = q.node1;
    }
    if (last_ms) {
        *last_ms = -1.0;
        if (q.timed) {
            DeviceGuard guard(q.device);
            QM_HIP(hipEventSynchronize(q.ev_t1));
            float f = 0.f;
            QM_HIP(hipEventElapsedTime(&f, q.ev_t0, q.ev_t1));
            *last_ms = f;
        }
    }
    return 0;
}

}  // extern "C"
