// qm_traveltimes.hip -- the travel-time stage's host side: argument checks, staging, one launch per call (kernels and
// their notes: qm_traveltimes.hpp).  Parameters are host arrays; every output goes to the caller's host or device
// pointer; the sweep's sections come from either side.  Each call synchronises: it reads back what it refuses on
// (the sections' status, the sweep's first node outside its section) and its stage time ("tt_ns_<stage>").
#define QM_TU_TRAVELTIMES 1
#include "qm_engine.hpp"

namespace {

int tt_check_grid(const char *what, const double *ll, const double *sp, const int32_t *n, int32_t n_rows, qm::TtGrid *g) {
    long long nodes = 1;
    for (int j = 0; j < 3; ++j) {
        if (n[j] < 1) return fail("%s: node_count[%d] = %d", what, j, n[j]);
        if (!std::isfinite(ll[j]) || !std::isfinite(sp[j]) || !(sp[j] > 0.0))
            return fail("%s: axis %d: ll_corner %g, node_spacing %g (finite, spacing > 0)", what, j, ll[j], sp[j]);
        nodes *= n[j];
        if (nodes > INT32_MAX) return fail("%s: more than 2^31 - 1 nodes", what);
        g->ll[j] = ll[j]; g->sp[j] = sp[j]; g->n[j] = n[j];
    }
    if (n_rows < 1) return fail("%s: n_rows = %d", what, n_rows);
    g->nodes = nodes;
    g->total = nodes * n_rows;
    g->rows = n_rows;
    return 0;
}

unsigned tt_grid_blocks(long long nodes) {            // (the launch grid strides over ONE row's nodes, row after row)
    return (unsigned)std::min<long long>((nodes + qm::kTtGridThreads - 1) / qm::kTtGridThreads, qm::kTtGridBlocks);
}

}  // namespace

extern "C" {

int qm_engine_tt_homogeneous(qm_engine *e, const double *ll_corner, const double *node_spacing,
                             const int32_t *node_count, int32_t n_rows, const double *row_params, double *out,
                             int out_on_device) {
    using namespace qm;
    const char *what = "qm_engine_tt_homogeneous";
    if (!e || !ll_corner || !node_spacing || !node_count || !row_params || !out) return fail("%s: NULL argument", what);
    TtGrid g{};
    if (tt_check_grid(what, ll_corner, node_spacing, node_count, n_rows, &g)) return 1;
    for (int r = 0; r < n_rows; ++r) {
        const double *p = row_params + 4 * (size_t)r;
        if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2]))
            return fail("%s: row %d: station at (%g, %g, %g)", what, r, p[0], p[1], p[2]);
        if (!std::isfinite(p[3]) || !(p[3] > 0.0)) return fail("%s: row %d: velocity %g (finite, > 0)", what, r, p[3]);
    }
    DeviceGuard guard(e->device);
    auto &tt = e->tt;
    const double *d_rows = stage_in(e, tt.par, row_params, 0, 4 * (size_t)n_rows);
    const StagedOut<double> grids = stage_host_out(tt.out, out, out_on_device, (size_t)g.total);
    if (!d_rows || !grids.d) return 1;
    tt.clock.begin(true, false);
    if (timed_launches(e, [&] {
            return tt.clock.launch(e->stream, kTtHomogeneous, tt_homogeneous_kernel, dim3(tt_grid_blocks(g.nodes)),
                                   dim3(kTtGridThreads), 0, g, d_rows, grids.d);
        }))
        return 1;
    if (grids.fetch(e)) return 1;
    QM_HIP(hipStreamSynchronize(e->stream));
    return tt.clock.collect();
}

int qm_engine_tt_sections(qm_engine *e, int32_t n_sections, int32_t nr, int32_t nz, double h, const double *slowness,
                          const double *source, double tol, int32_t max_iters, int force_scratch, double *T,
                          int32_t *rounds, int32_t *status, int out_on_device) {
    using namespace qm;
    const char *what = "qm_engine_tt_sections";
    if (!e || !slowness || !source || !T || !rounds || !status) return fail("%s: NULL argument", what);
    if (n_sections < 1 || nr < 2 || nz < 2 || (long long)nr * nz > (1ll << 28))
        return fail("%s: %d sections of %d x %d nodes (at least 1 of 2 x 2, at most 2^28 nodes each)", what, n_sections,
                    nr, nz);
    if (!std::isfinite(h) || !(h > 0.0)) return fail("%s: spacing %g (finite, > 0)", what, h);
    if (!(tol >= 0.0) || !(tol < 1.0)) return fail("%s: tol %g (0 <= tol < 1)", what, tol);
    if (max_iters < 1) return fail("%s: max_iters = %d", what, max_iters);
    for (int s = 0; s < n_sections; ++s) {
        for (int k = 0; k < nz; ++k) {
            const double v = slowness[(size_t)s * nz + k];
            if (!std::isfinite(v) || !(v > 0.0))
                return fail("%s: section %d: slowness %g in row %d (finite, > 0)", what, s, v, k);
        }
        const double zs = source[2 * (size_t)s], s0 = source[2 * (size_t)s + 1];
        // (the two rows that bracket the source are floor(zs / h) and the one below it)
        if (!std::isfinite(zs) || !(zs >= 0.0) || !(std::floor(zs / h) + 1.0 <= (double)(nz - 1)))
            return fail("%s: section %d: source at depth %g outside the section's rows [0, %g]", what, s, zs,
                        (double)(nz - 1) * h);
        if (!std::isfinite(s0) || !(s0 > 0.0))
            return fail("%s: section %d: slowness %g at the source (finite, > 0)", what, s, s0);
    }
    DeviceGuard guard(e->device);
    auto &tt = e->tt;
    const size_t n = (size_t)nr * nz, S = (size_t)n_sections;
    const bool lds = !force_scratch && n <= (size_t)kTtLdsNodes;
    std::vector<double> par(slowness, slowness + S * nz);
    par.insert(par.end(), source, source + 2 * S);
    // (copy_in goes through the pinned bounce buffer: `par` is consumed when stage_in returns, so the early returns
    // below may drop it with the copy still in flight -- as for every host array of this file)
    const double *d_par = stage_in(e, tt.par, par.data(), 0, par.size());
    const StagedOut<double> times = stage_host_out(tt.out, T, out_on_device, S * n);
    if (!d_par || !times.d || tt.meta.ensure(2 * S) || (!lds && tt.tau.ensure(S * n))) return 1;
    TtSectionArgs a{};
    a.slow = d_par;
    a.src = d_par + S * nz;
    a.T = times.d;
    a.scratch = tt.tau.p;
    a.rounds = out_on_device ? rounds : tt.meta.p;
    a.status = out_on_device ? status : tt.meta.p + S;
    a.nr = nr; a.nz = nz; a.max_iters = max_iters;
    a.h = h; a.tol = tol;
    tt.clock.begin(true, false);
    if (timed_launches(e, [&]() -> int {
            if (!lds)
                return tt.clock.launch(e->stream, kTtSections, tt_sections_kernel<false>, dim3((unsigned)S),
                                       dim3(kTtSectionThreads), 0, a);
            QM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(tt_sections_kernel<true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)tt_lds_bytes(kTtLdsNodes)));
            return tt.clock.launch(e->stream, kTtSections, tt_sections_kernel<true>, dim3((unsigned)S),
                                   dim3(kTtSectionThreads), tt_lds_bytes((long long)n), a);
        }))
        return 1;
    std::vector<int32_t> h_meta(2 * S);
    QM_HIP(copy_back(h_meta.data(), a.rounds, S * sizeof(int32_t), e->stream));
    QM_HIP(copy_back(h_meta.data() + S, a.status, S * sizeof(int32_t), e->stream));
    if (times.fetch(e)) return 1;
    QM_HIP(hipStreamSynchronize(e->stream));
    if (tt.clock.collect()) return 1;
    if (!out_on_device) {
        std::copy(h_meta.begin(), h_meta.begin() + S, rounds);
        std::copy(h_meta.begin() + S, h_meta.end(), status);
    }
    for (size_t s = 0; s < S; ++s)
        if (h_meta[S + s] != 0)
            return fail("%s: section %d: not settled after %d rounds (max_iters)", what, (int)s, max_iters);
    return 0;
}

int qm_engine_tt_sweep(qm_engine *e, const double *ll_corner, const double *node_spacing, const int32_t *node_count,
                       int32_t n_rows, const double *row_params, const int32_t *row_section, const double *sections,
                       int sections_on_device, int32_t n_sections, int32_t nr, int32_t nz, double h, double *out,
                       int out_on_device) {
    using namespace qm;
    const char *what = "qm_engine_tt_sweep";
    if (!e || !ll_corner || !node_spacing || !node_count || !row_params || !row_section || !sections || !out)
        return fail("%s: NULL argument", what);
    TtGrid g{};
    if (tt_check_grid(what, ll_corner, node_spacing, node_count, n_rows, &g)) return 1;
    if (n_sections < 1 || nr < 2 || nz < 2 || (long long)nr * nz > (1ll << 28))
        return fail("%s: %d sections of %d x %d nodes (at least 1 of 2 x 2, at most 2^28 nodes each)", what, n_sections,
                    nr, nz);
    if (!std::isfinite(h) || !(h > 0.0)) return fail("%s: spacing %g (finite, > 0)", what, h);
    for (int r = 0; r < n_rows; ++r) {
        const double *p = row_params + 4 * (size_t)r;
        if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2]) || !std::isfinite(p[3]))
            return fail("%s: row %d: station at (%g, %g), section origin (%g, %g)", what, r, p[0], p[1], p[2], p[3]);
        if (row_section[r] < 0 || row_section[r] >= n_sections)
            return fail("%s: row %d: section %d of %d", what, r, row_section[r], n_sections);
    }
    DeviceGuard guard(e->device);
    auto &tt = e->tt;
    const size_t R = (size_t)n_rows;
    TtSweepArgs a{};
    a.g = g;
    a.rows = stage_in(e, tt.par, row_params, 0, 4 * R);
    a.row_sec = stage_in(e, tt.meta, row_section, 0, R);
    a.sections = stage_in(e, tt.sec, sections, sections_on_device, (size_t)n_sections * nr * nz);
    const StagedOut<double> grids = stage_host_out(tt.out, out, out_on_device, (size_t)g.total);
    if (!a.rows || !a.row_sec || !a.sections || !grids.d || tt.bad.ensure(R)) return 1;
    a.nr = nr; a.nz = nz; a.h = h;
    a.out = grids.d;
    a.bad = tt.bad.p;
    QM_HIP(hipMemsetAsync(a.bad, 0xff, R * sizeof(unsigned long long), e->stream));
    tt.clock.begin(true, false);
    if (timed_launches(e, [&] {
            return tt.clock.launch(e->stream, kTtSweep, tt_sweep_kernel, dim3(tt_grid_blocks(g.nodes)),
                                   dim3(kTtGridThreads), 0, a);
        }))
        return 1;
    std::vector<unsigned long long> h_bad(R);
    QM_HIP(copy_back(h_bad.data(), a.bad, R * sizeof(unsigned long long), e->stream));
    if (grids.fetch(e)) return 1;
    QM_HIP(hipStreamSynchronize(e->stream));
    if (tt.clock.collect()) return 1;
    for (size_t r = 0; r < R; ++r)
        if (h_bad[r] != kTtNone) {
            const long long node = (long long)h_bad[r], t = node / g.n[2];
            return fail("%s: row %d: node %lld (%lld, %lld, %lld) lies outside section %d (%d x %d nodes of %g from "
                        "(%g, %g))", what, (int)r, node, t / g.n[1], t % g.n[1], node % g.n[2], row_section[r], nr, nz,
                        h, row_params[4 * r + 2], row_params[4 * r + 3]);
        }
    return 0;
}

int qm_engine_tt_eikonal3d(qm_engine *e, const double *ll_corner, const double *node_spacing, const int32_t *node_count,
                           int32_t n_rows, const double *row_params, const int32_t *row_model, int32_t n_models,
                           const double *slowness, int slowness_on_device, double tol, int32_t max_iters, double *out,
                           int out_on_device, int32_t *rounds, int32_t *status) {
    using namespace qm;
    const char *what = "qm_engine_tt_eikonal3d";
    if (!e || !ll_corner || !node_spacing || !node_count || !row_params || !row_model || !slowness || !out || !rounds ||
        !status)
        return fail("%s: NULL argument", what);
    for (int j = 0; j < 3; ++j)
        if (node_count[j] < 2) return fail("%s: axis %d: %d nodes (at least 2)", what, j, node_count[j]);
    TtGrid g{};
    if (tt_check_grid(what, ll_corner, node_spacing, node_count, n_rows, &g)) return 1;
    if (n_rows > kTtPlaneMaxRows) return fail("%s: %d rows (at most %d in one call)", what, n_rows, kTtPlaneMaxRows);
    if (n_models < 1) return fail("%s: n_models = %d", what, n_models);
    if (!(tol >= 0.0) || !(tol < 1.0)) return fail("%s: tol %g (0 <= tol < 1)", what, tol);
    if (max_iters < 1) return fail("%s: max_iters = %d", what, max_iters);
    const size_t R = (size_t)n_rows, n_slow = (size_t)n_models * (size_t)g.nodes;
    // row -> model, the source's cell, the two sets of row flags: the first one's "previous round" is all rows live
    std::vector<int32_t> meta(6 * R, 0);
    for (size_t r = 0; r < R; ++r) {
        const double *p = row_params + 4 * r;
        for (int j = 0; j < 3; ++j) {
            const double ur = g.ll[j] + (double)(g.n[j] - 1) * g.sp[j];
            if (!(p[j] >= g.ll[j] && p[j] <= ur))
                return fail("%s: row %d: source at (%g, %g, %g) outside the grid: axis %d spans [%g, %g]", what, (int)r,
                            p[0], p[1], p[2], j, g.ll[j], ur);
            // the cell that holds the source: floor((src - ll) / h), clipped to n - 2
            const double c = std::floor((p[j] - g.ll[j]) / g.sp[j]);
            meta[R + 3 * r + j] = (int32_t)std::min(std::max(c, 0.0), (double)(g.n[j] - 2));
        }
        if (!std::isfinite(p[3]) || !(p[3] > 0.0))
            return fail("%s: row %d: slowness %g at the source (finite, > 0)", what, (int)r, p[3]);
        if (row_model[r] < 0 || row_model[r] >= n_models)
            return fail("%s: row %d: model %d of %d", what, (int)r, row_model[r], n_models);
        meta[r] = row_model[r];
        meta[4 * R + r] = 1;
    }
    DeviceGuard guard(e->device);
    auto &tt = e->tt;
    TtEikonalArgs a{};
    a.g = g;
    a.rows = stage_in(e, tt.par, row_params, 0, 4 * R);
    a.row_model = stage_in(e, tt.meta, meta.data(), 0, meta.size());
    a.slow = stage_in(e, tt.sec, slowness, slowness_on_device, n_slow);
    const StagedOut<double> grids = stage_host_out(tt.out, out, out_on_device, (size_t)g.total);
    if (!a.rows || !a.row_model || !a.slow || !grids.d || tt.bad.ensure(1)) return 1;
    a.cell = a.row_model + R;
    a.tau = grids.d;
    a.tol = tol;
    int32_t *const flags[2] = {tt.meta.p + 4 * R, tt.meta.p + 5 * R};

    // the volumes, wherever they came from: the first element that is not finite and positive is refused by name
    QM_HIP(hipMemsetAsync(tt.bad.p, 0xff, sizeof(unsigned long long), e->stream));
    hipLaunchKernelGGL(tt_slowness_check_kernel, dim3(tt_grid_blocks((long long)std::min<size_t>(n_slow, INT32_MAX))),
                       dim3(kTtGridThreads), 0, e->stream, a.slow, (unsigned long long)n_slow, tt.bad.p);
    QM_HIP(hipGetLastError());
    unsigned long long h_bad = kTtNone;
    QM_HIP(copy_back(&h_bad, tt.bad.p, sizeof(h_bad), e->stream));
    QM_HIP(hipStreamSynchronize(e->stream));
    if (h_bad != kTtNone) {
        double v = 0.0;
        QM_HIP(copy_back(&v, a.slow + h_bad, sizeof(v), e->stream));
        QM_HIP(hipStreamSynchronize(e->stream));
        return fail("%s: model %d: slowness %g at node %lld (finite, > 0)", what, (int)(h_bad / (size_t)g.nodes), v,
                    (long long)(h_bad % (size_t)g.nodes));
    }

    std::vector<int32_t> h_flag(R), h_rounds(R, 0), h_status(R, 1);
    const unsigned node_blocks = tt_grid_blocks(g.nodes);
    const auto solve = [&]() -> int {
        hipLaunchKernelGGL(tt_eikonal_init_kernel, dim3(node_blocks), dim3(kTtGridThreads), 0, e->stream, a);
        size_t open = R;
        for (int round = 0; round < max_iters && open; ++round) {
            a.live = flags[round & 1];
            a.flag = flags[(round & 1) ^ 1];
            QM_HIP(hipMemsetAsync(a.flag, 0, R * sizeof(int32_t), e->stream));
            for (int o = 0; o < 8; ++o) {               // itertools.product((+1, -1), repeat=3) over (x, y, z)
                TtPlane p{};
                p.rev[0] = (o >> 2) & 1; p.rev[1] = (o >> 1) & 1; p.rev[2] = o & 1;
                for (p.d = 0; p.d < g.n[0] + g.n[1] + g.n[2] - 2; ++p.d) {
                    // the plane's rectangle: i' from lo0 to hi0, over those j' from lo1 to hi1
                    const int hi0 = std::min(g.n[0] - 1, p.d);
                    p.lo0 = std::max(0, p.d - (g.n[1] - 1) - (g.n[2] - 1));
                    p.lo1 = std::max(0, p.d - hi0 - (g.n[2] - 1));
                    p.n0 = hi0 - p.lo0 + 1;
                    p.n1 = std::min(g.n[1] - 1, p.d - p.lo0) - p.lo1 + 1;
                    const unsigned cells = (unsigned)p.n0 * (unsigned)p.n1;
                    hipLaunchKernelGGL(tt_eikonal_plane_kernel, dim3((cells + kTtPlaneThreads - 1) / kTtPlaneThreads,
                                                                     (unsigned)R),
                                       dim3(kTtPlaneThreads), 0, e->stream, a, p);
                }
            }
            QM_HIP(hipGetLastError());
            // the round's one synchronisation: the row flags, through the pinned staging
            QM_HIP(copy_back(h_flag.data(), a.flag, R * sizeof(int32_t), e->stream));
            for (size_t r = 0; r < R; ++r) {
                if (!h_status[r]) continue;
                ++h_rounds[r];
                if (!h_flag[r]) {
                    h_status[r] = 0;
                    --open;
                }
            }
        }
        hipLaunchKernelGGL(tt_eikonal_finish_kernel, dim3(node_blocks), dim3(kTtGridThreads), 0, e->stream, a);
        return 0;
    };
    tt.clock.begin(true, false);
    if (timed_launches(e, [&]() -> int {
            int rc = 0;
            return tt.clock.stage(e->stream, kTtEikonal3d, [&] { rc = solve(); }) || rc;
        }))
        return 1;
    if (grids.fetch(e)) return 1;
    QM_HIP(hipStreamSynchronize(e->stream));
    if (tt.clock.collect()) return 1;
    std::copy(h_rounds.begin(), h_rounds.end(), rounds);
    std::copy(h_status.begin(), h_status.end(), status);
    for (size_t r = 0; r < R; ++r)
        if (h_status[r] != 0) return fail("%s: row %d: not settled after %d rounds (max_iters)", what, (int)r, max_iters);
    return 0;
}

}  // extern "C"
