// qm_engine.hip -- the engine handle and the steps (C ABI part 2, include/qmhip.h).
//
// One engine = one GPU.  It keeps the travel-time table resident together with the tables derived
// from it (qm_tables.hip), owns the scratch for partial reductions, and launches the stacking kernels
// (qm_launch_*.hip) on a caller-supplied (e.g. torch) or private HIP stream.  Nothing here falls back
// to the CPU: if HIP fails, the call fails.
#define QM_TU_STEPS 1
#include "qm_engine.hpp"

namespace {

using qm::kPairLdsBytes;

qm::LaunchShape stack_shape(const qm_engine *e, const qm::StackArgs &a, int threads, size_t lds) {
    // the grid is padded to a multiple of 8 groups (XCD-aware workgroup -> (tile, group) map)
    // (several timesteps per launch: the tile axis runs over (step, tile))
    const int steps = a.n_steps > 1 ? a.n_steps : 1;
    return {(unsigned)(steps * a.ntiles * ((a.ngroups + 7) / 8 * 8)), threads, lds, e->stream};
}

bool pair_built(int S) { return S >= 1 && S <= qm::kPairMaxRows; }

// ---- shift-reuse layout (qm_shift.hpp) ----------------------------------------------------------
// (the layouts themselves: ShiftLayout, qm_engine.hpp; built by ensure_shift_tables, qm_tables.hip)

// does this launch take the shift-reuse kernel?  Whole 256-sample tiles plus, for what a scan leaves
// beyond them, one tail tile of 64 / 128 / 192 samples (qm_shift.hpp: shift_work); the kernels
// without tail flavours (row blocks, the 12-wave shape) and remainders of more than 192 samples pull a
// last whole tile back over its predecessor, which needs a scan of at least one tile.
bool shift_wanted(const qm_engine *e, int n_chunk, bool plain, bool volume, int64_t vol_stride) {
    if (!plain || e->cfg.shift == 0 || e->cfg.generic || e->cfg.force_direct ||
        e->cfg.user_waves || e->cfg.user_lds || e->cfg.samples_per_lane > 0 || e->cfg.pair == 2)
        return false;
    // volume-writing launches: the row stride goes into a 32-bit byte count (as do, for the marginal
    // map, the offsets of a group's nodes: an x-plane of fewer than 2^29 nodes)
    if (volume && vol_stride * 8 >= ((int64_t)1 << 32)) return false;
    if ((int64_t)e->g.ny * e->g.nz * 8 >= ((int64_t)1 << 32)) return false;
    return n_chunk >= 1;
}

// samples per lane of the scan's tail tile (0: none -- whole tiles only, the last one pulled back), for the
// `rest` samples a scan leaves beyond the tiles in front
int shift_tail_spl(const qm_engine *e, int rest) {
    const int rem = rest % qm::kShiftKT;
    if (rem == 0 || rem > 192 || !e->cfg.shift_tail) return 0;
    return (rem + qm::kWave - 1) / qm::kWave;
}

// Tiles of a fused detect on the wide layout: 384-sample tiles in front; what the scan leaves beyond them runs
// as ONE tail tile (<= 192 samples), ONE 256-sample tile pulled back over its predecessor (<= 256), or one more
// wide tile pulled back (qm_shift.hpp: shift_work).
void shift_wide_tiles(const qm_engine *e, int n_chunk, bool only_wide, StackPlan &p) {
    int wide = n_chunk / qm::kShiftWideKT;
    const int rest = n_chunk - wide * qm::kShiftWideKT;
    p.tail_spl = 0;
    int behind = 0;
    if (rest > qm::kShiftKT || (only_wide && rest > 0)) ++wide;      // (row blocks: no other tile kinds)
    else if (rest > 0) {
        p.tail_spl = shift_tail_spl(e, rest);
        behind = 1;
    }
    p.wide_tiles = wide;
    p.ntiles = wide + behind;
}

}  // namespace

int auto_groups(const qm_engine *e, int ntiles, int units, int blocks_per_cu, int rounds) {
    // Workgroups all do the same amount of work, so the grid should be a whole number of
    // "rounds" over the resident slots (n_cu * blocks_per_cu): ntiles * groups <= rounds * slots,
    // as close from below as possible.  12 rounds measured best on C2/C3 (finer load balance
    // than 4; flat beyond); the partial sets stay a few tens of MB.  Never more groups than
    // there are bricks.
    const int64_t slots = (int64_t)e->n_cu * blocks_per_cu;
    int64_t want = ((int64_t)(rounds > 0 ? rounds : e->cfg.rounds) * slots) / ntiles;
    if (want < 1) want = std::max<int64_t>(1, slots / ntiles);
    want = std::max<int64_t>(1, std::min<int64_t>(want, units));
    // Group g runs on XCD g % 8 (the XCD-aware workgroup map of the stacking kernels), so a
    // group count that is not a multiple of 8 leaves some XCDs one group short: 65 groups = 9 on
    // one XCD, 8 on the others = 11 % of the step spent waiting for one XCD (C3 x 60 rows at
    // 12000 samples: 255 -> see profiles/r02_ab_runs.txt).  Round down to a multiple of 8.
    if (want > 8) want -= want % 8;
    return (int)want;
}

namespace {

// Everything that is decided about the stacking launch `s`, into *out: kernel family, layout, tiles, group counts,
// what its partial sets will stand for.  Builds the family's tables on first use (device work); launches no stacking
// kernel and leaves e->last alone.  out->batched = false: the launch cannot hold its n_steps timesteps.
int plan_stack(qm_engine *e, const StackLaunch &s, StackPlan *out) {
    StackPlan p;
    const auto *vol = std::get_if<StackLaunch::Volume>(&s.kind);
    const bool volume = vol && vol->p, marginal = std::holds_alternative<StackLaunch::Marginal>(s.kind);
    const int64_t vol_stride = vol ? vol->stride : 0;
    const int accumulate = vol ? vol->accumulate : 0;
    const bool want_scan = s.want_scan;
    const int n_chunk = s.n_chunk;
    const int J = run_j(e, n_chunk);
    if (plan_wide(e, J)) return 1;
    const int KT = qm::kWave * J;
    // The bricks the launch runs on, those of them that go to the direct kernel and the LDS kernel's tables are those
    // of ONE layout: the round-2 kernels' unless the shift-reuse or the paired kernel takes the launch below
    p.layout = &e->r2();
    p.ntiles = (n_chunk + KT - 1) / KT;
    p.cap_doubles = lds_cap_doubles(e);

    // ---- the shift-reuse kernel (qm_shift.hpp): the fused detect's default where the table fits
    bool shift = shift_wanted(e, n_chunk, !accumulate && (volume || marginal || want_scan), volume, vol_stride);
    p.shift_mode = marginal ? qm::kShiftMarginal : volume ? qm::kShiftVolume : qm::kShiftDetect;
    // Round 6: the fused detect of a scan that holds at least one 384-sample tile runs on the WIDE layout where
    // the table has one (ShiftLayout, qm_engine.hpp): its own brick grid, the 8-wave shape
    // (automatic: only where one timestep is at least eight rounds of one-brick workgroups over the CUs and holds
    // four wide tiles -- the Icequake-sized C1, 288 bricks x 2 tiles, runs 0.49 ms on the wide layout and 0.42 on
    // the other, C3's 401-sample locate window 5.4 against 4.0: one wide tile and a short tail tile side by side
    // leave the CUs with the short one idle; the count is the single step's, so that a step's bits do not depend
    // on how many share its launch)
    const ShiftLayout *L = &e->sh;
    const int64_t wide_work = (int64_t)((e->g.nx + 7) / 8) * ((e->g.ny + 7) / 8) * ((e->g.nz + 15) / 16) *
                              ((n_chunk + qm::kShiftWideKT - 1) / qm::kShiftWideKT);
    if (shift && p.shift_mode == qm::kShiftDetect && e->cfg.shift_wide != 0 && n_chunk >= qm::kShiftWideKT &&
        // (tie_rule = 1 WITHOUT a row of maxima per brick -- tie_sets = 0, round 5's form -- re-stacks one set of bricks per
        // sample: the wide layout's few long workgroups would publish sets of tens of thousands of nodes)
        (e->cfg.shift_wide == 1 || (wide_work >= 8 * (int64_t)e->n_cu && n_chunk >= 4 * qm::kShiftWideKT &&
                                    (!e->cfg.tie_rule || e->cfg.tie_sets) &&
                                    std::min(e->g.nx, std::min(e->g.ny, e->g.nz)) >= 8)) &&   // (thin boxes of a
                                    // rank's column partition: their 8 x 8 x 16 bricks would be mostly empty)
        e->cfg.shift_waves == 0) {
        if (ensure_shift_tables(e, e->shw)) return 1;
        if (e->shw.ok) L = &e->shw;
    }
    const bool wide = L == &e->shw;
    if (shift && !wide) {
        if (ensure_shift_tables(e, e->sh)) return 1;
        // the 12-wave shape and the register-staged row blocks are built for the fused detect only,
        // row blocks have no marginal-map flavour; none of the three has tail tiles
        shift = L->ok && (L->plain() || (p.shift_mode == qm::kShiftDetect) ||
                          (p.shift_mode == qm::kShiftVolume && L->nblk > 1 && L->direct));
        p.tail_spl = (shift && L->plain()) ? shift_tail_spl(e, n_chunk) : 0;
        // a last tile that is pulled back needs a whole tile of scan (and the detect flavours of the
        // kernels without tail tiles keep their former lower bound)
        if (shift && p.tail_spl == 0 && n_chunk % qm::kShiftKT != 0 &&
            (p.shift_mode == qm::kShiftDetect ? n_chunk < 192 : n_chunk < qm::kShiftKT))
            shift = false;
    }
    if (shift) {
        p.layout = p.shift = L;                         // (its tables travel in ShiftArgs: launch_shift_lds)
        p.ntiles = (n_chunk + qm::kShiftKT - 1) / qm::kShiftKT;
        p.cap_doubles = qm::kShiftLdsBytes / 8;
        if (wide) shift_wide_tiles(e, n_chunk, L->direct, p);        // (direct: the wide layout's row-block form)
    } else {
        p.tail_spl = 0;
    }
    // ---- the paired (16-byte operand) kernel where it applies and the shift-reuse kernel does not
    // take the launch: own brick grid and tables (built only then)
    int jp = (shift || accumulate || marginal) ? 0 : pair_jp(e, n_chunk, volume);
    if (jp > 0) {
        if (!pair_built(e->g.n_rows)) jp = 0;
        else if (ensure_pair_tables(e, jp) != 0) return 1;   // a HIP failure while building the tables
        else if (!e->pair.ok) jp = 0;                         // the layout does not fit this table
    }
    if (jp > 0) {
        const int PKT = 128 * jp;
        p.layout = &e->pair;
        p.ntiles = (n_chunk + PKT - 1) / PKT;
        p.cap_doubles = kPairLdsBytes / 8;
    }
    if (s.n_steps > 1) {
        p.batched = !volume && !marginal && !accumulate && s.run_if == nullptr && want_scan && (!shift || L->plain());
        if (!p.batched) {
            *out = p;
            return 0;
        }
        p.steps = s.n_steps;
    }
    if (!shift && jp == 0) {                            // the round-2 kernels' own offsets
        if (J != 1 && J != 2 && J != 4) return fail("samples_per_lane must be 1, 2 or 4 (got %d)", J);
        if (ensure_rel(e)) return 1;
    }
    if (marginal) p.marg_tiles = p.ntiles;
    const int n_wide_now = p.layout->n_list, nbricks_now = p.layout->g.nbricks;
    p.use_direct = e->cfg.force_direct || n_wide_now > 0;
    p.use_lds = !e->cfg.force_direct && n_wide_now < nbricks_now;
    // the direct launch: the LDS kernel's tile length (64 * J = 128 * JP; the shift-reuse launch's bricks on whole
    // 256-sample tiles of their own, clamped), the wavefronts' publish area
    p.direct_j = shift ? 4 : jp > 0 ? 2 * jp : J;
    p.direct_threads = shift ? 512 : jp > 0 ? 1024 : run_waves(e) * qm::kWave;
    p.direct_publish = (size_t)3 * (p.direct_threads / qm::kWave) * qm::kWave * p.direct_j * sizeof(double);
    const int threads = p.direct_threads;
    const int lds_blocks_per_cu =
        shift ? (L->nw == qm::kShiftWaves ? 2 : 1) : jp > 0 ? 1
               : std::max(1, std::min(160 * 1024 / std::max(1, run_lds_bytes(e)), 2048 / threads));
    if (p.use_lds) {
        // (several timesteps per launch: the group count is the single step's -- the groups are the
        // order in which a sample's coalescence is summed over the nodes, and a step's result must
        // not depend on how many steps share its launch; the extra steps only make the grid longer)
        // (bricks of <= 64 nodes -- coarse grids with wide tables, 4 nodes per wavefront and brick: a
        // workgroup's fixed costs weigh more than the grid's tail, three rounds instead of twelve:
        // E2 0.418 -> 0.394 ms, profiles/r04_rounds_sweep.txt)
        int rounds = (!shift && jp == 0 && !e->cfg.user_rounds && e->g.brick_nodes <= 64) ? 3 : 0;
        // (the wide layout's 8-wave workgroups, one per CU: FEW, long workgroups -- C3 41.7 / 42.1 / 42.3 / 42.6 ms
        // at 1 / 4 / 8 / 12 rounds, where the 4-wave shape runs 50.1 / 46.5 / 45.7 at 4 / 8 / 12,
        // profiles/r06_ab_runs.txt: the fewest rounds that leave no slot idle, 0.2 % charged per round)
        // (the 8-wave shape of 33-64 rows likewise: a C4 slab, 47 tiles, 170.2 ms at 12 rounds = 64 groups, 168.6 at
        // 16 groups = 2.94 rounds, 181.5 at 40 groups = 7.3 rounds: what the count must avoid is a last round that is
        // mostly empty)
        if (shift && (wide || (L->nw == qm::kShiftWaves8 && L->nblk == 1)) && !e->cfg.user_rounds) {
            double best = 1e300;
            for (int r = 1; r <= e->cfg.rounds; ++r) {
                const int g = auto_groups(e, p.ntiles, nbricks_now, lds_blocks_per_cu, r);
                const double busy = (double)p.ntiles * g / ((double)r * e->n_cu * lds_blocks_per_cu);
                const double cost = (1.0 - std::min(1.0, busy)) + 0.002 * r;
                if (cost < best - 1e-9) { best = cost; rounds = r; }
            }
        }
        // (tie_rule = 1 stacks one SET of bricks again per sample, qm_ties.hpp: eight times as many,
        // smaller sets -- the refinement's cost falls with the set size, the stacking launch loses ~1 %)
        p.groups_lds = e->cfg.groups > 0 ? std::min(e->cfg.groups, nbricks_now)
                                         : auto_groups(e, p.ntiles, nbricks_now, lds_blocks_per_cu, rounds);
        // Round 6: the shift-reuse fused detect leaves the largest z PER BRICK and sample beside its workgroups'
        // partial sets (StackArgs::brick_max): the refinement stacks one brick per sample, the launch keeps its
        // group count -- and its bits
        p.brick_rows = (e->cfg.tie_rule && want_scan && e->cfg.tie_sets && shift && p.shift_mode == qm::kShiftDetect &&
                        L->plain()) ? nbricks_now : 0;
        if (e->cfg.tie_rule && want_scan && !p.brick_rows && !e->cfg.user_rounds && e->cfg.groups == 0) {
            // ... the other kernels: eight times as many, smaller sets, but never sets of fewer than four bricks:
            // the workgroup's fixed costs (C2: +8 % on the stacking launch at one brick per set)
            const int fine = auto_groups(e, p.ntiles, std::max(1, nbricks_now / 4), lds_blocks_per_cu,
                                         8 * (rounds > 0 ? rounds : e->cfg.rounds));
            p.groups_lds = std::max(p.groups_lds, fine);
        }
        // which LDS kernel (the read-outs last_kernel / last_kernel_j; a direct-only launch keeps 0 and 0)
        if (shift) {
            p.family = kFamilyShift;
            p.j = p.wide_tiles > 0 ? qm::kShiftWideSpl : 4;
            // groups a wavefront sees before its running maximum is reset: bricks per workgroup x
            // groups per (brick, wavefront)
            // (brick maxima, tie_rule = 1: the wide tiles' loop raises them itself -- the running maximum lives as long
            // as ever --, the other tiles fold and reset it after every brick)
            const bool per_brick = p.brick_rows && p.wide_tiles == 0;
            const int64_t life = (per_brick ? 1 : (int64_t)L->g.nbricks / std::max(1, p.groups_lds)) *
                                 std::max(1, L->g.brick_nodes / 8 / L->nw);
            p.lazy = e->cfg.shift_lazy >= 0 ? e->cfg.shift_lazy : (life >= qm::kShiftLazyGroups ? 1 : 0);
            if (L->nblk > 1 && !L->direct) p.lazy = 0;  // (the register-staged form: eager only)
        } else if (jp > 0) {
            p.family = kFamilyPair;
            p.j = 2 * jp;
        } else {
            // the exact-row-count kernels: fused detect and the marginalised map for up to 64 rows,
            // volume-writing for 33-64 rows (up to 32 the paired kernel writes volumes), when the
            // launch uses the table width's own samples per lane
            const int S = e->g.n_rows;
            const bool exact = e->cfg.exact && !e->cfg.generic && !accumulate && qm::exact_built(S, J) &&
                               (marginal || !volume || S > qm::kPairMaxRows);
            p.family = exact ? kFamilyExact : kFamilyChunked;
            p.j = J;
        }
    }
    if (p.use_direct) {
        const int units = e->cfg.force_direct ? nbricks_now : n_wide_now;
        p.groups_direct = e->cfg.groups > 0 ? std::min(e->cfg.groups, units)
                                            : auto_groups(e, p.ntiles, units, 2048 / threads);
        // (force_direct: every brick, no list)
        p.list = e->cfg.force_direct ? nullptr : p.layout->list.p;
        p.n_list = units;
    }
    p.g = p.layout->g;
    p.sets = p.groups_lds + p.groups_direct;
    p.scan_n = p.steps * n_chunk;
    *out = p;
    return 0;
}

// The arguments of the plan's LDS launch (over every brick that fits: no list) or of its direct launch (the list)
qm::StackArgs stack_args(const qm_engine *e, const StackLaunch &s, const StackPlan &p, bool direct) {
    const auto *vol = std::get_if<StackLaunch::Volume>(&s.kind);
    const auto *marg = std::get_if<StackLaunch::Marginal>(&s.kind);
    qm::StackArgs a{};
    a.g = p.g;
    a.onsets = s.onsets;
    a.lut = e->d_lut.p;
    if (!p.shift) {                                     // (the shift-reuse tables travel in ShiftArgs)
        a.rel = p.layout->rel.p;
        a.brick_meta = p.layout->meta.p;
        a.brick_total = p.layout->total.p;
    }
    a.brick_list = direct ? p.list : nullptr;
    a.n_list = direct ? p.n_list : 0;
    a.T = s.T;
    a.fsmp = s.fsmp;
    a.n_samples = s.n_samples;
    a.sample0 = s.sample0;
    a.n_chunk = s.n_chunk;
    // (the direct launch beside a shift-reuse one: its own whole tiles of 256 samples, clamped)
    a.ntiles = direct && p.shift ? (s.n_chunk + qm::kShiftKT - 1) / qm::kShiftKT : p.ntiles;
    a.ngroups = direct ? p.groups_direct : p.groups_lds;
    a.tail_spl = direct ? 0 : p.tail_spl;
    a.wide_tiles = direct ? 0 : p.wide_tiles;
    if (p.steps > 1) {
        a.n_steps = p.steps;
        a.step_stride = s.step_stride;
    }
    a.part_stride = p.scan_n;
    a.cap_doubles = p.cap_doubles;
    // coa = exp(stack/available) = 2^(stack * log2(e)/available)
    a.z_scale = 1.4426950408889634074 / (double)s.available;
    a.volume = vol ? vol->p : nullptr;
    a.vol_stride = vol ? vol->stride : 0;
    a.accumulate = vol ? vol->accumulate : 0;
    a.part_max = e->d_pmax.p;
    a.part_idx = e->d_pidx.p;
    a.part_sum = e->d_psum.p;
    a.set0 = direct && p.use_lds ? p.groups_lds : 0;
    a.brick_max = p.brick_rows && !direct ? e->d_bmax.p : nullptr;
    a.want_scan = s.want_scan ? 1 : 0;
    a.marginal = marg ? e->d_marg.p : nullptr;
    a.m0 = marg ? marg->first : 0;
    a.m1 = marg ? marg->end : 0;
    a.n_nodes = e->n_nodes;
    a.run_if = s.run_if;
    return a;
}

// ---- the families' launch tables: the LDS launch of a plan -----------------------------------------
// the round-2 kernels (they have the direct kernel's workgroup shape and publish area).  An exact-row-count kernel
// the tables do not hold: the chunked kernel runs, and the plan says so.
int launch_round2_lds(qm_engine *e, const qm::StackArgs &a, StackPlan *p) {
    const int J = p->j, S = e->g.n_rows;
    const bool VOLUME = a.volume != nullptr || a.marginal != nullptr;
    const qm::LaunchShape shape = stack_shape(e, a, p->direct_threads,
                                              std::max((size_t)run_lds_bytes(e), p->direct_publish));
    bool exact = false;
    if (p->family == kFamilyExact) {
        const bool j4_wide = J == 4 && S > 40;     // the second variant of 41-64 rows
        if (a.marginal != nullptr) {
            if (S <= 32) QM_TABLE(qm::launch_exact_marginal_1_32(S, a, shape, &exact));
            else if (!j4_wide) QM_TABLE(qm::launch_exact_marginal_33_64(S, a, shape, &exact));
            else QM_TABLE(qm::launch_exact_marginal_j4_41_64(S, a, shape, &exact));
        } else if (!VOLUME) {
            if (S <= 32) QM_TABLE(qm::launch_exact_detect_1_32(S, a, shape, &exact));
            else if (!j4_wide) QM_TABLE(qm::launch_exact_detect_33_64(S, a, shape, &exact));
            else QM_TABLE(qm::launch_exact_detect_j4_41_64(S, a, shape, &exact));
        } else {
            if (!j4_wide) QM_TABLE(qm::launch_exact_volume_33_64(S, a, shape, &exact));
            else QM_TABLE(qm::launch_exact_volume_j4_41_64(S, a, shape, &exact));
        }
    }
    // Variants specialised on the number of 8-row offset chunks (whole-node offset prefetch;
    // detect: software-pipelined node loop) for up to 64 table rows; otherwise, and for the
    // reference's accumulate-into-volume semantics, the generic kernel.
    if (!exact) {
        p->family = kFamilyChunked;
        int nch = (e->cfg.generic || a.accumulate) ? 0 : e->g.row_pad / 8;
        if (nch > 8) nch = 0;
        bool built = false;
        if (VOLUME) QM_TABLE(qm::launch_chunked_volume(J, nch, a, shape, &built));
        else QM_TABLE(qm::launch_chunked_detect(J, nch, a, shape, &built));
        if (!built) return fail("no chunked stacking kernel for %d samples per lane", J);
    }
    return 0;
}

int launch_pair_lds(qm_engine *e, const qm::StackArgs &a) {
    bool done = false;
    const qm::LaunchShape shape = stack_shape(e, a, 1024, kPairLdsBytes);
    if (a.volume) QM_TABLE(qm::launch_pair_volume(e->g.n_rows, a, shape, &done));
    else QM_TABLE(qm::launch_pair_detect(e->g.n_rows, a, shape, &done));
    if (!done) return fail("no paired kernel built for %d rows", e->g.n_rows);
    return 0;
}

int launch_shift_lds(qm_engine *e, const qm::StackArgs &a, const StackPlan &p) {
    const ShiftLayout &L = *p.shift;
    const int mode = p.shift_mode;
    qm::ShiftArgs s{};
    s.a = a;
    s.smeta = reinterpret_cast<const int4 *>(L.meta.p);
    s.stotal = L.total.p;
    s.sfit = L.fit.p;
    s.stream = reinterpret_cast<const char *>(L.stream.p);
    s.wmeta = reinterpret_cast<const int4 *>(L.wmeta.p);
    s.wtotal = L.wtotal.p;
    s.wstream = reinterpret_cast<const char *>(L.wstream.p);
    s.rows2 = L.rows2;
    s.nw = L.nw;
    s.nblk = L.nblk;
    s.sb = L.sb;
    s.stage_slots = L.stage_slots;
    s.stage_reach = L.stage_reach;
    s.lazy = p.lazy;
    const qm::LaunchShape shape = stack_shape(e, a, L.nw * qm::kWave, qm::shift_lds_bytes(L.nw));
    const bool rows = L.nblk > 1, big = L.nw == qm::kShiftWaves8;
    if (L.wide && L.direct) QM_TABLE(qm::launch_shift_wide_rows(s, shape));   // (also a single block)
    else if (rows && L.quad && mode == qm::kShiftVolume) QM_TABLE(qm::launch_shift_rows4_volume(s, shape));
    else if (rows && L.quad) QM_TABLE(qm::launch_shift_rows4(s, shape));
    else if (rows && L.direct && mode == qm::kShiftVolume) QM_TABLE(qm::launch_shift_rows2_volume(s, shape));
    else if (rows && L.direct) QM_TABLE(qm::launch_shift_rows2(s, shape));
    else if (rows) QM_TABLE(qm::launch_shift_rows8(s, shape));
    else if (mode == qm::kShiftMarginal && big) QM_TABLE(qm::launch_shift_marginal8(s, shape));
    else if (mode == qm::kShiftMarginal) QM_TABLE(qm::launch_shift_marginal(s, shape));
    else if (mode == qm::kShiftVolume && big) QM_TABLE(qm::launch_shift_volume8(s, shape));
    else if (mode == qm::kShiftVolume) QM_TABLE(qm::launch_shift_volume(s, shape));
    else if (L.nw == qm::kShiftWaves3) QM_TABLE(qm::launch_shift_detect3(s, shape));
    else if (a.brick_max && big) QM_TABLE(qm::launch_shift_detect8_sets(s, shape));
    else if (a.brick_max) QM_TABLE(qm::launch_shift_detect_sets(s, shape));
    else if (big) QM_TABLE(qm::launch_shift_detect8(s, shape));
    else QM_TABLE(qm::launch_shift_detect(s, shape));
    return 0;
}

int launch_direct(qm_engine *e, const qm::StackArgs &a, const StackPlan &p) {
    const qm::LaunchShape shape = stack_shape(e, a, p.direct_threads, p.direct_publish);
    bool built = false;
    // (the direct kernel's VOLUME covers the map too)
    if (a.volume || a.marginal) QM_TABLE(qm::launch_direct_volume(p.direct_j, a, shape, &built));
    else QM_TABLE(qm::launch_direct_detect(p.direct_j, a, shape, &built));
    if (!built) return fail("no direct stacking kernel for %d samples per lane", p.direct_j);
    return 0;
}

// The plan's launches, enqueued: scratch, the LDS launch over the bricks that fit the family's layout, the direct
// launch over those on the layout's list (their partial sets behind the LDS launch's), the timing events around both
int issue_stack(qm_engine *e, const StackLaunch &s, StackPlan *p) {
    if (p->marg_tiles && e->d_marg.ensure((size_t)p->marg_tiles * e->n_nodes)) return 1;
    const size_t rows_n = (size_t)p->brick_rows * p->scan_n;
    if (s.want_scan) {
        const size_t need = (size_t)p->sets * p->scan_n;
        if (e->d_pmax.ensure(need) || e->d_psum.ensure(need) || e->d_pidx.ensure(need)) return 1;
        if (p->brick_rows && e->d_bmax.ensure(rows_n)) return 1;
    }
    if (p->brick_rows && p->wide_tiles > 0) {
        // (the wide tiles' loop raises its rows by atomic maxima, and only where a group comes near the running
        // maximum: they start at -inf; the other tiles write theirs whole)
        hipLaunchKernelGGL(qm::fill_kernel, dim3((unsigned)std::min<size_t>((rows_n + 1023) / 1024, 65535)), dim3(256),
                           0, e->stream, e->d_bmax.p, rows_n, -std::numeric_limits<double>::infinity());
        QM_HIP(hipGetLastError());
    }
    // a conditional launch (the fallback of a screened step) is not part of the timing log: it
    // returns at once unless the step has to be redone
    const bool logged = s.run_if == nullptr;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    if (logged) {
        if (timing_events(e, &ev_begin, &ev_end)) return 1;
        QM_HIP(hipEventRecord(ev_begin, e->stream));
    }
    if (p->use_lds) {
        const qm::StackArgs a = stack_args(e, s, *p, false);
        if (p->family == kFamilyShift ? launch_shift_lds(e, a, *p)
            : p->family == kFamilyPair ? launch_pair_lds(e, a) : launch_round2_lds(e, a, p))
            return 1;
    }
    if (p->use_direct && launch_direct(e, stack_args(e, s, *p, true), *p)) return 1;
    if (logged) {
        QM_HIP(hipEventRecord(ev_end, e->stream));
        e->timed = !e->cfg.log_timing;
    }
    return 0;
}

}  // namespace

// the events around a launch: the engine's own pair, or -- the timing log -- the log's next two
int timing_events(qm_engine *e, hipEvent_t *begin, hipEvent_t *end) {
    *begin = e->ev0;
    *end = e->ev1;
    if (!e->cfg.log_timing) return 0;
    while (e->ev_used + 2 > e->ev_log.size()) {
        Event ev;
        QM_HIP(ev.create());
        e->ev_log.push_back(std::move(ev));
    }
    *begin = e->ev_log[e->ev_used];
    *end = e->ev_log[e->ev_used + 1];
    e->ev_used += 2;
    return 0;
}

// Stack samples [sample0, sample0+n_chunk) of the scan: plan, issue, and e->last describes the launch.  Partials (if
// want_scan) land in e->d_pmax/d_pidx/d_psum as [sets][n_steps * n_chunk]; a marginal launch leaves per-tile sums
// over the samples [first, end) in e->d_marg as [e->last.marg_tiles][n_nodes] (the kernels differ in their tile
// length).  n_steps > 1: that many timesteps in ONE launch (fused detect only); not every kernel can -- batched =
// false then, and nothing was launched.
StackResult run_stack(qm_engine *e, const StackLaunch &s) {
    // (from here on d_pmax describes THIS launch: whatever a detect left for qm_engine_tie_partial is gone --
    // detect_core and the group's partial launches say so again)
    e->last.sets_own = false;
    StackPlan p;
    if (plan_stack(e, s, &p)) return 1;
    StackResult r;
    r.batched = p.batched;
    if (!p.batched) return r;
    if (issue_stack(e, s, &p)) return 1;
    e->last = p;
    r.sets = p.sets;
    return r;
}

SetView engine_sets(const qm_engine *e, int n_sets, int n) {
    return {e->d_pmax.p, e->d_pidx.p, e->d_psum.p, n_sets, n, n};
}

SetView packed_sets(const double *d_packed, int n_sets, int n) {
    return {d_packed, reinterpret_cast<const int64_t *>(d_packed + n), d_packed + 2 * (int64_t)n, n_sets, n,
            3 * (int64_t)n};
}

OutSeries packed_set(double *d_packed, int n) {
    return {d_packed, d_packed + 2 * (int64_t)n, reinterpret_cast<int64_t *>(d_packed + n)};
}

int combine(qm_engine *e, const SetView &in, CombineMode mode, int64_t node_offset, int64_t n_nodes_total,
            const OutSeries &out, const int32_t *run_if) {
    // (tie_rule = 1 with a row of maxima per brick: the fold of the workgroups' own sets also leaves the largest z)
    double *o_z = nullptr;
    if (e->cfg.tie_rule && e->last.brick_rows > 0 && in.max == e->d_pmax.p && run_if == nullptr) {
        if (e->tie.zext.ensure(in.n)) return 1;
        o_z = e->tie.zext.p;
    }
    hipLaunchKernelGGL(qm::combine_kernel, dim3((in.n + qm::kWave - 1) / qm::kWave),
                       dim3(qm::kCombineWaves * qm::kWave), 0,
                       e->stream, in.max, in.idx, in.sum, in.n_sets, in.n, in.stride, (int)mode, node_offset,
                       (double)n_nodes_total, out.max, out.second, out.idx, run_if, o_z);
    QM_HIP(hipGetLastError());
    return 0;
}

StackResult stack_fold(qm_engine *e, const StackLaunch &s, CombineMode mode, int64_t n_nodes_total,
                       const OutSeries &out) {
    const StackResult r = run_stack(e, s);
    if (r.rc || !r.batched) return r;
    if (const auto *m = std::get_if<StackLaunch::Marginal>(&s.kind)) {
        hipLaunchKernelGGL(qm::marginal_reduce_kernel, dim3((unsigned)((e->n_nodes + 255) / 256)), dim3(256), 0,
                           e->stream, e->d_marg.p, e->last.marg_tiles, e->n_nodes, m->map);
        QM_HIP(hipGetLastError());
    }
    if (!s.want_scan) return r;
    const OutSeries o = out.at(s.sample0);
    if (combine(e, engine_sets(e, r.sets, s.n_chunk * s.n_steps), mode, e->node_offset, n_nodes_total, o,
                s.run_if))
        return 1;
    // (the reference's rule on near-ties: final series of this engine's own nodes only -- the partial
    // sets of a sharded detect leave the engine before anyone knows the global maximum -- and not on the
    // screened step's fallback)
    if (mode == kCombineFinal && e->cfg.tie_rule && s.run_if == nullptr && refine_ties(e, s, o.idx, nullptr, nullptr))
        return 1;
    return r;
}

// Detect-type stacking of the whole scan plus the combine of its partial sets into the three
// output series.  With screening: the screened result is combined first;
// then the float64 kernel and its combine are enqueued conditionally on the step's flag word, so a
// step that could not be screened (too many candidate cells, non-finite onsets) is redone on the
// device without the host ever waiting -- those launches return at once otherwise.
int detect_core(qm_engine *e, const double *d_on, int T, int fsmp, int ns, int available, CombineMode mode,
                int64_t n_nodes_total, const OutSeries &out) {
    int sets = 0;
    bool screened = false;
    // (the screened sweep leaves no float64 sets to refine near-ties from, and its conditional fallback cannot be
    // followed by a refinement nobody waits for: the two opt-ins exclude each other on the detect calls)
    e->last.sets_own = false;                           // (the screened sweep writes d_pmax as well; a refused
                                                        // call is no detect_partial either)
    if (e->cfg.screen && e->cfg.tie_rule)
        return fail("detect: the config keys screen = 1 and tie_rule = 1 cannot be combined (the screened detect "
                    "has no near-tie refinement): set one of them to 0");
    if (run_screen(e, d_on, T, fsmp, ns, available, &sets, &screened)) return 1;
    StackLaunch s(d_on, T, fsmp, ns, available);
    if (screened) {
        if (combine(e, engine_sets(e, sets, ns), mode, e->node_offset, n_nodes_total, out, nullptr)) return 1;
        s.run_if = e->sweep.flags.p;
    }
    if (stack_fold(e, s, mode, n_nodes_total, out).rc) return 1;
    // (d_pmax holds the float64 launch's sets for certain -- and they are those of a detect_partial, the only call
    // qm_engine_tie_partial follows: a final detect of other onsets at the same sample count is refused like any
    // other launch in between)
    e->last.sets_own = !screened && mode == kCombinePartial;
    return 0;
}

int scan_fold(qm_engine *e, const double *vol, int64_t stride, int ns, int64_t n_nodes, int64_t node0,
              CombineMode mode, const OutSeries &out) {
    // a workgroup = up to 16 adjacent tiles (one wavefront each); ~cfg.scan_waves wavefronts
    // per CU in total; at least 256 nodes per chunk
    const int tiles = (ns + qm::kWave - 1) / qm::kWave;
    const int groups = (tiles + qm::kScanWaves - 1) / qm::kScanWaves;
    const int waves = (tiles + groups - 1) / groups;          // per workgroup, balanced
    const int xgroups = (tiles + waves - 1) / waves;
    int64_t sets = std::max<int64_t>(1, ((int64_t)e->cfg.scan_waves * e->n_cu + tiles - 1) / tiles);
    sets = std::min<int64_t>(sets, std::max<int64_t>(1, n_nodes / 256));
    sets = std::min<int64_t>(sets, 65535);
    const int64_t per = (n_nodes + sets - 1) / sets;
    sets = (n_nodes + per - 1) / per;
    const size_t need = (size_t)sets * ns;
    e->last.sets_own = false;                           // (a volume's sets overwrite a detect's: qm_engine_tie_partial)
    if (e->d_pmax.ensure(need) || e->d_psum.ensure(need) || e->d_pidx.ensure(need)) return 1;
    hipLaunchKernelGGL(qm::scan_volume_kernel, dim3(xgroups, (unsigned)sets), dim3(waves * qm::kWave), 0, e->stream,
                       vol, stride, ns, n_nodes, per, e->d_pmax.p, e->d_pidx.p, e->d_psum.p);
    QM_HIP(hipGetLastError());
    // (a partial has no normalisation: n_nodes_total only matters for the values' series)
    return combine(e, engine_sets(e, (int)sets, ns), mode, node0, mode == kCombinePartial ? 0 : n_nodes, out,
                   nullptr);
}

// tie_rule = 1 (qm_ties.hpp): the index series o_idx of `launch`, whose partial sets lie in d_pmax (as
// e->last describes them), refined.  n_steps > 1: the launch held several timesteps.  zext / o_key:
// a sharded detect's engine -- its sets against the grid's maxima, the outcome exported (tie_export_kernel)
// instead of applied.
int refine_ties(qm_engine *e, const StackLaunch &launch, int64_t *o_idx, const double *zext,
                unsigned long long *o_key) {
    const int n_steps = launch.n_steps, n_chunk = launch.n_chunk, sets = e->last.sets;
    const int n = n_chunk * std::max(1, n_steps);
    if (n > INT32_MAX / (2 * qm::kTieMaxSets)) return fail("tie_rule: %d samples in one launch are too many", n);
    const int max_pairs = qm::kTieMaxSets * n;
    const int max_cands = 4 * n + 65536;
    if (e->tie.z.ensure(n) || e->tie.pairs.ensure(2 * (size_t)max_pairs) || e->tie.imin.ensure(n) ||
        e->tie.count.ensure(4) || e->tie.emax.ensure(n) || e->tie.cands.ensure(2 * (size_t)max_cands) ||
        e->tie.keys.ensure(max_cands))
        return 1;
    hipStream_t s = e->stream;
    QM_HIP(hipMemsetAsync(e->tie.count.p, 0, 4 * sizeof(int32_t), s));
    int2 *pairs = reinterpret_cast<int2 *>(e->tie.pairs.p);
    // (brick maxima: the sample's largest z is already in the workgroups' few partial sets; the per-brick rows are
    // read once, for the candidates)
    // (... and the sample's largest z came out of the combine that preceded this call)
    const int rows = e->last.brick_rows;
    if (rows > 0 && !zext) zext = e->tie.zext.p;
    hipLaunchKernelGGL(qm::tie_pairs_kernel, dim3((n + 63) / 64), dim3(64, qm::kTieSetLanes), 0, s,
                       rows > 0 ? (const double *)e->d_bmax.p : (const double *)e->d_pmax.p, rows > 0 ? rows : sets,
                       (const double *)e->d_pmax.p + (int64_t)e->last.groups_lds * n,
                       rows > 0 ? e->last.groups_direct : 0, n, (int64_t)n, e->tie.z.p, pairs,
                       e->tie.count.p, max_pairs, e->tie.emax.p, e->tie.imin.p, e->tie.count.p + 1, zext);
    QM_HIP(hipGetLastError());
    // How many pairs there are is known on the device only, and nobody waits for it: the evaluation is
    // launched for what a generic step has (one pair per sample) with room to spare; workgroups beyond the
    // list return at once, a longer list is covered by the grid's stride.  The
    // counters travel to the host when somebody asks (qm_engine_get "tie_pairs", "tie_overflow_samples").
    ++e->tie.refined_steps;
    e->tie.counts_pending = true;
    qm::TieArgs a{};
    a.g = e->last.g;
    a.onsets = launch.onsets;
    a.lut = e->d_lut.p;
    a.T = launch.T; a.fsmp = launch.fsmp; a.sample0 = launch.sample0; a.n_chunk = n;
    a.ns_step = n_steps > 1 ? n_chunk : 0;
    a.step_stride = launch.step_stride;
    a.z_scale = 1.4426950408889634074 / (double)launch.available;
    a.recip = 1.0 / (double)launch.available;
    a.groups_lds = e->last.groups_lds;
    a.groups_direct = e->last.groups_direct;
    a.brick_rows = rows;
    a.brick_list = e->last.list;
    a.n_list = e->last.n_list;
    // workgroups per pair: ~2048 nodes each
    const int64_t per_set = (int64_t)e->n_nodes / std::max(1, e->last.groups_lds + e->last.groups_direct);
    a.chunks = rows > 0 ? 1 : (int)std::max<int64_t>(1, std::min<int64_t>(64, per_set / 2048));   // (rows: a brick)
    a.zbest = e->tie.z.p;
    a.pairs = pairs;
    a.n_pairs = e->tie.count.p;
    a.emax = e->tie.emax.p;
    a.imin = e->tie.imin.p;
    a.cands = reinterpret_cast<int2 *>(e->tie.cands.p);
    a.cand_keys = e->tie.keys.p;
    a.n_cands = e->tie.count.p + 2;
    a.max_cands = max_cands;
    const unsigned grid = (unsigned)((int64_t)(n + 1024) * a.chunks);
    hipLaunchKernelGGL(qm::tie_eval_kernel<0>, dim3(grid), dim3(256), 0, s, a);
    hipLaunchKernelGGL(qm::tie_pick_kernel, dim3(256), dim3(256), 0, s, a);
    hipLaunchKernelGGL(qm::tie_eval_kernel<1>, dim3(grid), dim3(256), 0, s, a);   // (returns at once unless the list overflowed)
    if (o_key)
        hipLaunchKernelGGL(qm::tie_export_kernel, dim3((n + 255) / 256), dim3(256), 0, s,
                           (const unsigned long long *)e->tie.emax.p, (const int32_t *)e->tie.imin.p, n,
                           e->node_offset, o_key, o_idx);
    else
        hipLaunchKernelGGL(qm::tie_apply_kernel, dim3((n + 255) / 256), dim3(256), 0, s,
                           (const int32_t *)e->tie.imin.p, n, e->node_offset, o_idx);
    QM_HIP(hipGetLastError());
    return 0;
}

int check_step(qm_engine *e, int T, int fsmp, int lsmp, int available, int *n_samples) {
    if (!e->have_lut) return fail("no travel-time table resident: call qm_engine_load_lut first");
    if (fsmp < 0 || lsmp < 0) return fail("negative pad (fsmp=%d, lsmp=%d)", fsmp, lsmp);
    const int ns = T - fsmp - lsmp;
    if (ns <= 0) return fail("no samples to scan: T=%d fsmp=%d lsmp=%d", T, fsmp, lsmp);
    if (available <= 0) return fail("available must be positive (got %d)", available);
    if (e->lut_max > lsmp)
        return fail("largest travel time (%d samples) exceeds the post-pad lsmp=%d: the scan "
                    "would read past the onset rows (undefined behaviour in the reference)",
                    e->lut_max, lsmp);
    *n_samples = ns;
    return 0;
}

int stage_out(qm_engine *e, int n, int out_on_device, const OutSeries &user, OutSeries *st) {
    if (out_on_device) {
        *st = user;
        return 0;
    }
    // (the three series back to back in ONE buffer: they travel to the host as one copy, fetch_out)
    if (e->d_out_a.ensure(3 * (size_t)n)) return 1;
    *st = OutSeries{e->d_out_a.p, e->d_out_a.p + n, reinterpret_cast<int64_t *>(e->d_out_a.p + 2 * (size_t)n)};
    return 0;
}

int fetch_out(qm_engine *e, int n, int out_on_device, const OutSeries &st, const OutSeries &user) {
    if (out_on_device) return 0;
    // one DMA of the packed [3][n] buffer, three CPU copies out of the pinned half (round 4: three
    // DMAs with a wait each -- two round trips more per host-array call)
    void *dst[3] = {user.max, user.second, user.idx};
    QM_HIP(copy_back_pieces(dst, st.max, 3, (size_t)n * sizeof(double), e->stream));
    return 0;
}

namespace {

// qm_engine_finalize / _finalize_packed: the final series of partial sets, on host or device
int finalize_sets(qm_engine *e, const SetView &in, int64_t n_nodes_total, const OutSeries &user, int out_on_device) {
    DeviceGuard guard(e->device);
    OutSeries st;
    if (stage_out(e, in.n, out_on_device, user, &st) || combine(e, in, kCombineFinal, 0, n_nodes_total, st, nullptr))
        return 1;
    return fetch_out(e, in.n, out_on_device, st, user);
}

// The read-outs that are no tunables: name, value and -- where the value is still on the device -- what brings it to
// the host first (run under a DeviceGuard).  waves, lds_bytes, screen_pairs, screen_big, shift_waves and shift_lazy
// shadow the tunable of the same name with the live value.
struct Readout {
    const char *name;
    int64_t (*value)(const qm_engine *e);
    int (*fetch)(qm_engine *e);
};
int fetch_tie_counts(qm_engine *e) {                    // (the last refinement's counters: now)
    if (!e->tie.counts_pending) return 0;
    int32_t h[2] = {0, 0};
    QM_HIP(copy_back(h, e->tie.count.p, sizeof(h), e->stream));
    e->tie.pairs_last = h[0];
    e->tie.overflow_last = h[1];
    e->tie.counts_pending = false;
    return 0;
}
#define V(expr) [](const qm_engine *e) -> int64_t { return (expr); }
const Readout kReadouts[] = {
    {"waves", V(run_waves(e))}, {"lds_bytes", V(run_lds_bytes(e))},
    {"screen_pairs", V(e->sweep.last_plan_jp)}, {"screen_big", V(e->sweep.last_plan_big)},
    // (of the layout the last launch ran on, if shift-reuse and still this table's: a table change voids the layouts,
    // invalidate_derived)
    {"shift_waves", V(e->last.shift && e->last.shift->ok ? e->last.shift->nw : e->sh.ok ? e->sh.nw : e->cfg.shift_waves)},
    // the screened detect
    {"screened_steps", V(e->sweep.screened_steps), drain_flags}, {"fallback_steps", V(e->sweep.fallback_steps), drain_flags},
    {"last_candidates", V(e->sweep.last_candidates), drain_flags}, {"screen_brick_nodes", V(e->screen.g.brick_nodes)},
    // the last stacking launch and the shift-reuse layouts
    {"last_kernel", V(e->last.family)}, {"last_kernel_j", V(e->last.j)}, {"steps_per_launch", V(e->last_batched)},
    {"shift_tail_spl", V(e->last.tail_spl)}, {"shift_wide_tiles", V(e->last.wide_tiles)},
    {"shift_ok", V(e->sh.built && e->sh.ok ? 1 : 0)}, {"shift_wide_ok", V(e->shw.built && e->shw.ok ? 1 : 0)},
    {"shift_row_blocks", V(e->sh.ok ? e->sh.nblk : 0)}, {"shift_wide_row_blocks", V(e->shw.ok ? e->shw.nblk : 0)},
    {"shift_brick_nodes", V(e->sh.ok ? e->sh.g.brick_nodes : 0)},
    {"shift_wide_brick_nodes", V(e->shw.ok ? e->shw.g.brick_nodes : 0)},
    {"shift_wide_bricks", V(e->sh.ok ? e->sh.n_list : 0)}, {"shift_wide_direct_bricks", V(e->shw.ok ? e->shw.n_list : 0)},
    // 8-byte LDS operands fetched per add (x 1000); per add of a wide tile
    {"shift_operands_per_add_x1000",
     V(e->sh.ok && e->sh.group_rows > 0 ? (e->sh.quads * 4 * 1000) / (e->sh.group_rows * 32) : 0)},
    {"shift_wide_operands_per_add_x1000",
     V(e->shw.ok && e->shw.group_rows > 0 ? (e->shw.wquads * 4 * 1000) / (e->shw.group_rows * 48) : 0)},
    {"pair_brick_nodes", V(e->pair.kt ? e->pair.g.brick_nodes : 0)}, {"pair_tile", V(e->pair.ok ? e->pair.kt : 0)},
    {"pair_wide_bricks", V(e->pair.kt ? e->pair.n_list : 0)}, {"shift_lazy", V(e->last.lazy)},
    // the stage kernels' constants
    {"pick_lds_samples", V(qm::kPicksLdsSamples)}, {"amp_lds_samples", V(qm::kAmpLdsSamples)},
    {"trigger_max_radius", V(qm::kTrigMaxRadius)}, {"trigger_smooth_tile", V(qm::kTrigSmoothTile)},
    {"trigger_run_block", V(qm::kTrigRunBlock)}, {"trigger_merge_stride", V(qm::kTrigMergeThreads)},
    {"scanmseed_tile", V(qm::kSmsTile)}, {"scanmseed_compose_chunk", V(qm::kSmsComposeChunk)},
    {"tt_lds_nodes", V(qm::kTtLdsNodes)}, {"tt_section_threads", V(qm::kTtSectionThreads)},
    {"tt_grid_blocks", V(qm::kTtGridBlocks)}, {"tt_grid_threads", V(qm::kTtGridThreads)},
    {"tt_plane_threads", V(qm::kTtPlaneThreads)}, {"tt_plane_max_rows", V(qm::kTtPlaneMaxRows)},
    // the near-tie refinement
    {"tie_brick_rows", V(e->last.brick_rows)}, {"tie_refined_steps", V(e->tie.refined_steps)},
    {"tie_overflow_samples", V(e->tie.overflow_last), fetch_tie_counts}, {"tie_pairs", V(e->tie.pairs_last), fetch_tie_counts},
    // tables: parked ones, device bytes of the resident table's state and of the parked ones, the process's pool
    {"table_hits", V(e->table_hits)}, {"table_misses", V(e->table_misses)}, {"table_evictions", V(e->table_evictions)},
    {"table_digests", V(e->table_digests)}, {"table_bytes", V(e->device_bytes())},
    {"tables_parked", V(std::count_if(e->slots.begin(), e->slots.end(), [](const TableSlot &sl) { return sl.used; }))},
    {"tables_parked_bytes", [](const qm_engine *e) -> int64_t {
         int64_t sum = 0;
         for (const TableSlot &sl : e->slots) sum += sl.used ? (int64_t)sl.state.device_bytes() : 0;
         return sum;
     }},
    {"pool_live_bytes", V(pool_live_bytes(e->device))},
    // the resident table and the device
    {"n_bricks", V(e->g.nbricks)},
    {"n_wide_bricks", V(e->r2().n_list), [](qm_engine *e) { return e->have_lut ? plan_wide(e, eff_j(e)) : 0; }},
    {"mean_span", [](const qm_engine *e) -> int64_t {   // mean delay span per (brick, row), samples
         int64_t sum = 0;
         const std::vector<int32_t> &totals = e->r2().h_total;
         for (int32_t t : totals) sum += t;
         return totals.empty() ? 0 : sum / ((int64_t)totals.size() * std::max(1, e->g.n_rows));
     }},
    {"n_cu", V(e->n_cu)}, {"n_nodes", V(e->n_nodes)}, {"n_rows", V(e->g.n_rows)},
    {"nx", V(e->g.nx)}, {"ny", V(e->g.ny)}, {"nz", V(e->g.nz)},
};
#undef V

// "<prefix><stage name>" of a stage clock: the last call's time for that stage
template <int N>
bool clock_readout(const StageClock<N> &clock, const std::string &prefix, const std::string &key, int64_t *v) {
    for (int st = 0; st < N; ++st)
        if (key == prefix + clock.names[st]) return *v = clock.ns[st], true;
    return false;
}

}  // namespace

// ------------------------------------------------------------------------------- C ABI
extern "C" {

int qm_engine_create(int device_id, qm_engine **out) {
    if (!out) return fail("qm_engine_create: out is NULL");
    int n = 0;
    QM_HIP(hipGetDeviceCount(&n));
    if (device_id < 0 || device_id >= n)
        return fail("device %d not available (%d HIP devices visible)", device_id, n);
    DeviceGuard guard(device_id);
    // (destroyed as any engine is if a step below fails: what it holds by then goes back)
    std::unique_ptr<qm_engine, decltype(&qm_engine_destroy)> e(new qm_engine(), qm_engine_destroy);
    e->device = device_id;
    hipDeviceProp_t prop;
    QM_HIP(hipGetDeviceProperties(&prop, device_id));
    e->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    QM_HIP(acquire_stream(device_id, &e->own_stream));
    e->stream = e->own_stream;
    QM_HIP(e->ev0.create());
    QM_HIP(e->ev1.create());
    *out = e.release();
    return 0;
}

void qm_engine_destroy(qm_engine *e) {
    if (!e) return;
    DeviceGuard guard(e->device);
    (void)hipStreamSynchronize(e->stream);
    streams_orphan(e);                                  // (before the engine's own buffers go)
    if (e->own_stream) {
        (void)hipStreamSynchronize(e->own_stream);
        park_stream(e->device, e->own_stream);
    }
    PoolReleaseScope one_wait;                          // every buffer of the engine behind ONE device-wide wait
    delete e;
}

int qm_engine_set_stream(qm_engine *e, void *hip_stream, int use_own) {
    if (!e) return fail("engine is NULL");
    // NULL with use_own == 0 is the device's default (null) stream -- what
    // torch.cuda.current_stream().cuda_stream is unless a stream context is active
    {
        DeviceGuard guard(e->device);
        if (drain_flags(e)) return 1;       // per-step outcomes still travelling on the old stream
    }
    e->stream = use_own ? e->own_stream : reinterpret_cast<hipStream_t>(hip_stream);
    return 0;
}

int qm_engine_synchronize(qm_engine *e) {
    if (!e) return fail("engine is NULL");
    DeviceGuard guard(e->device);
    QM_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

int qm_engine_config(qm_engine *e, const char *key, int64_t v) {
    if (!e || !key) return fail("qm_engine_config: NULL argument");
    unsigned effects = 0;
    if (config_set(e->cfg, key, v, &effects)) return 1;
    if (effects & kVoidShift) e->sh.invalidate();
    if (effects & kVoidShiftWide) e->shw.invalidate();
    if (effects & kVoidScreen) e->screen.invalidate();
    if (effects & kResetTimingLog) e->ev_used = 0;
    return 0;
}

// In this order: the resident table's brick shape and samples per lane where there is a table, the read-outs of
// kReadouts (above) and of the stage clocks, the tunables as set (config_get).
int qm_engine_get(qm_engine *e, const char *key, int64_t *v) {
    if (!e || !key || !v) return fail("qm_engine_get: NULL argument");
    const std::string k(key);
    if (e->have_lut && (k == "brick_x" || k == "brick_y" || k == "brick_z" || k == "samples_per_lane")) {
        *v = k == "brick_x" ? e->g.bx : k == "brick_y" ? e->g.by : k == "brick_z" ? e->g.bz : eff_j(e);
        return 0;
    }
    for (const Readout &r : kReadouts) {
        if (k != r.name) continue;
        if (r.fetch) {
            DeviceGuard guard(e->device);
            if (r.fetch(e)) return 1;
        }
        *v = r.value(e);
        return 0;
    }
    if (clock_readout(e->trig.clock, "trigger_ns_", k, v) || clock_readout(e->sms.clock, "scanmseed_ns_", k, v) ||
        clock_readout(e->tt.clock, "tt_ns_", k, v) ||
        config_get(e->cfg, key, v))
        return 0;
    return fail("unknown key '%s'", key);
}

int qm_engine_detect_partial(qm_engine *e, const double *log_onsets, int onsets_on_device,
                             int32_t T, int32_t fsmp, int32_t lsmp, int32_t available,
                             double *d_part_max, int64_t *d_part_idx, double *d_part_sum) {
    if (!e || !log_onsets || !d_part_max || !d_part_idx || !d_part_sum)
        return fail("qm_engine_detect_partial: NULL argument");
    DeviceGuard guard(e->device);
    int ns = 0;
    const double *d_on = nullptr;
    if (check_step(e, T, fsmp, lsmp, available, &ns) || !(d_on = stage_onsets(e, log_onsets, onsets_on_device, T)))
        return 1;
    return detect_core(e, d_on, T, fsmp, ns, available, kCombinePartial, 0,
                       OutSeries{d_part_max, d_part_sum, d_part_idx});
}

int qm_engine_finalize(qm_engine *e, const double *d_part_max, const int64_t *d_part_idx,
                       const double *d_part_sum, int32_t n_sets, int32_t n_samples,
                       int64_t n_nodes_total, double *max_coa, double *max_norm_coa,
                       int64_t *max_coa_idx, int out_on_device) {
    if (!e || !d_part_max || !d_part_idx || !d_part_sum || !max_coa || !max_norm_coa ||
        !max_coa_idx)
        return fail("qm_engine_finalize: NULL argument");
    if (n_sets < 1 || n_samples < 1) return fail("qm_engine_finalize: empty input");
    return finalize_sets(e, SetView{d_part_max, d_part_idx, d_part_sum, n_sets, n_samples, n_samples},
                         n_nodes_total, OutSeries{max_coa, max_norm_coa, max_coa_idx}, out_on_device);
}

int qm_engine_finalize_packed(qm_engine *e, const double *d_packed, int32_t n_sets,
                              int32_t n_samples, int64_t n_nodes_total, double *max_coa,
                              double *max_norm_coa, int64_t *max_coa_idx, int out_on_device) {
    if (!e || !d_packed || !max_coa || !max_norm_coa || !max_coa_idx)
        return fail("qm_engine_finalize_packed: NULL argument");
    if (n_sets < 1 || n_samples < 1) return fail("qm_engine_finalize_packed: empty input");
    return finalize_sets(e, packed_sets(d_packed, n_sets, n_samples), n_nodes_total,
                         OutSeries{max_coa, max_norm_coa, max_coa_idx}, out_on_device);
}

int qm_engine_detect(qm_engine *e, const double *log_onsets, int onsets_on_device, int32_t T,
                     int32_t fsmp, int32_t lsmp, int32_t available, int64_t n_nodes_total,
                     double *max_coa, double *max_norm_coa, int64_t *max_coa_idx,
                     int out_on_device) {
    if (!e || !log_onsets || !max_coa || !max_norm_coa || !max_coa_idx)
        return fail("qm_engine_detect: NULL argument");
    DeviceGuard guard(e->device);
    int ns = 0;
    const double *d_on = nullptr;
    const OutSeries user{max_coa, max_norm_coa, max_coa_idx};
    OutSeries st;
    if (check_step(e, T, fsmp, lsmp, available, &ns) || !(d_on = stage_onsets(e, log_onsets, onsets_on_device, T)) ||
        stage_out(e, ns, out_on_device, user, &st))
        return 1;
    if (detect_core(e, d_on, T, fsmp, ns, available, kCombineFinal, n_nodes_total, st)) return 1;
    return fetch_out(e, ns, out_on_device, st, user);
}

int qm_engine_detect_batch(qm_engine *e, const double *log_onsets, int onsets_on_device,
                           int32_t n_steps, int32_t T, int32_t fsmp, int32_t lsmp, int32_t available,
                           int64_t n_nodes_total, double *max_coa, double *max_norm_coa,
                           int64_t *max_coa_idx, int out_on_device) {
    if (!e || !log_onsets || !max_coa || !max_norm_coa || !max_coa_idx)
        return fail("qm_engine_detect_batch: NULL argument");
    if (n_steps < 1) return fail("qm_engine_detect_batch: n_steps must be >= 1 (got %d)", n_steps);
    DeviceGuard guard(e->device);
    int ns = 0;
    if (check_step(e, T, fsmp, lsmp, available, &ns)) return 1;
    if ((int64_t)n_steps * ns >= INT32_MAX) return fail("qm_engine_detect_batch: too many samples");
    const size_t per_step = (size_t)e->g.n_rows * T;
    const double *d_on = stage_onsets(e, log_onsets, onsets_on_device, T, n_steps);
    if (!d_on) return 1;
    const int n_all = n_steps * ns;
    const OutSeries user{max_coa, max_norm_coa, max_coa_idx};
    OutSeries st;
    if (stage_out(e, n_all, out_on_device, user, &st)) return 1;
    bool batched = false;
    if (n_steps > 1 && !e->cfg.screen) {
        // partial sets [sets][n_steps * ns] -> the steps' series back to back (tie_rule = 1 keeps the step
        // axis: the refinement reads the launch's sets with sample t = step * ns + ...)
        StackLaunch s(d_on, T, fsmp, ns, available);
        s.n_steps = n_steps;
        s.step_stride = (int64_t)per_step;
        const StackResult r = stack_fold(e, s, kCombineFinal, n_nodes_total, st);
        if (r.rc) return 1;
        batched = r.batched;
    }
    if (!batched)                                       // step by step (a single step, the screened
        for (int k = 0; k < n_steps; ++k)               // detect, kernels without the step axis)
            if (detect_core(e, d_on + (size_t)k * per_step, T, fsmp, ns, available, kCombineFinal, n_nodes_total,
                            st.at((int64_t)k * ns)))
                return 1;
    e->last_batched = batched ? n_steps : 1;
    return fetch_out(e, n_all, out_on_device, st, user);
}

// tie_rule = 1 on a sharded detect (qm_ties.hpp, tie_export_kernel / tie_fold_kernel): after the exchange of
// the ranks' partials, every engine examines the sets its last qm_engine_detect_partial left behind against the
// GRID's maxima ...
int qm_engine_tie_partial(qm_engine *e, const double *log_onsets, int onsets_on_device, int32_t T,
                          int32_t fsmp, int32_t lsmp, int32_t available, const double *d_packed,
                          int32_t n_sets, double *d_tie_packed) {
    if (!e || !log_onsets || !d_packed || !d_tie_packed) return fail("qm_engine_tie_partial: NULL argument");
    if (n_sets < 1) return fail("qm_engine_tie_partial: empty input");
    DeviceGuard guard(e->device);
    int ns = 0;
    if (check_step(e, T, fsmp, lsmp, available, &ns)) return 1;
    if (!e->cfg.tie_rule) return fail("qm_engine_tie_partial: the engine was not configured with tie_rule = 1");
    if (e->last.scan_n != ns || e->last.sets < 1 || !e->last.sets_own)
        return fail("qm_engine_tie_partial: no partial sets of a float64 detect of %d samples on this engine "
                    "(call qm_engine_detect_partial for the step first, with no other launch, volume scan or "
                    "table change in between; the screened sweep leaves none)", ns);
    const double *d_on = nullptr;
    if (!(d_on = stage_onsets(e, log_onsets, onsets_on_device, T))) return 1;
    // the grid's largest z per sample: the fold of the gathered maxima (rows [s][0] of [n_sets][3][ns])
    if (e->tie.zgrid.ensure(ns)) return 1;
    hipLaunchKernelGGL(qm::tie_zmax_kernel, dim3((ns + 255) / 256), dim3(256), 0, e->stream, d_packed, (int)n_sets,
                       ns, 3 * (int64_t)ns, e->tie.zgrid.p);
    QM_HIP(hipGetLastError());
    return refine_ties(e, StackLaunch(d_on, T, fsmp, ns, available), reinterpret_cast<int64_t *>(d_tie_packed + ns),
                       e->tie.zgrid.p, reinterpret_cast<unsigned long long *>(d_tie_packed));
}

// ... and folds the gathered outcomes [n_sets][2][n_samples] into the index series (device, in place).
int qm_engine_tie_fold(qm_engine *e, const double *d_tie_gathered, int32_t n_sets, int32_t n_samples,
                       int64_t *d_max_coa_idx) {
    if (!e || !d_tie_gathered || !d_max_coa_idx) return fail("qm_engine_tie_fold: NULL argument");
    if (n_sets < 1 || n_samples < 1) return fail("qm_engine_tie_fold: empty input");
    DeviceGuard guard(e->device);
    hipLaunchKernelGGL(qm::tie_fold_kernel, dim3((n_samples + 255) / 256), dim3(256), 0, e->stream,
                       reinterpret_cast<const unsigned long long *>(d_tie_gathered), (int)n_sets, (int)n_samples,
                       d_max_coa_idx);
    QM_HIP(hipGetLastError());
    return 0;
}

int qm_engine_migrate(qm_engine *e, const double *log_onsets, int onsets_on_device, int32_t T,
                      int32_t fsmp, int32_t lsmp, int32_t available, int64_t n_nodes_total,
                      double *map4d, int map_on_device, int accumulate, double *max_coa,
                      double *max_norm_coa, int64_t *max_coa_idx, int out_on_device) {
    if (!e || !log_onsets || !map4d) return fail("qm_engine_migrate: NULL argument");
    const bool want_scan = max_coa != nullptr;
    if (want_scan && (!max_norm_coa || !max_coa_idx))
        return fail("qm_engine_migrate: all three scan outputs or none");
    DeviceGuard guard(e->device);
    int ns = 0;
    const double *d_on = nullptr;
    const OutSeries user{max_coa, max_norm_coa, max_coa_idx};
    OutSeries st;
    if (check_step(e, T, fsmp, lsmp, available, &ns) || !(d_on = stage_onsets(e, log_onsets, onsets_on_device, T)) ||
        (want_scan && stage_out(e, ns, out_on_device, user, &st)))
        return 1;
    StackLaunch s(d_on, T, fsmp, ns, available);
    s.want_scan = want_scan;
    if (map_on_device) {
        s.kind = StackLaunch::Volume{map4d, ns, accumulate};
        if (stack_fold(e, s, kCombineFinal, n_nodes_total, st).rc) return 1;
    } else {
        // host volume: stream it through a device chunk buffer, time-chunk by time-chunk
        const int KT = qm::kWave * eff_j(e);
        int64_t chunk = e->cfg.chunk_bytes / (8 * e->n_nodes);
        chunk = std::max<int64_t>(KT, chunk / KT * KT);
        chunk = std::min<int64_t>(chunk, ns);
        if (e->d_chunk.ensure((size_t)e->n_nodes * chunk)) return 1;
        for (int k0 = 0; k0 < ns; k0 += (int)chunk) {
            const int nk = (int)std::min<int64_t>(chunk, ns - k0);
            if (accumulate)
                QM_HIP(copy_in_2d(e->d_chunk.p, nk * sizeof(double), map4d + k0,
                                        (size_t)ns * sizeof(double), nk * sizeof(double),
                                        e->n_nodes, e->stream));
            s.sample0 = k0;
            s.n_chunk = nk;
            s.kind = StackLaunch::Volume{e->d_chunk.p, nk, accumulate};
            if (stack_fold(e, s, kCombineFinal, n_nodes_total, st).rc) return 1;
            QM_HIP(copy_back_2d(map4d + k0, (size_t)ns * sizeof(double), e->d_chunk.p,
                                    nk * sizeof(double), nk * sizeof(double), e->n_nodes, e->stream));
            QM_HIP(hipStreamSynchronize(e->stream));
        }
    }
    if (want_scan) return fetch_out(e, ns, out_on_device, st, user);
    if (!map_on_device) QM_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

int qm_engine_marginal(qm_engine *e, const double *log_onsets, int onsets_on_device, int32_t T,
                       int32_t fsmp, int32_t lsmp, int32_t available, int64_t n_nodes_total,
                       int32_t first_sample, int32_t end_sample, double *coa_map,
                       int map_on_device, double *max_coa, double *max_norm_coa,
                       int64_t *max_coa_idx, int out_on_device) {
    if (!e || !log_onsets || !coa_map) return fail("qm_engine_marginal: NULL argument");
    const bool want_scan = max_coa != nullptr;
    if (want_scan && (!max_norm_coa || !max_coa_idx))
        return fail("qm_engine_marginal: all three scan outputs or none");
    DeviceGuard guard(e->device);
    int ns = 0;
    if (check_step(e, T, fsmp, lsmp, available, &ns)) return 1;
    if (first_sample < 0 || end_sample > ns || first_sample >= end_sample)
        return fail("marginal window [%d, %d) outside the %d scanned samples", first_sample,
                    end_sample, ns);
    const double *d_on = nullptr;
    const OutSeries user{max_coa, max_norm_coa, max_coa_idx};
    OutSeries st;
    if (!(d_on = stage_onsets(e, log_onsets, onsets_on_device, T)) ||
        (want_scan && stage_out(e, ns, out_on_device, user, &st)))
        return 1;
    const StagedOut<double> map = stage_host_out(e->d_marg_out, coa_map, map_on_device, (size_t)e->n_nodes);
    if (!map.d) return 1;
    StackLaunch s(d_on, T, fsmp, ns, available);
    s.want_scan = want_scan;
    s.kind = StackLaunch::Marginal{first_sample, end_sample, map.d};
    if (stack_fold(e, s, kCombineFinal, n_nodes_total, st).rc || map.fetch(e)) return 1;
    if (!map_on_device) QM_HIP(hipStreamSynchronize(e->stream));
    if (want_scan) return fetch_out(e, ns, out_on_device, st, user);
    return 0;
}

int qm_engine_find_max_coa(qm_engine *e, const double *map4d, int map_on_device,
                           int32_t n_samples, int64_t n_nodes, double *max_coa,
                           double *max_norm_coa, int64_t *max_coa_idx, int out_on_device) {
    if (!e || !map4d || !max_coa || !max_norm_coa || !max_coa_idx)
        return fail("qm_engine_find_max_coa: NULL argument");
    if (n_samples < 1 || n_nodes < 1) return fail("qm_engine_find_max_coa: empty volume");
    DeviceGuard guard(e->device);
    const OutSeries user{max_coa, max_norm_coa, max_coa_idx};
    OutSeries st;
    if (stage_out(e, n_samples, out_on_device, user, &st)) return 1;
    if (map_on_device) {
        if (scan_fold(e, map4d, n_samples, n_samples, n_nodes, 0, kCombineValues, st)) return 1;
    } else {
        int64_t chunk = std::max<int64_t>(1, e->cfg.chunk_bytes / (8 * n_nodes));
        chunk = std::min<int64_t>(chunk, n_samples);
        if (e->d_chunk.ensure((size_t)n_nodes * chunk)) return 1;
        for (int k0 = 0; k0 < n_samples; k0 += (int)chunk) {
            const int nk = (int)std::min<int64_t>(chunk, n_samples - k0);
            QM_HIP(copy_in_2d(e->d_chunk.p, nk * sizeof(double), map4d + k0,
                                    (size_t)n_samples * sizeof(double), nk * sizeof(double),
                                    n_nodes, e->stream));
            if (scan_fold(e, e->d_chunk.p, nk, nk, n_nodes, 0, kCombineValues, st.at(k0))) return 1;
            QM_HIP(hipStreamSynchronize(e->stream));
        }
    }
    return fetch_out(e, n_samples, out_on_device, st, user);
}

double qm_exp_correctly_rounded(double x) { return qm::exp_correctly_rounded(x); }

int qm_engine_exp_correctly_rounded(qm_engine *e, const double *x, int64_t n, double *out) {
    if (!e || !x || !out) return fail("qm_engine_exp_correctly_rounded: NULL argument");
    if (n < 1) return 0;
    DeviceGuard guard(e->device);
    // (in and out through two of the locate fits' map-sized buffers: FitScratch says so)
    const double *d_x = stage_in(e, e->fit.a, x, 0, (size_t)n);
    if (!d_x) return 1;
    const StagedOut<double> res = stage_host_out(e->fit.b, out, 0, (size_t)n);
    if (!res.d) return 1;
    hipLaunchKernelGGL(qm::exp_cr_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, d_x, n, res.d);
    QM_HIP(hipGetLastError());
    return res.fetch(e);
}

int qm_engine_kernel_log(qm_engine *e, double *total_ms, int32_t *n_calls) {
    if (!e || !total_ms || !n_calls) return fail("NULL argument");
    DeviceGuard guard(e->device);
    double sum = 0.0;
    for (size_t i = 0; i + 1 < e->ev_used; i += 2) {
        QM_HIP(hipEventSynchronize(e->ev_log[i + 1]));
        float f = 0.f;
        QM_HIP(hipEventElapsedTime(&f, e->ev_log[i], e->ev_log[i + 1]));
        sum += f;
    }
    *total_ms = sum;
    *n_calls = (int32_t)(e->ev_used / 2);
    e->ev_used = 0;
    return 0;
}

int qm_engine_last_kernel_ms(qm_engine *e, double *ms) {
    if (!e || !ms) return fail("NULL argument");
    *ms = -1.0;
    if (!e->timed) return 0;
    DeviceGuard guard(e->device);
    QM_HIP(hipEventSynchronize(e->ev1));
    float f = 0.f;
    QM_HIP(hipEventElapsedTime(&f, e->ev0, e->ev1));
    *ms = f;
    return 0;
}

}  // extern "C"
