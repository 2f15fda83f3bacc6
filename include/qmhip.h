/*
 * qmhip.h -- C ABI of the MI355X (gfx950) coalescence-migration engine.
 *
 * The shared library (quakemigrate_amd/csrc/libqmhip.so, also installed under
 * the reference's own name qmlib<EXT_SUFFIX>) is the drop-in boundary for the
 * hot path of QuakeMigrate: quakemigrate.core's `migrate` + `find_max_coa`.
 * Signatures use plain pointers and sizes only (no torch / HIP types).
 *
 * Part 1 are the five symbols the reference binds at import
 * (quakemigrate/core/lib.py:38-49,128,173,211,249; prototypes
 * quakemigrate/core/src/qmlib.h:28-44, export list qmlib.def:3-7) with
 * identical signatures, so the UNMODIFIED reference front-end runs on this
 * library.  Part 2 is the handle API (resident travel-time table, fused
 * stack + exp + scan that never materialises the 4-D volume) that this
 * repository's own host side (quakemigrate_amd/) drives.  Part 3 is the
 * continuous detect sweep as a pipeline (pinned ring, copies overlapped with
 * compute) -- the loop of QuakeScan._continuous_compute around part 2's call.  Part 4 are engine
 * groups: one process driving the grid on several GPUs (or several parts of one).
 *
 * Conventions: every function of part 2 returns 0 on success, non-zero on
 * failure; qm_last_error() returns a thread-local message.  `*_on_device`
 * flags say whether a pointer is host memory (synchronous, copied internally)
 * or device memory on the engine's GPU (asynchronous on the engine stream).
 * Host buffers may be any memory, pageable included: inputs and results are moved
 * through a pinned buffer of the library's own and copied with the CPU, the
 * caller's pointers are never handed to the HIP runtime.
 * An engine's private stream and its device memory come from process-wide pools
 * and return to them (qm_release_cached_memory()).
 * Layouts are the reference's: onsets f64 [n_rows][T] (already log(clip)),
 * travel-times i32 [nx][ny][nz][n_rows] (C order, flat node = (ix*ny+iy)*nz+iz,
 * quakemigrate/lut/lut.py:165-166), volume f64 [n_nodes][n_samples].
 */
#ifndef QMHIP_H
#define QMHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ part 1 */
/* reference-compatible symbols (host pointers, synchronous, `threads` ignored) */

/* replaces migrate(), quakemigrate/core/src/migratelib.c:40-65 (qmlib.h:28-29).
 * map4d is accumulated INTO (the reference's `+=`), then exp(./available). */
void migrate(double *onsets, int32_t *lookup_tables, double *map4d,
             int32_t fsmp, int32_t lsmp, int32_t n_samples, int32_t n_stations,
             int32_t available, int64_t n_nodes, int64_t threads);

/* replaces find_max_coa(), migratelib.c:85-111 (qmlib.h:31-32). */
void find_max_coa(double *map4d, double *max_coa, double *max_norm_coa,
                  int64_t *max_coa_idx, int32_t n_samples, int64_t n_nodes,
                  int64_t threads);

/* The two symbols above return void, like the reference's.  If one of them fails (no HIP device,
 * a travel time beyond the post-pad, ...) it prints the reason to stderr, fills its outputs with
 * NaN (indices with 0) and leaves a non-zero status here until the next call (text:
 * qm_last_error()); QM_HIP_COMPAT_ON_ERROR=abort in the environment aborts the process instead.
 * The travel-time table is kept resident between calls and re-uploaded only when its content or
 * shape changes.  "Content" = two independent 64-bit hashes of every word (qm_table_hash): a stale
 * table would need both to collide at once; callers who will not accept even that set
 * QM_HIP_COMPAT_REUPLOAD=1 (upload on every call, the reference's cost model).
 * QM_HIP_GRID=nx,ny,nz tells migrate() the grid shape its signature cannot carry (nx*ny*nz must be
 * n_nodes): the table is then bricked in 3-D (8x8x8 where it fits) instead of 1x1x32 along the
 * flat index.  QM_HIP_ASSUME_ZERO_MAP=1 skips the scan of map4d for non-zero content (the
 * reference's binding always passes zeros, lib.py:101). */
int qm_compat_status(void);
/* the two content hashes the drop-in migrate() keys its resident table on (host code) */
void qm_table_hash(const int32_t *table, int64_t n_words, uint64_t *hash_a, uint64_t *hash_b);

typedef struct {
    int n;
    int nsta;
    int nlta;
} stalta_header; /* qmlib.h:34-38, numpy mirror lib.py:33-36 */

/* onsetlib.c:35-59, :79-108, :126-148.  Upstream of the hot path and serial
 * O(n) per trace in the reference; host code here too (must be exported
 * because lib.py binds them at import). */
void overlapping_sta_lta(const double *signal, const stalta_header *head,
                         double *onset);
void centred_sta_lta(const double *signal, const stalta_header *head,
                     double *onset);
void recursive_sta_lta(const double *signal, const stalta_header *head,
                       double *onset);

/* ------------------------------------------------------------------ part 2 */
typedef struct qm_engine qm_engine;

const char *qm_last_error(void);
/* number of HIP devices visible, or -1 */
int qm_device_count(void);
/* What the library was built from: the constants and source digest of the generated shift-reuse loops and
 * the development defines of the kernels' unit ("overlay=none", "defines=none" in the product build;
 * tools/shift_variants.sh makes the others).  bench.py prints it, the GPU suite asserts it. */
const char *qm_build_info(void);
/* Device memory released by engines (destroyed engines, replaced tables) is parked in the process
 * and reused by the next request of its size (up to QM_HIP_POOL_KEEP_MB, default 2 GB, stay parked per device); this returns all of it to
 * the driver.  Always 0. */
int qm_release_cached_memory(void);

int qm_engine_create(int device_id, qm_engine **out);
void qm_engine_destroy(qm_engine *e);

/* run all asynchronous work on this hipStream_t (e.g. torch's current stream; a
 * NULL handle is the device's default stream), or, with use_own != 0, on the
 * engine's private non-blocking stream (the initial state). */
int qm_engine_set_stream(qm_engine *e, void *hip_stream, int use_own);
int qm_engine_synchronize(qm_engine *e);

/* Tunables (qm_engine_config) and read-outs (qm_engine_get).  Nothing has to be set: every default is
 * the automatic choice, every setting gives the same max_coa / max_coa_idx bits
 * and the same stored values unless the row says otherwise.  Layout keys take effect at the next
 * qm_engine_load_lut / qm_engine_serve.  A refused value changes nothing.
 * Every key can be read with qm_engine_get.  It reads back AS SET, except:
 *   brick_x, _y, _z, samples_per_lane   once a table is resident: that table's brick shape and samples per lane
 *   waves, lds_bytes                    as set where the caller set them; else the resident table's layout's
 *                                       (no table: the defaults, 8 and 80 KiB)
 *   shift_waves                         the last launch's layout's, else the resident table's 256-sample layout's,
 *                                       else as set
 *   shift_lazy                          the last launch's flavour (0 before any)
 *   screen_pairs, screen_big            the last screened step's plan (0 before any)
 *
 * key (config)          values [default]         meaning
 * --------------------  -----------------------  -------------------------------------------------------
 * -- precision / rule (opt-in; the only keys that change results) --
 * screen                0 / 1 [0]                1: screened detect (qm_screen.hpp): exact-integer sweep over
 *                                                every node-sample + float64 re-evaluation of every cell that
 *                                                can hold the maximum; max_coa, max_coa_idx identical,
 *                                                max_norm_coa within 6.7e-7 (checked bound, else redone in f64)
 * tie_rule              0 / 1 [0]                0: largest float64 sum, lowest flat index among equal sums;
 *                                                1: the reference's rule on near-ties (csrc/qm_ties.hpp): sums
 *                                                within two ulps of a sample's largest compared on a correctly
 *                                                rounded exp(sum / available), lowest index among equal values
 *                                                (migratelib.c:98-105 as its scalar-libm build computes it);
 *                                                final series of detect / detect_batch (the step axis kept) /
 *                                                migrate / marginal, and sharded detects through
 *                                                qm_engine_tie_partial / _tie_fold; values unchanged.  REFUSED
 *                                                together with screen = 1 by every detect call (detect,
 *                                                detect_batch, detect_partial, the stream): an error naming the
 *                                                two keys, nothing is computed -- the screened detect has no
 *                                                refinement; migrate / marginal of such an engine refine.  Device
 *                                                memory: 8 bytes per brick (512-1024 nodes) and scanned sample
 *                                                besides the partial sets (C3: 227 MB per timestep of a launch)
 * tie_sets              0 / 1 [1]                (measurements) 1: with tie_rule = 1 the shift-reuse fused detect
 *                                                publishes a partial set per brick, the refinement re-stacks one
 *                                                brick per sample; 0: sets of four bricks from more workgroups
 * -- layout of the round-2 kernels (qm_kernels.hpp, qm_pair.hpp) --
 * brick_x, _y, _z       0..64 [0 = automatic]    node-brick shape; automatic = the largest of 8x8x8 .. 1x1x1
 *                                                whose windows fit LDS for >= 99.5 % of the bricks
 * samples_per_lane      0, 1, 2, 4 [0]           time tile = 64 x this; 0 = by table width and scan length
 * waves                 1..16 [by table]         wavefronts per workgroup
 * lds_bytes             1 KiB..160 KiB [by table] window budget per workgroup
 * groups                >= 0 [0 = automatic]     brick groups per time tile (= partial sets)
 * rounds                1..1024 [12; 3 for       grid size of the automatic group count, in rounds over the
 *                       bricks of <= 64 nodes]   resident workgroup slots
 * exact                 0 / 1 [1]                the exact-row-count kernels where one is built
 * pair                  0, 1, 2 [1]              16-byte-operand kernel: 1 = volume-writing launches the
 *                                                shift-reuse kernel does not take, 2 = every launch, 0 = never
 * generic, force_direct 0 / 1 [0]                the any-row-count LDS kernel / the direct (no LDS) kernel
 *                                                for everything: cross-checks
 * scan_waves            1..4096 [32]             find_max_coa of a volume: wavefronts per CU
 * chunk_bytes           >= 1 MiB [4 GiB]         device chunk of a HOST volume (migrate / find_max_coa)
 * -- the shift-reuse kernel (qm_shift.hpp) --
 * shift                 -1, 0, 1 [-1]            -1: where the table qualifies (every 2x2x2 group's delay
 *                                                spread <= 20 samples for >= 99.5 % of the bricks, no grid
 *                                                dimension of 1); 0: never (round-2 kernels); 1: as -1, also
 *                                                on grids one node thick
 * shift_waves           0, 4, 8, 12 [0]          workgroup shape: automatic = two 4-wave workgroups per CU up to
 *                                                ~32 rows, one 8-wave workgroup (all 160 KB) to 64 rows; 12 =
 *                                                running state in LDS (measured no faster)
 * shift_lazy            -1, 0, 1 [-1]            detect loop flavour: lazy arg-max recovery from 160 groups per
 *                                                wavefront on (max_norm_coa within 1e-15 of the eager one)
 * shift_tail            0 / 1 [1]                a scan's remainder of <= 192 samples as ONE tail tile of
 *                                                64 / 128 / 192 samples; 0 = whole 256-sample tiles only
 * shift_wide            -1, 0, 1 [-1]            fused detect on WIDE tiles (384 samples, six per lane, 8-wave
 *                                                workgroups, own brick grid) where the table's windows fit and the
 *                                                scan holds at least one; 0 = the 256-sample tiles of rounds 3-5.
 *                                                max_coa / max_coa_idx bit-equal, max_norm_coa within 1e-14 (the
 *                                                sum over the nodes is formed in another order)
 * shift_wide_rows       0, 1, 2 [1]              wide tiles on ROW BLOCKS (4x4x4 bricks, blocks of <= 20 rows through a
 *                                                double-buffered LDS) where the 384-sample windows of all rows do not
 *                                                fit a CU's LDS (BASELINE configs[3]: 60 rows); 0 = never, 2 = always
 * shift_rows_direct     0, 1, 2 [1]              tables of > 64 rows (row blocks): 1 = blocks of <= 34 rows,
 *                                                double-buffered LDS, LDS-direct loads; 0 = blocks of <= 64
 *                                                through registers; 2 = two 4-wave workgroups per CU
 * -- screened detect's launch shape --
 * screen_pairs          0, 1, 2, 4 [0]           pairs of samples per lane in the sweep
 * screen_big            -1, 0, 1 [-1]            one 16-wave workgroup with 160 KB
 * screen_brick16        0 / 1 [0]                also try 16x8x8 bricks
 * -- the continuous pipeline (part 3) --
 * stream_pull           -1, 0, 1 [-1]            a slot's pinned inputs are PULLED by a small kernel on the engine's
 *                                                stream instead of copied by a command on a second stream: -1 =
 *                                                slots of <= 1 MB (example-sized grids, few steps per launch), 1 =
 *                                                always, 0 = never; same results
 * -- the pre-processing stage --
 * preproc_skew          0 / 1 [1]                the band-pass recurrence with section s on lane s, one sample behind
 *                                                lane s - 1 (critical path T + n_sections); 0 = every section on one
 *                                                lane (T x n_sections): the in-device cross-check; same bits
 * -- measurement --
 * stream_stamps         0 / 1 [0]                qm_stream: a one-thread kernel before and behind every launch stores
 *                                                the GPU's clock; busy time per launch and the gaps between launches
 *                                                go to stderr when the stream is destroyed
 * log_timing            0 / 1 [0]                HIP events around every stacking launch (qm_engine_kernel_log)
 * trigger_timing        0 / 1 [0]                HIP events around every stage of qm_engine_trigger: trigger_ns_* below
 *
 * read-outs (qm_engine_get), besides the keys above: n_cu, n_nodes, n_rows, nx, ny, nz, n_bricks,
 * n_wide_bricks, mean_span; last_kernel (0 chunked, 1 exact-row-count, 2 paired, 3 shift-reuse),
 * last_kernel_j, steps_per_launch (timesteps the last detect_batch put into one launch);
 * shift_ok, shift_brick_nodes, shift_wide_bricks, shift_row_blocks, shift_operands_per_add_x1000,
 * shift_tail_spl; shift_wide_ok, shift_wide_tiles (of the last launch), shift_wide_brick_nodes,
 * shift_wide_direct_bricks, shift_wide_row_blocks, shift_wide_operands_per_add_x1000; pair_brick_nodes, pair_wide_bricks, pair_tile; screened_steps, fallback_steps,
 * last_candidates, screen_brick_nodes; tie_refined_steps, tie_pairs and tie_overflow_samples (of the last
 * refined launch), tie_brick_rows (rows of per-brick maxima the last stacking launch left: 0 = it refined from
 * sets of bricks);
 * The read-outs of a launch -- last_kernel, last_kernel_j, shift_waves, shift_lazy, shift_tail_spl, shift_wide_tiles,
 * tie_brick_rows -- describe the LAST stacking launch, whatever its family: after a launch that is not shift-reuse
 * shift_lazy, shift_tail_spl and shift_wide_tiles are 0 (shift_waves: the resident table's 256-sample layout's),
 * after a launch of the direct kernel alone (force_direct, every brick too wide) last_kernel and last_kernel_j are 0.
 * table_hits, table_misses, table_evictions, tables_parked, table_bytes, tables_parked_bytes, table_digests;
 * pool_live_bytes (the bytes the process's device-memory pool has handed out on this engine's device and not yet got
 * back -- parked or freed; blocks whose release waits for the end of a teardown still count.  Per device and per
 * process, every engine, stream and group on that device included: equal before and after a stretch of work means the
 * stretch gave back all it took; not comparable across the engines of a multi-device group);
 * pick_lds_samples (the longest onset row qm_engine_pick_phases takes: row and selection keys live in LDS);
 * amp_lds_samples (the longest window qm_engine_measure_amplitudes keeps in LDS; longer ones work from scratch);
 * the trigger stage's compile-time tunables (csrc/qm_trigger.hpp): trigger_max_radius (the largest smoothing radius
 * qm_engine_trigger takes), trigger_smooth_tile, trigger_run_block, trigger_merge_stride; with the key
 * trigger_timing set, the last call's
 * stage times in nanoseconds: trigger_ns_smooth, trigger_ns_stats, trigger_ns_runs (count and scan),
 * trigger_ns_compact, trigger_ns_peaks, trigger_ns_merge (0: the stage did not run);
 * the .scanmseed codec's compile-time constants (csrc/qm_scanmseed.hpp): scanmseed_tile (positions per workgroup of
 * the chain kernels), scanmseed_compose_chunk, and the last codec call's stage times in nanoseconds:
 * scanmseed_ns_quantise, scanmseed_ns_scan, scanmseed_ns_compose, scanmseed_ns_pack, scanmseed_ns_frame (encode),
 * scanmseed_ns_decode (0: the stage did not run);
 * the travel-time stage's compile-time constants (csrc/qm_traveltimes.hpp): tt_lds_nodes (the largest section whose
 * tau qm_engine_tt_sections keeps in LDS), tt_section_threads, tt_grid_blocks and tt_grid_threads (the launch grid of
 * the two per-node kernels, which stride over it), tt_plane_threads (a workgroup of qm_engine_tt_eikonal3d's plane
 * launch, one node at most per thread) and tt_plane_max_rows (the most rows it takes in one call), and the last call's
 * launch time in nanoseconds: tt_ns_homogeneous, tt_ns_sections, tt_ns_sweep, tt_ns_eikonal3d (first launch to last,
 * the per-round flag read-backs included). */
int qm_engine_config(qm_engine *e, const char *key, int64_t value);
int qm_engine_get(qm_engine *e, const char *key, int64_t *value);

/* Make a travel-time table resident.  lut: i32 [nx][ny][nz][n_rows].
 * node_offset: flat index of this table's first node inside the full grid
 * (non-zero when the grid is sharded over GPUs by x-planes).  Builds the
 * per-brick window tables on the device.  Replaces the per-call
 * `lookup_tables` argument of migrate() (lib.py:112-123). */
int qm_engine_load_lut(qm_engine *e, const int32_t *lut, int lut_on_device,
                       int32_t nx, int32_t ny, int32_t nz, int32_t n_rows,
                       int64_t node_offset);
/* Several resident tables.  The reference serves a table per timestep from the stations available
 * in it (LUT.serve_traveltimes, quakemigrate/lut/lut.py:502-538; QuakeScan._compute,
 * signal/scan.py:619-634): when a station drops out and comes back, the same few tables alternate.
 * qm_engine_table_select(key) declares which table the following calls work on: the state of the
 * current one (table, brick records, window offsets, the kernels' derived layouts -- about 4x the
 * table's size) is parked under its key, at most `capacity` of them, least recently used evicted,
 * and the state parked under `key` is brought back -- a swap of pointers, no device work.
 * *resident = 1: the table is there, go on; 0: nothing is resident now, load it (qm_engine_load_lut
 * / qm_engine_serve), it is then known under `key`.  The float64 grids of the serving path and all
 * per-step scratch are shared by every table.  capacity = 0 parks nothing (one resident table, as
 * without this call).  qm_engine_get: "table_hits", "table_misses", "table_evictions",
 * "tables_parked", "table_bytes", "tables_parked_bytes". */
int qm_engine_table_select(qm_engine *e, uint64_t key, int32_t capacity, int32_t *resident);

/* On-device table serving -- replaces LUT.serve_traveltimes (quakemigrate/lut/lut.py:502-538)
 * and Grid3D.decimate (lut.py:102-140) on the host.  Upload the float64 travel-time grids (seconds,
 * [nx][ny][nz] each, one per station/phase) once; qm_engine_serve then builds and makes
 * resident the int32 table of the selected grids, rint(tt * sampling_rate) in half-to-even
 * rounding like np.rint, decimated by (dfx, dfy, dfz) exactly like the reference. */
int qm_engine_grids_begin(qm_engine *e, int32_t nx, int32_t ny, int32_t nz, int32_t n_grids);
int qm_engine_grids_set(qm_engine *e, int32_t index, const double *grid, int on_device);
int qm_engine_serve(qm_engine *e, double sampling_rate, const int32_t *rows, int32_t n_rows,
                    int32_t dfx, int32_t dfy, int32_t dfz, int64_t node_offset);
/* copy the resident int32 table ([n_nodes][n_rows]) back to the host (tests, inspection) */
int qm_engine_lut_download(qm_engine *e, int32_t *out);
/* 64-bit digest of the resident int32 table ([n_nodes][n_rows] as qm_engine_lut_download returns it) mixed with
 * nx, ny, nz, n_rows and node_offset; computed on the device, cached per table (a table brought back by
 * qm_engine_table_select is not hashed again; qm_engine_get "table_digests" counts the passes).  With
 * mix = the splitmix64 finalizer and i the flat element index: sum = SUM_i mix(mix(i) + (uint32)v_i) mod 2^64,
 * then digest = sum; digest = mix(digest + f) for f in nx, ny, nz, n_rows, node_offset (as uint64).  One pass
 * over the table; the order of the sum does not matter, so the value is exact and reproducible anywhere.
 * What qm_stream_create_replicas compares. */
int qm_engine_table_digest(qm_engine *e, uint64_t *digest);

/* largest (clamped) delay in the resident table; callers must keep it <= lsmp */
int qm_engine_lut_max(qm_engine *e, int32_t *max_delay);

/* Fused detect step == migrate() + find_max_coa() of QuakeScan._compute
 * (quakemigrate/signal/scan.py:635-638) without the volume, float64 throughout (the screened
 * sweep is opt-in: qm_engine_config "screen"; with device buffers the call never waits on the
 * host).
 * n_nodes_total: node count of the FULL grid (normalisation, migratelib.c:108).
 * Outputs [n_samples]: max_coa f64, max_norm_coa f64, max_coa_idx i64. */
int qm_engine_detect(qm_engine *e, const double *log_onsets, int onsets_on_device,
                     int32_t t_samples, int32_t fsmp, int32_t lsmp,
                     int32_t available, int64_t n_nodes_total, double *max_coa,
                     double *max_norm_coa, int64_t *max_coa_idx,
                     int out_on_device);

/* n_steps consecutive timesteps of the detect sweep in ONE launch: log_onsets f64
 * [n_steps][n_rows][t_samples] (every step with the same table, pads and `available`), outputs
 * [n_steps][n_samples].  What QuakeScan._continuous_compute (quakemigrate/signal/scan.py:407-470)
 * does one timestep at a time; timesteps are independent given their onsets, so a launch can hold
 * several -- which is what fills the GPU on the grids the reference's examples use (1e4-3e5 nodes:
 * one timestep is a fraction of a millisecond of work and a few workgroup rounds).  Every step's
 * result is the bits qm_engine_detect gives for it.  Launches that cannot carry a step axis (the
 * screened detect, tables of more than 64 rows on row blocks) run step by step inside the call;
 * qm_engine_get "steps_per_launch" reports what the last call did. */
int qm_engine_detect_batch(qm_engine *e, const double *log_onsets, int onsets_on_device,
                           int32_t n_steps, int32_t t_samples, int32_t fsmp, int32_t lsmp,
                           int32_t available, int64_t n_nodes_total, double *max_coa,
                           double *max_norm_coa, int64_t *max_coa_idx, int out_on_device);

/* Same step, but stop before the final normalisation: this engine's partial
 * (log2-domain maximum, global node index, sum of coalescence) per sample, on
 * the device, ready for the cross-GPU exchange.  [n_samples] each. */
int qm_engine_detect_partial(qm_engine *e, const double *log_onsets,
                             int onsets_on_device, int32_t t_samples,
                             int32_t fsmp, int32_t lsmp, int32_t available,
                             double *d_part_max, int64_t *d_part_idx,
                             double *d_part_sum);

/* Combine n_sets partials (device, [n_sets][n_samples]) -- e.g. the all-gathered
 * per-GPU partials, in rank order -- into the final series.  Ties go to the
 * lowest node index, as in migratelib.c:102. */
int qm_engine_finalize(qm_engine *e, const double *d_part_max,
                       const int64_t *d_part_idx, const double *d_part_sum,
                       int32_t n_sets, int32_t n_samples, int64_t n_nodes_total,
                       double *max_coa, double *max_norm_coa,
                       int64_t *max_coa_idx, int out_on_device);

/* The same for the packed layout of the cross-GPU exchange: d_packed is f64 [n_sets][3][n_samples]
 * on the device, per set the rows (maxima, indices as int64 bit patterns, sums) -- what one
 * all-gather of every rank's [3][n_samples] partial produces ("one
 * ncclAllGather of a packed [3][ns] buffer + local combine"). */
int qm_engine_finalize_packed(qm_engine *e, const double *d_packed, int32_t n_sets,
                              int32_t n_samples, int64_t n_nodes_total, double *max_coa,
                              double *max_norm_coa, int64_t *max_coa_idx, int out_on_device);

/* "tie_rule" = 1 on a sharded detect -- the reference's arg-max rule on near-ties (migratelib.c:98-105: strict
 * '>' over EXPONENTIATED stacks) across ranks.  After the exchange of the partials:
 * qm_engine_tie_partial examines the partial sets this engine's last qm_engine_detect_partial of the same step
 * left behind against the GRID's largest z per sample (taken from d_packed = the gathered partials, f64
 * [n_sets][3][n_samples] as for qm_engine_finalize_packed) and writes d_tie_packed f64 [2][n_samples] (bit
 * patterns): row 0 the largest correctly rounded exp among its nodes within the slack (0: none), row 1 the
 * lowest GLOBAL node index reaching it -- ready for one more all-gather;
 * qm_engine_tie_fold takes the gathered [n_sets][2][n_samples] and overwrites, in the device series
 * d_max_coa_idx [n_samples], every sample some rank refined: largest exp, lowest index among the ranks reaching
 * it (what the reference's loop over ascending flat indices returns).  Samples nobody refined keep the default
 * rule's index.  Both calls only enqueue.  qm_engine_tie_partial is refused (an error that asks for
 * qm_engine_detect_partial first) unless that detect_partial was the engine's LAST launch: any other stacking
 * launch, qm_engine_find_max_coa, qm_engine_load_lut / _serve or qm_engine_table_select in between overwrites or
 * re-describes the sets it would read. */
int qm_engine_tie_partial(qm_engine *e, const double *log_onsets, int onsets_on_device,
                          int32_t t_samples, int32_t fsmp, int32_t lsmp, int32_t available,
                          const double *d_packed, int32_t n_sets, double *d_tie_packed);
int qm_engine_tie_fold(qm_engine *e, const double *d_tie_gathered, int32_t n_sets, int32_t n_samples,
                       int64_t *d_max_coa_idx);

/* Materialising step (locate): volume f64 [n_nodes_local][n_samples] is written
 * (accumulate != 0: added on top of its current content first, the reference's
 * `+=`), and, if max_coa != NULL, the scan outputs too (same meaning as
 * qm_engine_detect).  map4d may be host or device memory. */
int qm_engine_migrate(qm_engine *e, const double *log_onsets, int onsets_on_device,
                      int32_t t_samples, int32_t fsmp, int32_t lsmp,
                      int32_t available, int64_t n_nodes_total, double *map4d,
                      int map_on_device, int accumulate, double *max_coa,
                      double *max_norm_coa, int64_t *max_coa_idx,
                      int out_on_device);

/* Locate without the volume: the coalescence of every node summed over the scanned samples
 * [first_sample, end_sample) -- what `event.trim2window()` followed by
 * `np.sum(event.map4d, axis=-1)` computes from the 4-D map (quakemigrate/io/event.py:421-439,
 * signal/scan.py:720) -- written as f64 [n_nodes_local]; the scan outputs as in
 * qm_engine_migrate if max_coa != NULL.  Nothing of size n_nodes x n_samples is stored. */
int qm_engine_marginal(qm_engine *e, const double *log_onsets, int onsets_on_device,
                       int32_t t_samples, int32_t fsmp, int32_t lsmp, int32_t available,
                       int64_t n_nodes_total, int32_t first_sample, int32_t end_sample,
                       double *coa_map, int map_on_device, double *max_coa,
                       double *max_norm_coa, int64_t *max_coa_idx, int out_on_device);

/* Locate post-reductions of a marginalised 3-D coalescence map f64 [nx][ny][nz] (the output of
 * qm_engine_marginal), on the device -- QuakeScan._calculate_location's array work
 * (quakemigrate/signal/scan.py:696-733):
 *   - coa_map / nanmax(coa_map)                                       (scan.py:721)
 *   - _gaufilt3d: fftconvolve with util.gaussian_3d(nx, ny, nz, sgm), mode "same", twice, the
 *     second time mirrored, each normalised by its maximum           (scan.py:1008-1043,
 *     util.py:76-116), evaluated as a separable direct convolution
 *   - _covfit3d: weights = map where map > cov_thresh; expectation and 3x3 covariance of the
 *     node positions ix*node_spacing[0], ...                          (scan.py:939-1005)
 *   - the 7x7x7 window of the smoothed map around its maximum that _gaufit3d fits and the
 *     5x5x5 window of the normalised map that _splineloc interpolates (scan.py:736-936);
 *     nodes outside the grid are NaN.  The 10-parameter least squares / RBF solves on those
 *     few hundred values stay with the caller.
 * norm_map / smoothed_map: optional f64 [nx*ny*nz] outputs (host or device per out_on_device).
 * summary (host, 16 doubles): 0 nanmax of the input; 1 flat index of the first maximum of the
 * normalised map; 2 mean of the smoothed map; 3 flat index of the first maximum of the
 * smoothed map; 4 total weight; 5-7 expectation (xe, ye, ze); 8-13 covariance xx, yy, zz, xy,
 * xz, yz; 14, 15 the maxima the two smoothing passes were normalised by.
 * gau_window: host f64 [343]; spline_window: host f64 [125]. */
int qm_engine_locate_fits(qm_engine *e, const double *coa_map, int map_on_device, int32_t nx,
                          int32_t ny, int32_t nz, double sgm, double cov_thresh,
                          const double *node_spacing, double *norm_map, double *smoothed_map,
                          int out_on_device, double *summary, double *gau_window,
                          double *spline_window);

/* _splineloc's refinement (quakemigrate/signal/scan.py:777-812): the cubic radial-basis
 * interpolant through an n x n x n window -- scipy.interpolate.Rbf(x, y, z, values,
 * function="cubic") with the reference's "xy" meshgrid pairing -- evaluated on the device on the
 * `upscale`-times finer grid of ((n-1)*upscale + 1)^3 points, and its first maximum.
 * weights: host f64 [n][n][n], the solution of  |c_i - c_j|^3 w = values  (a 125 x 125 solve for
 * the reference's 5^3 window: left to the caller's LAPACK).  peak_index: flat C-order index
 * (i*m + j)*m + k into the fine grid, m = (n-1)*upscale + 1 -- what
 * np.unravel_index(np.nanargmax(dense), dense.shape) receives in scan.py:806-808. */
int qm_engine_rbf_peak(qm_engine *e, const double *weights, int32_t n, int32_t upscale,
                       double *peak_value, int64_t *peak_index);

/* Onset stage on the device -- the step immediately upstream of the path:
 * STALTAOnset._onset (quakemigrate/signal/onsets/stalta.py:491-548: signal transform, STA/LTA
 * per component trace with the arithmetic of core/src/onsetlib.c, taper windows :550-583,
 * root-mean-square over the components, clip at min_onset_value) and then lib.migrate's
 * log(clip(., 0.01)) (core/lib.py:93-94).
 *   signals    f64 [n_traces][t_samples], pre-processed (filtered / resampled) waveforms
 *   trace_row  [n_traces] onset row each trace feeds (the components of one station/phase)
 *   nsta/nlta  [n_rows] window lengths in samples;  transform 0 = energy (x*x), 1 = abs.
 *              The reference's "env" / "env_squared" (stalta.py:518-521) are abs / energy of the
 *              envelope |hilbert(x)|: the Hilbert transform is an upstream signal transform like
 *              the band-pass filters and stays with the caller (the Python binding applies
 *              scipy.signal.hilbert, the reference's own call, to host signals).
 *   position   0 = classic / overlapping (onsetlib.c:35-59), 1 = centred (:79-108),
 *              2 = recursive (:126-148; exported by the reference's lib, not used by
 *              STALTAOnset);  taper_pad < 0 = no taper windows
 *   raw_onsets (optional) and log_onsets: f64 [n_rows][t_samples]; log_onsets is what
 *   qm_engine_detect takes (pass it with onsets_on_device = 1 to keep everything on the GPU). */
int qm_engine_onsets(qm_engine *e, const double *signals, int signals_on_device,
                     int32_t n_traces, int32_t t_samples, const int32_t *trace_row,
                     int32_t n_rows, const int32_t *nsta, const int32_t *nlta, int transform,
                     int position, int32_t taper_pad, double min_onset_value,
                     double *raw_onsets, double *log_onsets, int out_on_device);

/* Pre-processing on the device -- the step upstream of the onset stage: what STALTAOnset.calculate_onsets does to
 * every component trace before the STA/LTA (stalta.py:137-211, :353-489) for gap-free traces of the full timespan
 * (the reference's default, full_timespan = True, allow_gaps = False; gappy traces: qm_engine_preprocess_segments
 * below, resampling: qm_engine_resample; the envelope transforms stay with the caller).  Per trace, one workgroup:
 *   1. detrend = 1: the least-squares line over t = 0..T-1 is subtracted in its centred form,
 *      y = x - (mean(x) + slope (t - mean(t))), slope = sum (t - mean t)(x - mean x) / sum (t - mean t)^2,
 *      then the mean of y (the reference detrends "linear", then "constant").  The sums are fixed-order
 *      reductions: the same bits in every run.
 *   2. y[k] *= taper_left[k] (k < n_left), y[T - n_right + k] *= taper_right[k] (k < n_right): the weights are the
 *      caller's (a 5 % cosine taper in the reference); either length may be 0.
 *   3. the cascade of n_sections second-order sections sos[trace_filter[i]] ([n_filters][n_sections][6] as SciPy
 *      lays them out: b0 b1 b2 a0 a1 a2, a0 == 1), direct form II transposed from a zero state, in the operation
 *      order of scipy.signal.sosfilt and without contraction: its bits.  zero_phase = 1: the same filter again over
 *      the reversed result, reversed back (the reference's zerophase band-pass).
 * signals / filtered: f64 [n_traces][t_samples], host or device (filtered may be signals on the device).
 * Refused: n_sections outside 1..8, a trace_filter entry outside [0, n_filters), n_left + n_right > t_samples,
 * a section whose a0 is not 1. */
int qm_engine_preprocess(qm_engine *e, const double *signals, int signals_on_device, int32_t n_traces,
                         int32_t t_samples, const int32_t *trace_filter, const double *sos, int32_t n_filters,
                         int32_t n_sections, int detrend, const double *taper_left, int32_t n_left,
                         const double *taper_right, int32_t n_right, int zero_phase, double *filtered,
                         int out_on_device);

/* Pre-processing of GAPPY traces on the device -- what STALTAOnset.calculate_onsets does with allow_gaps = True or
 * full_timespan = False (stalta.py:137-211, :442-461): every trace SEGMENT is detrended, tapered and filtered on its
 * own, a second taper takes the filter's transients off each segment, and the gaps and the window's ends are filled
 * with sqrt(finfo(float).tiny) before the STA/LTA runs over the full-length trace.  signals / filtered: f64
 * [n_traces][t_samples] in window layout, host or device (filtered may be signals on the device); a segment is samples
 * [first, first + n) of its trace's row, and samples outside every segment are never read.  The caller plans the work
 * (Python: quakemigrate_amd.preprocess.plan_segments): records [n_segments][8] int64, per segment
 *    0 trace                 its row
 *    1 first, 2 n            its samples, n >= 1
 *    3 fill_before           filtered[first - fill_before .. first) = fill_value
 *    4 fill_after            filtered[first + n .. first + n + fill_after) = fill_value
 *    5 w_offset, 6 m         its taper: w = taper_weights + w_offset, w[0 .. m) the weights of the first m samples,
 *                            w[m .. 2 m) of the last m
 *    7                       0
 * Per record, one workgroup -- the segments of a trace are conditioned in parallel, no workgroup waits on another --
 * with y = x[first .. first + n):
 *   1. detrend = 1: qm_engine_preprocess' step 1 over y (the same fixed-order sums; slope 0 where n == 1).
 *   2. y[k] *= w[k], y[n - m + k] *= w[m + k] for k < m.
 *   3. the cascade sos[trace_filter[trace]] over y, forward and with zero_phase = 1 backward as well:
 *      scipy.signal.sosfilt's bits, as in qm_engine_preprocess; "preproc_skew" = 0 selects the plain form here too.
 *   4. second_taper = 1: step 2 again with the same weights (the reference calls taper(type="cosine",
 *      max_percentage=0.05) twice on traces of one length).
 *   5. filtered[first .. first + n) = y, then the record's two fills.
 * y lives in LDS up to 20 480 samples, else in place in its output row: the same bits.  With one record per trace,
 * n = t_samples, no fill and second_taper = 0 the result is qm_engine_preprocess' of the same weights, bit for bit.
 * Refused, with the output untouched: what qm_engine_preprocess refuses, n_segments < 1, a record whose trace is out
 * of range, n < 1, a negative fill, a range [first - fill_before, first + n + fill_after) that leaves [0, t_samples),
 * weights that leave taper_weights, 2 m > n, field 7 non-zero, a fill_value that is not finite, and a trace whose
 * records' ranges do not tile [0, t_samples) exactly once (an overlap, a hole, a trace without a record).
 * qm_engine_last_kernel_ms reports the launch. */
int qm_engine_preprocess_segments(qm_engine *e, const double *signals, int signals_on_device, int32_t n_traces,
                                  int32_t t_samples, const int32_t *trace_filter, const double *sos,
                                  int32_t n_filters, int32_t n_sections, int detrend, int zero_phase,
                                  const int64_t *records, int32_t n_segments, const double *taper_weights,
                                  int64_t n_taper_weights, int second_taper, double fill_value, double *filtered,
                                  int out_on_device);

/* Resampling on the device -- the step upstream of the pre-processing: what util.resample does to every raw trace of
 * a timestep (quakemigrate/util.py:404-604): upsampling by linear interpolation with constant pads at the window's
 * ends, decimation behind a detrend, a taper and a zero-phase low-pass, the trims to the window.  Raw traces go in,
 * each at its own rate and length, packed into one buffer of int32 (raw_dtype 0, as miniSEED holds them; converted
 * exactly) or float64 (raw_dtype 1) samples, host or device; out: f64 [n_traces][t_samples], host or device, what
 * qm_engine_preprocess takes.  The caller plans the work (Python: quakemigrate_amd.preprocess.ResampleStage):
 * records [n_traces][11] int64, per trace
 *    0 raw_offset, 1 n_raw   its samples x[0..n_raw) in the raw buffer (elements), n_raw >= 1
 *    2 up                    u >= 1
 *    3 pad_left, 4 pad_right copies of x[0] in front of / of x[n_raw - 1] behind the upsampled series (0 with u == 1)
 *    5 up_first, 6 n_up      the slice of the padded series that is kept (the reference's trim)
 *    7 dec                   d >= 1
 *    8 lowpass               d > 1: its low-pass, an index into sos_lp [n_lowpass][n_sections_lp][6] (SciPy's layout,
 *                            a0 == 1)
 *    9 taper                 d > 1: its taper, an index into taper_table [n_tapers][2] = (offset, m): the weights
 *                            taper_weights[offset .. offset + m) of the first m samples, then [offset + m .. offset + 2 m)
 *                            of the last m
 *   10 out_first             first decimated sample of the output row
 * Per trace, one workgroup:
 *   1. upsample: the series of (n_raw - 1) u + 1 samples with sample j u = x[j] and sample j u + i, 0 < i < u,
 *      = (double(i) / u) x[j + 1] + (double(u - i) / u) x[j] -- two quotients, two products, one sum, no contraction:
 *      NumPy's bits for the reference's expression -- then the pads; K = samples [up_first, up_first + n_up) of it.
 *   2. d > 1: detrend = 1: qm_engine_preprocess' step 1 over K (the same fixed-order sums); K[k] *= w[k],
 *      K[n_up - m + k] *= w[m + k] for k < m with w the taper's weights; the cascade of the low-pass forward, then over
 *      the reversed result, reversed back: scipy.signal.sosfilt's bits, as in qm_engine_preprocess; then D[k] = K[k d]
 *      for k < ceil(n_up / d) (obspy's decimate without its own filter, data[::d]).  d == 1: D = K, nothing else runs.
 *   3. out[i][0 .. t_samples) = D[out_first .. out_first + t_samples).
 * K lives in LDS up to 20 480 samples, else in engine scratch: the same bits.  "preproc_skew" = 0 selects the plain
 * filter form here too.
 * Refused, with the output untouched: a NULL argument (sos_lp, taper_table, taper_weights may be NULL where their
 * count is 0), a raw_dtype other than 0 / 1, n_traces < 1, t_samples < 1, n_raw < 1, raw samples outside
 * [0, total_raw_samples), up < 1, dec < 1, a pad with up == 1 or below 0, a kept slice that leaves the padded series,
 * out_first + t_samples > ceil(n_up / d), n_sections_lp outside 1..8, a section whose a0 is not 1, a taper that
 * leaves taper_weights, and for d > 1 a lowpass or taper index out of range or 2 m > n_up.
 * qm_engine_last_kernel_ms reports the launch. */
int qm_engine_resample(qm_engine *e, const void *raw, int raw_dtype, int raw_on_device, int64_t total_raw_samples,
                       int32_t n_traces, const int64_t *records, const double *sos_lp, int32_t n_lowpass,
                       int32_t n_sections_lp, int detrend, const int32_t *taper_table, int32_t n_tapers,
                       const double *taper_weights, int64_t n_taper_weights, int32_t t_samples, double *out,
                       int out_on_device);

/* Phase picks on the device -- the step after the location: what GaussianPicker.pick_phases does to every onset row
 * (one station x phase) of a located event (quakemigrate/signal/pickers/gaussian.py:319-560).  One launch, one
 * workgroup per row; onsets: f64 [n_rows][t_samples], the UN-LOGGED onset functions (qm_engine_onsets' raw_onsets
 * with the taper windows set to 1), host or device; every other array is a host array.  Per row:
 *   1. noise set: the samples that lie in no window [lo, hi) of any row with the same row_group (the phases of one
 *      station mask each other, gaussian.py:341-343) and whose value is > 1 (the taper pads are 1).
 *   2. threshold_mode 0: med = median(noise), mad = 1.4826 median(|noise - med|), threshold = med + mad *
 *      mad_multiplier -- exact selection, NumPy's operation order, no contraction: NumPy's bits; an empty noise set
 *      gives NaN and no pick.  threshold_mode 1: thresholds_in[row] as given (the percentile method, by the caller).
 *   3. peak (_find_peak): the FIRST maximum of [lo, hi) and the maximal run of consecutive samples > threshold
 *      around it; the fit range [f0, f1) is the run padded by one sample on each side.
 *   4. fit of a exp(-(x - b)^2 / (2 c^2)) to (k / sampling_rate, onsets[k]), k in [f0, f1), from p0 = [max y,
 *      (f0 + argmax y) / rate, halfwidth[row] / rate] (halfwidth in samples): Levenberg-Marquardt on the 3x3 normal
 *      equations, analytic Jacobian, damping mu D^2 with D the running maximum of the Jacobian's column norms, a step
 *      accepted when the gain ratio rho exceeds 1e-4, mu *= max(1/3, 1 - (2 rho - 1)^3) then, mu *= nu, nu *= 2
 *      otherwise (mu = 1e-3, nu = 2 at the start), until every |dp_i| <= 1e-13 (|p_i| + 1e-13), at most 200
 *      iterations.  All sums are fixed-order reductions: a call gives the same bits every time.
 *   5. the pick stands if lo < b sampling_rate < hi (strict, gaussian.py:459).
 * picks [n_rows][8]: 0 threshold, 1 a (SNR), 2 b (s from the row's first sample), 3 |c| (pick error, s),
 * 4 c as fitted, 5 f0, 6 f1, 7 iterations.  Columns 1-4 are -1 unless status == 0; 5-6 are -1 for status 1, 2, 6.
 * status [n_rows]: 0 picked, 1 nothing above the threshold, 2 peak of one sample, 3 fit range leaves the trace
 * (the reference makes no pick there either: it fails at the trace's start and curve_fit refuses the ragged arrays
 * at its end), 4 not converged, 5 mean outside the window, 6 non-finite input (threshold NaN; a deviation: the
 * reference's result there is an accident of np.argmax on NaN).
 * Rows of several events may share a call: row_group distinct per event and station.
 * Refused, with the outputs untouched: a NULL argument, n_rows < 1, t_samples < 1 or above "pick_lds_samples", a
 * window with lo < 0, hi > t_samples or lo > hi, sampling_rate <= 0, a threshold_mode other than 0 / 1,
 * threshold_mode 1 without thresholds_in.  qm_engine_last_kernel_ms reports the launch. */
int qm_engine_pick_phases(qm_engine *e, const double *onsets, int onsets_on_device, int32_t n_rows,
                          int32_t t_samples, const int32_t *windows /*[n_rows][3]: lo, arrival, hi*/,
                          const int32_t *row_group, double sampling_rate, const double *halfwidth,
                          int threshold_mode, double mad_multiplier, const double *thresholds_in,
                          double *picks, int32_t *status);

/* Local-magnitude amplitudes on the device -- the step after the picks: what Amplitude.get_amplitudes does to every
 * component trace of a located event (quakemigrate/signal/local_mag/amplitude.py:174-371; the rules on arrays:
 * tests/amplitudes_ref.py).  Wood-Anderson displacement traces go in (response removal stays with the caller), each at
 * its own rate and length, packed into one buffer of float64 samples, host or device; every other array is a host
 * array.  Two launches.
 *   trace_records  [n_traces][4] int64: 0 offset, 1 n -- its samples x[0..n) in the buffer (elements), n >= 1;
 *                  2 filter: an index into sos [n_filters][n_sections][6] (SciPy's layout, a0 == 1), -1: none;
 *                  3 taper: an index into taper_table [n_tapers][2] = (offset, m) laid out as qm_engine_resample's,
 *                  -1: none (read only where the trace has a filter).  Traces may share samples only where neither
 *                  of them has a filter (stage A filters in place in the engine's working copy).
 *   window_records [n_windows][4] int64: 0 trace, 1 lo, 2 hi -- samples [lo, hi) of that trace; 3 kind: 0 noise,
 *                  1 signal.  Records are independent: the rows of several events may share a call.
 * Stage A, per trace whose filter is >= 0, one workgroup (_filter_trace, amplitude.py:413-539):
 *   1. the least-squares line over t = 0..n-1 subtracted in the centred form of qm_engine_preprocess' step 1, the
 *      LINE ONLY (the reference calls detrend("linear") alone, :478, :529); the same fixed-order sums.
 *   2. x[k] *= w[k], x[n - m + k] *= w[m + k] for k < m with w the taper's weights.
 *   3. ONE forward pass of the cascade from a zero state (zerophase=False): scipy.signal.sosfilt's bits, as in
 *      qm_engine_preprocess.  "preproc_skew" = 0 selects the plain filter form here too.
 *   The trace lives in LDS up to 20 480 samples, else in the engine's working copy: the same bits.  Traces without a
 *   filter are measured as given.  filtered_out (optional, f64 [total_samples], host): every trace as stage B saw it.
 * Stage B, per window record, one wavefront, y = samples [lo, hi) of the record's trace:
 *   1. hi == lo: status 1.  A non-finite sample: status 5.
 *   2. kind 0 (noise, :954-962): max(y) == min(y): status 1 -- tested BEFORE the detrend; then the detrend and the
 *      average.  kind 1 (signal, :763-817): the detrend first, then max(y) == min(y) on the detrended samples: status 1.
 *   3. the detrend (detrend_windows = 1): y[i] = x[i] - (mean + slope (i - tbar)), tbar = (n - 1) / 2, slope =
 *      sum (i - tbar)(x[i] - mean) / sum (i - tbar)^2 (0 where n == 1), three fixed-order sums, no second demean.
 *      detrend_windows = 0: the window is measured as it is.
 *   4. the average: average_method 0 RMS sqrt(mean(y^2)), 1 STD sqrt(mean(|y - mean(y)|^2)), fixed-order sums; and
 *      max|y|.
 *   5. kind 1: peaks as scipy.signal.find_peaks gives them (_local_maxima_1d): a sample, or a plateau of equal
 *      samples, strictly above both neighbours counts once, at (left + right) / 2 rounded down; a window's first and
 *      last sample are never peaks.  Troughs: the same on -y.
 *   6. prominence_multiplier > 0: a peak stays if its prominence is >= prominence_multiplier * max|y|
 *      (_peak_prominences without wlen: to each side walk from the peak until a sample HIGHER than it or the window's
 *      end, take the minimum over each walk; the prominence is the peak minus the larger of the two minima); troughs
 *      the same on -y.  With the multiplier 0 nothing is computed.
 *   7. pairing (:862-901, in its order), P peaks and T troughs in sample order: P == 0 or T == 0: status 2.
 *      P == T == 1: full = |y[p0] - y[t0]|; full == 0: status 4.  P == T: (a, b) = (peaks, troughs) and, where
 *      p0 < t0, (c, d) = (peaks[1:], troughs[:-1]), else (peaks[:-1], troughs[1:]).  |P - T| != 1: status 3.
 *      P > T: p0 < t0 or status 3; (a, b, c, d) = (peaks[:-1], troughs, peaks[1:], troughs).  P < T: p0 > t0 or status
 *      3; (a, b, c, d) = (peaks, troughs[1:], peaks, troughs[:-1]).  fp1 = |y[a] - y[b]|, fp2 = |y[c] - y[d]|;
 *      max fp1 >= max fp2: the FIRST argmax of fp1 gives the pair, else the first argmax of fp2.
 * values [n_windows][4] f64: 0 full peak-to-trough |y[p] - y[t]| (input units; 0 without a measurement), 1 the average
 * (input units), 2 max|y|, 3 reserved: 0.  Columns 1 and 2 are written for status 0, 2, 3, 4 (the caller applies the
 * reference's `continue`), 0 for status 1 and 5.
 * index [n_windows][4] i32: 0 status, 1 peak sample, 2 trough sample (both counted from the trace's first sample, -1
 * without a measurement), 3 peaks kept (0 for kind 0).
 * status: 0 measured; 1 empty or flat; 2 no peak or no trough; 3 "consecutive peaks/troughs", both of the reference's
 * cases; 4 one peak and one trough of equal value (a DEVIATION: the reference's `if not full_amp` falls through to
 * unbound names there and raises UnboundLocalError.  It cannot occur on finite samples: between such a peak and
 * trough, say the peak first, the samples fall below their common value v and rise above it again, so the highest
 * of them, M > v, is a peak; both of its prominence walks pass samples <= v, so its prominence is >= M - v, while the
 * trough's left walk meets nothing above M and its prominence is <= M - v: the peak at M is kept whenever the trough
 * is, and there are two peaks.  The status is a guard); 5 a non-finite sample in the window (a DEVIATION: the reference's
 * result there is an accident of comparisons with NaN).
 * A window keeps its samples and its extremum lists in LDS up to "amp_lds_samples" samples (qm_engine_get), above
 * that in engine scratch: the same results.  All reductions and the ordered compaction of the extrema are fixed-order
 * (lane-strided sums, ballots and prefix counts, no atomics): a call gives the same bits every time.
 * Not here: the envelope average (noise_measure "ENV": scipy.signal.hilbert stays with the caller, as for the "env"
 * onset transforms, see qm_engine_onsets), the units, frequencies, times and the filter gain (quakemigrate_amd/
 * amplitudes.py).
 * Refused, with the outputs untouched: a NULL argument (sos, taper_table, taper_weights may be NULL where their count
 * is 0; filtered_out is optional), n_traces < 1, n_windows < 1, total_samples < 1, a trace with n < 1 or that leaves
 * the buffer, a window whose trace is out of range, that leaves its trace or has lo > hi, a kind other than 0 / 1, an
 * average_method or detrend_windows other than 0 / 1, a negative or non-finite prominence_multiplier, n_sections
 * outside 1..8, a section whose a0 is not 1, a filter or taper index out of range (below -1 included), a taper that
 * leaves taper_weights, a filtered trace whose taper has 2 m > n, a filtered trace that shares samples with another
 * trace.  qm_engine_last_kernel_ms reports the two launches. */
int qm_engine_measure_amplitudes(qm_engine *e, const double *traces, int traces_on_device, int64_t total_samples,
                                 int32_t n_traces, const int64_t *trace_records, const double *sos, int32_t n_filters,
                                 int32_t n_sections, const int32_t *taper_table, int32_t n_tapers,
                                 const double *taper_weights, int64_t n_taper_weights, int32_t n_windows,
                                 const int64_t *window_records, int detrend_windows, int average_method,
                                 double prominence_multiplier, double *values /*[n_windows][4]*/,
                                 int32_t *index /*[n_windows][4]*/, double *filtered_out);

/* Travel-time tables on the device -- the float64 grids in seconds that qm_engine_grids_set and qm_engine_serve work
 * from, computed where they live: the reference's compute_traveltimes (quakemigrate/lut/create_lut.py) for the two
 * methods that need no external program.  The rules on arrays: tests/traveltimes_ref.py; the kernels and what bounds
 * them: csrc/qm_traveltimes.hpp.  All arithmetic is float64 without contraction, IEEE divide and square root: every
 * output has the bits of the NumPy restatement.  A grid is ll_corner [3], node_spacing [3] (> 0), node_count [3]; node
 * (ix, iy, iz) lies at ll_corner[j] + index * node_spacing[j] (Grid3D.grid_xyz) and is element (ix ny + iy) nz + iz
 * of its row.  Units are the caller's: one unit of length throughout, seconds per that unit.  Parameter arrays are
 * host arrays; out_on_device says where the outputs are.  Every call synchronises and leaves its launch's time in
 * "tt_ns_homogeneous" / "tt_ns_sections" / "tt_ns_sweep" / "tt_ns_eikonal3d" (qm_engine_get, nanoseconds) and
 * qm_engine_last_kernel_ms.
 *
 * qm_engine_tt_homogeneous (create_lut.py:241-265): row_params [n_rows][4] = station x, y, z, velocity; out
 * [n_rows][nodes] = sqrt(dx dx + dy dy + dz dz) / v, the sum taken left to right.
 *
 * qm_engine_tt_sections: |grad T| = s(z) on n_sections (distance, depth) sections of nr x nz nodes of spacing h, node
 * (i, k) at distance i h and depth k h below the section's first row, element i nz + k.  slowness [n_sections][nz]:
 * per depth row; source [n_sections][2]: the source's depth zs below the first row -- the source sits in column 0 --
 * and the slowness s0 there.  The scheme is the multiplicatively factored first-order upwind one, T = T0 tau with
 * T0 = s0 rho, rho = sqrt(x x + z z) from the source: a node takes the smallest candidate over its available
 * neighbours (finite tau) -- per horizontal neighbour (i - sx, k), sx = +-1, ax = T0 sx / h + T0x, bx = T0 sx tau_a / h,
 * the same in z; the two-sided candidate is the larger root of (ax tau - bx)^2 + (az tau - bz)^2 = s[k]^2, kept where
 * sx (ax tau - bx) >= 0 and sz (az tau - bz) >= 0 (the only causality tests); the one-sided ones are
 * (bx + sx s[k]) / ax where sx ax > 0 and the result is > 0 -- and only where that is below its value by more than
 * tol times the value (tol = 2^-40 stops the creep in the last bits; 0: strict).  Columns 0 and 1 of the two rows
 * that bracket zs (floor(zs / h) and the next) are frozen at tau = (s0 + s[k]) / (2 s0), the node at the source at
 * tau = 1.  Gauss-Seidel sweeps in the orderings (+,+) (-,+) (-,-) (+,-) of (i, k) make a round; rounds repeat until
 * one accepts nothing.  One workgroup per section runs every anti-diagonal of a sweep in parallel, which reads what
 * the serial i-outer / k-inner loop reads: the values are that loop's.  tau lives in LDS up to "tt_lds_nodes" nodes
 * (qm_engine_get), above that -- or with force_scratch = 1 -- in engine scratch: the same bits.  T [n_sections][nr][nz]
 * f64, rounds [n_sections] i32 (rounds run, the last, idle one included), status [n_sections] i32 (0 settled, 1 not
 * settled in max_iters rounds), all three on the side out_on_device says.  Refused: a NULL argument, n_sections < 1,
 * nr or nz < 2, h or a slowness not finite and > 0 (the section and row are named), a source outside the section's
 * rows or in its last row's cell below (named), tol outside [0, 1), max_iters < 1; and, with the outputs written, a
 * section that max_iters rounds did not settle (named).
 *
 * qm_engine_tt_sweep (create_lut.py:471-474, 504-513, 746-762): row_params [n_rows][4] = station x, y, the origin x0,
 * z0 of the row's section; row_section [n_rows]: which of the n_sections sections [n_sections][nr][nz] (host or
 * device: a caller's own, NonLinLoc's for instance, or qm_engine_tt_sections') the row is swept from.  Per node
 * d = sqrt(dx dx + dy dy), z, and then _bilinear_interpolate literally: i, k = floor((d - x0) / h), floor((z - z0) / h);
 * fractions np.remainder(d, h) / h and np.remainder(z, h) / h -- of the coordinates, not of the offsets from the origin:
 * the reference's rule, which names the cell of the floor only where x0 and z0 are multiples of h --; c0 = c00 (1 - xd)
 * + c10 xd, c1 = c01 (1 - xd) + c11 xd, c0 (1 - zd) + c1 zd.  out [n_rows][nodes].  Refused besides the arguments: a
 * node whose four corners are not all inside its section -- NumPy would raise, or wrap a negative index --, with the
 * row and its first such node named; the other nodes of out are written, such nodes hold NaN.
 *
 * qm_engine_tt_eikonal3d: |grad T| = s(x, y, z) on the grid's own nodes, one solve per row -- what the reference
 * leaves to scikit-fmm (1dfmm) and NonLinLoc (3-D models); the rules on arrays: tests/traveltimes3d_ref.py.
 * row_params [n_rows][4] = source x, y, z and the slowness s0 at the source; row_model [n_rows]: which of the n_models
 * volumes slowness [n_models][nodes] (host or device) the row is solved in.  The scheme is qm_engine_tt_sections' with
 * one axis more: T = T0 tau, T0 = s0 rho, rho = sqrt(dx dx + dy dy + dz dz) from the source, d = (ll + index spacing)
 * - source per axis.  Per axis d and side sg = +1 (the neighbour at index - 1), -1 (at index + 1): a = T0 sg / h_d +
 * dT0/dd, b = T0 sg tau_nb / h_d.  A node takes the smallest candidate over its available neighbours (finite tau), one
 * neighbour at most per axis, in this order: the 6 one-sided ones (b + sg s) / a, kept where sg a > 0 and the result
 * is > 0, axis x side +1, x side -1, y, z; the 12 two-sided ones, axes (x, y), (x, z), (y, z), sides (+,+) (+,-)
 * (-,+) (-,-), the larger root of sum (a tau - b)^2 = s^2 -- qa = sum a a, qb = sum a b, qc = sum b b - s s, every sum
 * left to right, (qb + sqrt(qb qb - qa qc)) / qa -- kept where the discriminant is >= 0 and sg (a tau - b) >= 0 on both
 * axes; the 8 three-sided ones, the same with three terms, sides of x outermost -- and only where that is below its
 * value by more than tol times the value.  The eight nodes of the cell that holds the source (per axis
 * floor((src - ll) / h), clipped to n - 2) are frozen at tau = (s0 + s_node) / (2 s0), a node at the source at 1; out
 * is T0 tau, 0 where T0 = 0.  Gauss-Seidel sweeps in the eight orderings itertools.product((+1, -1), repeat=3) of
 * (x, y, z) make a round; rounds repeat until one accepts nothing in the row.  One launch per plane i' + j' + k' = d
 * of a sweep (indices counted from the far end of an axis the ordering runs backwards), all rows in it: a node's six
 * neighbours lie in the planes d - 1 and d + 1, so the plane at once reads what the serial x-outer / z-inner loop
 * reads, and the values are that loop's.  8 (nx + ny + nz - 2) launches per round, then the host reads the rows'
 * "accepted something" flags: the one synchronisation per round.  out [n_rows][nodes] f64 on the side out_on_device
 * says; rounds, status [n_rows] i32, HOST arrays: a row's rounds run (the last, idle one included; a settled row's
 * further rounds, run for the others, change nothing and are not counted), 0 settled / 1 not settled in max_iters.
 * Deviations from the reference's _eikonal_fmm: first order, not scikit-fmm's second-order march -- the values differ
 * by the schemes' discretisation errors --; the source is the station's true position, not the nearest node.
 * Refused, by name: a NULL argument, an axis shorter than 2 nodes, more than "tt_plane_max_rows" rows, a source
 * outside [ll, ur], s0 or a slowness not finite and > 0 (model and node named, host or device input alike),
 * row_model outside [0, n_models), tol outside [0, 1), max_iters < 1; and, with the outputs written, a row that
 * max_iters rounds did not settle ("row R: not settled after N rounds"). */
int qm_engine_tt_homogeneous(qm_engine *e, const double *ll_corner, const double *node_spacing,
                             const int32_t *node_count, int32_t n_rows, const double *row_params /*[n_rows][4]*/,
                             double *out, int out_on_device);
int qm_engine_tt_sections(qm_engine *e, int32_t n_sections, int32_t nr, int32_t nz, double h,
                          const double *slowness /*[n_sections][nz]*/, const double *source /*[n_sections][2]*/,
                          double tol, int32_t max_iters, int force_scratch, double *T, int32_t *rounds,
                          int32_t *status, int out_on_device);
int qm_engine_tt_sweep(qm_engine *e, const double *ll_corner, const double *node_spacing, const int32_t *node_count,
                       int32_t n_rows, const double *row_params /*[n_rows][4]*/, const int32_t *row_section,
                       const double *sections, int sections_on_device, int32_t n_sections, int32_t nr, int32_t nz,
                       double h, double *out, int out_on_device);
int qm_engine_tt_eikonal3d(qm_engine *e, const double *ll_corner, const double *node_spacing, const int32_t *node_count,
                           int32_t n_rows, const double *row_params /*[n_rows][4]*/, const int32_t *row_model,
                           int32_t n_models, const double *slowness /*[n_models][nodes]*/, int slowness_on_device,
                           double tol, int32_t max_iters, double *out, int out_on_device, int32_t *rounds,
                           int32_t *status);

/* Trigger on the device -- the step between the detect sweep and the location: what Trigger._trigger_batch does to
 * the coalescence series of a batch (quakemigrate/signal/trigger.py:318-638; the rules on arrays:
 * tests/trigger_ref.py).  coa, coa_n: f64 [n], host arrays, uniformly sampled, already cut to the batch and its pads.
 * All times are int64 nanoseconds from the first sample, t(i) = i period_ns.
 *   a. smooth_weights != NULL: both series go through scipy.ndimage.gaussian_filter1d -- smooth_weights [2 r + 1]
 *      with r = smooth_radius, symmetric, as the caller computed them; boundary "reflect" (d c b a | a b c d | d c b a,
 *      also for n <= r); out = x[i] w[r], then for j = r .. 1: out += (x[i - j] + x[i + j]) w[r - j], no contraction:
 *      SciPy's bits.
 *   b. the trigger series is coa_n (trigger_on = 1) or coa (0), smoothed if a. ran.  threshold_method 0: the constant
 *      threshold_value.  1 / 2: per chunk of chunk_samples samples counted from sample 0 (the last one shorter, one
 *      chunk when n < chunk_samples) med = median(chunk) and 1: med + (1.4826 median(|chunk - med|)) threshold_value,
 *      2: med threshold_value -- exact selection, NumPy's operation order, no contraction: NumPy's bits.
 *   c. candidates: the maximal runs [f, l] of trig[i] >= threshold[i / chunk_samples]; p = the FIRST maximum of COA
 *      (not of the trigger series) over the run; MinTime = t(p) - mei_ns if t(p) - t(f) < mw_ns else t(f) - (mei_ns -
 *      mw_ns); MaxTime = t(p) + mei_ns if t(l) - t(p) < mw_ns else t(l) + (mei_ns - mw_ns).
 *   d. candidates k and k + 1 are separate events iff MaxTime[k] < t(p[k + 1]) - mw_ns and MinTime[k + 1] > t(p[k]) +
 *      mw_ns; per event the member with the FIRST largest trig[p] gives the peak, MinTime is the members' smallest,
 *      MaxTime their largest.
 * Out: *n_candidates, *n_events; events_i i64 [n_events][4]: peak index, MinTime, MaxTime, members; events_f f64
 * [n_events][3]: TRIG_COA = trig[p], COA = coa[p], COA_NORM = coa_n[p] (smoothed if a. ran).  Optional (NULL: not
 * wanted): thresholds f64 [chunks] (one value under method 0), smoothed f64 [2][n] (written only when a. ran),
 * candidates i64 [n_candidates][5]: f, l, p, MinTime, MaxTime, with room for max_candidates rows.
 * The time window, the region test and the EventID are the caller's (quakemigrate_amd/trigger.py).
 * Refused, with every output untouched: a NULL argument (the optional ones excepted), n < 1 or above 2^30, a
 * trigger_on other than 0 / 1, a threshold_method outside 0..2, chunk_samples < 1 under method 1 / 2, smooth_radius
 * outside 0.."trigger_max_radius", period_ns < 1, mw_ns < 0, mei_ns < 2 mw_ns, a non-finite sample in either series
 * (the message names their number; the reference would compute NaN thresholds and trigger nothing), more candidates
 * than max_candidates where the table is wanted, more events than max_events (the message names the number needed).
 * qm_engine_last_kernel_ms reports the launch sequence, its two read-backs of counts included. */
typedef struct {
    int32_t trigger_on;             /* 0: COA, 1: COA_N */
    int32_t threshold_method;       /* 0: static, 1: MAD, 2: median ratio */
    double threshold_value;         /* the constant (method 0) or the multiplier */
    int64_t chunk_samples;          /* methods 1 and 2 */
    int32_t smooth_radius;          /* r */
    int32_t reserved;               /* 0 */
    const double *smooth_weights;   /* [2 r + 1], NULL: no smoothing */
    int64_t period_ns, mw_ns, mei_ns;
} qm_trigger_params;
int qm_engine_trigger(qm_engine *e, const double *coa, const double *coa_n, int64_t n, const qm_trigger_params *params,
                      int64_t max_events, int64_t *n_candidates, int64_t *n_events, int64_t *events_i,
                      double *events_f, double *thresholds, double *smoothed, int64_t *candidates,
                      int64_t max_candidates);
/* ... the same call on series that are on the engine's GPU already (coa, coa_n: device f64 [n], read on the engine's
 * stream; what qm_engine_scanmseed_decode leaves with out_on_device = 1): no host copy of the series is made.  Every
 * other argument, every output and every refusal as above. */
int qm_engine_trigger_resident(qm_engine *e, const double *coa, const double *coa_n, int64_t n,
                               const qm_trigger_params *params, int64_t max_events, int64_t *n_candidates,
                               int64_t *n_events, int64_t *events_i, double *events_f, double *thresholds,
                               double *smoothed, int64_t *candidates, int64_t max_candidates);

/* The day file's codec on the device -- the step between the detect sweep and the trigger: the STEIM2 payloads of the
 * .scanmseed records that quakemigrate_amd/scanmseed.py writes and reads (what obspy / libmseed write for the
 * reference: miniSEED 2, 4096-byte records, encoding 11; the rules on arrays: tests/scanmseed_ref.py; kernels:
 * csrc/qm_scanmseed.hpp).  A record is 64 header bytes and 63 frames of 16 big-endian words; word 0 of a frame holds
 * fifteen 2-bit codes, words 1 and 2 of frame 0 the record's first and last sample: 943 data words per record.
 *
 * qm_engine_scanmseed_encode.  series: [5][n], the channels COA, COA_N, X, Y, Z in this order, host or device
 * (series_on_device), series_dtype 0: int32, already quantised (factors, clips: not read, may be NULL); 1: float64,
 * quantised on the device as scanmseed.quantise does: min(x, clips[c]) (clips[c] = +infinity: no clip) times
 * factors[c], rounded half to even, int32.
 *   Differences are global and 64-bit: d[0] = 0, d[p] = x[p] - x[p - 1], across record boundaries too.  Words are
 *   packed greedily: the first of 7x4, 6x5, 5x6, 4x8, 3x10, 2x15, 1x30 bits whose count is at most the differences
 *   left in the TRACE and whose differences all fit.  A trace's words are cut into records every 943.
 * Out: n_records i64 [5], the channels' record counts; records u8 [sum][4096], channel after channel: the 64 header
 * bytes ZERO (BTIME, sequence number, blockette 1000 and the rest of the header are the caller's: scanmseed.py's
 * write_trace), the payload complete, unused words and frames of a trace's last record zero; rec_first, rec_count
 * i32 [sum]: every record's first sample index in its channel and its sample count.  All three have room for
 * max_records records (never more than 5 ceil(n / 943) are needed); the count is known on the host before the device
 * output is sized, as the trigger's candidate count is.  The same input gives the same bytes on every run.
 * Deviations from the Python, all refusals: a float64 sample that is NaN, or whose scaled value is outside int32, is
 * refused by channel and index -- NumPy's cast to int32 is platform-defined there, so there are no bytes to match; a
 * difference outside 30 bits is refused by channel and index (the Python raises OverflowError).
 * Refused, with every output untouched: a NULL argument (factors / clips under series_dtype 0 excepted), a
 * series_dtype other than 0 / 1, n < 1 or above 2^28, a non-finite factor, a NaN clip, the three above, more records
 * than max_records (the message names the number needed).  qm_engine_last_kernel_ms reports the launch sequence, its
 * read-back of counts included.
 *
 * qm_engine_scanmseed_decode.  records: host u8 [n_records][4096], whole records with the payload at byte 64 (header
 * parsing -- station, BTIME, sample count, blockette 1000, the 4096 / big-endian / encoding-11 checks -- is the
 * caller's: scanmseed.py); rec_samples i32 [n_records]: the header's sample counts; rec_offset i64 [n_records]: where
 * in `out` each record's samples go (the caller orders and concatenates: any channel layout); rec_factor f64
 * [n_records], needed with out_f64 only.  Out: out i32 [n_total]; out_f64 (NULL: not wanted) f64 [n_total], sample /
 * rec_factor: one IEEE division, NumPy's bits; both host, or both on the engine's GPU with out_on_device = 1 (then
 * valid on the engine's stream; the call has waited for it when it returns).
 * Refused: a NULL argument (the optional ones excepted), n_records < 1, n_total < 1, a record with fewer than 1
 * sample or whose samples leave `out`, and -- naming the record, the smallest such index -- the Python's three
 * ValueErrors in its order: an invalid code / dnib pair before the record's last difference, fewer differences than
 * samples (a sample count above 6601 included), a last sample that is not the reverse integration constant.  None
 * of these faults: every launch stays in bounds.  Host outputs are untouched by a refused call; device outputs may
 * hold the records decoded so far. */
int qm_engine_scanmseed_encode(qm_engine *e, const void *series, int series_dtype, int series_on_device, int64_t n,
                               const double *factors /*[5]*/, const double *clips /*[5]*/, int64_t max_records,
                               int64_t *n_records /*[5]*/, uint8_t *records, int32_t *rec_first, int32_t *rec_count);
int qm_engine_scanmseed_decode(qm_engine *e, const uint8_t *records, int64_t n_records, const int32_t *rec_samples,
                               const int64_t *rec_offset, const double *rec_factor, int64_t n_total, int32_t *out,
                               double *out_f64, int out_on_device);

/* exp(x) rounded to nearest from a double-double evaluation (csrc/qm_ties.hpp): the function the
 * opt-in arg-max rule "tie_rule" = 1 compares near-tied nodes on (the reference exponentiates, then
 * compares: migratelib.c:60-62, :98-105).  Host code, exported for the tests that pin it. */
double qm_exp_correctly_rounded(double x);
/* ... and the GPU's evaluation of the same source, host arrays in and out (the tests pin the two together) */
int qm_engine_exp_correctly_rounded(qm_engine *e, const double *x, int64_t n, double *out);

/* Self-check behind the screened detect's error bound (qm_screen.hpp): the largest relative
 * deviation of the device's v_exp_f32 from the float64 exp2 over EVERY float32 in [lo, hi]
 * (lo <= hi, same sign).  The bound quotes <= 2^-23 for it. */
int qm_exp2f_max_error(qm_engine *e, float lo, float hi, double *max_rel_error);

/* Scan of an existing volume (find_max_coa semantics, no table needed). */
int qm_engine_find_max_coa(qm_engine *e, const double *map4d, int map_on_device,
                           int32_t n_samples, int64_t n_nodes, double *max_coa,
                           double *max_norm_coa, int64_t *max_coa_idx,
                           int out_on_device);

/* ------------------------------------------------------------------ part 3 */
/* The continuous detect sweep as a pipeline -- the hot-path part of the loop of
 * QuakeScan._continuous_compute (quakemigrate/signal/scan.py:434-448: one timestep after the other:
 * onsets -> migrate -> find_max_coa -> append), with host-resident onsets going in and the three
 * series coming out per timestep.  A ring of `depth` slots of `steps_per_launch` timesteps each;
 * qm_stream_push copies one timestep's log-onsets (host f64 [n_rows][t_samples], the resident table's
 * row count) into pinned memory and, when a slot is full, enqueues its H2D copy (own stream) and ONE
 * fused-detect launch for its timesteps on the engine's stream (qm_engine_detect_batch: every
 * timestep's bits are the single-step call's) whose last kernel writes the results straight into the
 * slot's pinned host buffer; nothing waits.  qm_stream_pop hands out the results of the oldest timesteps in push order and is the
 * only call that blocks (for the launch they belong to).
 * qm_stream_push returns 0, or 2 when every slot holds results that have not been popped (pop, then
 * push again), or 1 on error.  qm_stream_flush launches a partly filled slot (end of the data).
 * The engine's table, stream and tunables must not change while a stream exists on it. */
typedef struct qm_stream qm_stream;
int qm_stream_create(qm_engine *e, int32_t t_samples, int32_t fsmp, int32_t lsmp, int32_t available,
                     int64_t n_nodes_total, int32_t steps_per_launch, int32_t depth, qm_stream **out);
void qm_stream_destroy(qm_stream *s);
int qm_stream_push(qm_stream *s, const double *log_onsets);
int qm_stream_flush(qm_stream *s);
/* the next n_steps timesteps (<= launched and not yet popped): host f64 / f64 / i64 [n_steps][n_samples] */
int qm_stream_pop(qm_stream *s, int32_t n_steps, double *max_coa, double *max_norm_coa,
                  int64_t *max_coa_idx);
int qm_stream_pending(qm_stream *s, int32_t *launched_not_popped, int32_t *pushed_not_launched);
/* What crosses the bus is ONE KIND OF INPUT per stream, and a slot's launch is the part of one chain that kind still
 * needs -- pull or copy of the input -> (signals made on the device) -> (conditioning) -> (onsets) -> fused detect:
 *   log-onsets     qm_stream_push             no stage: taken from creation on
 *   signals        qm_stream_push_signals     the onset stage        qm_stream_set_onset_stage
 *   raw traces     qm_stream_push_raw         the resampling stage   qm_stream_set_resample_stage, on the onset stage
 *   gappy traces   qm_stream_push_segments    the segment feed       qm_stream_set_segment_feed, on the onset stage
 * The rules are the same for every kind (csrc/qm_stream.hip: kFeedTable), and every refusal leaves the stream as it was:
 *   - a set call is refused when the stage it stands on is not set ("... comes first"), when its own is set already
 *     ("it is set once"), when the other stage on the onset stage is set ("this stream takes ..."), and after the
 *     first push -- launched or not ("... is set before the first push");
 *   - a push is refused when its stage is not set ("the stream has no ..."), when a stage stands on its own (signals,
 *     once the resampling stage or the segment feed is set), and when the stream has taken a step of another kind;
 *   - every array of a set call is copied to the device there, so no launch waits on a host buffer; a stage that
 *     fails -- over replicas: on any lane -- leaves the stream as it was; stage and pushes go lane by lane;
 *   - every push returns what qm_stream_push returns; flush / pop / pending do not depend on the kind.
 *
 * Waveforms in: a timestep's resampled component traces (host f64 [n_traces][t_samples]).  A slot's launch is
 * qm_engine_preprocess's kernel (zero-phase) over the slot's (step, trace)s -> qm_engine_onsets' kernels over its
 * (step, trace)s and (step, row)s -> the fused detect: every timestep's bits are those of the three staged calls.  The
 * arguments are those of qm_engine_preprocess and qm_engine_onsets (n_rows is the resident table's).  Refused too: a
 * trace_row entry out of range or a row without a trace, and what qm_engine_preprocess refuses. */
int qm_stream_set_onset_stage(qm_stream *s, int32_t n_traces, const int32_t *trace_row,
                              const int32_t *trace_filter, const double *sos, int32_t n_filters,
                              int32_t n_sections, int detrend, const double *taper_left,
                              int32_t n_left, const double *taper_right, int32_t n_right,
                              const int32_t *nsta, const int32_t *nlta, int transform, int position,
                              int32_t taper_pad, double min_onset_value);
int qm_stream_push_signals(qm_stream *s, const double *signals);
/* Raw waveforms in: a timestep's packed raw traces (host, total_raw_samples int32 or float64 samples, laid out as the
 * records say).  A slot's launch starts with qm_engine_resample's kernel over the slot's (step, trace)s, which makes
 * the signals; then as above.  The arguments are qm_engine_resample's; t_samples must be the stream's and n_traces the
 * onset stage's.  The ring's pinned slots are sized for the raw bytes (the signals' pinned buffers go at the first
 * qm_stream_push_raw).  Refused too: what qm_engine_resample refuses. */
int qm_stream_set_resample_stage(qm_stream *s, int32_t n_traces, const int64_t *records, const double *sos_lp,
                                 int32_t n_lowpass, int32_t n_sections_lp, int detrend,
                                 const int32_t *taper_table, int32_t n_tapers, const double *taper_weights,
                                 int64_t n_taper_weights, int32_t t_samples, int raw_dtype,
                                 int64_t total_raw_samples);
int qm_stream_push_raw(qm_stream *s, const void *raw);
/* Gappy waveforms in: a timestep's component traces in window layout TOGETHER WITH their segment layout -- it changes
 * from timestep to timestep, so it travels with the push: signals host f64 [n_traces][t_samples], records
 * [n_segments][8] and taper_weights as qm_engine_preprocess_segments takes them.  A step is three parts in one pinned
 * slot -- n_traces x t_samples doubles, 8 x max_segments int64, max_taper_weights doubles -- which one pull or copy
 * moves, bits unchanged; records the push does not use are padded with n = 0.  A slot's launch starts with
 * qm_engine_preprocess_segments' kernel over the slot's (step, record)s, from the slot's buffer into the slot's signals
 * (filters, detrend and zero phase are the onset stage's; its tapers are not used); then the onset kernels and the
 * detect.  The signals' pinned buffers go at the first push, as with raw traces.  Refused too: max_segments < 1,
 * max_taper_weights < 0, a fill_value that is not finite; and by the push, which checks the records on the caller's
 * thread: what qm_engine_preprocess_segments refuses in them, n_segments > max_segments and n_taper_weights >
 * max_taper_weights. */
int qm_stream_set_segment_feed(qm_stream *s, int32_t max_segments, int64_t max_taper_weights, int second_taper,
                               double fill_value);
int qm_stream_push_segments(qm_stream *s, const double *signals, const int64_t *records, int32_t n_segments,
                            const double *taper_weights, int64_t n_taper_weights);
/* One pipeline over several engines that hold the SAME table (checked by digest): the continuous stream split by
 * time, not by grid.  Launch j (K timesteps) runs on engine j mod n_engines, each engine with
 * `depth` slots of its own; qm_stream_pop returns timesteps in push order.  Same qm_stream handle: push / flush /
 * pop / pending / destroy work unchanged (push returns 2 when every slot of the engine next in turn holds
 * un-popped results: all n_engines x depth launches are then un-popped, and popping the oldest one frees it).
 * Refused: fewer than one engine, a NULL entry, the same engine twice (two engines on one device are fine), an
 * engine without a table, tables of differing shape or node offset, differing digests.  Destroying an engine makes
 * every call on the stream fail; qm_stream_destroy still frees it. */
int qm_stream_create_replicas(qm_engine *const *engines, int32_t n_engines, int32_t t_samples, int32_t fsmp,
                              int32_t lsmp, int32_t available, int64_t n_nodes_total, int32_t steps_per_launch,
                              int32_t depth, qm_stream **out);

/* Duration (ms, HIP events on the engine stream) of the stacking kernel(s) of
 * the most recent detect / migrate call, or of the kernel of a more recent
 * qm_engine_pick_phases, qm_engine_resample or qm_engine_preprocess_segments, or of the two launches of a more recent
 * qm_engine_measure_amplitudes; negative if none.  Synchronises. */
int qm_engine_last_kernel_ms(qm_engine *e, double *ms);

/* With config "log_timing" = 1 every stacking launch is bracketed by its own
 * pair of HIP events (on the engine stream); this returns the summed duration
 * and the number of launches since the last call, and resets the log. */
int qm_engine_kernel_log(qm_engine *e, double *total_ms, int32_t *n_calls);

/* ------------------------------------------------------------------ part 4 */
/* Engine groups: ONE process and ONE host thread drive a grid on several devices (csrc/qm_group.hip; DESIGN.md
 * section 5), no collective library.  device_ids lists one PART per entry; ids may repeat ({0, 0}: two parts on
 * GPU 0).  Entry 0 is the lead device: the fold of the parts' partials, the outputs' staging and the near-tie
 * refinement's fold run there.  Below the handle each part holds one qm_engine per box of its share of the grid
 * (at most three), on its device and stream, with the box's slice of the table and its node offset -- the layout
 * of quakemigrate_amd/distributed.py's ColumnShardedDetector.  A step stages the log-onsets once into pinned
 * memory (one H2D per part), enqueues every box's partial, moves each part's packed [3 boxes][3][n_samples]
 * partials to the lead (hipMemcpyPeerAsync; a direct write on the lead's own device) ordered by events, folds
 * them there over n_parts * 3 sets (as qm_engine_finalize_packed), and only then waits -- once.  tie_rule = 1
 * adds the second exchange of qm_engine_tie_partial / _tie_fold.  Host in, host out; results are those of one
 * engine over the whole table (max_coa and max_coa_idx bit for bit; max_norm_coa's sum over the nodes is formed
 * in another order).  Not available on a group: screen = 1 (refused by qm_group_config), on-device serving,
 * detect_batch and the qm_stream pipeline (a continuous stream over several devices splits by time instead:
 * qm_stream_create_replicas, part 3), device pointers.  Every call returns 0 / non-zero + qm_last_error(). */
typedef struct qm_group qm_group;

/* The partition, host code: part `part` of n_parts as up to three boxes (x0, x1, y0, y1, z0, z1), ascending in
 * flat order, each a contiguous flat range starting at node (x0 * ny + y0) * nz + z0.  A 3-D grid is cut into
 * balanced ranges of (x, y) columns (distributed.shard_columns / column_boxes, z0 = 0, z1 = nz); a flat table
 * (nx = ny = 1: what the drop-in migrate() loads without QM_HIP_GRID) into balanced contiguous z-runs, one box
 * (0, 1, 0, 1, z0, z1) each.  A part may be empty (*n_boxes = 0) when there are more parts than columns. */
int qm_group_plan(int32_t nx, int32_t ny, int32_t nz, int32_t n_parts, int32_t part, int32_t *boxes /*[3][6]*/,
                  int32_t *n_boxes);
int qm_group_create(const int32_t *device_ids, int32_t n, qm_group **out);
void qm_group_destroy(qm_group *g);
/* a key of qm_engine_config to every engine of the group; qm_group_get: the engines' common value (fails if they
 * disagree), or the group's own read-outs n_parts, n_nodes, n_rows, nx, ny, nz, lut_max */
int qm_group_config(qm_group *g, const char *key, int64_t value);
int qm_group_get(qm_group *g, const char *key, int64_t *value);
/* host table i32 [nx][ny][nz][n_rows], sliced by the plan (flat tables: nx = ny = 1, nz = n_nodes) */
int qm_group_load_lut(qm_group *g, const int32_t *host_table, int32_t nx, int32_t ny, int32_t nz, int32_t n_rows);
/* qm_engine_table_select on every box engine; *resident = 1 only if every one has its slice resident.  The box
 * engines park and evict on their own, and one that has a box for only some of the grids' shapes has parked fewer
 * tables than the others: with a small capacity the group can therefore MISS a table that a single engine given the
 * same calls would still hold (never the reverse) -- the caller loads it again, a rebuild, never another table.  A
 * load after such a miss leaves every box engine's table known under the key. */
int qm_group_table_select(qm_group *g, uint64_t key, int32_t capacity, int32_t *resident);
/* qm_engine_detect / _marginal / _migrate / _find_max_coa over the whole grid, host arrays: log_onsets f64
 * [n_rows][t_samples], series [n_samples], coa_map f64 [n_nodes], map4d f64 [n_nodes][n_samples] (accumulate != 0:
 * added on top of its content).  max_coa == NULL: no series.  find_max_coa: part p scans the balanced flat range p
 * of the volume's nodes, the partials are folded on the lead. */
int qm_group_detect(qm_group *g, const double *log_onsets, int32_t t_samples, int32_t fsmp, int32_t lsmp,
                    int32_t available, double *max_coa, double *max_norm_coa, int64_t *max_coa_idx);
int qm_group_marginal(qm_group *g, const double *log_onsets, int32_t t_samples, int32_t fsmp, int32_t lsmp,
                      int32_t available, int32_t first_sample, int32_t end_sample, double *coa_map,
                      double *max_coa, double *max_norm_coa, int64_t *max_coa_idx);
int qm_group_migrate(qm_group *g, const double *log_onsets, int32_t t_samples, int32_t fsmp, int32_t lsmp,
                     int32_t available, double *map4d, int accumulate, double *max_coa, double *max_norm_coa,
                     int64_t *max_coa_idx);
int qm_group_find_max_coa(qm_group *g, const double *map4d, int32_t n_samples, int64_t n_nodes, double *max_coa,
                          double *max_norm_coa, int64_t *max_coa_idx);
int qm_group_synchronize(qm_group *g);
int qm_group_n_parts(qm_group *g, int32_t *n_parts);
/* part `part`: its device, boxes as qm_group_plan, flat node range [node_range[0], node_range[1]) and the device
 * time (ms) of its share of the last step, from behind its onsets' copy to its last kernel (-1: none yet).
 * Any pointer may be NULL. */
int qm_group_part_info(qm_group *g, int32_t part, int32_t *device, int32_t *boxes /*[3][6]*/, int32_t *n_boxes,
                       int64_t *node_range /*[2]*/, double *last_ms);

#ifdef __cplusplus
}
#endif
#endif /* QMHIP_H */
