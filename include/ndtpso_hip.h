/*
 * ndtpso_hip.h -- C-ABI of the MI355X (gfx950) NDT-PSO scan-alignment path.
 *
 * The reference (abougouffa/ndtpso_slam) has no FFI/plugin layer: its boundary
 * is the C++ class API of libndtpso_slam consumed by ndtpso_slam_node
 * (CMakeLists.txt:155-160,183-187).  This header is the thin C-ABI that the
 * drop-in host library (host/ndtpso_slam/ *.h, same class names and
 * signatures as include/ndtpso_slam/ndtframe.h:37-70 of the reference) calls
 * into; each entry point names the reference code it replaces.  Plain
 * pointers and sizes only; no C++/torch types.
 *
 * Conventions
 *   - every function returns 0 (NDTPSO_OK) or a negative NDTPSO_E_* code;
 *     ndtpso_last_error(ctx) gives the text.  Nothing throws across the ABI
 *     (the reference API never throws either; SURVEY 8b "Errors").
 *   - `_dev` variants take DEVICE pointers, enqueue on the context stream and
 *     return without synchronising; the others take HOST pointers and return
 *     after the results are back on the host.
 *   - there is no CPU fallback: with no usable HIP device every call fails
 *     with NDTPSO_E_HIP.
 *   - a context, and the resident scans / maps created from it, keep scratch
 *     buffers between calls and are not safe for concurrent use: one thread at
 *     a time per context (the reference's NDTFrame is single-threaded too);
 *     independent threads use independent contexts.
 *   - a frame may have at most 65535 cells per side (the reference keeps
 *     widthNumOfCells / heightNumOfCells in uint16_t, ndtframe.h:32); larger
 *     grids are refused with NDTPSO_E_ARG.
 */
#ifndef NDTPSO_HIP_H
#define NDTPSO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NDTPSO_OK 0
#define NDTPSO_E_HIP (-1)      /* HIP runtime error / no device */
#define NDTPSO_E_ARG (-2)      /* invalid argument */
#define NDTPSO_E_CAPACITY (-3) /* problem does not fit the on-chip (LDS) layout */
#define NDTPSO_E_STATE (-4)    /* call order (e.g. align before a reference table is set) */

/* score arithmetic after the fp64 transform + cell lookup */
#define NDTPSO_SCORE_F32 0 /* Mahalanobis + exp in fp32, fp64 accumulation (BASELINE config 2: "fp32") */
#define NDTPSO_SCORE_F64 1 /* everything in fp64, reference operation order */
/* NDTPSO_SCORE_EXACT: the results of NDTPSO_SCORE_F64 at (nearly) the speed of NDTPSO_SCORE_F32.  The PSO only ever
 * COMPARES costs (core.cpp:63,94,97), so the fp32 score decides every comparison whose two sides are further apart
 * than the margin tau = max(5e-6 x |gbest cost|, 7e-7 x points of the scan) -- the fp32 form's rounding error is below
 * 2.95e-7 per point whatever the cells look like (derivation: ndtpso_kernels.hpp verify_pose_wave), i.e.
 * below tau / 2 for ANY input, so a comparison outside the margin falls as it would in fp64 by proof, not by luck
 * (tests/test_gpu_margin.py checks the inequality for every evaluation with a diagnostic build) -- and the rest
 * ("near-ties", about 0.5 per 70 x 70 alignment) are arbitrated with the fp64 score of the poses involved, evaluated exactly as SCORE_F64 evaluates them;
 * the returned cost is the fp64 score of the returned pose.  Pose and cost equal SCORE_F64's bit for bit (tests:
 * every pair of BASELINE configs 3, 4 and 5).  Where the fp32 kernel cannot arbitrate (tables too large for the dense
 * LDS form, degenerate overlaps, swarms of near-identical costs) the fp64-score kernel does the alignment.
 * ndtpso_cost_batch / ndtpso_map_cost treat it as SCORE_F64. */
#define NDTPSO_SCORE_EXACT 2

typedef struct ndtpso_ctx ndtpso_ctx;

/* PSOConfig, include/ndtpso_slam/config.h:27-38 (field for field; num_threads is ignored on the device) */
typedef struct {
  int32_t iterations;
  int32_t population;
  int32_t num_threads;
  double w, c1, c2, w_damping;
} ndtpso_pso_config;

/* NDTFrame grid geometry: width/height in metres (uint16, ndtframe.h:32), cell_side (ndtframe.h:36) */
typedef struct {
  uint16_t width, height;
  double cell_side;
} ndtpso_grid;

/* arguments of NDTFrame::loadLaser (ndtframe.h:47-48) + NDTPSOConfig::laserIgnoreEpsilon (config.h:44) */
typedef struct {
  uint32_t n_beams;
  float min_angle, angle_increment, max_range;
  float laser_ignore_epsilon;
} ndtpso_scan_geom;

/* one row per created cell (ascending linear index), for inspection / parity tests */
typedef struct {
  int32_t index; /* ix + W*iy, NDTFrame::getCellIndex (ndtframe.cpp:244-245) */
  int32_t count; /* points accumulated */
  int32_t built; /* NDTCell::built (count > 2, ndtcell.cpp:43) */
  int32_t reserved;
  double mean[2];
  double icov[4]; /* row-major inverse covariance (ndtcell.cpp:109-110) */
} ndtpso_cell_row;

typedef struct {
  uint32_t n_points;      /* new-scan points that entered the PSO */
  uint32_t n_built;       /* built reference cells */
  uint32_t cost_evals;    /* particle evaluations incl. those thrown away behind a gbest update (the one-workgroup kernels deal an
                             iteration's items by ticket: how many were in flight then depends on timing -- poses and costs do not) */
  uint32_t rounds;        /* evaluation rounds (iterations + replays) */
  uint32_t gbest_updates; /* in-iteration gbest improvements */
  uint32_t status;        /* 0 ok; bit0: a reference point fell outside the staging window; bit1: more built cells
                             than record capacity; bit2: fp32 costs underflowed and the
                             fp64 redo did not fit; bit3: dense-table overflow and the bitmap redo did not fit.
                             Bits 16-31 (NDTPSO_SCORE_EXACT): number of pbest / gbest comparisons of this alignment
                             that were arbitrated with the fp64 score (saturating); flags = status & 0xffff */
  uint32_t t_start, t_end; /* low 32 bits of the device's 100 MHz real-time counter when the alignment's workgroup
                              started / finished (fused pairs kernel; load-balance diagnostics) */
} ndtpso_align_stats;
/* `status` is two fields in one word: test NDTPSO_STATUS_FLAGS(s) != 0 for "something went wrong", never the raw word
 * (in NDTPSO_SCORE_EXACT the upper half counts arbitrated comparisons of a perfectly good alignment). */
#define NDTPSO_STATUS_FLAGS(status) ((uint32_t)(status) & 0xffffu)
#define NDTPSO_STATUS_ARBITRATED(status) ((uint32_t)(status) >> 16)

/* ---- context --------------------------------------------------------- */
int ndtpso_ctx_create(int device, ndtpso_ctx **out);
void ndtpso_ctx_destroy(ndtpso_ctx *ctx);
const char *ndtpso_last_error(const ndtpso_ctx *ctx);
/* hipStream_t to enqueue on (NULL = the context's own stream) */
int ndtpso_set_stream(ndtpso_ctx *ctx, void *hip_stream);
int ndtpso_synchronize(ndtpso_ctx *ctx);
/* Process-wide telemetry of the single-alignment path (ndtpso_align, ndtpso_map_align -- the live node, or R replicas of it on
 * R host threads): out[0] alignments whose cluster of workgroups was not co-resident, ran into the exchange's bounded wait and
 * was redone on one workgroup (a latency spike each: a device shared with other work, or more streams than hardware queues);
 * out[1] waits for a kernel's result that slept between looks instead of spinning (more waiting threads than half the CPUs
 * the process may use: affinity mask cut by the control group's quota); out[2] that CPU budget; out[3] threads waiting now;
 * out[4] alignments kept on ONE workgroup because 16 (NDTPSO_CLUSTER_MAX_INFLIGHT) were already in flight in the process -- more
 * clusters than the device's hardware queues run side by side would wait for each other; out[5] (the batch path,
 * ndtpso_align_pairs*) batches whose few flagged pairs -- a cell table outgrown, an fp32 score in its underflow regime -- were
 * redone on clusters of workgroups instead of one workgroup each.  n: how many to write (1 .. 6).  The reference has nothing of
 * the kind (single-threaded caller, ndtpso_slam_node.cpp:182). */
int ndtpso_process_counters(uint64_t *out, int n);
/* Batches in flight.  depth 1 (default): every call is enqueued on the context's stream, one after the other.
 * depth 2: consecutive ndtpso_align_pairs_dev calls (batches of more pairs than half the device's compute units) run
 * on two internal streams with their own workspaces, so that the next batch's workgroups fill the compute units the
 * previous launch's tail leaves idle (one launch lasts as long as its slowest alignment).  Each call still starts
 * after everything enqueued on the context's stream before it (its inputs), but its OUTPUTS are ordered before later
 * work on the context's stream only by ndtpso_pipeline_flush / ndtpso_synchronize -- until then neither the inputs
 * nor the outputs of a call in flight may be touched, and two calls in flight need distinct output buffers.
 * The results do not depend on the depth (each alignment is its own workgroup).  Reference: none -- the reference
 * aligns one pair at a time (ndtpso_slam_node.cpp:194); this is the batch path of BASELINE configs 3/4. */
int ndtpso_set_pipeline_depth(ndtpso_ctx *ctx, int depth);
/* The context's stream waits (device-side, the host does not block) for the calls in flight, except the
 * `keep_newest` most recent ones (0: for all of them). */
int ndtpso_pipeline_flush(ndtpso_ctx *ctx, int keep_newest);
/* number of std::rand() draws one alignment consumes: 3 + 3P + 6PI (core.cpp:14,84) */
size_t ndtpso_rand_draws(const ndtpso_pso_config *cfg);

/* ---- K3 companions: scan ingest and cell statistics ------------------- */
/* NDTFrame::loadLaser's beam filter + index_to_angle + laser_to_point (+ s_trans transform)
 * (ndtframe.cpp:144-185, core.h:40-47).  xy_out: 2*n_beams doubles; *n_out = surviving points, beam order. */
int ndtpso_scan_to_points(ndtpso_ctx *ctx, const float *ranges, const ndtpso_scan_geom *geom,
                          const double trans[3], double *xy_out, uint32_t *n_out);

/* Reference table of a FRESH frame from points: NDTFrame::addPoint binning (ndtframe.cpp:215-235) +
 * NDTCell::build / s_calc_covar_inverse (ndtcell.cpp:36-68,93-111).  The table stays on the device
 * as the context's reference table. */
int ndtpso_ref_from_points(ndtpso_ctx *ctx, const ndtpso_grid *grid, const double *xy, uint32_t n_points);
/* same, starting from a LaserScan (loadLaser at pose `trans`, then build) */
int ndtpso_ref_from_scan(ndtpso_ctx *ctx, const ndtpso_grid *grid, const float *ranges,
                         const ndtpso_scan_geom *geom, const double trans[3]);
/* Reference table from host-side cell statistics (an accumulated map kept by the host NDTFrame):
 * built cells only; index[] ascending or not, mean 2*n, icov 4*n row-major. */
int ndtpso_ref_set_cells(ndtpso_ctx *ctx, const ndtpso_grid *grid, uint32_t n_cells, const int32_t *index,
                         const double *mean, const double *icov);
/* created cells of the table built by ndtpso_ref_from_points/_scan (parity inspection) */
int ndtpso_ref_get_cells(ndtpso_ctx *ctx, ndtpso_cell_row *rows, uint32_t max_rows, uint32_t *n_rows);

/* NDTFrame::update / NDTFrame::addPoint binning for a list of points (ndtframe.cpp:187-198, 215-235):
 * xy_out[i] = transform_point(xy[i], trans) (trans == NULL: identity, the loadLaser case),
 * cell_idx[i] = getCellIndex(xy_out[i]) or -1.  xy_out may alias xy. */
int ndtpso_points_to_cells(ndtpso_ctx *ctx, const ndtpso_grid *grid, const double *xy, uint32_t n_points,
                           const double trans[3], double *xy_out, int32_t *cell_idx);

/* NDTFrame::loadLaser in one launch: beam filter + polar->xy (+ s_trans) as ndtpso_scan_to_points, then the
 * binning of ndtpso_points_to_cells for every surviving point.  xy_out: 2*n_beams doubles, cell_idx: n_beams. */
int ndtpso_scan_to_cells(ndtpso_ctx *ctx, const float *ranges, const ndtpso_scan_geom *geom, const double trans[3],
                         const ndtpso_grid *grid, double *xy_out, int32_t *cell_idx, uint32_t *n_out);

/* The sliding-window state of one NDTCell that NDTCell::build reads and writes (ndtcell.h:65-68,
 * ndtcell.cpp:36-68); the host frame keeps it, the device does the arithmetic. */
typedef struct {
  double global_sum[2];       /* s_global_sum */
  double global_covar_sum[4]; /* s_global_covar_sum, row-major */
  double slot_sum[2];         /* s_partial_sums[s_current_window_id] */
  double slot_covar[4];       /* s_partial_covars[s_current_window_id] */
  double mean[2];             /* NDTCell::mean (out) */
  double icov[4];             /* s_inv_covar (out) */
  int32_t global_count;       /* s_global_count */
  int32_t slot_count;         /* s_partial_counts[s_current_window_id] */
  int32_t current_count;      /* s_current_count (in) */
  int32_t built;              /* NDTCell::built (in: before, out: after) */
} ndtpso_cell_window;

/* NDTCell::build + s_calc_covar_inverse for n_cells created cells at once (NDTFrame::build's loop,
 * ndtframe.cpp:73-76).  pts_offset[n_cells+1] delimits each cell's points_vector[s_current_window_id] (insertion
 * order) in pts_xy -- with current_count == 0 these are the stale points of the window's previous lap, which the
 * reference's covariance loop still visits (ndtcell.cpp:49) while its running sum is zero; cells[] is updated in
 * place.  The slot advance (ndtcell.cpp:61-65) is bookkeeping left to the host. */
int ndtpso_cells_build_windowed(ndtpso_ctx *ctx, uint32_t n_cells, ndtpso_cell_window *cells,
                                const uint32_t *pts_offset, const double *pts_xy);

/* Occupancy-grid rasterisation of NDTFrame::build (ndtframe.cpp:69-71,79-112; map export): for each
 * of n_cells BUILT cells and each of its k x k sub-cells (k = floor(cell_side / og_cell_size), j outer, k inner as
 * the reference loops), values[c*k*k + j*k + kk] = int8(100 * normalDistribution(sub-cell centre)), or -1 when the
 * Gaussian is exactly 0 there (the reference then leaves the grid untouched).  The row index of a cell is
 * index / heightNumOfCells, as in the reference (:81). */
int ndtpso_occupancy_values(ndtpso_ctx *ctx, const ndtpso_grid *grid, double og_cell_size, uint32_t n_cells,
                            const int32_t *index, const double *mean, const double *icov, int8_t *values);

/* ---- K1: cost_function (core.cpp:26-48) for M candidate poses ---------- */
/* xy: n_points new-frame points; poses: 3*M; costs: M; cell_idx (optional, M*n_points):
 * linear cell index scored against, -1 outside frame, -2 cell not built. */
int ndtpso_cost_batch(ndtpso_ctx *ctx, const double *xy, uint32_t n_points, const double *poses, uint32_t m,
                      int score_mode, double *costs, int32_t *cell_idx);

/* ---- K2: pso_optimization (core.cpp:50-116) --------------------------- */
/* rand_table: the std::rand() outputs the reference would draw (ndtpso_rand_draws() values), or NULL
 * to replay glibc's srand(seed) stream on the device. */
int ndtpso_align(ndtpso_ctx *ctx, const double *xy, uint32_t n_points, const double guess[3],
                 const double deviation[3], const ndtpso_pso_config *cfg, uint32_t seed,
                 const int32_t *rand_table, int score_mode, double out_pose[3], double *out_cost,
                 ndtpso_align_stats *stats);

/* ---- device-resident reference frame ---------------
 * The live node's path (ndtpso_slam_node.cpp:177-244) without the host touching a point: the map (NDTFrame with its
 * 100-slot sliding-window cells, ndtcell.h:62-70) and the loaded scan stay in HBM; per scan the host sends the ranges
 * and the std::rand() table and receives the pose.
 *   ndtpso_points_*      the node's one-cell per-scan frame (ndtpso_slam_node.cpp:229-230): a point list on the device
 *   ndtpso_map_insert    the addPoint loop of NDTFrame::update (ndtframe.cpp:190-197; pose != NULL: transform_point
 *                        first) / of loadLaser and addPoint on a multi-cell frame (:144-185, 215-235; pose == NULL):
 *                        NDTCell::addPoint (ndtcell.cpp:21-34) per point.  Like NDTFrame::addPoint it clears the
 *                        frame's `built` flag only if a point lands in the frame (:219-224)
 *   ndtpso_map_mark_unbuilt   the unconditional `built = false` at the top of update (:188) and loadLaser (:145) --
 *                        it decides whether the next cost_function builds again, and a build repeated on unchanged
 *                        cells is not a no-op in floating point (WINDOW_ADD, ndtcell.h:13-15)
 *   ndtpso_map_build     NDTFrame::build (:68-117): NDTCell::build (ndtcell.cpp:36-68) on every created cell, the
 *                        occupancy grid (:79-112), and the alignment table of the built cells
 *   ndtpso_map_align     NDTFrame::align's pso_optimization (core.cpp:50-116) against the map, building it first when
 *                        points were inserted since the last build (cost_function's lazy build, core.cpp:27-28)
 * insert and build only enqueue work; align and the get_* calls synchronise. */
#define NDTPSO_WINDOW_SIZE 100        /* NDT_WINDOW_SIZE, config.h:8 */
#define NDTPSO_MAX_POINTS_PER_CELL 50 /* NDT_MAX_POINTS_PER_CELL, config.h:5 */

typedef struct ndtpso_points ndtpso_points;
typedef struct ndtpso_map ndtpso_map;

typedef struct {
  uint32_t n_created, n_built; /* cells with points / cells in the alignment table (as of the last build) */
  uint32_t status;             /* bit 0: point pool exhausted, bit 1: an occupancy write fell outside the grid */
  uint32_t n_words;
  int32_t x0, x1, y0, y1;      /* bounding box of the built cells, cell coordinates */
  uint32_t og_min_x, og_max_x, og_min_y, og_max_y; /* s_occupancy_grid.{min,max}_{x,y}_ind (ndtframe.h:23-25) */
  int32_t pool_bump, pool_free; /* 512-byte point chunks handed out / on the free stack */
  uint64_t n_points;           /* points ever inserted */
} ndtpso_map_info;

int ndtpso_points_create(ndtpso_ctx *ctx, uint32_t capacity, ndtpso_points **out);
void ndtpso_points_destroy(ndtpso_points *pts);
/* loadLaser into a one-cell frame of `clip`'s size (NULL: unbounded); trans = the frame's s_trans (NULL = zero);
 * append != 0 keeps the points already loaded (a second loadLaser into the same frame).  Asynchronous. */
int ndtpso_points_load_scan(ndtpso_points *pts, const float *ranges, const ndtpso_scan_geom *geom, const double trans[3],
                            const ndtpso_grid *clip, int append);
int ndtpso_points_set(ndtpso_points *pts, const double *xy, uint32_t n);
int ndtpso_points_get(ndtpso_points *pts, double *xy, uint32_t max_points, uint32_t *n_points);

/* og_cell_size 0: no occupancy grid.  pool_bytes 0: 1 GiB of point storage (512 B per 32 points of one window slot).
 * Limit (the reference's `unsigned int numOfCells`, ndtframe.h:35, has none): fewer than 2^21 cells per frame (NDTPSO_E_ARG; a
 * frame costs 6.5 KB of HBM per cell: 9 GB for 300 m at 0.25 m).  The built cells may lie anywhere in it: a bounding box of more
 * than ~650 000 cells has its table assembled in HBM instead of LDS (build 0.24 ms instead of 0.05, alignment 0.5 instead of 0.36). */
int ndtpso_map_create(ndtpso_ctx *ctx, const ndtpso_grid *grid, double og_cell_size, uint64_t pool_bytes,
                      ndtpso_map **out);
void ndtpso_map_destroy(ndtpso_map *map);
/* NDTFrame::resetCells (ndtframe.cpp:208-212): NDTCell::reset (ndtcell.cpp:80-91) on every created cell -- sums, counts
 * and point vectors are cleared, the window's partial terms and created / built / mean / inverse covariance are kept */
int ndtpso_map_reset(ndtpso_map *map);
int ndtpso_map_clear(ndtpso_map *map); /* back to a freshly constructed frame */
int ndtpso_map_mark_unbuilt(ndtpso_map *map);
int ndtpso_map_insert(ndtpso_map *map, const ndtpso_points *pts, const double pose[3]);
int ndtpso_map_insert_host(ndtpso_map *map, const double *xy, uint32_t n, const double pose[3]);
int ndtpso_map_build(ndtpso_map *map);
/* Builds the cells and packs the alignment table NOW, ahead of the ndtpso_map_align (or ndtpso_map_build) that will ask
 * for them, so that they are off that call's critical path -- without changing what any call observes: everything the
 * build overwrites is logged, and an insert / reset / export arriving first puts the map back before it runs (the
 * reference builds lazily, core.cpp:27-28; a frame that is only ever updated is never built).  The occupancy grid is
 * rasterised when the speculation is committed.  A caller uses it after NDTFrame::update on a frame it aligns against. */
int ndtpso_map_speculate_build(ndtpso_map *map);
int ndtpso_map_align(ndtpso_map *map, const ndtpso_points *new_points, const double guess[3], const double deviation[3],
                     const ndtpso_pso_config *cfg, uint32_t seed, const int32_t *rand_table, int score_mode,
                     double out_pose[3], double *out_cost, ndtpso_align_stats *stats);
/* Several ndtpso_map_align calls of one context in ONE launch: the robots a process serves, or several start poses for one
 * scan.  The reference has no counterpart -- its node aligns one scan at a time (ndtpso_slam_node.cpp:182) -- so the contract is
 * the single call's: job j's pose, cost and stats (status, n_points, n_built, gbest_updates) are bit for bit what
 * ndtpso_map_align(jobs[j].map, ...) returns for the same arguments when called alone, in every score mode, and afterwards every
 * map is in the state the same calls made in job order would leave it (lazy build done, a pending speculative build committed,
 * header known to the host).  Jobs may name different maps -- grids, windows and table sizes may all differ -- or the same map
 * several times.  Each distinct map is prepared once; the jobs whose plan has a job kernel (fp32 score on the dense table,
 * plain or arbitrating, and the fp64 score on the bitmap of power-of-two cells, swarm in LDS) run as one workgroup or one
 * cluster of workgroups each in a common launch and report through one pinned result slot each; every other job, a call of one
 * job, and a job that comes back flagged (fp32 score in its underflow regime, a late-bound window outgrown, a cluster that did
 * not meet) runs alone through ndtpso_map_align's own path (route 0).
 * Returns NDTPSO_E_ARG before anything is enqueued for a null pointer, n_jobs == 0, a map or scan of another context or a bad
 * score mode; else NDTPSO_OK if every job's rc is 0, else the first failing job's rc (the other jobs are completed). */
typedef struct {
  ndtpso_map *map;                 /* in: reference frame (may repeat across jobs) */
  const ndtpso_points *new_points; /* in: loaded scan */
  double guess[3], deviation[3];   /* in */
  uint32_t seed, flags;            /* in: flags bit 0 = cost wanted */
  const int32_t *rand_table;       /* in: ndtpso_rand_draws(cfg) values, or NULL = device replay of srand(seed) */
  double pose[3], cost;            /* out */
  ndtpso_align_stats stats;        /* out */
  int32_t rc;                      /* out: NDTPSO_OK or this job's error */
  int32_t route;                   /* out: 1 = batch kernel on one workgroup, K >= 2 = batch kernel on a cluster of K,
                                      0 = the single-alignment path (ndtpso_map_align's) */
} ndtpso_map_align_job;
#define NDTPSO_MAP_ALIGN_JOB_BYTES 152
#if defined(__cplusplus)
static_assert(sizeof(ndtpso_map_align_job) == NDTPSO_MAP_ALIGN_JOB_BYTES, "ndtpso_map_align_job layout");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(ndtpso_map_align_job) == NDTPSO_MAP_ALIGN_JOB_BYTES, "ndtpso_map_align_job layout");
#endif
int ndtpso_map_align_batch(ndtpso_ctx *ctx, ndtpso_map_align_job *jobs, uint32_t n_jobs,
                           const ndtpso_pso_config *cfg, int score_mode);
/* Several ndtpso_points_load_scan calls of one context in ONE launch (NDTFrame::loadLaser of the R per-scan frames a process
 * serves, ndtpso_slam_node.cpp:186; the reference loads one scan at a time).  After the call every ndtpso_points -- its points
 * in order and its count on the device, the host's upper bound -- is bit for bit what
 *   ndtpso_points_load_scan(jobs[j].pts, jobs[j].ranges, &jobs[j].geom, trans or NULL, clip or NULL, append)
 * for j = 0 .. n_jobs - 1 in that order leaves.  All the jobs' ranges travel in one pinned block that the kernel reads in place,
 * so a call waits for the stream no more often than one single load does, however many jobs it has.  A scan buffer named a
 * second time closes the current launch (its second load follows its first); a call of one job is the single call.
 * Returns NDTPSO_E_ARG before anything is enqueued for a null pointer (ctx, jobs, a job's pts or ranges), n_jobs == 0 or a scan
 * of another context; else NDTPSO_OK if every job's rc is 0, else the first failing job's rc (the other jobs are completed). */
typedef struct {
  ndtpso_points *pts;      /* in: the resident scan to load into (may repeat across jobs) */
  const float *ranges;     /* in: geom.n_beams ranges; free to reuse when the call returns */
  double trans[3];         /* in: used when flags bit 0 is set */
  ndtpso_grid clip;        /* in: used when flags bit 1 is set */
  ndtpso_scan_geom geom;   /* in */
  uint32_t flags;          /* in: bit 0 = trans given, bit 1 = clip given, bit 2 = append */
  int32_t rc;              /* out: NDTPSO_OK or this job's error */
  int32_t reserved;
} ndtpso_points_load_job;
#define NDTPSO_POINTS_LOAD_JOB_BYTES 88
#define NDTPSO_POINTS_LOAD_JOB_RC_OFFSET 80
/* Several map updates of one context in shared launches (NDTFrame::update of the R maps a process serves,
 * ndtpso_slam_node.cpp:198; the reference updates one frame at a time): one insert launch, and for the jobs that ask for the
 * speculative build one build and one pack launch, where the single calls take three launches per map.  After the call every
 * map is bit for bit in the state that
 *   ndtpso_map_mark_unbuilt(map); ndtpso_map_insert(map, points, pose or NULL); [ndtpso_map_speculate_build(map);]
 * for j = 0 .. n_jobs - 1 in that order leaves it in: cells, window terms, every slot's points in order, header, packed table
 * image, the pinned header of the speculative build and its number on the device; built, the pending speculation, the bounds
 * of points and pool chunks and the late-binding figures on the host -- so a following ndtpso_map_align or
 * ndtpso_map_align_batch takes the path it would take after the single calls and returns the same bits.  (Which pool chunk a
 * point lands in is unordered inside one insert already, and stays so.)
 * Routing is decided per job, on the host, by the single calls' own rules (they share the code): a job whose preparation must
 * wait for the device -- a point pool to be measured or grown, an undo log or pinned header to be allocated -- runs through the
 * single calls in its place in job order (route 0), and so does a call of one job.  A map named a second time closes the
 * current set of launches, so per map the order is job order.  A pending speculation is taken back ahead of the shared insert,
 * on the same stream.  An empty scan inserts nothing and still takes the flagged build.
 * Returns NDTPSO_E_ARG before anything is enqueued for a null pointer, n_jobs == 0 or a map or scan of another context; else
 * NDTPSO_OK if every job's rc is 0, else the first failing job's rc (the other jobs are completed). */
typedef struct {
  ndtpso_map *map;             /* in (may repeat across jobs) */
  const ndtpso_points *points; /* in: a loaded resident scan */
  double pose[3];              /* in: used when flags bit 0 is set */
  uint32_t flags;              /* in: bit 0 = pose given, bit 1 = speculative build afterwards */
  int32_t rc;                  /* out: NDTPSO_OK or this job's error */
  int32_t route;               /* out: 1 = the shared launches, 0 = the single calls' path */
  int32_t reserved;
} ndtpso_map_update_job;
#define NDTPSO_MAP_UPDATE_JOB_BYTES 56
#define NDTPSO_MAP_UPDATE_JOB_RC_OFFSET 44
#define NDTPSO_MAP_UPDATE_JOB_ROUTE_OFFSET 48
#if defined(__cplusplus)
static_assert(sizeof(ndtpso_points_load_job) == NDTPSO_POINTS_LOAD_JOB_BYTES, "ndtpso_points_load_job layout");
static_assert(sizeof(ndtpso_map_update_job) == NDTPSO_MAP_UPDATE_JOB_BYTES, "ndtpso_map_update_job layout");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(ndtpso_points_load_job) == NDTPSO_POINTS_LOAD_JOB_BYTES, "ndtpso_points_load_job layout");
_Static_assert(sizeof(ndtpso_map_update_job) == NDTPSO_MAP_UPDATE_JOB_BYTES, "ndtpso_map_update_job layout");
#endif
int ndtpso_points_load_scans(ndtpso_ctx *ctx, ndtpso_points_load_job *jobs, uint32_t n_jobs);
int ndtpso_map_update_batch(ndtpso_ctx *ctx, ndtpso_map_update_job *jobs, uint32_t n_jobs);
/* cost_function (core.cpp:26-48) of a loaded scan against the map at n_poses candidate poses (3 doubles each) */
int ndtpso_map_cost(ndtpso_map *map, ndtpso_points *new_points, const double *poses, uint32_t n_poses, int score_mode,
                    double *costs);
/* cost_function (core.cpp:26-48) at every node of a pose lattice, and the best top_k nodes: the start poses of a
 * relocalization, where a guess is a metre or a radian off and ndtpso_map_align's +-0.1 m / +-3 mrad search (ndtframe.cpp:253)
 * would settle in the wrong basin.  The reference has no counterpart; a call stands for nx * ny * nth cost_function calls.
 *   - Node numbering: node (i, j, k) has index (k * ny + j) * nx + i.
 *   - Node pose: each component is origin + (double)i * step -- one multiplication, one addition, no FMA -- so a caller
 *     regenerates any node's pose bit for bit.  On an axis of one node the step is not read (the pose is origin + 0.).
 *   - Returned: *n_hits = min(top_k, n_nodes) hits in ascending cost, ties broken by ascending index.  A NaN cost ranks behind
 *     every number, NaNs among themselves by index.  Comparison is by value: -0. and +0. tie.  `hits` has room for top_k.
 *   - The map: built first if points were inserted since the last build, a pending speculation committed, exactly as
 *     ndtpso_map_cost does; synchronous; the map is left in the state ndtpso_map_cost would leave it in.
 *   - NDTPSO_SCORE_F64: every hit's cost is bit for bit what ndtpso_map_cost(map, new_points, hit.pose, 1, F64, ...) returns,
 *     and the hits are exactly the best n_hits of that function over all nodes (one wave per node, the four lane accumulators
 *     and the wave sum of the cost kernel: the summation order is the same).
 *   - NDTPSO_SCORE_F32: the fp32 sweep's own best nodes with their fp32 costs -- a tolerance mode, as everywhere.
 *   - NDTPSO_SCORE_EXACT: the F64 result bit for bit, from the fp32 sweep wherever its margin is proven: sweep in fp32, take the
 *     K-th smallest fp32 cost c32_K (K = n_hits), collect every node with c32 <= c32_K + 7e-7 * n_points, score those in fp64
 *     through ndtpso_map_cost's path, rank.  (The fp32 sum is within 2.95e-7 * n_points of the fp64 one, so the true K-th cost
 *     is <= c32_K + B and every true member has c32 <= c32_K + 2 B < c32_K + tau: DESIGN 3.5.)  The whole lattice runs in fp64
 *     instead -- stats->fell_back says why -- when the plan is not the dense table, when an fp32 cost is NaN, when c32_K lies in
 *     the fp32 underflow regime (> -1e-28), when more than NDTPSO_SEARCH_MAX_CANDIDATES nodes qualify, or when the process was
 *     refused the exact mode by the start-up check.
 * Nothing proportional to the node count crosses the host link: the node poses come from the descriptor, the selection runs on
 * the device (a cost per node stays in device memory: 8 bytes x nodes).
 * Errors, before anything is enqueued: NDTPSO_E_ARG for a null pointer, a count of 0, more than 2^24 nodes, top_k outside
 * 1 .. 64, a step that is not positive and finite on an axis of more than one node, a non-finite origin, a scan of another
 * context or a bad score mode; NDTPSO_E_CAPACITY when the plan does not fit, as ndtpso_map_cost says it. */
typedef struct {
  double origin[3];  /* pose of node (0,0,0): x, y, theta */
  double step[3];    /* > 0 and finite on every axis whose count > 1 */
  uint32_t count[3]; /* nx, ny, nth, each >= 1; nx*ny*nth <= 2^24 */
  uint32_t top_k;    /* 1 .. 64 */
} ndtpso_lattice;
typedef struct {
  double pose[3];
  double cost;
  uint32_t index, reserved;
} ndtpso_lattice_hit;
typedef struct {
  uint32_t n_nodes, n_points;
  uint32_t mode_run;     /* the score the sweep ran with: NDTPSO_SCORE_F32 or NDTPSO_SCORE_F64 */
  uint32_t path;         /* table plan: 0 / 1 bitmap (division / power-of-two cells), 2 dense, 4 / 5 as 0 / 1 from the HBM image */
  uint32_t n_candidates; /* EXACT: nodes rescored in fp64 */
  uint32_t fell_back;    /* EXACT: why the fp64 sweep ran instead (NDTPSO_SEARCH_FELL_*), 0 = it did not */
  uint32_t reserved[2];
} ndtpso_search_stats;
#define NDTPSO_LATTICE_BYTES 64
#define NDTPSO_LATTICE_HIT_BYTES 40
#define NDTPSO_SEARCH_STATS_BYTES 32
#define NDTPSO_SEARCH_MAX_NODES (1u << 24)
#define NDTPSO_SEARCH_MAX_TOP_K 64
#define NDTPSO_SEARCH_MAX_CANDIDATES 4096
#define NDTPSO_SEARCH_FELL_PLAN 1      /* the plan is not the dense table */
#define NDTPSO_SEARCH_FELL_NAN 2       /* an fp32 cost is NaN */
#define NDTPSO_SEARCH_FELL_UNDERFLOW 3 /* c32_K lies in the fp32 underflow regime */
#define NDTPSO_SEARCH_FELL_MANY 4      /* more than NDTPSO_SEARCH_MAX_CANDIDATES candidates */
#define NDTPSO_SEARCH_FELL_REFUSED 5   /* the start-up check refused the exact mode */
#if defined(__cplusplus)
static_assert(sizeof(ndtpso_lattice) == NDTPSO_LATTICE_BYTES, "ndtpso_lattice layout");
static_assert(sizeof(ndtpso_lattice_hit) == NDTPSO_LATTICE_HIT_BYTES, "ndtpso_lattice_hit layout");
static_assert(sizeof(ndtpso_search_stats) == NDTPSO_SEARCH_STATS_BYTES, "ndtpso_search_stats layout");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(ndtpso_lattice) == NDTPSO_LATTICE_BYTES, "ndtpso_lattice layout");
_Static_assert(sizeof(ndtpso_lattice_hit) == NDTPSO_LATTICE_HIT_BYTES, "ndtpso_lattice_hit layout");
_Static_assert(sizeof(ndtpso_search_stats) == NDTPSO_SEARCH_STATS_BYTES, "ndtpso_search_stats layout");
#endif
/* (stands for nx * ny * nth calls of cost_function, core.cpp:26-48) */
int ndtpso_map_search(ndtpso_map *map, ndtpso_points *new_points, const ndtpso_lattice *lattice, int score_mode,
                      ndtpso_lattice_hit *hits, uint32_t *n_hits, ndtpso_search_stats *stats /* may be NULL */);
/* Several ndtpso_map_search calls of one context in shared launches: the R robots a process relocalizes, or ONE scan against the
 * M submaps it may have been taken in (the same new_points in M jobs).  The reference has no counterpart, so the contract is the
 * single call's: job j's hits, n_hits and every field of its stats are bit for bit what
 *   ndtpso_map_search(jobs[j].map, jobs[j].new_points, &jobs[j].lattice, score_mode, jobs[j].hits, &n_hits, &stats)
 * returns when called alone, in every score mode (in NDTPSO_SCORE_F32 too: a node is still scored whole by one wave, with the same
 * trips and the same wave sum), and afterwards every map is in the state the single call leaves it in: a pending speculation
 * committed, an unbuilt insert built, the header with the host -- once per distinct map, ahead of the launches.
 *   - Launches: one sweep per kernel kind (score x table plan) present in the call, with the jobs' inputs in a table and the
 *     workgroups dealt to the jobs in proportion to their items; two selection launches; in the exact mode one collect launch
 *     (the threshold c32_K + 7e-7 * n_points is formed on the device, by the host's two operations) and one fp64 launch per table
 *     plan over the jobs' candidate lists.  The number of launches and of waits for the stream does not depend on the number of jobs.
 *   - Fallbacks are per job: a job whose exact mode sweeps in fp64 (fell_back 1 .. 4) shares one more fp64 sweep and selection
 *     with the other such jobs of the call and does not drag the rest with it.  A refusal by the start-up check (5) applies to
 *     every job, as it does to single calls.
 *   - Errors.  NDTPSO_E_ARG before anything is enqueued (and before any job's out fields are written) for a null pointer (ctx,
 *     jobs, a job's map, new_points or hits), n_jobs == 0, a map or scan of another context, a bad score mode, or node counts of
 *     the jobs' (valid) lattices that sum to more than NDTPSO_SEARCH_MAX_NODES: the jobs of a call share the single call's cost
 *     buffer of 8 bytes x 2^24.  A job whose own lattice the single call would refuse, or whose plan does not fit, gets that
 *     error in its rc and n_hits = 0; the other jobs complete.  Returns NDTPSO_OK if every job's rc is 0, else the first failing
 *     job's rc.
 *   - route: 1 = the shared launches; 0 = ndtpso_map_search's own path: a call of one job, and a job that is the only one of its
 *     call left with a valid lattice and plan.
 * stats (may be NULL), counted on the host: launches = kernel launches the searches enqueued (the maps' own builds not counted),
 * waits = waits for the stream, both of the shared path only; single_jobs = jobs that took route 0. */
typedef struct {
  ndtpso_map *map;            /* in: reference frame (may repeat across jobs) */
  ndtpso_points *new_points;  /* in: loaded scan (may repeat across jobs) */
  ndtpso_lattice lattice;     /* in */
  ndtpso_lattice_hit *hits;   /* in: room for lattice.top_k hits; out: the hits */
  uint32_t n_hits;            /* out */
  int32_t rc;                 /* out: NDTPSO_OK or this job's error */
  int32_t route;              /* out: 1 = the shared launches, 0 = ndtpso_map_search's own path */
  uint32_t reserved;
  ndtpso_search_stats stats;  /* out */
} ndtpso_map_search_job;
typedef struct {
  uint32_t launches, waits, single_jobs, reserved;
} ndtpso_search_batch_stats;
#define NDTPSO_MAP_SEARCH_JOB_BYTES 136
#define NDTPSO_MAP_SEARCH_JOB_HITS_OFFSET 80
#define NDTPSO_MAP_SEARCH_JOB_RC_OFFSET 92
#define NDTPSO_MAP_SEARCH_JOB_STATS_OFFSET 104
#define NDTPSO_SEARCH_BATCH_STATS_BYTES 16
#if defined(__cplusplus)
static_assert(sizeof(ndtpso_map_search_job) == NDTPSO_MAP_SEARCH_JOB_BYTES, "ndtpso_map_search_job layout");
static_assert(sizeof(ndtpso_search_batch_stats) == NDTPSO_SEARCH_BATCH_STATS_BYTES, "ndtpso_search_batch_stats layout");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(ndtpso_map_search_job) == NDTPSO_MAP_SEARCH_JOB_BYTES, "ndtpso_map_search_job layout");
_Static_assert(sizeof(ndtpso_search_batch_stats) == NDTPSO_SEARCH_BATCH_STATS_BYTES, "ndtpso_search_batch_stats layout");
#endif
int ndtpso_map_search_batch(ndtpso_ctx *ctx, ndtpso_map_search_job *jobs, uint32_t n_jobs, int score_mode,
                            ndtpso_search_batch_stats *stats /* may be NULL */);

/* ---- curvature of the score at a pose: gradient, Hessian, pose covariance ------------------------------------------
 * cost_function (core.cpp:26-48) with NDTCell::normalDistribution (ndtcell.cpp:70-78), differentiated once and twice by the pose
 * (x, y, theta) of a loaded scan against the map, at n_poses poses (3 doubles each).  The reference has no counterpart: it returns
 * a pose and a cost and says nothing of how well the pose is constrained.  Per scan point (x, y) that lands in a built cell, with
 * A = s_inv_covar (row-major a00 a01 a10 a11, not assumed symmetric) and mu the cell's mean, in the reference's operations:
 *   c, s = cos theta, sin theta;  rx, ry = x c - y s, x s + y c;  q = (rx + tx, ry + ty);  d = q - mu;  Q = (d^T A) d;  e = exp(-Q / 2)
 *   B = A + A^T:  b00, b01, b11 = 2 a00, a01 + a10, 2 a11;   v = B d
 *   g = (v0, v1, -ry v0 + rx v1)                                             (dQ / dx, dQ / dy, dQ / dtheta)
 *   h00, h01, h11 = b00, b01, b11;  h02 = -b00 ry + b01 rx;  h12 = -b01 ry + b11 rx
 *   h22 = ry^2 b00 - 2 rx ry b01 + rx^2 b11 - (v0 rx + v1 ry)
 *   cost = -sum e;   gradient_k = sum e g_k / 2;   hessian_kl = sum e (h_kl / 2 - g_k g_l / 4)
 * Cell membership is held fixed: the score is piecewise smooth, as in every NDT formulation.
 *   - cost is bit for bit ndtpso_map_cost(map, new_points, pose, 1, NDTPSO_SCORE_F64, ...) on every table plan: the same lookup,
 *     the same exponential, the terms summed in its order.  Always fp64: there is no score mode.
 *   - The ten sums are a pure function of (map state, scan points, pose): the same bits whether the pose is alone or at any index
 *     among many, in this call or in a job of ndtpso_map_curvature_batch, on any grid.  One wave owns a pose from the first
 *     point to the last; no atomics, no reduction across waves.
 *   - A point whose e is exactly +0. (outside the frame, in a cell that is not built, or Q beyond the exponential's range) adds
 *     exactly zero to every sum.  A NaN e (a cell built from coincident points) makes all ten sums NaN.
 *   - n_hit: the points that landed in a built cell.  path: the table plan, as ndtpso_search_stats.path (0, 1, 4, 5).
 *   - The map: exactly ndtpso_map_cost's side effects -- a pending speculative build committed, an unbuilt map built, the header
 *     fetched; synchronous.  An empty scan is no error: all zeros, the cost as ndtpso_map_cost gives it.
 * Errors: NDTPSO_E_ARG for a null pointer, n_poses == 0 or more than NDTPSO_CURVATURE_MAX_POSES, a scan of another context, a
 * pose that is not finite; NDTPSO_E_CAPACITY when the plan does not fit, as ndtpso_map_cost says it. */
typedef struct {
  double cost;         /* == ndtpso_map_cost(F64) bit for bit */
  double gradient[3];  /* d cost / d (x, y, theta) */
  double hessian[6];   /* d2 cost: xx, xy, xth, yy, yth, thth */
  uint32_t n_points, n_hit;
  uint32_t path, reserved;
} ndtpso_curvature;
#define NDTPSO_CURVATURE_BYTES 96
#define NDTPSO_CURVATURE_MAX_POSES 65536
#if defined(__cplusplus)
static_assert(sizeof(ndtpso_curvature) == NDTPSO_CURVATURE_BYTES, "ndtpso_curvature layout");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(ndtpso_curvature) == NDTPSO_CURVATURE_BYTES, "ndtpso_curvature layout");
#endif
/* (stands for cost_function, core.cpp:26-48, and normalDistribution, ndtcell.cpp:70-78, differentiated; no counterpart) */
int ndtpso_map_curvature(ndtpso_map *map, ndtpso_points *new_points, const double *poses, uint32_t n_poses,
                         ndtpso_curvature *out);
/* Several ndtpso_map_curvature calls of one context in shared launches: the R robots of a fleet, or the top-K hits of a
 * relocalization told apart by curvature.  cost_function and normalDistribution differentiated, as above; the reference has no
 * counterpart, so the contract is the single call's: job j's out[0 .. n_poses) is bit for bit what
 *   ndtpso_map_curvature(jobs[j].map, jobs[j].new_points, jobs[j].poses, jobs[j].n_poses, jobs[j].out)
 * writes when called alone, and afterwards every map is in the state the single call leaves it in.  Maps and scans may repeat.
 *   - Every distinct map is prepared once, ahead of the launches (its own build if it needs one; one wait for all the maps'
 *     headers and the scans' point counts, which the plans are made from).  Then one launch per table plan present in the call
 *     and one wait for the stream, whatever the number of jobs.
 *   - Errors.  NDTPSO_E_ARG before anything is enqueued or written for a null pointer (ctx, jobs, a job's map, new_points, poses
 *     or out), n_jobs == 0, a map or scan of another context, or poses that sum to more than NDTPSO_CURVATURE_MAX_POSES.  A job
 *     with n_poses == 0 or a pose that is not finite gets NDTPSO_E_ARG in its rc, a job whose plan does not fit
 *     NDTPSO_E_CAPACITY; the other jobs complete.  Returns NDTPSO_OK if every job's rc is 0, else the first failing job's rc.
 *   - route: 1 = the shared launches; 0 = ndtpso_map_curvature's own call: a call of one job, and a job that is the only valid
 *     one of its call.  (Both go through the same kernel: the single call is a table of one job.)
 * stats (may be NULL), counted on the host, of the shared path only: launches = kernel launches enqueued for the curvatures,
 * waits = waits for the stream behind them (the preparation of the maps is not counted: neither their builds nor the wait for
 * their headers); single_jobs = jobs that took route 0. */
typedef struct {
  ndtpso_map *map;            /* in: reference frame (may repeat across jobs) */
  ndtpso_points *new_points;  /* in: loaded scan (may repeat across jobs) */
  const double *poses;        /* in: n_poses x 3 */
  uint32_t n_poses;           /* in */
  int32_t rc;                 /* out: NDTPSO_OK or this job's error */
  ndtpso_curvature *out;      /* in: room for n_poses records; out: the records */
  int32_t route;              /* out: 1 = the shared launches, 0 = ndtpso_map_curvature's own call */
  uint32_t reserved;
} ndtpso_map_curvature_job;
typedef struct {
  uint32_t launches, waits, single_jobs, reserved;
} ndtpso_curvature_batch_stats;
#define NDTPSO_MAP_CURVATURE_JOB_BYTES 48
#define NDTPSO_MAP_CURVATURE_JOB_POSES_OFFSET 16
#define NDTPSO_MAP_CURVATURE_JOB_RC_OFFSET 28
#define NDTPSO_MAP_CURVATURE_JOB_OUT_OFFSET 32
#define NDTPSO_MAP_CURVATURE_JOB_ROUTE_OFFSET 40
#define NDTPSO_CURVATURE_BATCH_STATS_BYTES 16
#if defined(__cplusplus)
static_assert(sizeof(ndtpso_map_curvature_job) == NDTPSO_MAP_CURVATURE_JOB_BYTES, "ndtpso_map_curvature_job layout");
static_assert(sizeof(ndtpso_curvature_batch_stats) == NDTPSO_CURVATURE_BATCH_STATS_BYTES, "ndtpso_curvature_batch_stats layout");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(ndtpso_map_curvature_job) == NDTPSO_MAP_CURVATURE_JOB_BYTES, "ndtpso_map_curvature_job layout");
_Static_assert(sizeof(ndtpso_curvature_batch_stats) == NDTPSO_CURVATURE_BATCH_STATS_BYTES, "ndtpso_curvature_batch_stats layout");
#endif
int ndtpso_map_curvature_batch(ndtpso_ctx *ctx, ndtpso_map_curvature_job *jobs, uint32_t n_jobs,
                               ndtpso_curvature_batch_stats *stats /* may be NULL */);
/* The pose covariance a curvature stands for: the plain inverse of its Hessian (the standard estimate for NDT: the inverse
 * Hessian of the score at the optimum; cost_function and normalDistribution differentiated, the reference has no counterpart).
 * It is a RELATIVE measure: the score has no unit of measurement noise in it, so the caller owns the scale factor for their
 * sensor; what it tells as it stands is which directions are constrained and how they compare.
 *   - definite = 1: every entry of the curvature's Hessian is finite and the Hessian is positive definite (its Cholesky factor
 *     exists); cov is its inverse, symmetric; xy_major >= xy_minor are the eigenvalues of cov's translational 2 x 2 block and
 *     xy_angle the major axis' direction in (-pi/2, pi/2].
 *   - definite = 0: a saddle, a pose without overlap (all zeros) or a NaN; cov and the three xy fields are zeros.  No error:
 *     the call returns NDTPSO_OK.
 * Host only: no context, no device.  NDTPSO_E_ARG for a null pointer. */
typedef struct {
  double cov[9];                        /* inverse of the Hessian, row-major, symmetric; zeros unless definite */
  double xy_major, xy_minor, xy_angle;  /* of cov's translational block; zeros unless definite */
  int32_t definite;
  int32_t reserved;
} ndtpso_pose_covariance;
#define NDTPSO_POSE_COVARIANCE_BYTES 104
#if defined(__cplusplus)
static_assert(sizeof(ndtpso_pose_covariance) == NDTPSO_POSE_COVARIANCE_BYTES, "ndtpso_pose_covariance layout");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(ndtpso_pose_covariance) == NDTPSO_POSE_COVARIANCE_BYTES, "ndtpso_pose_covariance layout");
#endif
int ndtpso_curvature_covariance(const ndtpso_curvature *c, ndtpso_pose_covariance *out);

int ndtpso_map_get_info(ndtpso_map *map, ndtpso_map_info *info);
/* created cells in ascending index order (row.reserved = the cell's current window slot) */
int ndtpso_map_get_cells(ndtpso_map *map, ndtpso_cell_row *rows, uint32_t max_rows, uint32_t *n_rows);
/* stored points in cell order, window-slot order, insertion order (dumpMap's order, ndtframe.cpp:314-328);
 * slot0_only: the points cost_function visits when the frame is the NEW frame (core.cpp:33-36) */
int ndtpso_map_get_points(ndtpso_map *map, int slot0_only, double *xy, uint64_t max_points, uint64_t *n_points);
/* og[x + og_height * y] as the reference indexes it; extent = {min_x, max_x, min_y, max_y} */
int ndtpso_map_get_occupancy(ndtpso_map *map, int8_t *og, uint64_t og_bytes, uint32_t *og_width, uint32_t *og_height,
                             uint32_t extent[4]);

/* ---- free space: every beam of a scan traced through the occupancy grid --------------------------------------------
 * The reference has no counterpart: its occupancy grid (ndtframe.cpp:79-112) holds int8(100 * normalDistribution) where a built
 * cell's Gaussian was rasterised and 0 everywhere else, so "never seen" and "seen through, nothing there" are the same entry.
 * Tracing keeps, per entry of that same grid, how many beams ended there (hits, uint32) and how many went through (passes,
 * uint64: the origin's cell takes every beam of every scan).
 *   The grid is the map's occupancy grid: og_width = ceil(width / og_cell_size), og_height likewise; cell (ox, oy) of a point q
 *   is ox = floor((q.x + width / 2.) / og_cell_size), oy likewise (getCellIndex's arithmetic, ndtframe.cpp:240-249: true
 *   division); the entry is at = ox + og_height * oy, as ndtpso_map_get_occupancy addresses it, so the grids overlay entry for
 *   entry.  With og_width != og_height that addressing makes distinct cells collide (the reference's quirk): NDTPSO_E_ARG.
 *   One quirk of the reference is kept: for the last double below the bound fl(q.x + width / 2.) == width, so ox == og_width (oy
 *   likewise).  Such a cell is addressed like any other: with oy < og_height - 1 its entry is (0, oy + 1)'s -- the wrap into the
 *   next row that the reference's own linear index makes (getCellIndex) -- and is counted there, the extent's max ox becomes
 *   og_width; an entry at or beyond og_width * og_height is counted in the totals and the extent and not written.  This
 *   concerns rays that end (or start) within one ulp of the frame's upper bound.
 *   One ray per point p of the scan: from o = (pose[0], pose[1]) to e = (x c - y s + pose[0], x s + y c + pose[1]) with
 *   (c, s) = the DEVICE's sincos of pose[2] (ndtpso_device_math kind 2), no fused operations.  A ray whose origin or end is not
 *   strictly inside the frame (|q.x| < width / 2, |q.y| < height / 2) is skipped and counted in n_skipped.
 *   The traversal, in plain IEEE fp64 (hw = width / 2., cs = og_cell_size):
 *     fx0 = (o.x + hw) / cs, fy0 likewise;  fx1 = (e.x + hw) / cs, fy1 likewise
 *     ix, iy = floor(fx0), floor(fy0);  jx, jy = floor(fx1), floor(fy1);  dx, dy = fx1 - fx0, fy1 - fy0
 *     sx = jx > ix ? 1 : -1, sy likewise;  nx = |jx - ix|, ny = |jy - iy|
 *     tdx = nx ? 1. / |dx| : inf;  tx0 = nx ? ((sx > 0 ? ix + 1 : ix) - fx0) / dx : inf   (y likewise)
 *     x-crossing i (0 <= i < nx) is at tx_i = tx0 + (double)i * tdx, y-crossing j at ty_j = ty0 + (double)j * tdy
 *   The visited cells are the staircase from (ix, iy) to (jx, jy) that merges the two crossing sequences: x-crossing i goes
 *   before y-crossing j iff tx_i <= ty_j (a tie steps x first); an axis whose crossings are used up no longer competes.  A ray
 *   visits exactly nx + ny + 1 distinct cells and ends in (jx, jy).  Every visited cell but the last gets passes += 1, the last
 *   gets hits += 1.  The adds are integer atomics: the counters are a pure function of the multiset of (scan, pose) traced,
 *   whatever the order of the calls, alone or in a batch.
 * ndtpso_map_trace only enqueues on the context's stream, as ndtpso_map_insert does.  It is an observer: it reads nothing of the
 * cells, writes nothing but its own buffers, neither settles nor disturbs a pending speculative build, and no later align, cost,
 * search, curvature, export or snapshot changes by a bit.  The counters are allocated and zeroed at a map's first trace; a map
 * that is never traced pays nothing.  An empty scan is no error.  ndtpso_map_clear zeroes counters and totals, ndtpso_map_reset
 * keeps them, ndtpso_map_destroy frees them.  Snapshot format 1 does not carry them: a restored map starts with none.
 * Errors: NDTPSO_E_ARG for a null pointer (pose is required), a pose that is not finite, a scan of another context, a grid that
 * is not square; NDTPSO_E_STATE for a map without an occupancy grid (og_cell_size 0).  Out of scope: beams without a return,
 * per-scan de-duplication, decay, clipping of rays that leave the frame. */
int ndtpso_map_trace(ndtpso_map *map, const ndtpso_points *points, const double pose[3]);
/* Several ndtpso_map_trace calls of one context -- several robots' scans, or several scans of one map -- in ONE launch, whatever
 * n_jobs (the reference has no counterpart).  Maps and scans may repeat; nothing needs ordering because the adds commute, and
 * every map's counters are what the single calls give.  NDTPSO_E_ARG before anything is enqueued or written for a null pointer
 * (ctx, jobs, a job's map or points), n_jobs == 0, or a map or scan of another context.  A job whose own map or pose
 * ndtpso_map_trace would refuse carries that error in its rc and the other jobs complete.  Returns NDTPSO_OK, or the first
 * failing job's rc. */
typedef struct {
  ndtpso_map *map;             /* in (may repeat across jobs) */
  const ndtpso_points *points; /* in: loaded scan (may repeat across jobs) */
  double pose[3];              /* in */
  int32_t rc;                  /* out: NDTPSO_OK or this job's error */
  uint32_t reserved;
} ndtpso_map_trace_job;
#define NDTPSO_MAP_TRACE_JOB_BYTES 48
#define NDTPSO_MAP_TRACE_JOB_POSE_OFFSET 16
#define NDTPSO_MAP_TRACE_JOB_RC_OFFSET 40
int ndtpso_map_trace_batch(ndtpso_ctx *ctx, ndtpso_map_trace_job *jobs, uint32_t n_jobs);
/* What has been traced since the last clear (the reference has no counterpart).  allocated: the map has counters (0: never
 * traced; everything else but width and height is then as of an untraced map).  extent = {min ox, max ox, min oy, max oy} of the
 * cells with any count, kept by device-side min / max as the occupancy extents are ({UINT32_MAX, 0, UINT32_MAX, 0}: none).
 * n_rays: rays traced; n_skipped: rays skipped at the frame's bound; n_steps: the sum of nx + ny == the sum of passes.
 * Synchronous. */
typedef struct {
  uint32_t allocated, width, height, reserved;
  uint32_t extent[4];
  uint64_t n_rays, n_skipped, n_steps;
} ndtpso_trace_info;
#define NDTPSO_TRACE_INFO_BYTES 56
#define NDTPSO_TRACE_INFO_EXTENT_OFFSET 16
#define NDTPSO_TRACE_INFO_N_RAYS_OFFSET 32
#if defined(__cplusplus)
static_assert(sizeof(ndtpso_map_trace_job) == NDTPSO_MAP_TRACE_JOB_BYTES, "ndtpso_map_trace_job layout");
static_assert(sizeof(ndtpso_trace_info) == NDTPSO_TRACE_INFO_BYTES, "ndtpso_trace_info layout");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(ndtpso_map_trace_job) == NDTPSO_MAP_TRACE_JOB_BYTES, "ndtpso_map_trace_job layout");
_Static_assert(sizeof(ndtpso_trace_info) == NDTPSO_TRACE_INFO_BYTES, "ndtpso_trace_info layout");
#endif
int ndtpso_map_get_trace_info(ndtpso_map *map, ndtpso_trace_info *info);
/* The raw counters, og_width * og_height entries each, addressed as the occupancy grid is (the reference has no counterpart).
 * Either pointer may be NULL; capacity_entries too small: NDTPSO_E_ARG.  Of a map never traced: zeros.  Synchronous. */
int ndtpso_map_get_trace(ndtpso_map *map, uint32_t *hits, uint64_t *passes, uint64_t capacity_entries);
/* The three-state grid a planner wants (nav_msgs/OccupancyGrid's convention; the reference has no counterpart), formed on the
 * device from the occupancy keys and the counters, one byte per entry across the host link.  Settles the map exactly as
 * ndtpso_map_get_occupancy does.  Per entry, with v the byte ndtpso_map_get_occupancy returns, h = hits, p = passes:
 *   v > 0       -> v: the reference's word stands
 *   h + p == 0  -> -1: unknown
 *   else        -> (100 * h + (h + p) / 2) / (h + p) in unsigned 64-bit integer arithmetic: 0 for a cell only ever seen through
 * (v is never negative -- the reference's grid starts as zeros and int8(100 * p) of a Gaussian is 0 .. 100 --, and its own
 * picture draws og > 0 only, ndtframe.cpp:408: a 0 of the reference says nothing, so the counters speak there.)
 * NDTPSO_E_STATE without an occupancy grid, NDTPSO_E_ARG for a null pointer or fewer than og_width * og_height bytes. */
int ndtpso_map_get_nav_grid(ndtpso_map *map, int8_t *grid, uint64_t bytes);

/* ---- a resident map saved to a blob and restored bit for bit ---------------------------------------------------
 * The reference has no counterpart (dumpMap, ndtframe.cpp:314-328, writes points for a plot; nothing reads them back).  A
 * snapshot is a compact, deterministic, versioned image of everything about a map that is primary state: the created cells in
 * creation order, of each the cell record and the window slots in use (partial sums, covariances, counts, the stored points in
 * insertion order), the header, the occupancy keys inside the rasterised box, and `built`, the build number and the host's
 * bounds.  The alignment table is derived and is packed again by the restore (of a map that is not built, the header's table
 * fields -- n_built, n_words, the built cells' box -- describe a table that is no longer current and are saved as zero: the
 * next build writes them).  A restored map behaves under every later call
 * exactly as the original would have: cells, points, occupancy, costs, alignments and searches are bit for bit the original's,
 * now and after any number of further inserts and builds.  The same map state gives the same bytes, and
 * snapshot(restore(blob)) == blob.  Size is proportional to content, never to the frame:
 *   bytes <= 4096 + 192 * n_created + 80 * n_slots_used + 528 * n_chunks + 8 * og_box_entries.
 * Format 1: little-endian, 16-byte aligned sections, 64-bit sizes and offsets, magic, version, the constants it was made with
 * (NDTPSO_WINDOW_SIZE, NDTPSO_MAX_POINTS_PER_CELL, chunk size, cell record size), FNV-1a checksums of header and body.
 * Format 1 does not carry the free-space counters of ndtpso_map_trace (they are evidence about the world, not state any
 * alignment depends on): a restored map starts with none.  A format 2 that does is a follow-up. */
typedef struct {
  uint32_t version, n_created, n_built, built; /* format; created cells; cells of the table (0 unless built); NDTFrame::built */
  uint64_t n_slots_used, n_chunks, n_points_stored, og_box_entries, bytes;
  ndtpso_grid grid;
  double og_cell_size;
} ndtpso_snapshot_info;
#define NDTPSO_SNAPSHOT_INFO_BYTES 80
#define NDTPSO_SNAPSHOT_BYTES_OFFSET 32 /* format 1: the blob's own size, a little-endian uint64 at this byte (a blob inside a larger file) */
#if defined(__cplusplus)
static_assert(sizeof(ndtpso_snapshot_info) == NDTPSO_SNAPSHOT_INFO_BYTES, "ndtpso_snapshot_info layout");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(ndtpso_snapshot_info) == NDTPSO_SNAPSHOT_INFO_BYTES, "ndtpso_snapshot_info layout");
#endif
/* The size ndtpso_map_snapshot needs now.  Settles the map as the exports do (a pending speculative build is put back first;
 * NDTFrame::built stays what it is: a map with points inserted since its last build is saved unbuilt).  Synchronous. */
int ndtpso_map_snapshot_size(ndtpso_map *map, uint64_t *bytes);
/* Writes the blob; *bytes = its size.  capacity too small: NDTPSO_E_CAPACITY, *bytes = the size needed, nothing written.  A map
 * whose point pool has run out (ndtpso_map_info.status bit 0) has lost points and is refused with NDTPSO_E_CAPACITY.  Synchronous. */
int ndtpso_map_snapshot(ndtpso_map *map, void *blob, uint64_t capacity, uint64_t *bytes);
/* A new map of `ctx` -- any context: another thread's or another device's, which makes this the way to clone a map -- from a
 * blob.  pool_bytes as ndtpso_map_create's.  Everything is checked before device memory is allocated: magic, version, constants,
 * grid, counts (n_chunks == sum of ceil(slot_len / 32)), section bounds against `bytes`, checksums.  A mismatch returns
 * NDTPSO_E_ARG with a message that names the field, a pool too small for the blob's chunks NDTPSO_E_CAPACITY; *out is NULL then
 * and nothing stays allocated.  Synchronous. */
int ndtpso_map_restore(ndtpso_ctx *ctx, const void *blob, uint64_t bytes, uint64_t pool_bytes, ndtpso_map **out);
/* What a blob holds, after the same checks (NDTPSO_E_ARG if one fails).  Host only: no context, no device. */
int ndtpso_snapshot_describe(const void *blob, uint64_t bytes, ndtpso_snapshot_info *info);

/* ---- one alignment on several compute units --------------------------
 * ndtpso_align, ndtpso_map_align and small batches of ndtpso_align_pairs* spread an alignment over K workgroups (each
 * keeps the table, the points and the whole swarm and runs the identical control flow; the cost evaluations of a round
 * are divided one item per wave and exchanged once per round).  Results are bit-identical to one workgroup; a cluster
 * whose workgroups cannot run together gives up after a bounded wait and the alignment is redone on one workgroup
 * (status bit 16 is internal and never returned).  Environment: NDTPSO_CLUSTER=0|K, NDTPSO_CLUSTER_WAVES=w. */

/* ---- fused batched scan pairs (BASELINE configs 3/4) ------------------- */
/* For pair b: reference frame <- ref scan loaded at identity and built; new frame <- new scan
 * (ndtpso_slam_node.cpp:186,229-230); pose_b = pso_optimization(guess_b, ref, new, deviation_b, cfg)
 * under the srand(seeds[b]) stream (or rand_tables + b*ndtpso_rand_draws(cfg) when not NULL).
 * ranges are [n_pairs][n_beams] row-major; guess/deviation/out_pose [n_pairs][3].
 * A pair the fused kernels cannot hold -- an occupied box beyond the largest cell table of a workgroup whose bitmap form does not
 * fit LDS either: cells of 0.125 m in a 60 m frame, a dozen pairs in 600 -- comes out of them with NDTPSO_STATUS_FLAGS set.  This
 * entry (host buffers, synchronous) then aligns it through a resident frame (ndtpso_map_*: table in HBM), same pose bit for bit --
 * so does ndtpso_align_pairs_sharded, on its first device; ndtpso_align_pairs_dev / ndtpso_align_pairs_sharded_dev, asynchronous
 * on device buffers, leave the flag to the caller. */
int ndtpso_align_pairs(ndtpso_ctx *ctx, uint32_t n_pairs, const float *ref_ranges, const float *new_ranges,
                       const ndtpso_scan_geom *geom, const ndtpso_grid *grid, const double *guess,
                       const double *deviation, const ndtpso_pso_config *cfg, const uint32_t *seeds,
                       const int32_t *rand_tables, int score_mode, double *out_pose, double *out_cost,
                       ndtpso_align_stats *stats);
/* same with DEVICE pointers; asynchronous on the context stream */
int ndtpso_align_pairs_dev(ndtpso_ctx *ctx, uint32_t n_pairs, const float *d_ref_ranges,
                           const float *d_new_ranges, const ndtpso_scan_geom *geom, const ndtpso_grid *grid,
                           const double *d_guess, const double *d_deviation, const ndtpso_pso_config *cfg,
                           const uint32_t *d_seeds, const int32_t *d_rand_tables, int score_mode,
                           double *d_out_pose, double *d_out_cost, ndtpso_align_stats *d_stats);
/* LDS bytes and workgroup size the fused kernel would be launched with (occupancy study; 0 if it does not fit) */
int ndtpso_align_pairs_footprint(const ndtpso_scan_geom *geom, const ndtpso_grid *grid,
                                 const ndtpso_pso_config *cfg, uint32_t *lds_bytes, uint32_t *block_threads);

/* How ndtpso_align_pairs would run a configuration (LDS cell-table sizing / occupancy study, BASELINE config 5), for a
 * batch with more pairs than the device has compute units.  Smaller batches use 16-wave workgroups, and below half the
 * compute units several workgroups share a pair (cluster mode): same layout per workgroup, different shape. */
typedef struct {
  uint32_t lds_bytes;        /* dynamic LDS per workgroup (0 if the configuration does not fit) */
  uint32_t block_threads;    /* workgroup size */
  uint32_t workgroups_per_cu;/* by LDS and by the 16-waves-per-CU register budget */
  uint32_t table_form;       /* 0 bitmap + true division, 1 bitmap + power-of-two cells, 2 dense u16 table (fp32 records),
                                8 / 9 dense u16 table with fp64 records (fp64 score; true division / power-of-two cells) */
  uint32_t swarm_in_hbm;     /* 1: the swarm state lives in an HBM workspace instead of LDS */
  uint32_t window_w, window_h; /* staging window in cells */
  uint32_t table_bytes;      /* LDS bytes of the cell index + records */
} ndtpso_pairs_plan;
int ndtpso_align_pairs_describe(const ndtpso_scan_geom *geom, const ndtpso_grid *grid, const ndtpso_pso_config *cfg,
                                int score_mode, uint32_t n_pairs, ndtpso_pairs_plan *out);

/* ---- one batch on several devices, one process (BASELINE config 4) ---------------------------------
 * The pairs are independent (each is one NDTFrame::align of a recorded pair, ndtpso_slam_node.cpp:194; the reference's
 * own parallelism is an OpenMP loop over particles, core.cpp:81), so the batch is partitioned by contiguous index
 * range -- device d of G takes ndtpso_shard_range(n_pairs, d, G) -- and each device runs ndtpso_align_pairs_dev on its
 * shard in a context and stream of its own, with no traffic between devices.  The only exchange is ONE ncclAllGather
 * (RCCL over xGMI, single-process communicator from ncclCommInitAll) of pose + cost, 4 doubles per pair, after which
 * every device holds the poses of the whole batch; device 0's copy is returned.  Results are those of
 * ndtpso_align_pairs on the same arguments, bit for bit, whatever the number of devices.
 * RCCL is loaded at run time: ndtpso_shard_group_create returns NDTPSO_E_HIP when it (or a listed device) is absent.
 * A group is used by one host thread at a time.  Every device has a host thread of its own inside the group: the uploads
 * of device d (blocking staged copies when the caller's memory is pageable), its launch and the copy of its statistics are
 * issued by that thread, all devices at once; the calling thread joins the ENQUEUES, issues the collective, and only then
 * waits for the devices.  Two flavours: host buffers (the scatter is part of the call) and `_dev` (each device's shard
 * already resident: per-device arrays of device pointers, entry d = the slice [first_d, last_d) on device d, complete
 * before the call).  ndtpso_shard_last_timing reports, for the last call, per device {start after the call's entry, uploads,
 * launches} and per call {until every device's work was enqueued, the collective's enqueue, total} in microseconds of
 * host time; ndtpso_shard_gathered(group, d) is device d's copy of the gathered batch, G blocks of [pose (M x 3) |
 * cost (M)] doubles with M = ceil(n_pairs / G), valid until the group's next call. */
typedef struct ndtpso_shard_group ndtpso_shard_group;
int ndtpso_shard_group_create(const int *devices, int n_devices, ndtpso_shard_group **out);
void ndtpso_shard_group_destroy(ndtpso_shard_group *group);
int ndtpso_shard_group_size(const ndtpso_shard_group *group);
const char *ndtpso_shard_last_error(const ndtpso_shard_group *group);
/* [first, last) of device `rank` of `n_devices`: contiguous, sizes differing by at most one */
void ndtpso_shard_range(uint32_t n_pairs, int rank, int n_devices, uint32_t *first, uint32_t *last);
int ndtpso_align_pairs_sharded(ndtpso_shard_group *group, uint32_t n_pairs, const float *ref_ranges,
                               const float *new_ranges, const ndtpso_scan_geom *geom, const ndtpso_grid *grid,
                               const double *guess, const double *deviation, const ndtpso_pso_config *cfg,
                               const uint32_t *seeds, const int32_t *rand_tables, int score_mode, double *out_pose,
                               double *out_cost, ndtpso_align_stats *stats);
int ndtpso_align_pairs_sharded_dev(ndtpso_shard_group *group, uint32_t n_pairs, const float *const *d_ref_ranges,
                                   const float *const *d_new_ranges, const ndtpso_scan_geom *geom,
                                   const ndtpso_grid *grid, const double *const *d_guess,
                                   const double *const *d_deviation, const ndtpso_pso_config *cfg,
                                   const uint32_t *const *d_seeds, const int32_t *const *d_rand_tables, int score_mode,
                                   double *out_pose /* may be NULL: results stay on the devices */, double *out_cost,
                                   ndtpso_align_stats *stats);
int ndtpso_shard_last_timing(const ndtpso_shard_group *group, double *per_device /* [G][3] or NULL */,
                             double *call /* [3] or NULL */);
/* the last call's collective on shard 0's stream, by device events: from the end of shard 0's own launch to the end of its
 * share of the gather (the wait for the slowest shard included); microseconds, 0 if the call failed */
double ndtpso_shard_last_gather_device_us(const ndtpso_shard_group *group);
const double *ndtpso_shard_gathered(const ndtpso_shard_group *group, int index);
/* What the group is, for a caller's record: how many shards, over what the poses are gathered, which RCCL, how many ranks
 * its communicator holds.  gather_kind 0: ONE ncclAllGather over RCCL (the product path); 1: staged through the host -- the
 * TEST mode NDTPSO_SHARD_VIRTUAL=G in the environment, in which a group has G shards whatever the length of the device
 * list (shard i on devices[i mod n], a context, stream and host thread each) so that a box with one device can run the
 * partition, the thread-per-shard scatter and the error paths of a G-device call; never a measurement of the collective.
 * ndtpso_shard_verify_gather (after a successful call): the number of shards whose send block is found bit for bit in
 * EVERY shard's gathered copy, i.e. the ranks the collective has demonstrably moved; G when all is well. */
typedef struct {
  int32_t n_shards;
  int32_t gather_kind;   /* 0 RCCL ncclAllGather, 1 host-staged (test mode) */
  int32_t rccl_version;  /* ncclGetVersion's code, 0 if RCCL is not loaded */
  int32_t comm_ranks;    /* ncclCommCount of the group's communicator, 0 in the test mode */
  int32_t devices[64];   /* device of shard i */
} ndtpso_shard_info;
int ndtpso_shard_group_describe(const ndtpso_shard_group *group, ndtpso_shard_info *out);
int ndtpso_shard_verify_gather(ndtpso_shard_group *group, int *ranks_seen);

/* ---- probes of the device arithmetic the parity claims rest on (tests/test_gpu_exp.py) --------------------------
 * NDTCell::normalDistribution ends in exp() (ndtcell.cpp:76) and transform_point takes the cosine and sine of the pose's
 * heading (core.h:28-31): on the device those are the ROCm math library's exp / sincos, and the fp64 score's own spelling
 * of exp(-q / 2) (exp_neg_half, ndtpso_kernels.hpp: the library's operations without its two range guards).
 * ndtpso_selftest_exp: for every binade b in [exp2_lo, exp2_hi], per_binade pseudo-random arguments x = -(1 + u) 2^b
 * (positive != 0: +), the library's exp(x) against exp_neg_half(-2 x) bit for bit (two NaNs count as equal); returns the
 * number checked, the number that differ and one differing argument (NaN if none).
 * ndtpso_device_math: kind 0: out0 = exp(x) (library); 1: out0 = exp_neg_half(-2 x); 2: out0 = sin(x), out1 = cos(x) from
 * one sincos(x) -- HOST pointers, n arguments. */
int ndtpso_selftest_exp(ndtpso_ctx *ctx, int exp2_lo, int exp2_hi, uint32_t per_binade, uint32_t seed, int positive,
                        uint64_t *checked, uint64_t *mismatched, double *first_bad);
int ndtpso_device_math(ndtpso_ctx *ctx, int kind, const double *x, uint32_t n, double *out0, double *out1);
/* The start-up known-answer check of NDTPSO_SCORE_EXACT.  The first request for the exact mode on a device (any entry
 * point, any context of the process) first sends a fixed small problem through EVERY kernel instantiation that arbitrates
 * and that the library's dispatchers can reach -- the fused pairs kernels over table-entry form x {one workgroup per
 * alignment without / with clipping trips, clusters of workgroups} x swarm in LDS / in HBM x plain / box-guard copies, and the
 * lone alignment's kernel (ndtpso_align, ndtpso_map_align) on one workgroup and on a cluster: 16 families, each forced by a
 * plan override and confirmed by the instantiation its launch recorded -- in the exact mode and in NDTPSO_SCORE_F64, and
 * compares poses and costs bit for bit (and checks, per family, that comparisons were in fact arbitrated).  If any family
 * differs the device is refused the exact mode: every later request for it runs NDTPSO_SCORE_F64 (the same results by
 * definition, at its speed), and ndtpso_last_error explains.  A check that could not run (no memory for its context, a HIP
 * error) is no verdict: that request runs NDTPSO_SCORE_F64 and the next one runs the check again (three attempts).
 * ndtpso_exact_check runs the check if it has not run and reports: state 1 passed, 2 refused; the comparisons the check
 * arbitrated in the pairs / lone-alignment families; its duration in ms.  ndtpso_exact_check_report writes one JSON object
 * with a line per family (name, passed / refused / not reachable on this device, alignments, arbitrated, mismatched) into
 * buf (at most cap - 1 characters) and returns the length the whole text needs.  NDTPSO_EXACT_CHECK=0 in the environment
 * skips the check. */
int ndtpso_exact_check(ndtpso_ctx *ctx, int *state, uint32_t *arbitrated_batch, uint32_t *arbitrated_single, double *ms);
int ndtpso_exact_check_report(ndtpso_ctx *ctx, char *buf, uint32_t cap);
/* The same rule for the two arbitrating kernels of ndtpso_map_align_batch (jobs of one launch on one workgroup each, on a cluster
 * of workgroups each): the first exact-mode call of that entry on a device sends the same fixed problem through both, as jobs of
 * one launch against a resident map, and compares with the fp64 mode bit for bit.  A family that fails refuses the exact mode to
 * that entry only (its exact-mode jobs run NDTPSO_SCORE_F64; ndtpso_last_error explains).  ndtpso_exact_check_jobs runs it if it
 * has not run: state 1 passed, 2 refused, 0 no verdict.  ndtpso_exact_check_report lists the two under the key "job_families"
 * (same fields as "families"; empty until the check has run).  The reference has nothing of the kind: it has one score, in fp64
 * (ndtcell.cpp:70-77). */
int ndtpso_exact_check_jobs(ndtpso_ctx *ctx, int *state);

#ifdef __cplusplus
}
#endif
#endif
