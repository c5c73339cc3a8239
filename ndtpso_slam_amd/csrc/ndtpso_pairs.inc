// ndtpso_pairs.inc -- the fused scan-pair path on the host: ndtpso_align_pairs_footprint / _describe, ndtpso_align_pairs_dev and
// ndtpso_align_pairs.  Included by ndtpso_hip.hip inside its extern "C" block (same translation unit: shares the context, the
// planner and the k_align_pairs kernels).
//
//   pairs_plan                 the shape of a launch: grid, static window, score mode and table form, waves
//   launch_pairs               one launch of a PairsBatch as a PairsLaunch asks: the dispatch ladder over k_align_pairs / k_align_pairs_s
//   align_pairs_dev_on_stream  a call's launches: the main one, then the redo launches for the pairs it left flagged
//   resolve_flagged_pairs      what no fused kernel could serve, through the resident frame

// The shape of a fused-pairs launch: the grid and the static range box of the scan's geometry, the score mode and table form for
// them (resolve_score_plan -- `mode` may be NDTPSO_SCORE_EXACT; `ask` as make_plan's, the window is always dynamic here), and the
// waves of a workgroup when `n_pairs` alignments share `n_cus` compute units (0: not known, no device asked).
struct PairsShape {
  GridP g;
  WinP wn;
  ScorePlan score;
  int waves;
};
static int pairs_plan(const ndtpso_scan_geom* geom, const ndtpso_grid* grid, const ndtpso_pso_config* cfg, int mode, PlanAsk ask,
                      unsigned n_pairs, unsigned n_cus, PairsShape* out) {
  out->score = ScorePlan{false, mode == NDTPSO_SCORE_EXACT ? NDTPSO_SCORE_F64 : mode, false, Plan{}};
  out->waves = 0;
  if (!geom || geom->n_beams == 0 || !cfg || cfg->population < 1 || cfg->iterations < 0) return NDTPSO_E_ARG;
  if (make_grid(grid, &out->g) != NDTPSO_OK) return NDTPSO_E_ARG;
  const double r = (double)geom->max_range;
  out->wn = make_window(out->g, -r, r, -r, r, (int)(geom->n_beams / 3) + 1);
  ask.dynamic_window = true;
  out->score = resolve_score_plan(mode, out->g, out->wn, (int)geom->n_beams, cfg->population, ask);
  out->waves = pick_waves(cfg->population, out->score.plan.L.total, n_pairs, n_cus);
  return out->score.ok ? NDTPSO_OK : NDTPSO_E_CAPACITY;
}

int ndtpso_align_pairs_footprint(const ndtpso_scan_geom* geom, const ndtpso_grid* grid, const ndtpso_pso_config* cfg,
                                 uint32_t* lds_bytes, uint32_t* block_threads) {
  PairsShape shape;
  const int rc = pairs_plan(geom, grid, cfg, NDTPSO_SCORE_F32, PlanAsk{}, 512u, 0u, &shape);
  if (rc == NDTPSO_E_ARG) return rc;
  if (lds_bytes) *lds_bytes = (rc == NDTPSO_OK) ? (uint32_t)shape.score.plan.L.total : 0u;
  if (block_threads) *block_threads = (uint32_t)shape.waves * 64u;
  return rc;
}

int ndtpso_align_pairs_describe(const ndtpso_scan_geom* geom, const ndtpso_grid* grid, const ndtpso_pso_config* cfg,
                                int mode, uint32_t n_pairs, ndtpso_pairs_plan* out) {
  if (!out || check_mode(nullptr, mode)) return NDTPSO_E_ARG;
  // (the exact mode is described as the fp32 score's plan, whatever form the table takes: the same table forms, and the swarm
  // keeps four more arrays -- not as what a launch would fall back to)
  PlanAsk ask;
  ask.exact = mode == NDTPSO_SCORE_EXACT;
  if (ask.exact) mode = NDTPSO_SCORE_F32;
  std::memset(out, 0, sizeof(*out));
  PairsShape shape;
  const int rc = pairs_plan(geom, grid, cfg, mode, ask, n_pairs, 0u, &shape);
  if (rc == NDTPSO_E_ARG) return rc;
  const Plan& plan = shape.score.plan;
  out->block_threads = (uint32_t)shape.waves * 64u;
  out->window_w = (uint32_t)shape.wn.w;
  out->window_h = (uint32_t)shape.wn.h;
  if (rc != NDTPSO_OK) return rc;
  out->lds_bytes = (uint32_t)plan.L.total;
  out->table_form = (uint32_t)plan.path;
  out->swarm_in_hbm = (uint32_t)plan.L.swarm_global;
  out->workgroups_per_cu = (uint32_t)std::max(1, std::min(kMaxLds / plan.L.total, 16 / shape.waves));
  if (path_is_dense64(plan.path))
    out->table_bytes = (uint32_t)(plan.L.pts_off - plan.L.drec_off - kImageHeaderBytes);
  else
    out->table_bytes = (uint32_t)(plan.L.pts_off - (plan.path == 2 ? 0 : plan.L.bm_off) - (plan.path == 2 ? kCtrlBytes + kImageHeaderBytes : 0));
  return NDTPSO_OK;
}

// What one ndtpso_align_pairs_dev call aligns: every launch of it shares these (all pointers on the device but geom, grid, cfg).
struct PairsBatch {
  uint32_t n_pairs;
  const float *d_ref, *d_new;
  const ndtpso_scan_geom* geom;
  const ndtpso_grid* grid;
  const double *d_guess, *d_dev;
  const ndtpso_pso_config* cfg;
  const uint32_t* d_seeds;
  const int32_t* d_tables;
  double *d_pose, *d_cost;
  AlignStats* d_stats;  // never null: the launches hand flagged pairs on through it
};
// What one launch of a batch asks for.
struct PairsLaunch {
  PairsLaunch(int mode_, uint32_t gate_) : mode(mode_), gate(gate_) {}
  int mode;                     // NDTPSO_SCORE_F32 or NDTPSO_SCORE_F64 (the exact mode: F32 with `exact`)
  uint32_t gate;                // status bits: only the pairs that carry one of them are aligned (0: every pair, the main launch)
  bool allow_dense = true;
  bool allow_cluster = false;   // K workgroups per pair where the batch leaves compute units idle
  bool exact = false;           // the fp32 score arbitrating in fp64
  bool big_table = false;       // PlanAsk::big_table
  uint32_t* fb = nullptr;       // the pinned word that counts the pairs whose box outgrew the table
  // a redo launch on clusters: `redo_units` clusters, cluster i taking pair redo_list[1 + i] if i < redo_list[0]
  // (k_redo_list), clearing the flags `redo_mask` of the pairs it completes; E_STATE: no cluster shape for this
  const uint32_t* redo_list = nullptr;
  uint32_t redo_units = 0, redo_mask = 0;
};
struct PairsOutcome {  // the plan a launch was made with (Plan::path, Plan::shrunk); as initialised where the launch did not get to plan
  int path = 0;
  bool shrunk = false;
};
// A redo launch that cannot be made -- its form does not fit LDS: E_CAPACITY -- is no error of the call: the pairs it was for keep
// their flags, for the next launch or for the caller.  What each launch tolerates is written where it is made.
static int tolerating(int tolerated, int rc) { return rc == tolerated ? NDTPSO_OK : rc; }

static int launch_pairs(ndtpso_ctx* c, const PairsBatch& b, const PairsLaunch& l, PairsOutcome* outcome = nullptr) {
  const uint32_t n_pairs = b.n_pairs, gate = l.gate;
  const ndtpso_scan_geom* const geom = b.geom;
  const ndtpso_pso_config* const cfg = b.cfg;
  const int mode = l.mode;
  const uint32_t* const redo_list = l.redo_list;
  if (!cfg || cfg->population < 1) return fail(c, NDTPSO_E_ARG, "bad scan/grid/PSO configuration");
  // a batch smaller than the device: the idle compute units join in, K workgroups per alignment (ClusterP)
  int K = 1, cw = 4;
  const bool allow_cluster = t_plan_force.cluster >= 0 ? t_plan_force.cluster != 0 : l.allow_cluster;
  const uint32_t n_units = redo_list ? l.redo_units : n_pairs;  // alignments this launch provides for (scratch, exchange slots, grid)
  cluster_launch_k(c, cfg->population, n_units, allow_cluster && gate == 0, true, &K, &cw);
  if (redo_list && K < 2) return NDTPSO_E_STATE;  // (not an error of the call: the gated launches serve the pairs)
  PlanAsk ask;
  // (the fp64 score's dense form runs one workgroup per alignment: a cluster keeps the bitmap form)
  ask.allow_dense = l.allow_dense && !(mode == NDTPSO_SCORE_F64 && K > 1);
  ask.exact = l.exact;
  ask.big_table = l.big_table;
  PairsShape shape;
  const int rc = pairs_plan(geom, b.grid, cfg, mode, ask, n_units, (unsigned)c->n_cus, &shape);
  const GridP& g = shape.g;
  const WinP& wn = shape.wn;
  const Plan& plan = shape.score.plan;
  int waves = shape.waves;
  if (outcome) *outcome = PairsOutcome{plan.path, plan.shrunk};
  if (rc == NDTPSO_E_ARG) return fail(c, rc, "bad scan/grid/PSO configuration");
  if (rc == NDTPSO_E_CAPACITY) return redo_list ? NDTPSO_E_STATE : fail(c, rc, "scan pair working set does not fit in LDS");
  if (redo_list && plan.L.swarm_global) return NDTPSO_E_STATE;  // (a cluster keeps its swarm in LDS)
  ScanP sp;
  const double2* dirs = nullptr;
  if (int rc = make_scan(c, geom, &sp, &dirs)) return rc;
  if (K > 1) waves = cw;
  PsoP ps = make_pso(cfg, waves, mode, plan.L.swarm_global != 0);
  ClusterP cl;
  int lds_total = plan.L.total;
  size_t unit_slots = 0;
  cluster_launch_shape(c, cfg->population, K, waves, n_units, 0, redo_list, l.redo_mask, &lds_total, &ps, &cl, &unit_slots);
  if (K > 1)
    if (int rc = cluster_slots(c, (size_t)n_units * unit_slots * sizeof(uint4), &cl.xc)) return rc;
  const size_t stride = ndtpso_rand_draws(cfg);
  const size_t ws_stride = plan.L.swarm_global ? (size_t)swarm_bytes(cfg->population, true, true) : 0;
  if (ws_stride) HIP_TRY(c, c->ws.reserve(ws_stride * n_units * (size_t)K));
  // exact mode on the dense form: one fp64 table image per workgroup in HBM (bitmap of the per-alignment window, mean,
  // ab, cd), written by the table build and read by the arbitration only
  size_t ximg_stride = 0;
  if (l.exact && mode == NDTPSO_SCORE_F32 && plan.path == 2) {
    ximg_stride = (size_t)round_up(image_bytes(plan.dense_cap / 32 + 2, wn.rec_cap), 256);
    HIP_TRY(c, c->ximg.reserve(ximg_stride * n_units * (size_t)K));
  }
  unsigned char* d_ximg = ximg_stride ? (unsigned char*)c->ximg.p : nullptr;
  // a gated launch of a kernel that strides (gate_strides): eight workgroups, or twice the pairs the last gated launch of this
  // kind found flagged (its workgroup 0 leaves the count in the context's pinned feedback block, words 4 .. 7 by kind); a stale
  // or foreign count only changes how many workgroups share the flagged pairs
  uint32_t* gate_fb = nullptr;
  uint32_t gate_grid = n_pairs;
  if (gate != 0 && c->pairs_fb) {
    gate_fb = c->pairs_fb + 4 + ((mode == NDTPSO_SCORE_F64 ? 2 : 0) | (l.allow_dense ? 1 : 0));
    const uint32_t seen = __atomic_load_n(gate_fb, __ATOMIC_RELAXED);
    gate_grid = std::min<uint32_t>(n_pairs, std::max<uint32_t>(8u, 2u * seen));
    if (const char* e = std::getenv("NDTPSO_GATE_GRID")) gate_grid = std::min<uint32_t>(n_pairs, (uint32_t)std::max(1, std::atoi(e)));  // (diagnostics)
  }
  // Two items per wave (eval_pair_half, k_align_pairs<..., PAIR>): short scans with enough particles per wave.  What a pair
  // saves is around the trips (a third of a six-chunk evaluation, a tenth of a seventeen-chunk one); what it costs is at a
  // phase's end, where the waves wait for the last of units twice as long -- the fewer items a wave has per phase, the more.
  // Measured break-even, 8 waves (512 pairs, 0.5 m cells; scripts/pair_items_ab.py): 181 beams any swarm (+ 5-20 %), 361 beams
  // from 16 particles (+ 6 % there, + 15-21 % from 70), 541 beams from 30 (+ 1 %; + 6-10 % from 70), nothing at 721; fitted as
  // particles >= (5 (chunks - 3) + 1) waves / 8 for up to nine chunks.  NDTPSO_PAIR_ITEMS=0: never; NDTPSO_PAIR_MAX_BEAMS
  // (diagnostics): whatever the swarm, up to that many beams.
  const char* pair_env = std::getenv("NDTPSO_PAIR_ITEMS");
  static const int pair_max_beams = [] {
    const char* e = std::getenv("NDTPSO_PAIR_MAX_BEAMS");
    return e ? std::max(0, std::atoi(e)) : -1;
  }();
  const int pair_chunks = ((int)geom->n_beams + 63) / 64;
  const bool pair_pays = pair_max_beams >= 0 ? (int)geom->n_beams <= pair_max_beams
                                             : (pair_chunks <= 9 && cfg->population * 8 >= (5 * (pair_chunks - 3) + 1) * waves);
  const bool pair_items = t_plan_force.pair >= 0 ? t_plan_force.pair != 0 : (!(pair_env && pair_env[0] == '0') && pair_pays);
// what every form of the launch hands its kernel (k_align_pairs; k_align_pairs_s takes n_pairs and gate_fb behind them)
#define PAIRS_KERNEL_ARGS                                                                                          \
  b.d_ref, b.d_new, sp, g, wn, plan.L, plan.dn, plan.dense_cap, ps, b.d_guess, b.d_dev, b.d_seeds, b.d_tables, stride, \
  (unsigned char*)c->ws.p, ws_stride, b.d_pose, b.d_cost, b.d_stats, gate, cl, dirs, d_ximg, ximg_stride, l.fb
// the three forms: a gated launch of a kernel that strides, two items per wave, one workgroup (or cluster) per pair
#define LAUNCH_PAIRS_CANSB(MODE, PATH, CL, ARB, NOCLIP, SWARM, BOX)                                                \
  do {                                                                                                             \
    if (gate == 0 && !redo_list) t_last_launch = launch_code(MODE == kScoreF64, PATH, CL, ARB, NOCLIP, SWARM, BOX, true, pair_items && pair_items_kernel<MODE, PATH, CL, NOCLIP, SWARM, BOX>()); \
    if (gate != 0 && gate_strides<MODE, PATH, CL>() && gate_fb) {                                                  \
      launch_pairs_gated<MODE, PATH, CL, ARB, NOCLIP, SWARM, BOX>(dim3(gate_grid), dim3(waves * 64), lds_total, c->stream, \
                                                                  PAIRS_KERNEL_ARGS, n_pairs, gate_fb);            \
    } else if (pair_items && gate == 0 && pair_items_kernel<MODE, PATH, CL, NOCLIP, SWARM, BOX>()) {               \
      launch_pairs_pair_items<MODE, PATH, CL, ARB, NOCLIP, SWARM, BOX>(dim3(n_pairs), dim3(waves * 64), lds_total, c->stream, \
                                                                       PAIRS_KERNEL_ARGS);                         \
    } else {                                                                                                       \
      hipLaunchKernelGGL((k_align_pairs<MODE, PATH, CL, ARB, NOCLIP, SWARM, BOX>), dim3(CL ? cluster_grid(cl) : n_pairs), \
                         dim3(waves * 64), lds_total, c->stream, PAIRS_KERNEL_ARGS);                               \
    }                                                                                                              \
  } while (0)
// (a table much smaller than the static window -- Plan::boxy -- and the swarm in LDS: the copies that carry the box guard)
#define LAUNCH_PAIRS_CANS(MODE, PATH, CL, ARB, NOCLIP, SWARM)                                                      \
  do {                                                                                                             \
    if constexpr ((PATH == 2 || PATH == 3) && !CL && SWARM != 1) {                                                 \
      if (plan.boxy && !plan.L.swarm_global) LAUNCH_PAIRS_CANSB(MODE, PATH, CL, ARB, NOCLIP, SWARM, true);         \
      else LAUNCH_PAIRS_CANSB(MODE, PATH, CL, ARB, NOCLIP, SWARM, false);                                          \
    } else {                                                                                                       \
      LAUNCH_PAIRS_CANSB(MODE, PATH, CL, ARB, NOCLIP, SWARM, false);                                               \
    }                                                                                                              \
  } while (0)
// (the kernels without clipping trips exist per home of the swarm, the others carry both copies of the PSO)
#define LAUNCH_PAIRS_CAN(MODE, PATH, CL, ARB, NOCLIP)                                    \
  do {                                                                                   \
    if constexpr (NOCLIP) {                                                              \
      if (plan.L.swarm_global) LAUNCH_PAIRS_CANS(MODE, PATH, CL, ARB, NOCLIP, (NOCLIP ? 1 : 2)); \
      else LAUNCH_PAIRS_CANS(MODE, PATH, CL, ARB, NOCLIP, (NOCLIP ? 0 : 2));             \
    } else {                                                                             \
      LAUNCH_PAIRS_CANS(MODE, PATH, CL, ARB, NOCLIP, 2);                                 \
    }                                                                                    \
  } while (0)
// the dense-form kernels on one workgroup per alignment come in a variant without the frame-clipping trips, for grids
// whose cells do not overhang the frame (DenseP::clip == 0: the usual case) -- less code inlined, better registers:
// + 3 % in both the fp32 and the exact mode.  (Dropping the copy of the PSO that keeps its swarm in HBM as well took the
// fp32 kernel to 0 spills and + 0.5 %, the exact one from 61 to 36 spills and - 2 %: left in.)
#define LAUNCH_PAIRS_CA(MODE, PATH, CL, ARB)                                              \
  do {                                                                                    \
    if ((PATH == 3 || PATH == 2) && !CL && !plan.dn.clip) LAUNCH_PAIRS_CAN(MODE, PATH, CL, ARB, ((PATH == 3 || PATH == 2) && !CL)); \
    else LAUNCH_PAIRS_CAN(MODE, PATH, CL, ARB, false);                                    \
  } while (0)
#define LAUNCH_PAIRS_C(MODE, PATH, CL) LAUNCH_PAIRS_CA(MODE, PATH, CL, false)
#define LAUNCH_PAIRS(MODE, PATH) \
  do { if (K > 1) LAUNCH_PAIRS_C(MODE, PATH, true); else LAUNCH_PAIRS_C(MODE, PATH, false); } while (0)
#define LAUNCH_PAIRS_X(PATH) \
  do { if (K > 1) LAUNCH_PAIRS_CA(kScoreF32, PATH, true, true); else LAUNCH_PAIRS_CA(kScoreF32, PATH, false, true); } while (0)
  // dense form: when every record lies below 64 KB of LDS the table entries can be the records' byte addresses
  // (PATH 3: one shift less per point in the score loop); NDTPSO_BYTE_ENTRIES=0 keeps the general form
  static const bool allow_byte_entries = [] {
    const char* e = std::getenv("NDTPSO_BYTE_ENTRIES");
    return !(e && e[0] == '0');
  }();
  const bool byte_entries = plan.path == 2 && allow_byte_entries && t_plan_force.byte_entries != 0 &&
                            plan.dn.rec_off + dense_rec_bytes(wn.rec_cap + 1) <= 65536;
  if (d_ximg) {  // exact mode on the dense form
    if (byte_entries) LAUNCH_PAIRS_X(3); else LAUNCH_PAIRS_X(2);
  } else if (mode == NDTPSO_SCORE_F32) {
    if (byte_entries) LAUNCH_PAIRS(kScoreF32, 3); else if (plan.path == 2) LAUNCH_PAIRS(kScoreF32, 2); else if (plan.path == 1) LAUNCH_PAIRS(kScoreF32, 1); else LAUNCH_PAIRS(kScoreF32, 0);
  } else {
    if (plan.path == 9) { if (plan.boxy) LAUNCH_PAIRS_CANSB(kScoreF64, 9, false, false, false, 2, true); else LAUNCH_PAIRS_CANSB(kScoreF64, 9, false, false, false, 2, false); }
    else if (plan.path == 8) { if (plan.boxy) LAUNCH_PAIRS_CANSB(kScoreF64, 8, false, false, false, 2, true); else LAUNCH_PAIRS_CANSB(kScoreF64, 8, false, false, false, 2, false); }
    else if (plan.path == 1) LAUNCH_PAIRS(kScoreF64, 1); else LAUNCH_PAIRS(kScoreF64, 0);
  }
#undef LAUNCH_PAIRS
#undef LAUNCH_PAIRS_X
#undef LAUNCH_PAIRS_C
#undef LAUNCH_PAIRS_CA
#undef LAUNCH_PAIRS_CAN
#undef LAUNCH_PAIRS_CANS
#undef LAUNCH_PAIRS_CANSB
#undef PAIRS_KERNEL_ARGS
  HIP_TRY(c, hipGetLastError());
  return NDTPSO_OK;
}

static int align_pairs_dev_on_stream(ndtpso_ctx* c, uint32_t n_pairs, const float* d_ref, const float* d_new,
                                     const ndtpso_scan_geom* geom, const ndtpso_grid* grid, const double* d_guess,
                                     const double* d_dev, const ndtpso_pso_config* cfg, const uint32_t* d_seeds,
                                     const int32_t* d_tables, int mode, double* d_pose, double* d_cost,
                                     ndtpso_align_stats* d_stats);

int ndtpso_align_pairs_dev(ndtpso_ctx* c, uint32_t n_pairs, const float* d_ref, const float* d_new,
                           const ndtpso_scan_geom* geom, const ndtpso_grid* grid, const double* d_guess,
                           const double* d_dev, const ndtpso_pso_config* cfg, const uint32_t* d_seeds,
                           const int32_t* d_tables, int mode, double* d_pose, double* d_cost,
                           ndtpso_align_stats* d_stats) {
  if (!c) return NDTPSO_E_ARG;
  if (int rc = exact_mode_resolve(c, &mode)) return rc;
  // one batch at a time (the default), or a batch too small to fill the device (those run as clusters of workgroups
  // with per-context counters): on the context's stream, behind whatever is still in flight
  if (c->pipe_depth < 2 || n_pairs * 2u <= (uint32_t)c->n_cus) {
    if (c->pipe_depth > 1)
      if (int rc = ndtpso_pipeline_flush(c, 0)) return rc;
    return align_pairs_dev_on_stream(c, n_pairs, d_ref, d_new, geom, grid, d_guess, d_dev, cfg, d_seeds, d_tables, mode,
                                     d_pose, d_cost, d_stats);
  }
  HIP_TRY(c, hipSetDevice(c->device));
  ndtpso_ctx::PipeLane& lane = c->lanes[c->pipe_calls % (unsigned)c->pipe_depth];
  // the lane's previous call is ordered before this one by the lane's stream; the inputs by an event of the caller's
  HIP_TRY(c, hipEventRecord(c->pipe_in, c->stream));
  HIP_TRY(c, hipStreamWaitEvent(lane.stream, c->pipe_in, 0));
  hipStream_t caller = c->stream;
  c->stream = lane.stream;
  std::swap(c->ws, lane.ws);
  std::swap(c->gate, lane.gate);
  std::swap(c->ximg, lane.ximg);
  const int rc = align_pairs_dev_on_stream(c, n_pairs, d_ref, d_new, geom, grid, d_guess, d_dev, cfg, d_seeds, d_tables,
                                           mode, d_pose, d_cost, d_stats);
  std::swap(c->ws, lane.ws);
  std::swap(c->gate, lane.gate);
  std::swap(c->ximg, lane.ximg);
  c->stream = caller;
  if (rc != NDTPSO_OK) return rc;
  HIP_TRY(c, hipEventRecord(lane.done, lane.stream));
  lane.pending = true;
  lane.ticket = c->pipe_calls++;
  return NDTPSO_OK;
}

static int align_pairs_dev_on_stream(ndtpso_ctx* c, uint32_t n_pairs, const float* d_ref, const float* d_new,
                                     const ndtpso_scan_geom* geom, const ndtpso_grid* grid, const double* d_guess,
                                     const double* d_dev, const ndtpso_pso_config* cfg, const uint32_t* d_seeds,
                                     const int32_t* d_tables, int mode, double* d_pose, double* d_cost,
                                     ndtpso_align_stats* d_stats) {
  if (!c || !d_ref || !d_new || !d_guess || !d_dev || !d_pose || (!d_seeds && !d_tables))
    return fail(c, NDTPSO_E_ARG, "null argument");
  if (int rc = check_mode(c, mode)) return rc;
  if (n_pairs == 0) return NDTPSO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  AlignStats* st = reinterpret_cast<AlignStats*>(d_stats);
  if (!st) {  // the fp32 pass reports underflowed alignments through the stats block: keep one internally
    HIP_TRY(c, c->gate.reserve(sizeof(AlignStats) * (size_t)n_pairs));
    st = reinterpret_cast<AlignStats*>(c->gate.p);
  }
  const PairsBatch batch{n_pairs, d_ref, d_new, geom, grid, d_guess, d_dev, cfg, d_seeds, d_tables, d_pose, d_cost, st};
  const bool small_batch = n_pairs * 2u <= (uint32_t)c->n_cus;
  HIP_TRY(c, hipMemsetAsync(st, 0, sizeof(AlignStats) * (size_t)n_pairs, c->stream));
  // exact mode: the fp32-score kernel arbitrating in fp64 (dense form) -- or, where the dense form is not available,
  // the fp64 score itself (resolve_score_plan, for the pairs' own plan); flagged alignments are redone by the fp64-score kernel
  bool exact = false;
  if (mode == NDTPSO_SCORE_EXACT) {
    PairsShape asked;  // (arguments it refuses are the main launch's to report)
    pairs_plan(geom, grid, cfg, mode, PlanAsk{}, n_pairs, (unsigned)c->n_cus, &asked);
    mode = asked.score.mode;
    exact = asked.score.arbitrates;
  }
  // (what the previous call of this configuration reported: see ndtpso_ctx::pairs_fb)
  if (!c->pairs_fb) {
    HIP_TRY(c, hipHostMalloc((void**)&c->pairs_fb, 64, hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(c->pairs_fb, 0, 64);
  }
  uint32_t last_overflow = 0;  // pairs of the previous call (same configuration) whose box outgrew the two-per-CU table
  {
    uint64_t key = 1469598103934665603ull;
    const uint64_t key_before = c->fb_key;
    auto mix = [&key](uint64_t v) { key = (key ^ v) * 1099511628211ull; };
    mix(geom->n_beams), mix((uint64_t)(geom->max_range * 1024.f)), mix(grid->width), mix(grid->height), mix((uint64_t)(grid->cell_side * 65536.));
    mix((uint64_t)cfg->population), mix((uint64_t)mode), mix(exact ? 1 : 0);
    const uint32_t now = __atomic_load_n(c->pairs_fb, __ATOMIC_RELAXED);
    // (the gated largest-table launch below is issued only where tables have overflowed lately -- or nothing is known yet:
    // a batch of 512 workgroups that all leave at once still costs the device 4 us, and the benchmark's shape never needs it.
    // An overflow that comes as a surprise is still served, by the slower launches further down, and switches it on.)
    c->fb_overflowed = key != c->fb_key || now != c->fb_seen || c->fb_overflowed_calls > 0;
    if (key == c->fb_key && now != c->fb_seen) c->fb_overflowed_calls = 16;  // keep it on for the next calls
    else if (c->fb_overflowed_calls > 0) --c->fb_overflowed_calls;
    if (key != c->fb_key) {
      c->fb_key = key;
      c->fb_big_first = false;
      c->fb_big_calls = 0;
      c->fb_overflowed_calls = 1;
    } else if (!c->fb_big_first && c->fb_last_pairs && (uint64_t)(now - c->fb_seen) * 4u > c->fb_last_pairs) {
      c->fb_big_first = true;
      static const bool log_plan = std::getenv("NDTPSO_LOG_PLAN") != nullptr;  // diagnostics
      if (log_plan)
        std::fprintf(stderr, "ndtpso: %u of the last call's %u pairs outgrew the two-per-CU cell table: largest table first from now on\n",
                     now - c->fb_seen, c->fb_last_pairs);
    }
    // ... and not for ever: one burst of large rooms must not pin the configuration to one workgroup per compute unit for the
    // life of the context -- every 64 calls the two-per-CU table is tried again (and, if a quarter of the pairs still
    // outgrows it, the next call is back to the largest table)
    if (c->fb_big_first && ++c->fb_big_calls >= 64) {
      c->fb_big_first = false;
      c->fb_big_calls = 0;
    }
    last_overflow = (key == key_before) ? now - c->fb_seen : 0u;
    c->fb_seen = now;
    c->fb_last_pairs = n_pairs;
  }
  const bool big_first = c->fb_big_first && !small_batch;
  // (the fp64 score's bitmap form, gated: where either branch below ends)
  PairsLaunch bitmap64(NDTPSO_SCORE_F64, kStatusNeedsBitmap);
  bitmap64.allow_dense = false;
  PairsLaunch main_launch(mode, 0u);
  main_launch.allow_cluster = small_batch;
  main_launch.exact = exact;
  main_launch.big_table = big_first;
  main_launch.fb = big_first ? nullptr : c->pairs_fb;
  PairsOutcome planned;
  if (int rc = launch_pairs(c, batch, main_launch, &planned)) return rc;
  const int path = planned.path;
  const bool shrunk = planned.shrunk && !big_first;  // (the largest table first: nothing larger to fall back to)
  if (no_redo_requested()) return NDTPSO_OK;  // diagnostics only
  // A FEW flagged pairs in a batch that fills the device (1081 beams at 0.25 m: 7 rooms of 512 outgrow the table): on one
  // workgroup each, behind the main launch, they took as long again as the whole batch (fp64 score: 2.8 ms after 5.1 ms).  They
  // run as CLUSTERS instead -- the fp64 score on K workgroups per pair, as a batch too small for the device does -- through a
  // list a one-wave kernel makes of them: 0.9 ms.  Tried only where the previous calls of the configuration saw flagged pairs
  // (the list's own count, the striding redo's count, the main launch's overflow count: pinned words), for up to 32 of them,
  // with one batch at a time in the context (two in flight: the other lane's workgroups hold the compute units a cluster needs
  // together).  Whatever it does not serve -- pairs beyond the list, a cluster that gave up -- keeps its flags and goes through
  // the gated launches below as before.  Results: the fp64 score's, whichever form computes them.  NDTPSO_REDO_CLUSTERS=0: off.
  const char* redo_env = std::getenv("NDTPSO_REDO_CLUSTERS");
  if (!(redo_env && redo_env[0] == '0') && !small_batch && c->pipe_depth < 2 && (exact || mode == NDTPSO_SCORE_F64)) {
    const uint32_t mask = exact ? (kStatusNeedsF64 | kStatusNeedsBitmap) : kStatusNeedsBitmap;
    uint32_t* seen_w = c->pairs_fb + 8 + (exact ? 1 : 0);
    const uint32_t seen = std::max(std::max(__atomic_load_n(seen_w, __ATOMIC_RELAXED), __atomic_load_n(c->pairs_fb + 7, __ATOMIC_RELAXED)),
                                   (path == 2 || path >= 8) ? last_overflow : 0u);
    if (seen >= 1u && seen <= 32u) {
      const uint32_t cap = std::min<uint32_t>(n_pairs, std::max<uint32_t>(8u, 2u * seen));
      HIP_TRY(c, c->redo_list.reserve((size_t)(1u + 64u) * sizeof(uint32_t)));
      uint32_t* list = (uint32_t*)c->redo_list.p;
      hipLaunchKernelGGL(k_redo_list, dim3(1), dim3(kWave), 0, c->stream, (const AlignStats*)st, n_pairs, mask, list, cap, seen_w);
      HIP_TRY(c, hipGetLastError());
      PairsLaunch on_clusters(NDTPSO_SCORE_F64, 0u);
      on_clusters.allow_cluster = true;
      on_clusters.redo_list = list;
      on_clusters.redo_units = cap;
      on_clusters.redo_mask = mask;
      const int rc = launch_pairs(c, batch, on_clusters);
      if (rc == NDTPSO_OK) g_redo_cluster_launches.fetch_add(1, std::memory_order_relaxed);
      else if (rc != NDTPSO_E_STATE) return rc;  // (E_STATE: no cluster shape for these -- the gated launches below serve them)
    }
  }
  // Gated redo launches (every workgroup whose alignment is not flagged exits on its first instruction).  First of all: the
  // dense forms size their cell table so that two workgroups share a compute unit; an alignment whose box -- scan A's
  // occupied cells -- outgrew that table gets the same kernel again with the largest table a workgroup can hold (0.25 m cells,
  // a room seen at an angle: 7 of 512 pairs; 1441 beams at 0.3 m: 370 of 512), before anything slower is considered
  if (shrunk && c->fb_overflowed && (path == 2 || path >= 8) && !small_batch) {
    PairsLaunch largest_table(mode, kStatusNeedsBitmap);
    largest_table.exact = exact;
    largest_table.big_table = true;
    if (int rc = tolerating(NDTPSO_E_CAPACITY, launch_pairs(c, batch, largest_table))) return rc;
  }
  PairsOutcome alone;
  if (small_batch) {  // a cluster that was not co-resident gave up (bounded wait): those alignments on one workgroup each
    // (on one workgroup the fp64 score may take its dense form -- a cluster keeps the bitmap form --, which hands an alignment
    // whose box outgrows its table on to the bitmap form: the gated launch below must then be issued for THIS launch's path too)
    PairsLaunch one_workgroup(mode, kStatusClusterTimeout);
    one_workgroup.exact = exact;
    if (int rc = launch_pairs(c, batch, one_workgroup, &alone)) return rc;  // (no code tolerated: the main launch's forms, on one workgroup)
  }
  if (mode != NDTPSO_SCORE_F32) {
    // fp64 score on the dense table (path 8 / 9): an occupied box that outgrew the provisioned table, or a table holding a
    // cell whose exponents the spelt-out exponential must not be trusted with -> the bitmap form, gated
    if (path >= 8 || alone.path >= 8) return tolerating(NDTPSO_E_CAPACITY, launch_pairs(c, batch, bitmap64));
    return NDTPSO_OK;
  }
  // Gated redo launches (every workgroup whose alignment is not flagged exits on its first instruction):
  //  - dense form only: alignments whose occupied box exceeded the provisioned cell table -> bitmap form;
  //  - alignments whose fp32 costs fell in the underflow regime (degenerate overlap) -> fp64 score.
  // If a redo form does not fit in LDS its flag simply stays set in the stats block.
  // (exact mode: the bitmap form cannot arbitrate, so both kinds of flagged alignment go to the fp64-score kernel, in one launch)
  if (path == 2 && !exact) {
    PairsLaunch bitmap32(NDTPSO_SCORE_F32, kStatusNeedsBitmap);
    bitmap32.allow_dense = false;
    if (int rc = tolerating(NDTPSO_E_CAPACITY, launch_pairs(c, batch, bitmap32))) return rc;
  }
  // (the fp64 score's dense form first -- it sets kStatusNeedsBitmap itself where it cannot run --, the bitmap form for what is left)
  const PairsLaunch score64(NDTPSO_SCORE_F64, exact ? (kStatusNeedsF64 | kStatusNeedsBitmap) : kStatusNeedsF64);
  PairsOutcome redone;
  if (int rc = tolerating(NDTPSO_E_CAPACITY, launch_pairs(c, batch, score64, &redone))) return rc;
  if (redone.path >= 8) return tolerating(NDTPSO_E_CAPACITY, launch_pairs(c, batch, bitmap64));
  return NDTPSO_OK;
}

// What the fused kernels could not serve -- an occupied box beyond the largest table a workgroup holds whose bitmap form does
// not fit LDS either (cells of 0.125 m in a 60 m frame: a dozen pairs in 600) -- comes back flagged.  An entry that has the
// inputs on the host and has just synchronised (ndtpso_align_pairs, ndtpso_align_pairs_sharded) sends those pairs, one by one,
// through the RESIDENT frame (ndtpso_map_*: scan A inserted into a frame in HBM and built there, the alignment reading the
// packed table from its HBM image where LDS cannot hold it), whose results are the fused kernels' bit for bit.  One frame per
// call, cleared between pairs; nothing of this is allocated unless a pair needs it.  A frame the resident path cannot hold
// either -- a million cells -- leaves its pairs flagged, as the kernels did: the other pairs' results stand.
// (The asynchronous entries on device buffers leave the flag to their caller: NDTPSO_STATUS_FLAGS.)
static int resolve_flagged_pairs(ndtpso_ctx* c, size_t B, const float* ref_ranges, const float* new_ranges, const ndtpso_scan_geom* geom,
                                 const ndtpso_grid* grid, const double* guess, const double* deviation, const ndtpso_pso_config* cfg,
                                 const uint32_t* seeds, const int32_t* rand_tables, int mode, double* out_pose, double* out_cost,
                                 AlignStats* hs) {
  const size_t nb = geom->n_beams, n_draw = ndtpso_rand_draws(cfg);
  if (no_redo_requested()) return NDTPSO_OK;  // (diagnostics: what the main launch alone left flagged)
  ndtpso_map* fb_map = nullptr;
  ndtpso_points *fb_a = nullptr, *fb_b = nullptr;
  int fb_rc = NDTPSO_OK;
  for (size_t b = 0; b < B && fb_rc == NDTPSO_OK; ++b) {
    if (!(hs[b].status & (kStatusNeedsBitmap | kStatusNeedsF64 | kStatusClusterTimeout))) continue;
    const double zero3[3] = {0., 0., 0.};
    if (!fb_map) {
      fb_rc = ndtpso_map_create(c, grid, 0., (uint64_t)std::max<size_t>(nb, 4096) * 16 * 64, &fb_map);
      if (fb_rc == NDTPSO_OK) fb_rc = ndtpso_points_create(c, (uint32_t)nb, &fb_a);
      if (fb_rc == NDTPSO_OK) fb_rc = ndtpso_points_create(c, (uint32_t)nb, &fb_b);
    } else {
      fb_rc = ndtpso_map_clear(fb_map);
    }
    // reference frame <- scan A at identity; the frame being matched is a one-cell frame of the same size, its list the points
    // inside it (ndtpso_slam_node.cpp:229-230: `clip`)
    if (fb_rc == NDTPSO_OK) fb_rc = ndtpso_points_load_scan(fb_a, ref_ranges + b * nb, geom, zero3, grid, 0);
    if (fb_rc == NDTPSO_OK) fb_rc = ndtpso_map_insert(fb_map, fb_a, nullptr);
    if (fb_rc == NDTPSO_OK) fb_rc = ndtpso_map_build(fb_map);
    if (fb_rc == NDTPSO_OK) fb_rc = ndtpso_points_load_scan(fb_b, new_ranges + b * nb, geom, zero3, grid, 0);
    double pose[3] = {0., 0., 0.}, cost = 0.;
    ndtpso_align_stats st1;
    if (fb_rc == NDTPSO_OK)
      fb_rc = ndtpso_map_align(fb_map, fb_b, guess + 3 * b, deviation + 3 * b, cfg, seeds ? seeds[b] : 0u,
                               rand_tables ? rand_tables + b * n_draw : nullptr, mode, pose, &cost, &st1);
    if (fb_rc != NDTPSO_OK) break;
    std::memcpy(out_pose + 3 * b, pose, sizeof(pose));
    if (out_cost) out_cost[b] = cost;
    std::memcpy(&hs[b], &st1, sizeof(AlignStats));
  }
  if (fb_a) ndtpso_points_destroy(fb_a);
  if (fb_b) ndtpso_points_destroy(fb_b);
  if (fb_map) ndtpso_map_destroy(fb_map);
  return (fb_rc != NDTPSO_OK && fb_rc != NDTPSO_E_CAPACITY) ? fb_rc : NDTPSO_OK;
}

int ndtpso_align_pairs(ndtpso_ctx* c, uint32_t n_pairs, const float* ref_ranges, const float* new_ranges,
                       const ndtpso_scan_geom* geom, const ndtpso_grid* grid, const double* guess,
                       const double* deviation, const ndtpso_pso_config* cfg, const uint32_t* seeds,
                       const int32_t* rand_tables, int mode, double* out_pose, double* out_cost,
                       ndtpso_align_stats* stats) {
  if (!c || !ref_ranges || !new_ranges || !geom || !guess || !deviation || !out_pose || (!seeds && !rand_tables))
    return fail(c, NDTPSO_E_ARG, "null argument");
  if (int rc = check_pso(c, cfg)) return rc;
  if (n_pairs == 0) return NDTPSO_OK;
  if (int rc = exact_mode_resolve(c, &mode)) return rc;  // (before anything is staged in the context's buffers)
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t B = n_pairs, nb = geom->n_beams, n_draw = ndtpso_rand_draws(cfg);
  HIP_TRY(c, c->ranges.reserve(B * nb * 4));
  HIP_TRY(c, c->ranges2.reserve(B * nb * 4));
  HIP_TRY(c, c->poses.reserve(B * 48));
  HIP_TRY(c, c->out.reserve(B * (32 + sizeof(AlignStats))));
  HIP_TRY(c, c->seeds.reserve(B * 4));
  if (rand_tables) HIP_TRY(c, c->table.reserve(B * n_draw * 4));
  HIP_TRY(c, hipMemcpyAsync(c->ranges.p, ref_ranges, B * nb * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->ranges2.p, new_ranges, B * nb * 4, hipMemcpyHostToDevice, c->stream));
  double* d_guess = (double*)c->poses.p;
  double* d_dev = d_guess + 3 * B;
  HIP_TRY(c, hipMemcpyAsync(d_guess, guess, B * 24, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(d_dev, deviation, B * 24, hipMemcpyHostToDevice, c->stream));
  if (seeds) HIP_TRY(c, hipMemcpyAsync(c->seeds.p, seeds, B * 4, hipMemcpyHostToDevice, c->stream));
  if (rand_tables) HIP_TRY(c, hipMemcpyAsync(c->table.p, rand_tables, B * n_draw * 4, hipMemcpyHostToDevice, c->stream));
  double* d_pose = (double*)c->out.p;
  double* d_cost = d_pose + 3 * B;
  ndtpso_align_stats* d_stats = reinterpret_cast<ndtpso_align_stats*>(d_cost + B);
  HIP_TRY(c, hipMemsetAsync(c->out.p, 0, B * (32 + sizeof(AlignStats)), c->stream));
  const int rc = ndtpso_align_pairs_dev(c, n_pairs, (const float*)c->ranges.p, (const float*)c->ranges2.p, geom, grid,
                                        d_guess, d_dev, cfg, seeds ? (const uint32_t*)c->seeds.p : nullptr,
                                        rand_tables ? (const int32_t*)c->table.p : nullptr, mode, d_pose, d_cost,
                                        d_stats);
  if (rc != NDTPSO_OK) return rc;
  // with batches in flight (ndtpso_set_pipeline_depth) the launch went to a lane's stream: the copies below and the
  // next call's uploads into the same staging buffers must come behind it
  if (int frc = ndtpso_pipeline_flush(c, 0)) return frc;
  HIP_TRY(c, hipMemcpyAsync(out_pose, d_pose, B * 24, hipMemcpyDeviceToHost, c->stream));
  if (out_cost) HIP_TRY(c, hipMemcpyAsync(out_cost, d_cost, B * 8, hipMemcpyDeviceToHost, c->stream));
  std::vector<AlignStats> own_stats;
  AlignStats* hs = reinterpret_cast<AlignStats*>(stats);
  if (!hs) {
    own_stats.resize(B);
    hs = own_stats.data();
  }
  HIP_TRY(c, hipMemcpyAsync(hs, d_stats, B * sizeof(AlignStats), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (int rc = resolve_flagged_pairs(c, B, ref_ranges, new_ranges, geom, grid, guess, deviation, cfg, seeds, rand_tables, mode, out_pose,
                                     out_cost, hs))
    return rc;
  return NDTPSO_OK;
}
