// ndtpso_map_batch.inc -- ndtpso_map_align_batch: several ndtpso_map_align calls of one context in one launch (k_align_jobs).
// Included by ndtpso_map.inc behind ndtpso_map_align (whose path a lone or flagged job takes).

namespace {

constexpr size_t kJobSlotBytes = 128;  // a job's pinned result slot: [pose, cost | AlignStats | the job's number] (result_of)
constexpr uint32_t kLaunchJobForm = 1u << 13;  // t_last_launch: the instantiation was k_align_jobs' (launch_code's other bits as k_align's)

struct BatchMap {  // a distinct map of a call
  ndtpso_map* m;
  int rc;             // of its preparation: every job on it inherits a failure
  bool late;          // launched behind a speculative build whose header the host has not seen (map_late_bound)
  bool batched;       // at least one of its jobs is in a launch
  WinP wn;            // the window its jobs are planned with: the header's, or the late path's upper bound
};
struct BatchJob {
  int map;            // index into the call's distinct maps
  int kind;           // -1: the single path; 0 fp32 score, 1 fp32 score arbitrating, 2 fp64 score
  Plan plan;
  uint32_t n;         // the scan's capacity (its count lives on the device)
  int spec_off;       // ClusterP::spec_off behind this job's layout
  uint32_t seq;
};
struct BatchGroup {   // the jobs of one launch: one kernel instantiation
  int kind;
  std::vector<uint32_t> jobs;
  int K, cw, waves, lds_total;
  PsoP ps;
  ClusterP cl;
  size_t first;       // its first job's place among the call's batched jobs (descriptors, result slots, scratch)
  size_t xc_off;      // its exchange slots within c->cluster_xc, in uint4
};

// which job kernel, if any, runs an alignment of `mode` against a table of window `wn`: -1 none (the single path)
static int batch_plan_job(int mode, const GridP& g, const WinP& wn, uint32_t n, const ndtpso_pso_config* cfg, Plan* plan) {
  const ScorePlan resolved = resolve_score_plan(mode, g, wn, std::max<int>((int)n, 1), cfg->population, prebuilt_table_ask());  // (as align_once)
  *plan = resolved.plan;
  // the job kernels exist for the swarm in LDS, and for two table forms: the fp32 score's dense form (the other forms, the table
  // image in HBM: the single path) and the fp64 score's bitmap form on cells of a power of two
  if (!resolved.ok || plan->L.swarm_global) return -1;
  if (resolved.mode == NDTPSO_SCORE_F32) return plan->path == 2 ? (resolved.arbitrates ? 1 : 0) : -1;
  return plan->path == 1 ? 2 : -1;
}

static void batch_launch_kernel(ndtpso_ctx* c, const BatchGroup& gr, const AlignJob* d_jobs, int table_vec) {
  const bool f64 = gr.kind == 2, cluster = gr.K > 1;
  t_last_launch = launch_code(f64, f64 ? 1 : 2, cluster, gr.kind == 1, false, 0, false, false) | kLaunchJobForm;
  align_jobs_launch(gr.kind, cluster, cluster ? cluster_grid(gr.cl) : (unsigned)gr.jobs.size(), (unsigned)gr.waves * 64u, gr.lds_total,
                    c->stream, d_jobs, gr.ps, gr.cl, table_vec);
}

static int batch_single(ndtpso_map_align_job& j, const ndtpso_pso_config* cfg, int mode) {
  j.route = 0;
  j.rc = ndtpso_map_align(j.map, j.new_points, j.guess, j.deviation, cfg, j.seed, j.rand_table, mode, j.pose,
                          (j.flags & 1u) ? &j.cost : nullptr, &j.stats);
  return j.rc;
}

}  // namespace

extern "C" int ndtpso_map_align_batch(ndtpso_ctx* c, ndtpso_map_align_job* jobs, uint32_t n_jobs, const ndtpso_pso_config* cfg, int mode) {
  if (!c) return NDTPSO_E_ARG;
  if (!jobs || n_jobs == 0) return fail(c, NDTPSO_E_ARG, "no jobs");
  for (uint32_t i = 0; i < n_jobs; ++i) {
    if (!jobs[i].map || !jobs[i].new_points) return fail(c, NDTPSO_E_ARG, "null argument");
    if (jobs[i].map->ctx != c || jobs[i].new_points->ctx != c) return fail(c, NDTPSO_E_ARG, "a map or scan of another context");
  }
  if (int rc = check_mode(c, mode)) return rc;
  if (int rc = check_pso(c, cfg)) return rc;
  for (uint32_t i = 0; i < n_jobs; ++i) {
    ndtpso_map_align_job& j = jobs[i];
    j.pose[0] = j.pose[1] = j.pose[2] = j.cost = 0.;
    std::memset(&j.stats, 0, sizeof(j.stats));
    j.rc = NDTPSO_OK;
    j.route = 0;
  }
  if (n_jobs == 1) return batch_single(jobs[0], cfg, mode);  // a lone alignment: exactly ndtpso_map_align
  const int asked = mode;  // what a job that runs alone is asked for (ndtpso_map_align resolves it itself)
  if (int rc = exact_mode_resolve(c, &mode)) return rc;
  if (int rc = exact_jobs_resolve(c, asked, &mode)) return rc;
  HIP_TRY(c, hipSetDevice(c->device));

  // ---- every distinct map once -----------------------------------------------------------------------------------------
  std::vector<BatchMap> maps;
  std::vector<BatchJob> bj(n_jobs);
  for (uint32_t i = 0; i < n_jobs; ++i) {
    int at = -1;
    for (size_t k = 0; k < maps.size() && at < 0; ++k)
      if (maps[k].m == jobs[i].map) at = (int)k;
    if (at < 0) {
      at = (int)maps.size();
      maps.push_back(BatchMap{jobs[i].map, NDTPSO_OK, false, false, WinP{}});
    }
    bj[i].map = at;
    bj[i].kind = -1;
    bj[i].n = std::max<uint32_t>(jobs[i].new_points->n_upper, 1u);
    bj[i].spec_off = -1;
    bj[i].seq = 0;
  }
  for (size_t k = 0; k < maps.size(); ++k) {
    BatchMap& bm = maps[k];
    ndtpso_map* m = bm.m;
    if (!m->spec && !m->built) {  // cost_function's lazy build, core.cpp:27-28
      if ((bm.rc = map_enqueue_build(m)) != NDTPSO_OK) continue;
    }
    // late window binding, only if every job on the map has a dense-form job kernel
    WinP ub;
    if (map_late_bound(m, mode, &ub)) {
      bool all_dense = true;
      for (uint32_t i = 0; i < n_jobs && all_dense; ++i) {
        if (bj[i].map != (int)k) continue;
        Plan probe;
        const int kind = batch_plan_job(mode, m->p.g, ub, bj[i].n, cfg, &probe);
        all_dense = (kind == 0 || kind == 1) && probe.path == 2;
      }
      if (all_dense) {
        bm.late = true;
        bm.wn = ub;
        continue;
      }
    }
    if ((bm.rc = map_await_header(m)) != NDTPSO_OK) continue;
    bm.wn = window_of(m->host_hdr);
  }

  // ---- which jobs share a launch ---------------------------------------------------------------------------------------
  std::vector<BatchGroup> groups;
  size_t n_batched = 0;
  for (uint32_t i = 0; i < n_jobs; ++i) {
    const BatchMap& bm = maps[(size_t)bj[i].map];
    if (bm.rc != NDTPSO_OK) {
      jobs[i].rc = bm.rc;
      continue;
    }
    bj[i].kind = batch_plan_job(mode, bm.m->p.g, bm.wn, bj[i].n, cfg, &bj[i].plan);
    if (bj[i].kind < 0) continue;
    size_t g = 0;
    while (g < groups.size() && groups[g].kind != bj[i].kind) ++g;
    if (g == groups.size()) {
      groups.push_back(BatchGroup{});
      groups[g].kind = bj[i].kind;
    }
    groups[g].jobs.push_back(i);
    maps[(size_t)bj[i].map].batched = true;
    ++n_batched;
  }
  // (a job kernel for ONE job would be the single path with a table in between: it runs alone, and prepares its map itself)
  if (n_batched == 1) {
    for (uint32_t i = 0; i < n_jobs; ++i)
      if (bj[i].kind >= 0) bj[i].kind = -1;
    for (BatchMap& bm : maps) bm.late = bm.batched = false;
    groups.clear();
    n_batched = 0;
  }

  int first_rc = NDTPSO_OK;
  // A failure of the call itself once the batch is being put together: no job has a result yet, so every job that has not failed
  // on its own carries the call's code (a C caller reads per-job rc), and what was launched is waited for -- the kernels read the
  // pinned staging slot, which nothing else fences.
  bool launched = false;
  auto abandon = [&](int rc) {
    if (launched) (void)hipStreamSynchronize(c->stream);
    for (uint32_t i = 0; i < n_jobs; ++i)
      if (jobs[i].rc == NDTPSO_OK) jobs[i].rc = rc;
    return rc;
  };
#define BATCH_TRY(expr)                                                                                         \
  do {                                                                                                          \
    hipError_t e__ = (expr);                                                                                    \
    if (e__ != hipSuccess) return abandon(fail(c, NDTPSO_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e__))); \
  } while (0)
  if (n_batched) {
    c->clk_enter = std::chrono::steady_clock::now();
    ClusterAdmission admitted(c, (int)n_batched);
    bool allow_cluster = admitted.allow;
    if (t_plan_force.cluster >= 0) allow_cluster = t_plan_force.cluster != 0;  // (the check of the job kernels runs both forms)
    const int P = cfg->population;
    const size_t n_draw = ndtpso_rand_draws(cfg);
    const int table_vec = (int)((n_draw * 4 + 15) / 16);
    size_t first = 0, xc_total = 0, copies = 0, staged_bytes = round_up((int)(n_batched * sizeof(AlignJob)), 256);
    for (BatchGroup& gr : groups) {
      const uint32_t n = (uint32_t)gr.jobs.size();
      cluster_launch_k(c, P, n, allow_cluster, true, &gr.K, &gr.cw);
      gr.lds_total = 0;
      for (uint32_t i : gr.jobs) {  // (every job has a layout of its own, and its speculation scratch behind it)
        int lds = bj[i].plan.L.total;
        ClusterP room;
        room.spec_off = -1;
        if (gr.K > 1) cluster_spec_room(P, &lds, &room);
        bj[i].spec_off = room.spec_off;
        gr.lds_total = std::max(gr.lds_total, lds);  // the launch's dynamic LDS is its largest job's
      }
      gr.waves = gr.K > 1 ? gr.cw : pick_waves(P, gr.lds_total, 1);
      gr.ps = make_pso(cfg, gr.waves, gr.kind == 2 ? NDTPSO_SCORE_F64 : NDTPSO_SCORE_F32, false);
      size_t unit_slots = 0;  // (no lds_total: the speculation scratch was placed per job above, AlignJob::spec_off)
      cluster_launch_shape(c, P, gr.K, gr.waves, n, 0, nullptr, 0, nullptr, &gr.ps, &gr.cl, &unit_slots);
      gr.first = first;
      gr.xc_off = xc_total;
      xc_total += (size_t)n * unit_slots;
      for (uint32_t i : gr.jobs) {
        if (jobs[i].rand_table) {
          copies += (size_t)gr.K;
          staged_bytes += (size_t)table_vec * 16;
        }
        staged_bytes += kGuessBytes;
      }
      first += n;
    }
    // every buffer before the first launch: growing one frees it
    BATCH_TRY(c->jobs_out.reserve(n_batched * 64));
    if (copies) BATCH_TRY(c->jobs_table.reserve(copies * (size_t)table_vec * 16));
    if (xc_total) BATCH_TRY(c->cluster_xc.reserve(xc_total * sizeof(uint4)));
    if (c->jobs_pinned_cap < n_batched * kJobSlotBytes) {
      if (c->jobs_pinned) (void)hipHostFree(c->jobs_pinned);
      c->jobs_pinned = nullptr;
      c->jobs_pinned_cap = 0;
      const size_t want = std::max<size_t>(n_batched * kJobSlotBytes, 16 * kJobSlotBytes);
      BATCH_TRY(hipHostMalloc(&c->jobs_pinned, want, hipHostMallocMapped | hipHostMallocCoherent));
      std::memset(c->jobs_pinned, 0, want);
      c->jobs_pinned_cap = want;
    }
    // Descriptors, guesses and rand() tables travel as the single path's inputs do: a pinned slot the kernels read in place.
    // The call returns after the last kernel that reads it has reported, so the slot needs no fence.
    void* staged = nullptr;
    int slot = 0;
    BATCH_TRY(c->pinned.stage(staged_bytes, &staged, &slot, c->align_seen));
    AlignJob* desc = static_cast<AlignJob*>(staged);
    unsigned char* in_at = static_cast<unsigned char*>(staged) + round_up((int)(n_batched * sizeof(AlignJob)), 256);
    size_t copy_at = 0;
    for (BatchGroup& gr : groups) {
      if (gr.K > 1) gr.cl.xc = (uint4*)c->cluster_xc.p + gr.xc_off;
      size_t at = gr.first;
      for (uint32_t i : gr.jobs) {
        const ndtpso_map_align_job& j = jobs[i];
        const BatchMap& bm = maps[(size_t)bj[i].map];
        AlignJob d;
        std::memset(&d, 0, sizeof(d));
        d.image = (const unsigned char*)bm.m->image.p;
        d.xy = (const double2*)j.new_points->xy.p;
        d.n_ptr = (const uint32_t*)j.new_points->n_dev.p;
        double gd[8] = {j.guess[0], j.guess[1], j.guess[2], j.deviation[0], j.deviation[1], j.deviation[2], 0., 0.};
        std::memcpy(in_at, gd, sizeof(gd));
        d.guess = reinterpret_cast<const double*>(in_at);
        in_at += kGuessBytes;
        if (j.rand_table) {
          std::memcpy(in_at, j.rand_table, n_draw * 4);
          d.table_src = reinterpret_cast<const int4*>(in_at);
          d.table_dst = (int4*)c->jobs_table.p + copy_at * (size_t)table_vec;
          in_at += (size_t)table_vec * 16;
          copy_at += (size_t)gr.K;
        }
        d.out = (double*)c->jobs_out.p + at * 8;
        d.mirror = reinterpret_cast<double*>(static_cast<unsigned char*>(c->jobs_pinned) + at * kJobSlotBytes);
        d.late_hdr = (bm.late && bj[i].plan.path == 2) ? reinterpret_cast<const uint32_t*>(bm.m->hdr.p) : nullptr;
        d.g = bm.m->p.g;
        d.wn = bm.wn;
        d.L = bj[i].plan.L;
        d.dn = bj[i].plan.dn;
        d.n = (int)bj[i].n;
        d.late_table_cap = dense_entries(bj[i].plan.dn.dw, bj[i].plan.dn.dh);
        d.late_rec_cap = bm.wn.rec_cap;
        d.spec_off = bj[i].spec_off;
        d.seed = j.seed;
        if (++c->jobs_issued == 0u) c->jobs_issued = 1u;
        d.seq = bj[i].seq = c->jobs_issued;
        d.want_cost = (j.flags & 1u) ? 1 : 0;
        desc[at] = d;
        ++at;
      }
    }
    ++c->align_issued;  // (the launches stand for one alignment in the context's count: what a staged scan waits for, PinnedRing)
    for (const BatchGroup& gr : groups) {
      const AlignJob* d_jobs = desc + gr.first;
      batch_launch_kernel(c, gr, d_jobs, table_vec);
      launched = true;
      BATCH_TRY(hipGetLastError());
    }
    // the occupancy grid a committed speculation still owes is not read by the alignments: it follows them
    for (BatchMap& bm : maps)
      if (bm.batched && bm.m->spec)
        if (int rc = map_commit_speculation(bm.m)) return abandon(rc);
    for (const BatchGroup& gr : groups) {
      size_t at = gr.first;
      for (uint32_t i : gr.jobs) {
        const double* res = reinterpret_cast<const double*>(static_cast<const unsigned char*>(c->jobs_pinned) + at * kJobSlotBytes);
        if (int rc = wait_pinned_word(c, reinterpret_cast<const uint32_t*>(res + 8), bj[i].seq)) return abandon(rc);
        ++at;
      }
    }
    c->align_seen = c->align_issued;
    admitted.release();
    // the headers the late launches ran ahead of: written by the pack kernels, which precede the alignments on the stream
    for (BatchMap& bm : maps)
      if (bm.late) bm.rc = map_take_spec_header(bm.m);
    for (const BatchGroup& gr : groups) {
      size_t at = gr.first;
      for (uint32_t i : gr.jobs) {
        ndtpso_map_align_job& j = jobs[i];
        BatchMap& bm = maps[(size_t)bj[i].map];
        double host[kResultDoubles];
        std::memcpy(host, static_cast<const unsigned char*>(c->jobs_pinned) + at * kJobSlotBytes, sizeof(host));
        ++at;
        if (bm.rc != NDTPSO_OK) {
          j.rc = bm.rc;
          continue;
        }
        const AlignStats st = result_of(host);
        if (must_redo_alone(st)) {  // the fp64 score after the underflow flag, no cluster after a timeout
          if (bm.late) ++bm.m->late_fallbacks;
          if (st.status & kStatusClusterTimeout) note_cluster_timeout(c);
          bj[i].kind = (st.status & kStatusNeedsF64) ? -2 : -1;
          continue;
        }
        if (bm.late) ++bm.m->late_aligned;
        result_of(host, j.pose, (j.flags & 1u) ? &j.cost : nullptr, &j.stats);
        j.route = gr.K;
      }
    }
  }
#undef BATCH_TRY
  // ---- the jobs that run alone -----------------------------------------------------------------------------------------
  for (uint32_t i = 0; i < n_jobs; ++i) {
    if (jobs[i].rc == NDTPSO_OK && bj[i].kind < 0 && maps[(size_t)bj[i].map].rc == NDTPSO_OK)
      batch_single(jobs[i], cfg, bj[i].kind == -2 ? NDTPSO_SCORE_F64 : asked);
    if (jobs[i].rc != NDTPSO_OK && first_rc == NDTPSO_OK) first_rc = jobs[i].rc;
  }
  return first_rc;
}
