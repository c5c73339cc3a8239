// ndtpso_map_search_batch.inc -- ndtpso_map_search_batch: several ndtpso_map_search calls of one context in shared launches
// (kernels: ndtpso_map_search_jobs.hip).  Included by ndtpso_map.inc behind ndtpso_map_search.inc, whose rules it goes by:
// search_check_lattice, search_prepare_map, search_plans, lattice_items, the fallback rules, search_rank and search_report.
//
// A call is one or two ROUNDS.  A round takes a set of jobs, each with the score it runs in, and enqueues without a wait in
// between: one sweep per kernel kind (score x table plan), the two selection launches, and for the jobs in the exact mode the
// collect launch and one fp64 launch per table plan over the candidate lists; then it waits once.  The second round is the fp64
// sweep and selection of the exact-mode jobs that the first one's keys or candidates rule a fallback.

namespace {

struct SearchBatchJob {
  int rc = NDTPSO_OK;
  bool live = false;  // lattice accepted, map prepared, plan fits: a job of the shared launches
  double step[3] = {0., 0., 0.};
  uint32_t n_nodes = 0, k = 0, n = 0;
  int map = -1, scan = -1;  // among the call's distinct maps / scans
  int mode = 0;             // what it runs as: F32, F64, or EXACT (fp32 sweep, candidates rescored in fp64)
  uint32_t fell = 0, n_candidates = 0;
  Plan plan64, plan32;
  LatticeP lp;
  // its places in a round's buffers: costs (doubles), final keys and first-stage lists (SearchKey), candidates (uint32_t / SearchKey)
  uint32_t cost_off = 0, key_off = 0, list_off = 0, lists = 0, per_wg = 0;
  uint32_t exact_at = 0, cand_list = 0, cand_room = 0;
  std::vector<std::pair<double, uint32_t>> ranked;  // EXACT: the candidates' fp64 costs, in order
};

struct SearchSweepKind {  // the jobs of one sweep launch: one kernel instantiation
  int mode, path;
  bool cand;
  std::vector<uint32_t> jobs;
};

// How a launch's workgroups are dealt to its jobs (SweepJob): with fewer jobs than workgroups, every job one share and the rest
// of the grid in proportion to the jobs' items; else one share per job, which the workgroups take in turn.
void search_deal_shares(uint32_t grid_max, std::vector<SweepJob>* descs, std::vector<uint32_t>* share_job) {
  const uint32_t n = (uint32_t)descs->size();
  uint64_t items = 0;
  for (const SweepJob& d : *descs) items += d.lat.n_items;
  const uint64_t extra = n < grid_max ? grid_max - n : 0;
  uint32_t at = 0;
  share_job->clear();
  for (uint32_t j = 0; j < n; ++j) {
    SweepJob& d = (*descs)[j];
    const uint32_t more = (uint32_t)std::min<uint64_t>(d.lat.n_items - 1, extra * d.lat.n_items / std::max<uint64_t>(items, 1));
    d.share0 = at;
    d.share = 1 + more;
    at += d.share;
    share_job->insert(share_job->end(), d.share, j);
  }
}

#define SEARCH_ROUND_TRY(expr)                                                                                    \
  do {                                                                                                            \
    hipError_t e__ = (expr);                                                                                      \
    if (e__ != hipSuccess) {                                                                                      \
      if (launched) (void)hipStreamSynchronize(c->stream); /* the kernels read the pinned tables, which nothing else fences */ \
      return fail(c, NDTPSO_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));                           \
    }                                                                                                             \
  } while (0)

// One round over the jobs `run` (SearchBatchJob::mode says how each runs).  Afterwards keys[bj.key_off ..] are a job's best k keys,
// and for a job in the exact mode hdr[2 * exact_at] / [+ 1] are its candidates' count and the number of NaN costs and
// c->search_pinned[cand_list ..] its candidates' {fp64 cost, node}.
int search_round(ndtpso_ctx* c, const ndtpso_map_search_job* jobs, std::vector<SearchBatchJob>& bj, const std::vector<uint32_t>& run,
                 std::vector<SearchKey>* keys, std::vector<uint32_t>* hdr, ndtpso_search_batch_stats* bs) {
  bool launched = false;
  // ---- every job's place in the shared buffers -----------------------------------------------------------------------------
  uint32_t cost_total = 0, key_total = 0, list_total = 0, n_exact = 0, cand_total = 0;
  for (uint32_t i : run) {
    SearchBatchJob& b = bj[i];
    b.per_wg = std::max<uint32_t>(kSelectMinPerWg, (b.n_nodes + kSelectMaxLists - 1) / kSelectMaxLists);  // (search_sweep's parts)
    b.lists = (b.n_nodes + b.per_wg - 1) / b.per_wg;
    b.cost_off = cost_total;
    cost_total += b.n_nodes;
    b.key_off = key_total;
    key_total += b.k;
  }
  for (uint32_t i : run) {
    SearchBatchJob& b = bj[i];
    b.list_off = key_total + list_total;
    list_total += b.lists * b.k;
    if (b.mode == NDTPSO_SCORE_EXACT) {
      b.exact_at = n_exact++;
      b.cand_room = std::min<uint32_t>(NDTPSO_SEARCH_MAX_CANDIDATES, b.n_nodes);
      b.cand_list = cand_total;
      cand_total += b.cand_room;
    }
  }
  // every buffer before the first launch: growing one frees it
  SEARCH_ROUND_TRY(c->search_costs.reserve((size_t)cost_total * 8));
  SEARCH_ROUND_TRY(c->search_keys.reserve(((size_t)key_total + list_total) * sizeof(SearchKey)));
  if (n_exact) {
    SEARCH_ROUND_TRY(c->search_cand.reserve(((size_t)2 * n_exact + cand_total) * 4));
    if (c->search_pinned_cap < (size_t)cand_total * sizeof(SearchKey)) {
      if (c->search_pinned) (void)hipHostFree(c->search_pinned);
      c->search_pinned = nullptr;
      c->search_pinned_cap = 0;
      const size_t want = std::max<size_t>((size_t)cand_total * sizeof(SearchKey), 64 * 1024);
      SEARCH_ROUND_TRY(hipHostMalloc(&c->search_pinned, want, hipHostMallocMapped | hipHostMallocCoherent));
      c->search_pinned_cap = want;
    }
  }
  double* d_costs = (double*)c->search_costs.p;
  SearchKey* d_keys = (SearchKey*)c->search_keys.p;
  uint32_t* d_cand = (uint32_t*)c->search_cand.p;

  // ---- the tables -------------------------------------------------------------------------------------------------------------
  std::vector<SearchSweepKind> kinds;
  auto kind_of = [&](int mode, int path, bool cand) -> SearchSweepKind& {
    for (SearchSweepKind& k : kinds)
      if (k.mode == mode && k.path == path && k.cand == cand) return k;
    kinds.push_back(SearchSweepKind{mode, path, cand, {}});
    return kinds.back();
  };
  for (uint32_t i : run) {
    const SearchBatchJob& b = bj[i];
    if (b.mode == NDTPSO_SCORE_F64) {
      kind_of(NDTPSO_SCORE_F64, b.plan64.path, false).jobs.push_back(i);
    } else {
      kind_of(NDTPSO_SCORE_F32, b.plan32.path, false).jobs.push_back(i);
    }
  }
  for (uint32_t i : run)  // (behind every whole-lattice kind: launched in this order)
    if (bj[i].mode == NDTPSO_SCORE_EXACT) kind_of(NDTPSO_SCORE_F64, bj[i].plan64.path, true).jobs.push_back(i);
  const uint32_t grid_max = sweep_grid_max(c);
  std::vector<std::vector<SweepJob>> descs(kinds.size());
  std::vector<std::vector<uint32_t>> shares(kinds.size());
  std::vector<int> kind_lds(kinds.size(), 0);
  for (size_t q = 0; q < kinds.size(); ++q) {
    const SearchSweepKind& kd = kinds[q];
    for (uint32_t i : kd.jobs) {
      const SearchBatchJob& b = bj[i];
      const ndtpso_map* m = jobs[i].map;
      const Plan& plan = kd.mode == NDTPSO_SCORE_F64 ? b.plan64 : b.plan32;
      SweepJob d;
      std::memset(&d, 0, sizeof(d));
      d.image = (const unsigned char*)m->image.p;
      d.xy = (const double2*)jobs[i].new_points->xy.p;
      d.costs = d_costs + b.cost_off;
      d.g = m->p.g;
      d.wn = window_of(m->host_hdr);
      d.L = plan.L;
      d.dn = plan.dn;
      d.lat = b.lp;
      d.n = (int)b.n;
      if (kd.cand) {  // (dealt by the room of its list, a wave per candidate: the count is the device's)
        d.cand_hdr = d_cand + 2 * (size_t)b.exact_at;
        d.cand = d_cand + 2 * (size_t)n_exact + b.cand_list;
        d.out = static_cast<SearchKey*>(c->search_pinned) + b.cand_list;
        d.cand_cap = b.cand_room;
        d.lat.n_items = (b.cand_room + 7) / 8;  // (k_lattice_cost_jobs' eight waves)
      }
      kind_lds[q] = std::max(kind_lds[q], plan.L.total);  // the launch's dynamic LDS is its largest job's
      descs[q].push_back(d);
    }
    search_deal_shares(grid_max, &descs[q], &shares[q]);
  }
  std::vector<SelectPart> first, second, cparts;
  std::vector<CollectJob> cjobs(n_exact);
  for (uint32_t i : run) {
    const SearchBatchJob& b = bj[i];
    for (uint32_t l = 0; l < b.lists; ++l) {  // parts of >= kSelectMinPerWg nodes that never straddle two jobs
      SelectPart p{b.cost_off, l * b.per_wg, std::min(b.n_nodes, (l + 1) * b.per_wg), b.k, b.list_off + l * b.k, 0u, {0u, 0u}};
      first.push_back(p);
      if (b.mode == NDTPSO_SCORE_EXACT) {
        p.job = b.exact_at;
        cparts.push_back(p);
      }
    }
    second.push_back(SelectPart{b.list_off, 0u, b.lists * b.k, b.k, b.key_off, 0u, {0u, 0u}});
    if (b.mode == NDTPSO_SCORE_EXACT)
      cjobs[b.exact_at] = CollectJob{b.key_off + b.k - 1, b.n, 2 * b.exact_at, 2 * n_exact + b.cand_list, b.cand_room, {0u, 0u, 0u}};
  }
  // Descriptors and tables travel as the alignment jobs' do: one pinned block that the kernels read in place.  The round returns
  // after the last kernel that reads it has finished, so the block needs no fence.
  auto padded = [](size_t bytes) { return (bytes + 255) / 256 * 256; };
  size_t staged_bytes = 0;
  std::vector<size_t> desc_at(kinds.size()), share_at(kinds.size());
  for (size_t q = 0; q < kinds.size(); ++q) {
    desc_at[q] = staged_bytes;
    staged_bytes += padded(descs[q].size() * sizeof(SweepJob));
    share_at[q] = staged_bytes;
    staged_bytes += padded(shares[q].size() * 4);
  }
  const size_t first_at = staged_bytes;
  staged_bytes += padded(first.size() * sizeof(SelectPart));
  const size_t second_at = staged_bytes;
  staged_bytes += padded(second.size() * sizeof(SelectPart));
  const size_t cparts_at = staged_bytes;
  staged_bytes += padded(cparts.size() * sizeof(SelectPart));
  const size_t cjobs_at = staged_bytes;
  staged_bytes += padded(cjobs.size() * sizeof(CollectJob));
  void* staged = nullptr;
  int slot = 0;
  SEARCH_ROUND_TRY(c->pinned.stage(staged_bytes, &staged, &slot, c->align_seen));
  unsigned char* base = static_cast<unsigned char*>(staged);
  for (size_t q = 0; q < kinds.size(); ++q) {
    std::memcpy(base + desc_at[q], descs[q].data(), descs[q].size() * sizeof(SweepJob));
    std::memcpy(base + share_at[q], shares[q].data(), shares[q].size() * 4);
  }
  std::memcpy(base + first_at, first.data(), first.size() * sizeof(SelectPart));
  std::memcpy(base + second_at, second.data(), second.size() * sizeof(SelectPart));
  if (n_exact) {
    std::memcpy(base + cparts_at, cparts.data(), cparts.size() * sizeof(SelectPart));
    std::memcpy(base + cjobs_at, cjobs.data(), cjobs.size() * sizeof(CollectJob));
  }

  // ---- the launches: no wait in between --------------------------------------------------------------------------------------
  auto sweep = [&](size_t q) {
    const uint32_t n_shares = (uint32_t)shares[q].size();
    const uint32_t* share_job = reinterpret_cast<const uint32_t*>(base + share_at[q]);
    if (kinds[q].cand)
      return search_jobs_cost_launch(kinds[q].path, std::min(n_shares, grid_max), kind_lds[q], c->stream, base + desc_at[q], share_job, n_shares);
    return search_jobs_sweep_launch(kinds[q].mode, kinds[q].path, std::min(n_shares, grid_max), kind_lds[q], c->stream, base + desc_at[q],
                                    share_job, n_shares);
  };
  for (size_t q = 0; q < kinds.size(); ++q) {
    if (kinds[q].cand) continue;
    launched = true;
    SEARCH_ROUND_TRY(sweep(q));
    ++bs->launches;
  }
  SEARCH_ROUND_TRY(search_jobs_select_launch(c->stream, d_costs, d_keys, base + first_at, (uint32_t)first.size(), base + second_at,
                                             (uint32_t)second.size()));
  bs->launches += 2;
  hdr->assign(2 * (size_t)n_exact, 0u);
  if (n_exact) {
    SEARCH_ROUND_TRY(hipMemsetAsync(d_cand, 0, 8 * (size_t)n_exact, c->stream));
    SEARCH_ROUND_TRY(search_jobs_collect_launch(c->stream, d_costs, d_keys, base + cparts_at, (uint32_t)cparts.size(), base + cjobs_at, d_cand));
    ++bs->launches;
    for (size_t q = 0; q < kinds.size(); ++q) {
      if (!kinds[q].cand) continue;
      SEARCH_ROUND_TRY(sweep(q));
      ++bs->launches;
    }
    SEARCH_ROUND_TRY(hipMemcpyAsync(hdr->data(), d_cand, 8 * (size_t)n_exact, hipMemcpyDeviceToHost, c->stream));
  }
  keys->resize(key_total);
  SEARCH_ROUND_TRY(hipMemcpyAsync(keys->data(), d_keys, (size_t)key_total * sizeof(SearchKey), hipMemcpyDeviceToHost, c->stream));
  SEARCH_ROUND_TRY(hipStreamSynchronize(c->stream));
  ++bs->waits;
  return NDTPSO_OK;
}
#undef SEARCH_ROUND_TRY

int search_batch_single(ndtpso_map_search_job& j, int mode, ndtpso_search_batch_stats* bs) {
  j.route = 0;
  ++bs->single_jobs;
  j.rc = ndtpso_map_search(j.map, j.new_points, &j.lattice, mode, j.hits, &j.n_hits, &j.stats);
  return j.rc;
}

}  // namespace

extern "C" int ndtpso_map_search_batch(ndtpso_ctx* c, ndtpso_map_search_job* jobs, uint32_t n_jobs, int mode,
                                       ndtpso_search_batch_stats* stats) {
  if (!c) return NDTPSO_E_ARG;
  if (!jobs || n_jobs == 0) return fail(c, NDTPSO_E_ARG, "no jobs");
  for (uint32_t i = 0; i < n_jobs; ++i) {
    if (!jobs[i].map || !jobs[i].new_points || !jobs[i].hits) return fail(c, NDTPSO_E_ARG, "null argument");
    if (jobs[i].map->ctx != c || jobs[i].new_points->ctx != c) return fail(c, NDTPSO_E_ARG, "a map or scan of another context");
  }
  if (int rc = check_mode(c, mode)) return rc;
  // the jobs' own lattices: a refusal is the job's; the accepted ones share the cost buffer of one single call
  std::vector<SearchBatchJob> bj(n_jobs);
  uint64_t nodes = 0;
  for (uint32_t i = 0; i < n_jobs; ++i) {
    bj[i].rc = search_check_lattice(c, &jobs[i].lattice, bj[i].step, &bj[i].n_nodes);
    if (bj[i].rc == NDTPSO_OK) nodes += bj[i].n_nodes;
  }
  if (nodes > NDTPSO_SEARCH_MAX_NODES) return fail(c, NDTPSO_E_ARG, "the jobs' lattices have more than 2^24 nodes in all");
  ndtpso_search_batch_stats bs;
  std::memset(&bs, 0, sizeof(bs));
  if (stats) *stats = bs;
  for (uint32_t i = 0; i < n_jobs; ++i) {
    ndtpso_map_search_job& j = jobs[i];
    j.n_hits = 0;
    std::memset(&j.stats, 0, sizeof(j.stats));
    j.rc = bj[i].rc;
    j.route = 0;
    j.reserved = 0;
  }
  auto finish = [&]() {
    int first_rc = NDTPSO_OK;
    for (uint32_t i = 0; i < n_jobs && first_rc == NDTPSO_OK; ++i) first_rc = jobs[i].rc;
    if (stats) *stats = bs;
    return first_rc;
  };
  // A failure of the call itself once the launches are being put together: every job that has not failed on its own carries it.
  auto abandon = [&](int rc) {
    for (uint32_t i = 0; i < n_jobs; ++i)
      if (jobs[i].rc == NDTPSO_OK) {
        jobs[i].rc = rc;
        jobs[i].n_hits = 0;
      }
    if (stats) *stats = bs;
    return rc;
  };
  if (n_jobs == 1) {  // a lone search: exactly ndtpso_map_search
    search_batch_single(jobs[0], mode, &bs);
    return finish();
  }
  const int asked = mode;  // what a job that runs alone is asked for (ndtpso_map_search resolves it itself)
  uint32_t fell_all = 0;
  if (mode == NDTPSO_SCORE_EXACT) {
    if (int rc = exact_mode_resolve(c, &mode)) return abandon(rc);
    if (mode != NDTPSO_SCORE_EXACT) fell_all = NDTPSO_SEARCH_FELL_REFUSED;
  }
  if (hipSetDevice(c->device) != hipSuccess) return abandon(fail(c, NDTPSO_E_HIP, "hipSetDevice"));

  // ---- every distinct map and scan once, and one wait for all their headers and counts ----------------------------------------
  struct Prepared {
    ndtpso_map* m;
    int rc;
  };
  std::vector<Prepared> maps;
  std::vector<ndtpso_points*> scans;
  for (uint32_t i = 0; i < n_jobs; ++i) {
    if (bj[i].rc != NDTPSO_OK) continue;
    for (size_t k = 0; k < maps.size() && bj[i].map < 0; ++k)
      if (maps[k].m == jobs[i].map) bj[i].map = (int)k;
    if (bj[i].map < 0) {
      bj[i].map = (int)maps.size();
      maps.push_back(Prepared{jobs[i].map, NDTPSO_OK});
    }
    for (size_t k = 0; k < scans.size() && bj[i].scan < 0; ++k)
      if (scans[k] == jobs[i].new_points) bj[i].scan = (int)k;
    if (bj[i].scan < 0) {
      bj[i].scan = (int)scans.size();
      scans.push_back(jobs[i].new_points);
    }
  }
  if (!maps.empty()) {
    for (Prepared& pm : maps) {
      pm.rc = search_prepare_map(pm.m);
      if (pm.rc == NDTPSO_OK) pm.rc = map_fetch_header_enqueue(pm.m);
    }
    std::vector<uint32_t> counts(scans.size(), 0u);
    for (size_t k = 0; k < scans.size(); ++k)
      if (hipMemcpyAsync(&counts[k], scans[k]->n_dev.p, 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        return abandon(fail(c, NDTPSO_E_HIP, "copy of a scan's point count"));
      }
    if (hipStreamSynchronize(c->stream) != hipSuccess) return abandon(fail(c, NDTPSO_E_HIP, "wait for the maps' headers"));
    ++bs.waits;
    for (Prepared& pm : maps)
      if (pm.rc == NDTPSO_OK) pm.rc = map_fetch_header_arrived(pm.m);
    for (size_t k = 0; k < scans.size(); ++k) scans[k]->n_upper = counts[k];
  }

  // ---- every job's plan, by the single call's rule -------------------------------------------------------------------------------
  std::vector<uint32_t> run;
  for (uint32_t i = 0; i < n_jobs; ++i) {
    SearchBatchJob& b = bj[i];
    if (b.rc != NDTPSO_OK) continue;
    ndtpso_map* m = jobs[i].map;
    if ((b.rc = maps[(size_t)b.map].rc) == NDTPSO_OK) {
      b.n = jobs[i].new_points->n_upper;
      b.k = std::min<uint32_t>(jobs[i].lattice.top_k, b.n_nodes);
      b.mode = mode;
      b.fell = fell_all;
      b.rc = search_plans(c, m->p.g, window_of(m->host_hdr), b.n, &b.mode, &b.fell, &b.plan64, &b.plan32);
    }
    if (b.rc != NDTPSO_OK) {
      jobs[i].rc = b.rc;
      continue;
    }
    b.lp = lattice_items(&jobs[i].lattice, b.step, sweep_grid_max(c));
    b.live = true;
    run.push_back(i);
  }
  // (shared launches for ONE job would be the single call with tables in between: it runs alone, on its prepared map)
  if (run.size() == 1) {
    search_batch_single(jobs[run[0]], asked, &bs);
    return finish();
  }
  if (run.empty()) return finish();

  // ---- the rounds ----------------------------------------------------------------------------------------------------------------
  std::vector<SearchKey> keys;
  std::vector<uint32_t> hdr;
  auto report = [&](uint32_t i) {
    SearchBatchJob& b = bj[i];
    const Plan& plan = b.mode == NDTPSO_SCORE_F64 ? b.plan64 : b.plan32;
    search_report(&jobs[i].lattice, b.step, b.mode, b.k, keys.data() + b.key_off, b.ranked, b.n_nodes, b.n, plan.path, b.n_candidates,
                  b.fell, jobs[i].hits, &jobs[i].n_hits, &jobs[i].stats);
    jobs[i].route = 1;
  };
  if (int rc = search_round(c, jobs, bj, run, &keys, &hdr, &bs)) return abandon(rc);
  std::vector<uint32_t> again;  // the exact mode's fallbacks: the whole lattice in fp64
  for (uint32_t i : run) {
    SearchBatchJob& b = bj[i];
    if (b.mode == NDTPSO_SCORE_EXACT) {
      b.fell = search_fell_by_key(keys[b.key_off + b.k - 1].cost);
      if (!b.fell) b.fell = search_fell_by_candidates(hdr[2 * (size_t)b.exact_at], hdr[2 * (size_t)b.exact_at + 1]);
      if (b.fell) {
        b.mode = NDTPSO_SCORE_F64;
        again.push_back(i);
        continue;
      }
      // every node that can belong to the fp64 score's best k, scored in fp64 by the launch itself (DESIGN 3.5)
      b.n_candidates = hdr[2 * (size_t)b.exact_at];
      const SearchKey* scored = static_cast<const SearchKey*>(c->search_pinned) + b.cand_list;
      b.ranked.resize(b.n_candidates);
      for (uint32_t e = 0; e < b.n_candidates; ++e) b.ranked[e] = {scored[e].cost, scored[e].index};
      search_rank(&b.ranked);
    }
    report(i);
  }
  if (!again.empty()) {
    if (int rc = search_round(c, jobs, bj, again, &keys, &hdr, &bs)) {  // (the jobs that are done keep their results)
      for (uint32_t i : again) jobs[i].rc = rc;
      return finish();
    }
    for (uint32_t i : again) report(i);
  }
  return finish();
}
