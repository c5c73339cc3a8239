// ndtpso_map_search.inc -- ndtpso_map_search: cost_function (core.cpp:26-48) at every node of a pose lattice against a resident
// map and the best top_k nodes, picked on the device (kernels: ndtpso_map_search.hip).  Included by ndtpso_map.inc behind
// ndtpso_map_cost, whose preparation of the map and whose fp64 path (cost_launch) it shares.

namespace {

// the sweep's workgroups: two per compute unit (k_cost_batch's 512 on this chip), each staging the table once
uint32_t sweep_grid_max(const ndtpso_ctx* c) { return 2u * (uint32_t)std::max(c->n_cus, 1); }

// How a lattice is dealt to workgroups: items of one heading and a slab of its translations, a multiple of the 16 waves of a
// workgroup.  The workgroups take items in turn (item b, b + grid, ...), so a launch lasts as long as the workgroup with one item
// more than the others: about sixteen items per workgroup keep that tail near 6 % (1100 items on 512 workgroups -- two or three
// each -- made the fp64 sweep of 1e6 nodes no faster than k_cost_batch over the same poses), while turning the scan once per item
// (a sincos and two barriers: about a sixth of scoring one node) stays small beside a slab's nodes wherever the lattice is large
// enough to have the choice.  The result does not depend on it (one wave per node, whole).
LatticeP lattice_items(const ndtpso_lattice* lat, const double step[3], uint32_t grid_max) {
  LatticeP p;
  p.ox = lat->origin[0];
  p.oy = lat->origin[1];
  p.oth = lat->origin[2];
  p.sx = step[0];
  p.sy = step[1];
  p.sth = step[2];
  p.nx = lat->count[0];
  p.ny = lat->count[1];
  p.nth = lat->count[2];
  const uint32_t nxy = p.nx * p.ny;
  const uint32_t want = std::min<uint32_t>((nxy + 15) / 16, std::max<uint32_t>(1u, (16 * grid_max + p.nth - 1) / p.nth));
  p.slab = ((nxy + want - 1) / want + 15) / 16 * 16;
  p.slabs = (nxy + p.slab - 1) / p.slab;
  p.n_items = p.nth * p.slabs;
  return p;
}

// the order of the hits on the host (search_key_less on the device): cost by value, then index, a NaN behind every number
bool search_hit_less(double a, uint32_t ai, double b, uint32_t bi) {
  const bool an = a != a, bn = b != b;
  if (an || bn) return an == bn ? ai < bi : bn;
  return a < b || (a == b && ai < bi);
}

void lattice_node_pose(const ndtpso_lattice* lat, const double step[3], uint32_t index, double pose[3]) {
  const uint32_t nx = lat->count[0], ny = lat->count[1];
  const uint32_t ijk[3] = {index % nx, (index / nx) % ny, index / (nx * ny)};
  for (int a = 0; a < 3; ++a) {
    const double along = (double)ijk[a] * step[a];  // (its own statement: one multiplication, one addition)
    pose[a] = lat->origin[a] + along;
  }
}

// one sweep of the whole lattice in `mode` (fp32 or fp64) and the best k keys of it, on the host
int search_sweep(ndtpso_ctx* c, ndtpso_map* m, ndtpso_points* pts, uint32_t n, const Plan& plan, const LatticeP& lp, int mode, uint32_t k,
                 SearchKey* keys) {
  const uint32_t n_nodes = lp.nx * lp.ny * lp.nth;
  const uint32_t per_wg = std::max<uint32_t>(kSelectMinPerWg, (n_nodes + kSelectMaxLists - 1) / kSelectMaxLists);
  const uint32_t lists = (n_nodes + per_wg - 1) / per_wg;
  HIP_TRY(c, c->search_costs.reserve((size_t)n_nodes * 8));
  HIP_TRY(c, c->search_keys.reserve(((size_t)lists + 1) * k * sizeof(SearchKey)));
  SweepArgs a;
  a.image = (const unsigned char*)m->image.p;
  a.xy = (const double2*)pts->xy.p;
  a.costs = (double*)c->search_costs.p;
  a.g = m->p.g;
  a.wn = window_of(m->host_hdr);
  a.L = plan.L;
  a.dn = plan.dn;
  a.lat = lp;
  a.n = (int)n;
  const unsigned grid = std::min<uint32_t>(lp.n_items, sweep_grid_max(c));
  HIP_TRY(c, search_sweep_launch(mode, plan.path, grid, plan.L.total, c->stream, &a));
  SearchKey* d_keys = (SearchKey*)c->search_keys.p;
  HIP_TRY(c, search_select_launch(c->stream, a.costs, n_nodes, k, lists, per_wg, d_keys + k, d_keys));
  HIP_TRY(c, hipMemcpyAsync(keys, d_keys, (size_t)k * sizeof(SearchKey), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return NDTPSO_OK;
}

// ---- the single call's rules, cut out so that ndtpso_map_search_batch (ndtpso_map_search_batch.inc) goes by the same ones ----------

// a lattice the search accepts: its node count, and the step the nodes are generated with
int search_check_lattice(ndtpso_ctx* c, const ndtpso_lattice* lat, double step[3], uint32_t* n_nodes) {
  uint64_t nodes = 1;
  for (int a = 0; a < 3; ++a) {
    if (lat->count[a] == 0) return fail(c, NDTPSO_E_ARG, "a lattice axis without nodes");
    nodes *= lat->count[a];
    if (nodes > NDTPSO_SEARCH_MAX_NODES) return fail(c, NDTPSO_E_ARG, "more than 2^24 lattice nodes");
    if (!std::isfinite(lat->origin[a])) return fail(c, NDTPSO_E_ARG, "lattice origin not finite");
    if (lat->count[a] > 1 && !(lat->step[a] > 0. && std::isfinite(lat->step[a])))
      return fail(c, NDTPSO_E_ARG, "lattice step not positive and finite");
    step[a] = lat->count[a] > 1 ? lat->step[a] : 0.;  // (an axis of one node: its step is not read)
  }
  if (lat->top_k < 1 || lat->top_k > NDTPSO_SEARCH_MAX_TOP_K) return fail(c, NDTPSO_E_ARG, "top_k outside 1 .. 64");
  *n_nodes = (uint32_t)nodes;
  return NDTPSO_OK;
}

// the map as a search (or ndtpso_map_cost) wants it, enqueued: a pending speculation committed, an unbuilt insert built
int search_prepare_map(ndtpso_map* m) {
  if (m->spec) return map_commit_speculation(m);
  if (!m->built) return map_enqueue_build(m);
  return NDTPSO_OK;
}

// The plans of a search in `mode` (resolved: EXACT only where the start-up check allows it) of a scan of n points against the
// table of window `wn`; an exact mode whose fp32 plan is not the dense table becomes the fp64 score (*fell).
int search_plans(ndtpso_ctx* c, const GridP& g, const WinP& wn, uint32_t n, int* mode, uint32_t* fell, Plan* plan64, Plan* plan32) {
  const int n_max = std::max<int>((int)n, 1);
  if (*mode != NDTPSO_SCORE_F32 && !make_plan(NDTPSO_SCORE_F64, g, wn, n_max, 0, prebuilt_table_ask(), plan64))
    return fail(c, NDTPSO_E_CAPACITY, "points do not fit in LDS");
  if (*mode != NDTPSO_SCORE_F64) {
    const bool fits = make_plan(NDTPSO_SCORE_F32, g, wn, n_max, 0, prebuilt_table_ask(), plan32);
    if (*mode == NDTPSO_SCORE_F32 && !fits) return fail(c, NDTPSO_E_CAPACITY, "points do not fit in LDS");
    // the margin is proven on the dense table only (as resolve_score_plan rules for alignments)
    if (*mode == NDTPSO_SCORE_EXACT && !(fits && plan32->path == 2)) {
      *fell = NDTPSO_SEARCH_FELL_PLAN;
      *mode = NDTPSO_SCORE_F64;
    }
  }
  return NDTPSO_OK;
}

// what the exact mode makes of its K-th fp32 cost before it collects: 0, or why the whole lattice runs in fp64
uint32_t search_fell_by_key(double c32_k) {
  if (c32_k != c32_k) return NDTPSO_SEARCH_FELL_NAN;
  if (c32_k > -kTinyCost) return NDTPSO_SEARCH_FELL_UNDERFLOW;
  return 0;
}
// ... and of the collected candidates' count and the number of NaN costs
uint32_t search_fell_by_candidates(uint32_t n_candidates, uint32_t n_nan) {
  if (n_nan) return NDTPSO_SEARCH_FELL_NAN;
  if (n_candidates > NDTPSO_SEARCH_MAX_CANDIDATES) return NDTPSO_SEARCH_FELL_MANY;
  return 0;
}

void search_rank(std::vector<std::pair<double, uint32_t>>* ranked) {
  std::sort(ranked->begin(), ranked->end(), [](const std::pair<double, uint32_t>& a, const std::pair<double, uint32_t>& b) {
    return search_hit_less(a.first, a.second, b.first, b.second);
  });
}

// the hits and the statistics of a finished search: `mode` is what ran (EXACT: the ranked candidates, else the sweep's keys)
void search_report(const ndtpso_lattice* lat, const double step[3], int mode, uint32_t k, const SearchKey* keys,
                   const std::vector<std::pair<double, uint32_t>>& ranked, uint32_t n_nodes, uint32_t n, int path, uint32_t n_candidates,
                   uint32_t fell, ndtpso_lattice_hit* hits, uint32_t* n_hits, ndtpso_search_stats* stats) {
  for (uint32_t r = 0; r < k; ++r) {
    ndtpso_lattice_hit& h = hits[r];
    h.index = mode == NDTPSO_SCORE_EXACT ? ranked[r].second : keys[r].index;
    h.cost = mode == NDTPSO_SCORE_EXACT ? ranked[r].first : keys[r].cost;
    h.reserved = 0;
    lattice_node_pose(lat, step, h.index, h.pose);
  }
  *n_hits = k;
  if (stats) {
    stats->n_nodes = n_nodes;
    stats->n_points = n;
    stats->mode_run = mode == NDTPSO_SCORE_F64 ? NDTPSO_SCORE_F64 : NDTPSO_SCORE_F32;
    stats->path = (uint32_t)path;
    stats->n_candidates = n_candidates;
    stats->fell_back = fell;
  }
}

}  // namespace

extern "C" int ndtpso_map_search(ndtpso_map* m, ndtpso_points* pts, const ndtpso_lattice* lat, int mode, ndtpso_lattice_hit* hits,
                                 uint32_t* n_hits, ndtpso_search_stats* stats) {
  if (!m || !pts) return NDTPSO_E_ARG;
  ndtpso_ctx* c = m->ctx;
  if (!lat || !hits || !n_hits) return fail(c, NDTPSO_E_ARG, "null argument");
  *n_hits = 0;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (pts->ctx != c) return fail(c, NDTPSO_E_ARG, "a scan of another context");
  if (int rc = check_mode(c, mode)) return rc;
  double step[3];
  uint32_t n_nodes = 0;
  if (int rc = search_check_lattice(c, lat, step, &n_nodes)) return rc;
  const uint32_t k = std::min<uint32_t>(lat->top_k, n_nodes);
  uint32_t fell = 0;
  if (mode == NDTPSO_SCORE_EXACT) {
    if (int rc = exact_mode_resolve(c, &mode)) return rc;
    if (mode != NDTPSO_SCORE_EXACT) fell = NDTPSO_SEARCH_FELL_REFUSED;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = search_prepare_map(m)) return rc;  // (as ndtpso_map_cost)
  if (int rc = map_fetch_header(m)) return rc;
  uint32_t n = 0;
  HIP_TRY(c, hipMemcpy(&n, pts->n_dev.p, 4, hipMemcpyDeviceToHost));
  pts->n_upper = n;
  const GridP& g = m->p.g;
  const WinP wn = window_of(m->host_hdr);
  Plan plan64, plan32;
  if (int rc = search_plans(c, g, wn, n, &mode, &fell, &plan64, &plan32)) return rc;
  const LatticeP lp = lattice_items(lat, step, sweep_grid_max(c));
  SearchKey keys[NDTPSO_SEARCH_MAX_TOP_K];
  std::vector<std::pair<double, uint32_t>> ranked;  // EXACT: the candidates' fp64 costs
  uint32_t n_candidates = 0;
  if (mode == NDTPSO_SCORE_EXACT) {
    if (int rc = search_sweep(c, m, pts, n, plan32, lp, NDTPSO_SCORE_F32, k, keys)) return rc;
    const double c32_k = keys[k - 1].cost;
    fell = search_fell_by_key(c32_k);
    if (!fell) {
      // every node that can belong to the fp64 score's best k: c32 <= c32_K + tau(n) (DESIGN 3.5)
      const uint32_t cap = NDTPSO_SEARCH_MAX_CANDIDATES;
      std::vector<uint32_t> cand(2 + cap);
      HIP_TRY(c, c->search_cand.reserve(cand.size() * 4));
      HIP_TRY(c, hipMemsetAsync(c->search_cand.p, 0, 8, c->stream));
      HIP_TRY(c, search_collect_launch(c->stream, (const double*)c->search_costs.p, n_nodes, c32_k + kArbAbsPerPoint * (double)n, cap,
                                       (uint32_t*)c->search_cand.p));
      HIP_TRY(c, hipMemcpyAsync(cand.data(), c->search_cand.p, 8, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      fell = search_fell_by_candidates(cand[0], cand[1]);
      if (!fell) {
        n_candidates = cand[0];
        HIP_TRY(c, hipMemcpy(cand.data() + 2, (const uint32_t*)c->search_cand.p + 2, (size_t)n_candidates * 4, hipMemcpyDeviceToHost));
        std::sort(cand.begin() + 2, cand.begin() + 2 + n_candidates);
        std::vector<double> poses((size_t)n_candidates * 3), costs(n_candidates);
        for (uint32_t i = 0; i < n_candidates; ++i) lattice_node_pose(lat, step, cand[2 + i], &poses[(size_t)i * 3]);
        if (int rc = cost_launch(c, (const unsigned char*)m->image.p, g, wn, (const double2*)pts->xy.p, n, poses.data(), n_candidates,
                                 NDTPSO_SCORE_F64, costs.data(), nullptr))
          return rc;
        ranked.resize(n_candidates);
        for (uint32_t i = 0; i < n_candidates; ++i) ranked[i] = {costs[i], cand[2 + i]};
        search_rank(&ranked);
      }
    }
    if (fell) mode = NDTPSO_SCORE_F64;
  }
  const Plan& plan = mode == NDTPSO_SCORE_F64 ? plan64 : plan32;
  if (mode != NDTPSO_SCORE_EXACT) {
    if (int rc = search_sweep(c, m, pts, n, plan, lp, mode, k, keys)) return rc;
  }
  search_report(lat, step, mode, k, keys, ranked, n_nodes, n, plan.path, n_candidates, fell, hits, n_hits, stats);
  return NDTPSO_OK;
}
