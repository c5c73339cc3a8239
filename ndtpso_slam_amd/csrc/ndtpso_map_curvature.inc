// ndtpso_map_curvature.inc -- ndtpso_map_curvature, ndtpso_map_curvature_batch and ndtpso_curvature_covariance: gradient and
// Hessian of cost_function (core.cpp:26-48, with normalDistribution, ndtcell.cpp:70-78) by the pose, and the pose covariance
// they stand for (kernel: ndtpso_map_curvature.hip).  The reference has no counterpart.  Included by ndtpso_map.inc behind the
// search, whose preparation of the map (search_prepare_map) and whose grid (sweep_grid_max) it shares; the table plan is
// cost_launch's for NDTPSO_SCORE_F64.
//
// One host path: curvature_launches takes prepared jobs -- map built, header and point count with the host, plan made -- and
// enqueues one launch per table plan among them, then waits once.  The single call is a table of one job.

namespace {

struct CurvatureLive {  // a job of the launches
  ndtpso_map* m;
  ndtpso_points* pts;
  const double* poses;
  uint32_t n_poses;
  ndtpso_curvature* out;
  uint32_t n;  // the scan's points
  Plan plan;
  uint32_t pose_off;  // its place among the call's poses
};

// the plan of a curvature: ndtpso_map_cost's for the fp64 score
int curvature_plan(ndtpso_ctx* c, const ndtpso_map* m, uint32_t n, Plan* plan) {
  if (!make_plan(NDTPSO_SCORE_F64, m->p.g, window_of(m->host_hdr), std::max<int>((int)n, 1), 0, prebuilt_table_ask(), plan))
    return fail(c, NDTPSO_E_CAPACITY, "points do not fit in LDS");
  return NDTPSO_OK;
}

bool curvature_poses_finite(const double* poses, uint32_t n_poses) {
  for (size_t i = 0; i < (size_t)n_poses * 3; ++i)
    if (!std::isfinite(poses[i])) return false;
  return true;
}

// How a launch's workgroups are dealt to its jobs (search_deal_shares' rule, an item being the eight poses of a workgroup's waves)
void curvature_deal_shares(uint32_t grid_max, std::vector<CurvatureJob>* descs, std::vector<uint32_t>* share_job) {
  const uint32_t n = (uint32_t)descs->size();
  auto items_of = [](const CurvatureJob& d) { return (uint64_t)(d.n_poses + kCurvatureThreads / 64 - 1) / (kCurvatureThreads / 64); };
  uint64_t items = 0;
  for (const CurvatureJob& d : *descs) items += items_of(d);
  const uint64_t extra = n < grid_max ? grid_max - n : 0;
  uint32_t at = 0;
  share_job->clear();
  for (uint32_t j = 0; j < n; ++j) {
    CurvatureJob& d = (*descs)[j];
    const uint64_t it = items_of(d);
    const uint32_t more = (uint32_t)std::min<uint64_t>(it - 1, extra * it / std::max<uint64_t>(items, 1));
    d.share0 = at;
    d.share = 1 + more;
    at += d.share;
    share_job->insert(share_job->end(), d.share, j);
  }
}

#define CURVATURE_TRY(expr)                                                                                      \
  do {                                                                                                            \
    hipError_t e__ = (expr);                                                                                      \
    if (e__ != hipSuccess) {                                                                                      \
      if (launched) (void)hipStreamSynchronize(c->stream); /* the kernels read the pinned tables, which nothing else fences */ \
      return fail(c, NDTPSO_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));                           \
    }                                                                                                             \
  } while (0)

int curvature_launches(ndtpso_ctx* c, std::vector<CurvatureLive>& live, ndtpso_curvature_batch_stats* bs) {
  bool launched = false;
  uint32_t total = 0;
  for (CurvatureLive& j : live) {
    j.pose_off = total;
    total += j.n_poses;
  }
  // every buffer before the first launch: growing one frees it
  CURVATURE_TRY(c->poses.reserve((size_t)total * 24));
  CURVATURE_TRY(c->costs.reserve((size_t)total * sizeof(CurvatureOut)));
  const double* d_poses = (const double*)c->poses.p;
  CurvatureOut* d_out = (CurvatureOut*)c->costs.p;

  struct Kind {  // the jobs of one launch: one table plan
    int path;
    int lds;
    std::vector<CurvatureJob> descs;
    std::vector<uint32_t> shares;
  };
  std::vector<Kind> kinds;
  const uint32_t grid_max = sweep_grid_max(c);
  for (const CurvatureLive& j : live) {
    Kind* kd = nullptr;
    for (Kind& k : kinds)
      if (k.path == j.plan.path) kd = &k;
    if (!kd) {
      kinds.push_back(Kind{j.plan.path, 0, {}, {}});
      kd = &kinds.back();
    }
    CurvatureJob d;
    std::memset(&d, 0, sizeof(d));
    d.image = (const unsigned char*)j.m->image.p;
    d.xy = (const double2*)j.pts->xy.p;
    d.poses = d_poses + 3 * (size_t)j.pose_off;
    d.out = d_out + j.pose_off;
    d.g = j.m->p.g;
    d.wn = window_of(j.m->host_hdr);
    d.L = j.plan.L;
    d.dn = j.plan.dn;
    d.n = (int)j.n;
    d.n_poses = j.n_poses;
    kd->lds = std::max(kd->lds, j.plan.L.total);  // the launch's dynamic LDS is its largest job's
    kd->descs.push_back(d);
  }
  // Poses, descriptors and share tables travel in one pinned block: the poses are copied on from it, the tables are read in
  // place.  The call returns after the last kernel that reads it has finished, so the block needs no fence.
  auto padded = [](size_t bytes) { return (bytes + 255) / 256 * 256; };
  size_t staged_bytes = padded((size_t)total * 24);
  std::vector<size_t> desc_at(kinds.size()), share_at(kinds.size());
  for (size_t q = 0; q < kinds.size(); ++q) {
    curvature_deal_shares(grid_max, &kinds[q].descs, &kinds[q].shares);
    desc_at[q] = staged_bytes;
    staged_bytes += padded(kinds[q].descs.size() * sizeof(CurvatureJob));
    share_at[q] = staged_bytes;
    staged_bytes += padded(kinds[q].shares.size() * 4);
  }
  void* staged = nullptr;
  int slot = 0;
  CURVATURE_TRY(c->pinned.stage(staged_bytes, &staged, &slot, c->align_seen));
  unsigned char* base = static_cast<unsigned char*>(staged);
  for (const CurvatureLive& j : live) std::memcpy(base + 24 * (size_t)j.pose_off, j.poses, 24 * (size_t)j.n_poses);
  for (size_t q = 0; q < kinds.size(); ++q) {
    std::memcpy(base + desc_at[q], kinds[q].descs.data(), kinds[q].descs.size() * sizeof(CurvatureJob));
    std::memcpy(base + share_at[q], kinds[q].shares.data(), kinds[q].shares.size() * 4);
  }
  launched = true;
  CURVATURE_TRY(hipMemcpyAsync(c->poses.p, base, (size_t)total * 24, hipMemcpyHostToDevice, c->stream));
  for (size_t q = 0; q < kinds.size(); ++q) {
    const uint32_t n_shares = (uint32_t)kinds[q].shares.size();
    CURVATURE_TRY(curvature_jobs_launch(kinds[q].path, std::min(n_shares, grid_max), kinds[q].lds, c->stream, base + desc_at[q],
                                        reinterpret_cast<const uint32_t*>(base + share_at[q]), n_shares));
    ++bs->launches;
  }
  std::vector<CurvatureOut> host(total);
  CURVATURE_TRY(hipMemcpyAsync(host.data(), d_out, (size_t)total * sizeof(CurvatureOut), hipMemcpyDeviceToHost, c->stream));
  CURVATURE_TRY(hipStreamSynchronize(c->stream));
  ++bs->waits;
  for (const CurvatureLive& j : live) std::memcpy(j.out, host.data() + j.pose_off, (size_t)j.n_poses * sizeof(CurvatureOut));
  return NDTPSO_OK;
}
#undef CURVATURE_TRY

int curvature_batch_single(ndtpso_map_curvature_job& j, ndtpso_curvature_batch_stats* bs) {
  j.route = 0;
  ++bs->single_jobs;
  j.rc = ndtpso_map_curvature(j.map, j.new_points, j.poses, j.n_poses, j.out);
  return j.rc;
}

}  // namespace

extern "C" int ndtpso_map_curvature(ndtpso_map* m, ndtpso_points* pts, const double* poses, uint32_t n_poses, ndtpso_curvature* out) {
  if (!m || !pts) return NDTPSO_E_ARG;
  ndtpso_ctx* c = m->ctx;
  if (!poses || !out || n_poses == 0) return fail(c, NDTPSO_E_ARG, "null argument");
  if (pts->ctx != c) return fail(c, NDTPSO_E_ARG, "a scan of another context");
  if (n_poses > NDTPSO_CURVATURE_MAX_POSES) return fail(c, NDTPSO_E_ARG, "more than 65536 poses");
  if (!curvature_poses_finite(poses, n_poses)) return fail(c, NDTPSO_E_ARG, "a pose that is not finite");
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = search_prepare_map(m)) return rc;  // (as ndtpso_map_cost)
  if (int rc = map_fetch_header(m)) return rc;
  uint32_t n = 0;
  HIP_TRY(c, hipMemcpy(&n, pts->n_dev.p, 4, hipMemcpyDeviceToHost));
  pts->n_upper = n;
  std::vector<CurvatureLive> live(1);
  live[0] = CurvatureLive{m, pts, poses, n_poses, out, n, Plan{}, 0u};
  if (int rc = curvature_plan(c, m, n, &live[0].plan)) return rc;
  ndtpso_curvature_batch_stats bs;
  std::memset(&bs, 0, sizeof(bs));
  return curvature_launches(c, live, &bs);
}

extern "C" int ndtpso_map_curvature_batch(ndtpso_ctx* c, ndtpso_map_curvature_job* jobs, uint32_t n_jobs,
                                          ndtpso_curvature_batch_stats* stats) {
  if (!c) return NDTPSO_E_ARG;
  if (!jobs || n_jobs == 0) return fail(c, NDTPSO_E_ARG, "no jobs");
  uint64_t poses_all = 0;
  for (uint32_t i = 0; i < n_jobs; ++i) {
    if (!jobs[i].map || !jobs[i].new_points || !jobs[i].poses || !jobs[i].out) return fail(c, NDTPSO_E_ARG, "null argument");
    if (jobs[i].map->ctx != c || jobs[i].new_points->ctx != c) return fail(c, NDTPSO_E_ARG, "a map or scan of another context");
    poses_all += jobs[i].n_poses;
  }
  if (poses_all > NDTPSO_CURVATURE_MAX_POSES) return fail(c, NDTPSO_E_ARG, "the jobs have more than 65536 poses in all");
  ndtpso_curvature_batch_stats bs;
  std::memset(&bs, 0, sizeof(bs));
  if (stats) *stats = bs;
  std::vector<uint32_t> valid;
  for (uint32_t i = 0; i < n_jobs; ++i) {
    ndtpso_map_curvature_job& j = jobs[i];
    j.rc = NDTPSO_OK;
    j.route = 0;
    j.reserved = 0;
    if (j.n_poses == 0) j.rc = fail(c, NDTPSO_E_ARG, "a job without poses");
    else if (!curvature_poses_finite(j.poses, j.n_poses)) j.rc = fail(c, NDTPSO_E_ARG, "a pose that is not finite");
    else valid.push_back(i);
  }
  auto finish = [&]() {
    int first_rc = NDTPSO_OK;
    for (uint32_t i = 0; i < n_jobs && first_rc == NDTPSO_OK; ++i) first_rc = jobs[i].rc;
    if (stats) *stats = bs;
    return first_rc;
  };
  // a failure of the call itself once the launches are being put together: every job that has not failed on its own carries it
  auto abandon = [&](int rc) {
    for (uint32_t i = 0; i < n_jobs; ++i)
      if (jobs[i].rc == NDTPSO_OK) jobs[i].rc = rc;
    if (stats) *stats = bs;
    return rc;
  };
  if (n_jobs == 1) {  // a lone job: exactly ndtpso_map_curvature
    if (!valid.empty()) curvature_batch_single(jobs[0], &bs);
    return finish();
  }
  if (valid.empty()) return finish();
  if (hipSetDevice(c->device) != hipSuccess) return abandon(fail(c, NDTPSO_E_HIP, "hipSetDevice"));

  // ---- every distinct map and scan once, and one wait for all their headers and counts ----------------------------------------
  struct Prepared {
    ndtpso_map* m;
    int rc;
  };
  std::vector<Prepared> maps;
  std::vector<ndtpso_points*> scans;
  std::vector<int> map_of(n_jobs, -1), scan_of(n_jobs, -1);
  for (uint32_t i : valid) {
    for (size_t k = 0; k < maps.size() && map_of[i] < 0; ++k)
      if (maps[k].m == jobs[i].map) map_of[i] = (int)k;
    if (map_of[i] < 0) {
      map_of[i] = (int)maps.size();
      maps.push_back(Prepared{jobs[i].map, NDTPSO_OK});
    }
    for (size_t k = 0; k < scans.size() && scan_of[i] < 0; ++k)
      if (scans[k] == jobs[i].new_points) scan_of[i] = (int)k;
    if (scan_of[i] < 0) {
      scan_of[i] = (int)scans.size();
      scans.push_back(jobs[i].new_points);
    }
  }
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
  for (Prepared& pm : maps)
    if (pm.rc == NDTPSO_OK) pm.rc = map_fetch_header_arrived(pm.m);
  for (size_t k = 0; k < scans.size(); ++k) scans[k]->n_upper = counts[k];

  // ---- every job's plan, by the single call's rule ----------------------------------------------------------------------------
  std::vector<CurvatureLive> live;
  std::vector<uint32_t> live_job;
  for (uint32_t i : valid) {
    ndtpso_map_curvature_job& j = jobs[i];
    CurvatureLive l{j.map, j.new_points, j.poses, j.n_poses, j.out, j.new_points->n_upper, Plan{}, 0u};
    j.rc = maps[(size_t)map_of[i]].rc;
    if (j.rc == NDTPSO_OK) j.rc = curvature_plan(c, j.map, l.n, &l.plan);
    if (j.rc != NDTPSO_OK) continue;
    live.push_back(l);
    live_job.push_back(i);
  }
  // (shared launches for ONE job would be the single call over again: it runs alone, on its prepared map)
  if (live.size() == 1) {
    curvature_batch_single(jobs[live_job[0]], &bs);
    return finish();
  }
  if (live.empty()) return finish();
  if (int rc = curvature_launches(c, live, &bs)) return abandon(rc);
  for (uint32_t i : live_job) jobs[i].route = 1;
  return finish();
}

// The pose covariance of a curvature: the inverse of its Hessian by Cholesky (H = L L^T, cov = L^-T L^-1), and the principal
// axes of the translational block.  Host only.
extern "C" int ndtpso_curvature_covariance(const ndtpso_curvature* cv, ndtpso_pose_covariance* out) {
  if (!cv || !out) return NDTPSO_E_ARG;
  std::memset(out, 0, sizeof(*out));
  const double* h = cv->hessian;  // xx, xy, xth, yy, yth, thth
  for (int i = 0; i < 6; ++i)
    if (!std::isfinite(h[i])) return NDTPSO_OK;
  // Cholesky, row by row; a pivot that is not positive (or not a number) ends it: not definite
  if (!(h[0] > 0.)) return NDTPSO_OK;
  const double l00 = std::sqrt(h[0]);
  const double l10 = h[1] / l00, l20 = h[2] / l00;
  const double p1 = h[3] - l10 * l10;
  if (!(p1 > 0.)) return NDTPSO_OK;
  const double l11 = std::sqrt(p1);
  const double l21 = (h[4] - l20 * l10) / l11;
  const double p2 = h[5] - l20 * l20 - l21 * l21;
  if (!(p2 > 0.)) return NDTPSO_OK;
  const double l22 = std::sqrt(p2);
  // M = L^-1 (lower triangular)
  const double m00 = 1. / l00, m11 = 1. / l11, m22 = 1. / l22;
  const double m10 = -l10 * m00 / l11;
  const double m21 = -l21 * m11 / l22;
  const double m20 = -(l20 * m00 + l21 * m10) / l22;
  // cov = M^T M
  const double c00 = m00 * m00 + m10 * m10 + m20 * m20;
  const double c01 = m10 * m11 + m20 * m21;
  const double c02 = m20 * m22;
  const double c11 = m11 * m11 + m21 * m21;
  const double c12 = m21 * m22;
  const double c22 = m22 * m22;
  const double cov[9] = {c00, c01, c02, c01, c11, c12, c02, c12, c22};
  for (int i = 0; i < 9; ++i)
    if (!std::isfinite(cov[i])) return NDTPSO_OK;  // (an overflow on the way: no verdict to give)
  std::memcpy(out->cov, cov, sizeof(cov));
  // the symmetric 2 x 2 block [c00 c01; c01 c11]: eigenvalues mean +- radius, the major axis at atan2(2 c01, c00 - c11) / 2
  const double mean = (c00 + c11) / 2., half = (c00 - c11) / 2.;
  const double radius = std::hypot(half, c01);
  out->xy_major = mean + radius;
  out->xy_minor = mean - radius;
  double angle = 0.5 * std::atan2(2. * c01, c00 - c11);  // in [-pi/2, pi/2]
  if (angle <= -1.5707963267948966) angle = 1.5707963267948966;
  out->xy_angle = angle;
  out->definite = 1;
  return NDTPSO_OK;
}
