// ndtpso_map_trace.inc -- ndtpso_map_trace, ndtpso_map_trace_batch, ndtpso_map_get_trace_info, ndtpso_map_get_trace and
// ndtpso_map_get_nav_grid: the free space a scan's beams have seen, counted per entry of the map's occupancy grid (kernels:
// ndtpso_map_trace.hip).  The reference has no counterpart.  Included by ndtpso_map.inc behind the curvature.
//
// One host path: trace_launch takes the jobs of a call, checks each by the single call's rule, and enqueues ONE launch over a
// table of the valid ones in a pinned staging block.  The single call is a table of one job.  Nothing here waits for the device,
// settles the map or touches a cell: tracing is an observer.

namespace {

// the single call's refusals of a map and a pose (the call's own -- null pointers, another context -- are checked before)
int trace_check(ndtpso_ctx* c, const ndtpso_map* m, const double pose[3]) {
  if (!std::isfinite(pose[0]) || !std::isfinite(pose[1]) || !std::isfinite(pose[2])) return fail(c, NDTPSO_E_ARG, "a pose that is not finite");
  if (m->og_count == 0) return fail(c, NDTPSO_E_STATE, "the map has no occupancy grid");
  if (m->og_width != m->og_height) return fail(c, NDTPSO_E_ARG, "the occupancy grid is not square: og[x + height * y] makes cells collide");
  return NDTPSO_OK;
}

// the counters and totals as of a map nothing was traced into (enqueued)
int trace_zero(ndtpso_map* m) {
  ndtpso_ctx* c = m->ctx;
  HIP_TRY(c, hipMemsetAsync(m->trace_hits.p, 0, (size_t)m->og_count * 4, c->stream));
  HIP_TRY(c, hipMemsetAsync(m->trace_passes.p, 0, (size_t)m->og_count * 8, c->stream));
  unsigned char* tot = static_cast<unsigned char*>(m->trace_tot.p);
  HIP_TRY(c, hipMemsetAsync(tot, 0, sizeof(TraceTotals), c->stream));
  HIP_TRY(c, hipMemsetAsync(tot + offsetof(TraceTotals, min_x), 0xff, 4, c->stream));
  HIP_TRY(c, hipMemsetAsync(tot + offsetof(TraceTotals, min_y), 0xff, 4, c->stream));
  return NDTPSO_OK;
}

// allocated and zeroed at a map's first trace: a map that is never traced pays nothing
int trace_ensure(ndtpso_map* m) {
  if (m->trace_tot.p) return NDTPSO_OK;
  ndtpso_ctx* c = m->ctx;
  hipError_t e = m->trace_hits.reserve((size_t)m->og_count * 4);
  if (e == hipSuccess) e = m->trace_passes.reserve((size_t)m->og_count * 8);
  if (e == hipSuccess) e = m->trace_tot.reserve(256);
  if (e != hipSuccess) {
    m->trace_hits.release();
    m->trace_passes.release();
    m->trace_tot.release();
    return fail(c, NDTPSO_E_HIP, std::string("the trace counters: ") + hipGetErrorString(e));
  }
  const int rc = trace_zero(m);
  if (rc != NDTPSO_OK) {
    (void)hipStreamSynchronize(c->stream);
    m->trace_hits.release();
    m->trace_passes.release();
    m->trace_tot.release();
  }
  return rc;
}

bool trace_aggregates() {
  static const bool on = [] {
    const char* e = std::getenv("NDTPSO_TRACE_AGGREGATE");  // tuning / measurement knob: =0 every lane adds its own origin pass
    return !(e && e[0] == '0');
  }();
  return on;
}

// every job checked by the single call's rule, the valid ones in one launch; returns the first failing job's rc
int trace_launch(ndtpso_ctx* c, ndtpso_map_trace_job* jobs, uint32_t n_jobs) {
  HIP_TRY(c, hipSetDevice(c->device));
  std::vector<TraceJob> descs;
  std::vector<uint32_t> desc_job;
  unsigned blocks = 0;
  for (uint32_t i = 0; i < n_jobs; ++i) {
    ndtpso_map_trace_job& j = jobs[i];
    ndtpso_map* m = j.map;
    j.reserved = 0;
    if ((j.rc = trace_check(c, m, j.pose)) != NDTPSO_OK) continue;
    const uint32_t n = j.points->n_upper;
    if ((uint64_t)n > 65535ull * kTraceThreads) {
      j.rc = fail(c, NDTPSO_E_CAPACITY, "a scan of more than 65535 * 256 points");
      continue;
    }
    if ((j.rc = trace_ensure(m)) != NDTPSO_OK) continue;
    if (n == 0) continue;  // an empty scan is no error
    TraceJob d;
    std::memset(&d, 0, sizeof(d));
    d.xy = (const double2*)j.points->xy.p;
    d.n_ptr = (const uint32_t*)j.points->n_dev.p;
    d.hits = (uint32_t*)m->trace_hits.p;
    d.passes = (unsigned long long*)m->trace_passes.p;
    d.tot = (TraceTotals*)m->trace_tot.p;
    d.theta = j.pose[2];
    d.tx = j.pose[0];
    d.ty = j.pose[1];
    d.hw = m->grid.width / 2.;
    d.hh = m->grid.height / 2.;
    d.cs = m->og_cell_size;
    d.og_height = m->og_height;
    d.og_count = m->og_count;
    d.n = n;
    blocks = std::max(blocks, (n + kTraceThreads - 1) / kTraceThreads);
    descs.push_back(d);
    desc_job.push_back(i);
  }
  if (!descs.empty()) {
    void* staged = nullptr;
    int slot = 0;
    int rc = NDTPSO_OK;
    const hipError_t e = c->pinned.stage(descs.size() * sizeof(TraceJob), &staged, &slot, c->align_seen);
    if (e != hipSuccess) {
      rc = fail(c, NDTPSO_E_HIP, std::string("staging the traces: ") + hipGetErrorString(e));
    } else {
      std::memcpy(staged, descs.data(), descs.size() * sizeof(TraceJob));
      const hipError_t le = trace_jobs_launch(c->stream, staged, (unsigned)descs.size(), blocks, trace_aggregates() ? 1 : 0);
      stage_fence(c, slot);  // read by a kernel that precedes the context's next alignment on the stream, as a scan load's block is
      if (le != hipSuccess) rc = fail(c, NDTPSO_E_HIP, std::string("k_trace_jobs: ") + hipGetErrorString(le));
    }
    if (rc != NDTPSO_OK)
      for (uint32_t i : desc_job) jobs[i].rc = rc;
  }
  for (uint32_t i = 0; i < n_jobs; ++i)
    if (jobs[i].rc != NDTPSO_OK) return jobs[i].rc;
  return NDTPSO_OK;
}

}  // namespace

extern "C" int ndtpso_map_trace(ndtpso_map* m, const ndtpso_points* pts, const double pose[3]) {
  if (!m || !pts) return NDTPSO_E_ARG;
  ndtpso_ctx* c = m->ctx;
  if (!pose) return fail(c, NDTPSO_E_ARG, "null argument");
  if (pts->ctx != c) return fail(c, NDTPSO_E_ARG, "a scan of another context");
  ndtpso_map_trace_job j;
  std::memset(&j, 0, sizeof(j));
  j.map = m;
  j.points = pts;
  std::memcpy(j.pose, pose, sizeof(j.pose));
  return trace_launch(c, &j, 1);
}

extern "C" int ndtpso_map_trace_batch(ndtpso_ctx* c, ndtpso_map_trace_job* jobs, uint32_t n_jobs) {
  if (!c) return NDTPSO_E_ARG;
  if (!jobs || n_jobs == 0) return fail(c, NDTPSO_E_ARG, "no jobs");
  for (uint32_t i = 0; i < n_jobs; ++i) {
    if (!jobs[i].map || !jobs[i].points) return fail(c, NDTPSO_E_ARG, "null argument");
    if (jobs[i].map->ctx != c || jobs[i].points->ctx != c) return fail(c, NDTPSO_E_ARG, "a map or scan of another context");
  }
  return trace_launch(c, jobs, n_jobs);
}

extern "C" int ndtpso_map_get_trace_info(ndtpso_map* m, ndtpso_trace_info* info) {
  if (!m || !info) return NDTPSO_E_ARG;
  ndtpso_ctx* c = m->ctx;
  std::memset(info, 0, sizeof(*info));
  info->width = m->og_width;
  info->height = m->og_height;
  info->extent[0] = info->extent[2] = UINT32_MAX;
  if (!m->trace_tot.p) return NDTPSO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  TraceTotals t;
  HIP_TRY(c, hipMemcpyAsync(&t, m->trace_tot.p, sizeof(t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  info->allocated = 1;
  info->extent[0] = t.min_x;
  info->extent[1] = t.max_x;
  info->extent[2] = t.min_y;
  info->extent[3] = t.max_y;
  info->n_rays = t.n_rays;
  info->n_skipped = t.n_skipped;
  info->n_steps = t.n_steps;
  return NDTPSO_OK;
}

extern "C" int ndtpso_map_get_trace(ndtpso_map* m, uint32_t* hits, uint64_t* passes, uint64_t capacity_entries) {
  if (!m) return NDTPSO_E_ARG;
  ndtpso_ctx* c = m->ctx;
  if ((hits || passes) && capacity_entries < m->og_count) return fail(c, NDTPSO_E_ARG, "trace buffer too small");
  if (!m->og_count) return NDTPSO_OK;
  if (!m->trace_tot.p) {  // never traced: zeros
    if (hits) std::memset(hits, 0, (size_t)m->og_count * 4);
    if (passes) std::memset(passes, 0, (size_t)m->og_count * 8);
    return NDTPSO_OK;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  if (hits) HIP_TRY(c, hipMemcpyAsync(hits, m->trace_hits.p, (size_t)m->og_count * 4, hipMemcpyDeviceToHost, c->stream));
  if (passes) HIP_TRY(c, hipMemcpyAsync(passes, m->trace_passes.p, (size_t)m->og_count * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return NDTPSO_OK;
}

extern "C" int ndtpso_map_get_nav_grid(ndtpso_map* m, int8_t* grid, uint64_t bytes) {
  if (!m) return NDTPSO_E_ARG;
  ndtpso_ctx* c = m->ctx;
  if (!grid) return fail(c, NDTPSO_E_ARG, "null argument");
  if (!m->og_count) return fail(c, NDTPSO_E_STATE, "the map has no occupancy grid");
  if (bytes < m->og_count) return fail(c, NDTPSO_E_ARG, "nav grid buffer too small");
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = map_settle(m)) return rc;  // (as ndtpso_map_get_occupancy)
  if (int rc = map_fetch_header(m)) return rc;
  HIP_TRY(c, m->nav.reserve((size_t)m->og_count));
  HIP_TRY(c, nav_grid_launch(c->stream, (const unsigned long long*)m->og_key.p, (const uint32_t*)m->trace_hits.p,
                             (const unsigned long long*)m->trace_passes.p, m->og_count, (int8_t*)m->nav.p));
  HIP_TRY(c, hipMemcpyAsync(grid, m->nav.p, (size_t)m->og_count, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return NDTPSO_OK;
}
