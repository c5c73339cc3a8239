// ndtpso_map_update.inc -- ndtpso_points_load_scans and ndtpso_map_update_batch: the scan loads and the map updates of several
// single calls of one context in shared launches (ndtpso_map_jobs.hip).  Included by ndtpso_map.inc behind the single calls,
// whose steps (scan_load_check / scan_load_job; map_insert_prepare / _job / _after; map_speculate_prepare / _job / _after) both
// paths run: there is one statement of the bookkeeping.

namespace {

// A staged block -- descriptor tables, and for loads the ranges -- is read by kernels that precede the context's next alignment
// on the stream: its slot is free once that alignment has reported, as a single load's is (PinnedRing::fence_until).  One block
// per set of launches, so a step of R robots holds one slot per phase where R single loads went round the ring and waited.
void stage_fence(ndtpso_ctx* c, int slot) { c->pinned.fence_until(slot, c->stream, c->align_issued + 1); }

bool beam_directions_cached(const ndtpso_ctx* c, const ndtpso_scan_geom* s) {
  for (const BeamDirs& b : c->beam_dirs)
    if (b.n == s->n_beams && b.amin == s->min_angle && b.ainc == s->angle_increment && b.buf.p) return true;
  return false;
}

int load_single(ndtpso_points_load_job& j) {
  j.rc = ndtpso_points_load_scan(j.pts, j.ranges, &j.geom, (j.flags & 1u) ? j.trans : nullptr, (j.flags & 2u) ? &j.clip : nullptr,
                                 (j.flags & 4u) ? 1 : 0);
  return j.rc;
}

int update_single(ndtpso_map_update_job& j) {  // the single calls an update job stands for
  j.route = 0;
  j.rc = ndtpso_map_mark_unbuilt(j.map);
  if (j.rc == NDTPSO_OK) j.rc = ndtpso_map_insert(j.map, j.points, (j.flags & 1u) ? j.pose : nullptr);
  if (j.rc == NDTPSO_OK && (j.flags & 2u)) j.rc = ndtpso_map_speculate_build(j.map);
  return j.rc;
}

}  // namespace

extern "C" int ndtpso_points_load_scans(ndtpso_ctx* c, ndtpso_points_load_job* jobs, uint32_t n_jobs) {
  if (!c) return NDTPSO_E_ARG;
  if (!jobs || n_jobs == 0) return fail(c, NDTPSO_E_ARG, "no jobs");
  for (uint32_t i = 0; i < n_jobs; ++i) {
    if (!jobs[i].pts || !jobs[i].ranges) return fail(c, NDTPSO_E_ARG, "null argument");
    if (jobs[i].pts->ctx != c) return fail(c, NDTPSO_E_ARG, "a scan of another context");
  }
  for (uint32_t i = 0; i < n_jobs; ++i) jobs[i].rc = NDTPSO_OK;
  if (n_jobs == 1) return load_single(jobs[0]);  // a lone load: exactly ndtpso_points_load_scan
  HIP_TRY(c, hipSetDevice(c->device));

  std::vector<uint32_t> set;  // the jobs of the launch being put together
  std::vector<ScanLoadJob> desc;
  auto flush = [&]() -> int {
    if (set.empty()) return NDTPSO_OK;
    const size_t table = round_up((int)(desc.size() * sizeof(ScanLoadJob)), 256);
    size_t bytes = table;
    for (uint32_t i : set) bytes += round_up((int)(jobs[i].geom.n_beams * 4u), 16);
    void* staged = nullptr;
    int slot = 0;
    int rc = NDTPSO_OK;
    const hipError_t e = c->pinned.stage(bytes, &staged, &slot, c->align_seen);
    if (e != hipSuccess) {
      rc = fail(c, NDTPSO_E_HIP, std::string("staging the scans: ") + hipGetErrorString(e));
    } else {
      unsigned char* at = static_cast<unsigned char*>(staged) + table;
      for (size_t k = 0; k < set.size(); ++k) {
        const ndtpso_points_load_job& j = jobs[set[k]];
        std::memcpy(at, j.ranges, (size_t)j.geom.n_beams * 4);
        desc[k].ranges = reinterpret_cast<const float*>(at);
        at += round_up((int)(j.geom.n_beams * 4u), 16);
      }
      std::memcpy(staged, desc.data(), desc.size() * sizeof(ScanLoadJob));
      scan_jobs_launch(c->stream, staged, (unsigned)desc.size());
      const hipError_t le = hipGetLastError();
      stage_fence(c, slot);
      if (le != hipSuccess) rc = fail(c, NDTPSO_E_HIP, std::string("k_scans_to_resident_jobs: ") + hipGetErrorString(le));
    }
    if (rc != NDTPSO_OK)
      for (uint32_t i : set) jobs[i].rc = rc;
    set.clear();
    desc.clear();
    return rc;
  };

  for (uint32_t i = 0; i < n_jobs; ++i) {
    ndtpso_points_load_job& j = jobs[i];
    const int append = (j.flags & 4u) ? 1 : 0;
    bool again = false;
    for (uint32_t k : set) again = again || jobs[k].pts == j.pts;
    if (again) (void)flush();
    uint32_t upper = 0;
    if ((j.rc = scan_load_check(j.pts, j.ranges, &j.geom, append, &upper)) != NDTPSO_OK) continue;
    // (a geometry whose beam directions are yet to be made takes a slot of the context's small cache, perhaps one that a job of
    // the set not yet launched points at)
    if (!beam_directions_cached(c, &j.geom)) (void)flush();
    ScanLoadJob d;
    if ((j.rc = scan_load_job(j.pts, nullptr, &j.geom, (j.flags & 1u) ? j.trans : nullptr, (j.flags & 2u) ? &j.clip : nullptr, append,
                              &d)) != NDTPSO_OK)
      continue;
    j.pts->n_upper = upper;
    set.push_back(i);
    desc.push_back(d);
  }
  (void)flush();
  for (uint32_t i = 0; i < n_jobs; ++i)
    if (jobs[i].rc != NDTPSO_OK) return jobs[i].rc;
  return NDTPSO_OK;
}

extern "C" int ndtpso_map_update_batch(ndtpso_ctx* c, ndtpso_map_update_job* jobs, uint32_t n_jobs) {
  if (!c) return NDTPSO_E_ARG;
  if (!jobs || n_jobs == 0) return fail(c, NDTPSO_E_ARG, "no jobs");
  for (uint32_t i = 0; i < n_jobs; ++i) {
    if (!jobs[i].map || !jobs[i].points) return fail(c, NDTPSO_E_ARG, "null argument");
    if (jobs[i].map->ctx != c || jobs[i].points->ctx != c) return fail(c, NDTPSO_E_ARG, "a map or scan of another context");
  }
  for (uint32_t i = 0; i < n_jobs; ++i) {
    jobs[i].rc = NDTPSO_OK;
    jobs[i].route = 0;
  }
  if (n_jobs == 1) return update_single(jobs[0]);  // a lone update: exactly the single calls
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->map_jobs_big_lds) {  // (k_map_pack's own attribute is set by ndtpso_map_create)
    HIP_TRY(c, map_jobs_allow_big_lds());
    c->map_jobs_big_lds = true;
  }

  // the set of launches being put together: the inserting jobs' descriptors, the building jobs' descriptors
  std::vector<uint32_t> set;
  std::vector<MapUpdateJob> ins, bld;
  unsigned build_blocks = 0;
  int pack_lds = 0;
  auto flush = [&]() -> int {
    if (set.empty()) return NDTPSO_OK;
    int rc = NDTPSO_OK;
    if (!ins.empty() || !bld.empty()) {
      const size_t ins_bytes = round_up((int)(ins.size() * sizeof(MapUpdateJob)), 256);
      void* staged = nullptr;
      int slot = 0;
      const hipError_t e = c->pinned.stage(ins_bytes + bld.size() * sizeof(MapUpdateJob), &staged, &slot, c->align_seen);
      if (e != hipSuccess) {
        rc = fail(c, NDTPSO_E_HIP, std::string("staging the updates: ") + hipGetErrorString(e));
      } else {
        unsigned char* d_bld = static_cast<unsigned char*>(staged) + ins_bytes;
        if (!ins.empty()) std::memcpy(staged, ins.data(), ins.size() * sizeof(MapUpdateJob));
        if (!bld.empty()) std::memcpy(d_bld, bld.data(), bld.size() * sizeof(MapUpdateJob));
        hipError_t le = hipSuccess;
        if (!ins.empty()) {
          map_insert_jobs_launch(c->stream, staged, (unsigned)ins.size());
          le = hipGetLastError();
        }
        if (le == hipSuccess && !bld.empty() && build_blocks) {
          map_build_jobs_launch(c->stream, d_bld, (unsigned)bld.size(), build_blocks);
          le = hipGetLastError();
        }
        if (le == hipSuccess && !bld.empty()) {
          map_pack_jobs_launch(c->stream, d_bld, (unsigned)bld.size(), pack_lds);
          le = hipGetLastError();
        }
        stage_fence(c, slot);
        if (le != hipSuccess) rc = fail(c, NDTPSO_E_HIP, std::string("the update launches: ") + hipGetErrorString(le));
      }
    }
    for (uint32_t i : set) {
      jobs[i].route = 1;
      if (rc != NDTPSO_OK) jobs[i].rc = rc;
    }
    set.clear();
    ins.clear();
    bld.clear();
    build_blocks = 0;
    pack_lds = 0;
    return rc;
  };

  for (uint32_t i = 0; i < n_jobs; ++i) {
    ndtpso_map_update_job& j = jobs[i];
    ndtpso_map* m = j.map;
    bool again = false;
    for (uint32_t k : set) again = again || jobs[k].map == m;
    if (again) (void)flush();  // per map, job order
    const uint32_t n_upper = j.points->n_upper;
    const bool inserts = !map_insert_skips(n_upper, 1);
    // what the single calls would do next, asked of the map as ndtpso_map_mark_unbuilt leaves it: does any step wait for the device?
    const bool builds = (j.flags & 2u) && (inserts || !m->spec);
    if ((inserts && map_insert_asks_device(m, n_upper, 1)) ||
        (builds && map_speculate_allocates(m, m->points_upper + (inserts ? n_upper : 0u)))) {
      (void)flush();
      update_single(j);
      continue;
    }
    if ((j.rc = ndtpso_map_mark_unbuilt(m)) != NDTPSO_OK) continue;
    MapUpdateJob d;
    std::memset(&d, 0, sizeof(d));
    if (inserts) {
      InsertPrep prep;
      if ((j.rc = map_insert_prepare(m, n_upper, 1, &prep)) != NDTPSO_OK) continue;  // (a pending speculation's k_map_undo goes out here)
      d = map_insert_job(m, (const double2*)j.points->xy.p, n_upper, (const uint32_t*)j.points->n_dev.p, (j.flags & 1u) ? j.pose : nullptr);
      ins.push_back(d);
      if ((j.rc = map_insert_after(m, n_upper, prep)) != NDTPSO_OK) {
        ins.pop_back();
        continue;
      }
    }
    if ((j.flags & 2u) && map_speculate_wanted(m)) {
      if ((j.rc = map_speculate_prepare(m)) == NDTPSO_OK) {
        map_speculate_job(m, &d);
        bld.push_back(d);
        build_blocks = std::max(build_blocks, (created_upper(m) + 31u) / 32u);
        pack_lds = std::max(pack_lds, map_pack_lds(m));
        map_speculate_after(m);
      }
    }
    set.push_back(i);
  }
  (void)flush();
  for (uint32_t i = 0; i < n_jobs; ++i)
    if (jobs[i].rc != NDTPSO_OK) return jobs[i].rc;
  return NDTPSO_OK;
}
