// NDTFrame of the MI355X build: grid bookkeeping on the host, arithmetic on the GPU (see ndtframe.h).
// Reference behaviour cited as lib/ndtpso_slam/ndtframe.cpp:LINE.
#include "ndtpso_slam/ndtframe.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "device.h"
#include "ndtpso_slam/core.h"
#include "raster.h"

namespace {
ndtpso_grid grid_of(const NDTFrame& f) { return ndtpso_grid{f.width, f.height, f.cell_side}; }

ndtpso_pso_config to_abi(const PSOConfig& c) {
  ndtpso_pso_config o;
  o.iterations = c.iterations;
  o.population = c.populationSize;
  o.num_threads = c.num_threads;
  o.w = c.coeff.w;
  o.c1 = c.coeff.c1;
  o.c2 = c.coeff.c2;
  o.w_damping = c.coeff.w_dumping;
  return o;
}
thread_local bool t_last_align_failed = false;  // the calling thread's most recent align() / pso_optimization could not run
constexpr uint32_t kScanCapacity = 4096;  // points of a pooled device scan buffer (grown for longer scans)

uint64_t map_pool_bytes(unsigned num_cells) {
  // 512 B per 32 points of one window slot.  A one-cell frame that is only ever updated (the node's global_map_,
  // ndtpso_slam_node.cpp:70-72,200-203) is never built, so it never rotates and keeps every point it was given.
  const char* e = std::getenv(num_cells == 1 ? "NDTPSO_GLOBAL_MAP_POOL_MB" : "NDTPSO_MAP_POOL_MB");
  // (a fraction is taken as one: "0.03125" is a pool of 64 chunks, which the tests of the exhaustion path fill with one scan)
  const double mb = e ? std::strtod(e, nullptr) : (num_cells == 1 ? 4096. : 1024.);
  return (uint64_t)((mb > 0. ? mb : 1.) * 1048576.);
}
}  // namespace

// reference: constructor, ndtframe.cpp:19-66.  Cells are light (see ndtcell.h), so the dense vector is kept.
NDTFrame::NDTFrame(Vector3d trans, unsigned short width_, unsigned short height_, double cell_side_,
                   bool init_cell_windows, NDTPSOConfig config
#if BUILD_OCCUPANCY_GRID
                   ,
                   double occupancy_grid_cell_size
#endif
                   )
    : width(width_), height(height_), built(false), cell_side(cell_side_), s_trans(std::move(trans)),
      s_config(std::move(config)) {
  widthNumOfCells = uint16_t(std::ceil(width / cell_side));    // ndtframe.cpp:27
  heightNumOfCells = uint16_t(std::ceil(height / cell_side));  // ndtframe.cpp:28
  numOfCells = widthNumOfCells * heightNumOfCells;
  cells = vector<NDTCell>(numOfCells, NDTCell(init_cell_windows));
  s_x_min = -width / 2.;
  s_x_max = width / 2.;
  s_y_min = -height / 2.;
  s_y_max = height / 2.;
  // (a resident frame has fewer than 2^21 cells -- ndtpso_map_create, the insert's 32-bit sort key; the reference's `unsigned int
  // numOfCells` has no such bound: 300 m at 0.2 m cells is 2.25 M -- so a larger frame keeps its cells here, on the host's side of
  // the C-ABI, as every frame did before round 3: same device kernels for the table, the score and the PSO, same results)
  s_resident = ndtpso_host::resident_default() && numOfCells < (1u << 21);
#if BUILD_OCCUPANCY_GRID
  s_occupancy_grid.cell_size = occupancy_grid_cell_size;  // ndtframe.cpp:32-46; 0 = no grid (intermediate frames)
  if (occupancy_grid_cell_size > 0.) {
    s_occupancy_grid.width = uint32_t(std::ceil(width / occupancy_grid_cell_size));
    s_occupancy_grid.height = uint32_t(std::ceil(height / occupancy_grid_cell_size));
    s_occupancy_grid.count = s_occupancy_grid.width * s_occupancy_grid.height;
    s_occupancy_grid.og = vector<int8_t>(s_occupancy_grid.count, 0);
  }
#endif
}

ndtpso_host::Ctx* NDTFrame::dev() const {
  if (!s_dev) {
    s_dev = ndtpso_host::thread_ctx();
    ndtpso_host::bind_frame(s_dev);
  }
  return s_dev;
}

NDTFrame::~NDTFrame() {
  if (d_scan_ || d_map_) {
    ndtpso_host::Use use(dev());
    if (d_scan_) ndtpso_host::release_scan(d_scan_, d_scan_cap_);
    if (d_map_ && ndtpso_host::alive()) ndtpso_map_destroy(d_map_);
  }
  if (s_dev) ndtpso_host::unbind_frame(s_dev);
}

// ---- resident mode: the frame's state lives on the device (include/ndtpso_hip.h, ndtpso_map_* / ndtpso_points_*) ----

// A one-cell frame that only had scans loaded is just a point list (d_scan_).  Anything else -- several cells, or an
// update / addPoint / build on it -- is a map; a point list already loaded becomes the open slot of cell 0.
ndtpso_map* NDTFrame::ensureMap() {
  if (!d_map_) {
    const ndtpso_grid grid = grid_of(*this);
    double og_cell_size = 0.;
#if BUILD_OCCUPANCY_GRID
    og_cell_size = s_occupancy_grid.cell_size;
#endif
    if (!ndtpso_host::check(ndtpso_map_create(ndtpso_host::device(), &grid, og_cell_size, map_pool_bytes(numOfCells), &d_map_),
                            "device map")) {
      d_map_ = nullptr;  // every map call on this frame is then refused by the C-ABI (null handle) and skipped
      return nullptr;
    }
    if (d_scan_) {
      ndtpso_host::check(ndtpso_map_insert(d_map_, d_scan_, nullptr), "device map");
      ndtpso_host::release_scan(d_scan_, d_scan_cap_);
      d_scan_ = nullptr;
      d_scan_upper_ = 0;
    }
  }
  return d_map_;
}

void NDTFrame::residentPoints(bool slot0_only, std::vector<double>& xy) const {
  xy.clear();
  if (d_map_) {
    uint64_t n = 0;
    if (!ndtpso_host::check(ndtpso_map_get_points(d_map_, slot0_only ? 1 : 0, nullptr, 0, &n), "map points")) return;
    xy.resize(2 * (size_t)n);
    if (n && !ndtpso_host::check(ndtpso_map_get_points(d_map_, slot0_only ? 1 : 0, xy.data(), n, &n), "map points")) xy.clear();
  } else if (d_scan_) {
    uint32_t n = 0;
    xy.resize(2 * (size_t)d_scan_upper_);
    if (!ndtpso_host::check(ndtpso_points_get(d_scan_, xy.data(), d_scan_upper_, &n), "scan points")) n = 0;
    xy.resize(2 * (size_t)n);
  }
}

void NDTFrame::syncHostView() {
  ndtpso_host::Use use(dev());
  if (!s_resident) return;
  if (!d_map_) {
    if (d_scan_) {  // a one-cell frame holding loaded scans: its only cell exists as soon as one point survived
      uint32_t n = 0;
      if (!ndtpso_host::check(ndtpso_points_get(d_scan_, nullptr, 0, &n), "scan points")) return;
      cells[0].created = cells[0].created || n > 0;
    }
    return;
  }
  uint32_t n = 0;
  if (!ndtpso_host::check(ndtpso_map_get_cells(d_map_, nullptr, 0, &n), "map cells")) return;
  std::vector<ndtpso_cell_row> rows(n ? n : 1);
  if (!ndtpso_host::check(ndtpso_map_get_cells(d_map_, rows.data(), n, &n), "map cells")) return;
  for (NDTCell& c : cells) c.created = c.built = false;
  for (uint32_t k = 0; k < n; ++k) {
    NDTCell& c = cells[(size_t)rows[k].index];
    c.created = true;
    c.built = rows[k].built != 0;
    c.mean = Vector2d(rows[k].mean[0], rows[k].mean[1]);
  }
}

// points + their cells (as binned on the device) -> per-cell open slots; NDTFrame::addPoint's effect, ndtframe.cpp:215-235
void NDTFrame::append(const double* xy, const int32_t* idx, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) {
    if (idx[i] < 0 || (unsigned)idx[i] >= numOfCells) continue;  // outside the frame: dropped (ndtframe.cpp:220)
    NDTCell& c = cells[(size_t)idx[i]];
    if (!c.created) s_created.push_back((uint32_t)idx[i]);
    c.addPoint(Vector2d(xy[2 * i], xy[2 * i + 1]));
    built = false;
  }
  s_table_dirty = true;
}

// reference: loadLaser, ndtframe.cpp:144-185 (beam filter, fp32 angle, fp64 polar->xy, s_trans, binning)
void NDTFrame::loadLaser(const vector<float>& laser_data, const float& min_angle, const float& angle_increment,
                         const float& max_range) {
  ndtpso_host::Use use(dev());
  built = false;
  const uint32_t n = (uint32_t)laser_data.size();
  if (n == 0) {
    // ndtframe.cpp:145 clears `built` before anything else: an empty scan still makes the next cost_function() build
    // again, and a build repeated on unchanged cells is not a no-op in floating point (include/ndtpso_hip.h)
    if (s_resident && d_map_) ndtpso_host::check(ndtpso_map_mark_unbuilt(d_map_), "loadLaser");
    return;
  }
  ndtpso_ctx* dev = ndtpso_host::device();
  ndtpso_scan_geom geom{n, min_angle, angle_increment, max_range, s_config.laserIgnoreEpsilon};
  const double t[3] = {s_trans.x(), s_trans.y(), s_trans.z()};
  if (s_resident) {
    const ndtpso_grid frame = grid_of(*this);
    if (numOfCells == 1 && !d_map_) {  // the node's per-scan frame: the scan stays a point list on the device
      if (!d_scan_) {
        d_scan_cap_ = std::max(kScanCapacity, n);
        d_scan_ = ndtpso_host::acquire_scan(d_scan_cap_);
        d_scan_upper_ = 0;
        if (!d_scan_) return;  // no device memory: the scan is dropped (error recorded)
      }
      if (d_scan_upper_ + n <= d_scan_cap_) {
        if (ndtpso_host::check(ndtpso_points_load_scan(d_scan_, laser_data.data(), &geom, t, &frame, d_scan_upper_ > 0), "loadLaser"))
          d_scan_upper_ += n;
        return;
      }
    }
    ndtpso_map* m = ensureMap();
    if (!ndtpso_host::check(ndtpso_map_mark_unbuilt(m), "loadLaser")) return;  // ndtframe.cpp:145
    const uint32_t cap = std::max(kScanCapacity, n);
    ndtpso_points* tmp = ndtpso_host::acquire_scan(cap);
    if (ndtpso_host::check(ndtpso_points_load_scan(tmp, laser_data.data(), &geom, t, nullptr, 0), "loadLaser"))
      ndtpso_host::check(ndtpso_map_insert(m, tmp, nullptr), "loadLaser");
    ndtpso_host::release_scan(tmp, cap);  // stream order keeps the buffer intact until the insert has read it
    return;
  }
  std::vector<double> xy(2 * (size_t)n);
  std::vector<int32_t> idx(n);
  uint32_t kept = 0;
  const ndtpso_grid grid = grid_of(*this);
  if (!ndtpso_host::check(ndtpso_scan_to_cells(dev, laser_data.data(), &geom, t, &grid, xy.data(), idx.data(), &kept), "loadLaser"))
    return;
  append(xy.data(), idx.data(), kept);
}

void NDTFrame::collectPoints(std::vector<double>& xy) const {
  ndtpso_host::Use use(dev());
  xy.clear();
  if (s_resident) {
    residentPoints(true, xy);
    return;
  }
  if (numOfCells == 1) {  // the node's per-scan frame (ndtpso_slam_node.cpp:229-230)
    for (const Vector2d& p : cells[0].points_vector[0]) {
      xy.push_back(p.x());
      xy.push_back(p.y());
    }
    return;
  }
  for (const NDTCell& c : cells) {  // cell order, then insertion order (core.cpp:33-36)
    if (!c.created) continue;
    for (const Vector2d& p : c.points_vector[0]) {
      xy.push_back(p.x());
      xy.push_back(p.y());
    }
  }
}

namespace {
bool speculate_after_update() {
  static const bool speculate = [] {
    const char* e = std::getenv("NDTPSO_SPECULATE");  // =0: leave every build to the call that asks for it
    return !(e && e[0] == '0');
  }();
  return speculate;
}
const char* const kUpdateRefused = "update after a failed align (scan not merged)";
}  // namespace

// reference: update, ndtframe.cpp:187-198 (transform every slot-0 point of new_frame by `trans`, re-bin here)
void NDTFrame::update(Vector3d trans, NDTFrame* const new_frame) {
  // The node merges every scan at the pose align() has just returned (ndtpso_slam_node.cpp:194-198) and never asks whether
  // that alignment ran: the reference's cannot fail.  Here it can (a device fault: align() then returns its initial guess,
  // lastAlignOk() says so), and a scan merged at an unrefined guess would corrupt the map for good.  So an update() that
  // follows a failed align() against this frame is REFUSED -- the scan is dropped, counted (updatesRefused()) and recorded
  // in the error state (ndtpso_slam/status.h) -- and the next successful align() clears the condition.
  // ... and so is an update() of ANY frame by the thread whose most recent align() failed: the node merges the same pose into
  // its global map as well (global_map_->update, ndtpso_slam_node.cpp:202), a frame that never aligns and so never learns of it.
  if (!s_last_align_ok || t_last_align_failed) {
    ++s_updates_refused;
    ndtpso_host::check(NDTPSO_E_STATE, kUpdateRefused);
    return;
  }
  // a frame that lives in another thread's device context: its points travel through the host (collected under ITS context)
  std::vector<double> foreign;
  const bool is_foreign = new_frame->dev() != dev();
  if (is_foreign) new_frame->collectPoints(foreign);
  ndtpso_host::Use use(dev());
  built = false;
  if (s_resident) {
    const double pose[3] = {trans.x(), trans.y(), trans.z()};
    ndtpso_map* m = ensureMap();
    if (!ndtpso_host::check(ndtpso_map_mark_unbuilt(m), "update")) return;  // ndtframe.cpp:188, also when no point follows
    std::vector<double> pts;
    const bool on_device = !is_foreign && new_frame->s_resident && new_frame->d_scan_ && !new_frame->d_map_;
    if (on_device) {  // device to device, nothing to wait for
      if (!ndtpso_host::check(ndtpso_map_insert(m, new_frame->d_scan_, pose), "update")) return;
    } else {
      if (is_foreign) pts.swap(foreign); else new_frame->collectPoints(pts);
      if (!ndtpso_host::check(ndtpso_map_insert_host(m, pts.data(), (uint32_t)(pts.size() / 2), pose), "update")) return;
    }
    // A frame that is aligned against gets its cells built and its table packed right away, off the next align()'s
    // critical path; should something other than align / build come first, the device takes the build back
    // (ndtpso_map_speculate_build), so the lazy build of the reference is what every caller still observes.
    if (s_iter > 0 && speculate_after_update()) ndtpso_host::check(ndtpso_map_speculate_build(m), "update");
    if (s_trace_on_update && traceRefusal()) {  // (as traceFreeSpace refuses)
      ndtpso_host::check(NDTPSO_E_STATE, (std::string("update: trace: ") + traceRefusal()).c_str());
    } else if (s_trace_on_update) {  // the same scan at the same pose through the occupancy grid (setTraceOnUpdate), behind the build
      if (on_device) {
        ndtpso_host::check(ndtpso_map_trace(m, new_frame->d_scan_, pose), "update: trace");
      } else {
        const uint32_t cap = std::max(kScanCapacity, (uint32_t)(pts.size() / 2));
        ndtpso_points* tmp = ndtpso_host::acquire_scan(cap);
        if (ndtpso_host::check(ndtpso_points_set(tmp, pts.data(), (uint32_t)(pts.size() / 2)), "update: trace"))
          ndtpso_host::check(ndtpso_map_trace(m, tmp, pose), "update: trace");
        ndtpso_host::release_scan(tmp, cap);
      }
    }
    return;
  }
  if (s_trace_on_update) ndtpso_host::check(NDTPSO_E_STATE, (std::string("update: trace: ") + traceRefusal()).c_str());  // (as traceFreeSpace refuses)
  std::vector<double> xy;
  if (is_foreign) xy.swap(foreign); else new_frame->collectPoints(xy);
  const uint32_t n = (uint32_t)(xy.size() / 2);
  if (n == 0) return;
  std::vector<int32_t> idx(n);
  const double t[3] = {trans.x(), trans.y(), trans.z()};
  const ndtpso_grid grid = grid_of(*this);
  if (!ndtpso_host::check(ndtpso_points_to_cells(ndtpso_host::device(), &grid, xy.data(), n, t, xy.data(), idx.data()), "update"))
    return;
  append(xy.data(), idx.data(), n);
}

// north star's addScan(): loadLaser() into a one-cell per-scan frame + update() with it (see ndtframe.h)
void NDTFrame::addScan(const Vector3d& pose, const vector<float>& laser_data, const float& min_angle,
                       const float& angle_increment, const float& max_range) {
  ndtpso_host::Use use(dev());  // (the scratch frame below binds to the active context: this frame's)
  NDTFrame scan(Vector3d::Zero(), width, height, (double)std::max(width, height), false, s_config);  // ndtpso_slam_node.cpp:229-230
  scan.s_dev = dev();
  ndtpso_host::bind_frame(scan.s_dev);
  scan.loadLaser(laser_data, min_angle, angle_increment, max_range);
  update(pose, &scan);
}

// reference: getCellIndex, ndtframe.cpp:240-249 (public single-point utility)
int NDTFrame::getCellIndex(Vector2d point, int grid_width, double cell_side_) {
  if ((point.x() > s_x_min) && (point.x() < s_x_max) && (point.y() > s_y_min) && (point.y() < s_y_max))
    return static_cast<int>(std::floor((point.x() + (width / 2.)) / cell_side_) +
                            grid_width * (std::floor((point.y() + (height / 2.)) / cell_side_)));
  return -1;
}

// reference: addPoint, ndtframe.cpp:215-235
void NDTFrame::addPoint(Vector2d& point) {
  ndtpso_host::Use use(dev());
  if (s_resident) {
    if (getCellIndex(point, widthNumOfCells, cell_side) == -1) return;  // outside the frame: dropped, `built` untouched
    const double p[2] = {point.x(), point.y()};
    if (ndtpso_host::check(ndtpso_map_insert_host(ensureMap(), p, 1, nullptr), "addPoint")) built = false;
    return;
  }
  const int32_t idx = getCellIndex(point, widthNumOfCells, cell_side);
  const double xy[2] = {point.x(), point.y()};
  append(xy, &idx, 1);
}

// reference: build, ndtframe.cpp:68-117 -- NDTCell::build for every created cell, batched into one device call
void NDTFrame::build() {
  ndtpso_host::Use use(dev());
  if (s_resident) {
    if (ndtpso_host::check(ndtpso_map_build(ensureMap()), "build")) built = true;
    return;
  }
  const uint32_t n = (uint32_t)s_created.size();
  if (n) {
    std::vector<ndtpso_cell_window> cw(n);
    std::vector<uint32_t> off(n + 1, 0);
    std::vector<double> xy;
    for (uint32_t k = 0; k < n; ++k) {
      NDTCell& c = cells[s_created[k]];
      NDTCell::Window& w = c.ensure_window();
      const size_t id = w.current_window_id;
      ndtpso_cell_window& s = cw[k];
      std::memset(&s, 0, sizeof(s));
      s.global_sum[0] = w.global_sum.x();
      s.global_sum[1] = w.global_sum.y();
      s.slot_sum[0] = w.partial_sums[id].x();
      s.slot_sum[1] = w.partial_sums[id].y();
      for (int j = 0; j < 4; ++j) {
        s.global_covar_sum[j] = w.global_covar_sum[j];
        s.slot_covar[j] = w.partial_covars[id][j];
      }
      s.global_count = w.global_count;
      s.slot_count = w.partial_counts[id];
      s.current_count = w.current_count;
      s.built = c.built ? 1 : 0;
      for (const Vector2d& p : w.points[id]) {
        xy.push_back(p.x());
        xy.push_back(p.y());
      }
      off[k + 1] = (uint32_t)(xy.size() / 2);
    }
    if (!ndtpso_host::check(ndtpso_cells_build_windowed(ndtpso_host::device(), n, cw.data(), off.data(), xy.data()), "build"))
      return;  // the cells keep their previous statistics; the frame stays un-built
    for (uint32_t k = 0; k < n; ++k) {
      NDTCell& c = cells[s_created[k]];
      NDTCell::Window& w = *c.win_;
      const size_t id = w.current_window_id;
      const ndtpso_cell_window& s = cw[k];
      w.global_sum = Vector2d(s.global_sum[0], s.global_sum[1]);
      w.partial_sums[id] = Vector2d(s.slot_sum[0], s.slot_sum[1]);
      for (int j = 0; j < 4; ++j) {
        w.global_covar_sum[j] = s.global_covar_sum[j];
        w.partial_covars[id][j] = s.slot_covar[j];
      }
      w.global_count = s.global_count;
      w.partial_counts[id] = s.slot_count;
      if (s.global_count > 2) {  // ndtcell.cpp:43-58
        for (int j = 0; j < 4; ++j) w.inv_covar[j] = s.icov[j];
        c.mean = Vector2d(s.mean[0], s.mean[1]);
        c.built = true;
      }
      if (w.current_count > NDT_MAX_POINTS_PER_CELL) {  // ndtcell.cpp:61-65
        w.current_window_id = (w.current_window_id + 1) % NDT_WINDOW_SIZE;
        w.current_count = 0;
      }
    }
  }
#if BUILD_OCCUPANCY_GRID
  if (s_occupancy_grid.cell_size > 0.) rasteriseOccupancy();
#endif
  built = true;
  s_table_dirty = true;
}

#if BUILD_OCCUPANCY_GRID
// reference: the occupancy-grid branch of build(), ndtframe.cpp:79-112.  The Gaussians are evaluated on the device
// (ndtpso_occupancy_values); the scatter keeps the reference's order (ascending cell index, j outer, k inner) and
// its indexing, including row = index / heightNumOfCells and og[x + height * y].
void NDTFrame::rasteriseOccupancy() {
  auto& g = s_occupancy_grid;
  const uint32_t per_cell = (uint32_t)std::floor(cell_side / g.cell_size);
  if (per_cell == 0) return;
  std::vector<uint32_t> order(s_created);
  std::sort(order.begin(), order.end());
  std::vector<int32_t> index;
  std::vector<double> mean, icov;
  for (uint32_t i : order) {
    const NDTCell& c = cells[i];
    if (!c.built) continue;  // normalDistribution of an un-built cell is 0: nothing is written (ndtcell.cpp:70-78)
    index.push_back((int32_t)i);
    mean.push_back(c.mean.x());
    mean.push_back(c.mean.y());
    for (int j = 0; j < 4; ++j) icov.push_back(c.win_->inv_covar[j]);
  }
  if (index.empty()) return;
  std::vector<int8_t> v(index.size() * per_cell * per_cell);
  const ndtpso_grid grid = grid_of(*this);
  if (!ndtpso_host::check(ndtpso_occupancy_values(ndtpso_host::device(), &grid, g.cell_size, (uint32_t)index.size(),
                                                  index.data(), mean.data(), icov.data(), v.data()),
                          "occupancy grid"))
    return;
  size_t t = 0;
  for (int32_t i : index) {
    const uint32_t cx = (uint32_t)i % widthNumOfCells, cy = (uint32_t)i / heightNumOfCells;
    for (uint32_t j = 0; j < per_cell; ++j)
      for (uint32_t k = 0; k < per_cell; ++k, ++t) {
        if (v[t] < 0) continue;  // p == 0
        const uint32_t ox = cx * per_cell + j, oy = cy * per_cell + k;
        g.min_x_ind = std::min(ox, g.min_x_ind);
        g.max_x_ind = std::max(ox, g.max_x_ind);
        g.min_y_ind = std::min(oy, g.min_y_ind);
        g.max_y_ind = std::max(oy, g.max_y_ind);
        const size_t at = (size_t)ox + (size_t)g.height * oy;
        if (at < g.og.size()) g.og[at] = v[t];  // (the reference writes unchecked)
      }
  }
}

void NDTFrame::fetchOccupancy() const {
  auto& g = s_occupancy_grid;
  if (!s_resident || !d_map_ || !(g.cell_size > 0.)) return;
  uint32_t ext[4] = {UINT32_MAX, 0, UINT32_MAX, 0};
  if (!ndtpso_host::check(ndtpso_map_get_occupancy(d_map_, g.og.data(), g.og.size(), nullptr, nullptr, ext), "occupancy grid"))
    return;
  g.min_x_ind = ext[0], g.max_x_ind = ext[1], g.min_y_ind = ext[2], g.max_y_ind = ext[3];
}

const vector<int8_t>& NDTFrame::occupancyGrid(uint32_t* og_width, uint32_t* og_height, uint32_t extent[4]) const {
  ndtpso_host::Use use(dev());
  fetchOccupancy();
  if (og_width) *og_width = s_occupancy_grid.width;
  if (og_height) *og_height = s_occupancy_grid.height;
  if (extent) {
    extent[0] = s_occupancy_grid.min_x_ind, extent[1] = s_occupancy_grid.max_x_ind;
    extent[2] = s_occupancy_grid.min_y_ind, extent[3] = s_occupancy_grid.max_y_ind;
  }
  return s_occupancy_grid.og;
}
#endif

// built cells -> device reference table (LDS image packed by ndtpso_ref_set_cells)
bool NDTFrame::uploadTable() {
  if (!s_table_dirty && ndtpso_host::table_owner() == this) return true;
  std::vector<int32_t> index;
  std::vector<double> mean, icov;
  for (uint32_t i : s_created) {
    const NDTCell& c = cells[i];
    if (!c.built) continue;
    index.push_back((int32_t)i);
    mean.push_back(c.mean.x());
    mean.push_back(c.mean.y());
    for (int j = 0; j < 4; ++j) icov.push_back(c.win_->inv_covar[j]);
  }
  const ndtpso_grid grid = grid_of(*this);
  if (!ndtpso_host::check(ndtpso_ref_set_cells(ndtpso_host::device(), &grid, (uint32_t)index.size(), index.data(),
                                               mean.data(), icov.data()), "reference table upload")) {
    ndtpso_host::table_owner() = nullptr;
    return false;
  }
  ndtpso_host::table_owner() = this;
  s_table_dirty = false;
  return true;
}

// A new frame's points as an ndtpso_points of the active context: the frame's resident scan in place, or a pooled temporary
// scan filled through the host (`foreign`: a frame of another thread's context, its points already collected) and released
// with this object.
struct NDTFrame::DeviceScan {
  ndtpso_points* pts = nullptr;
  DeviceScan(const NDTFrame* f, bool is_foreign, std::vector<double>& foreign, const char* what) {
    if (!is_foreign && f->s_resident && f->d_scan_ && !f->d_map_) {
      pts = f->d_scan_;
      return;
    }
    std::vector<double> xy;
    if (is_foreign) xy.swap(foreign); else f->collectPoints(xy);
    cap_ = std::max(kScanCapacity, (uint32_t)(xy.size() / 2));
    pts = tmp_ = ndtpso_host::acquire_scan(cap_);
    ndtpso_host::check(ndtpso_points_set(tmp_, xy.data(), (uint32_t)(xy.size() / 2)), what);
  }
  ~DeviceScan() {
    if (tmp_) ndtpso_host::release_scan(tmp_, cap_);
  }
  DeviceScan(const DeviceScan&) = delete;
  DeviceScan& operator=(const DeviceScan&) = delete;

 private:
  ndtpso_points* tmp_ = nullptr;
  uint32_t cap_ = 0;
};

void NDTFrame::recordAlignOutcome(bool ok) {
  if (ok) built = true;  // (the alignment built first if need be: cost_function's lazy build, core.cpp:27-28)
  s_last_align_ok = ok;
  t_last_align_failed = !ok;
}

// pso_optimization against this frame, core.cpp:50-116.  The std::rand() stream is drawn here, in the order and
// quantity the reference consumes it (3 + 3P + 6PI), so srand() by the caller has the reference's meaning.
Vector3d NDTFrame::optimize(const Vector3d& guess, const NDTFrame* new_frame, const Vector3d& deviation,
                            const PSOConfig& cfg) {
  std::vector<double> foreign;  // (a frame of another thread's context: its points through the host, see update())
  const bool is_foreign = new_frame->dev() != dev();
  if (is_foreign) new_frame->collectPoints(foreign);
  ndtpso_host::Use use(dev());
  const ndtpso_pso_config abi = to_abi(cfg);
  std::vector<int32_t> draws(ndtpso_rand_draws(&abi));
  ndtpso_host::draw_rand(draws.data(), draws.size());  // drawn even if a device call fails: the caller's stream moves on as it would have
  const double g[3] = {guess.x(), guess.y(), guess.z()};
  const double dv[3] = {deviation.x(), deviation.y(), deviation.z()};
  double pose[3] = {g[0], g[1], g[2]};
  bool ok;
  if (s_resident) {
    ndtpso_map* m = ensureMap();  // ndtpso_map_align builds first if need be (cost_function's lazy build, core.cpp:27-28)
    const DeviceScan scan(new_frame, is_foreign, foreign, "align");
    ok = ndtpso_host::check(ndtpso_map_align(m, scan.pts, g, dv, &abi, 0u, draws.data(), ndtpso_host::score_mode(), pose, nullptr, nullptr),
                            "align");
  } else {
    if (!built) build();  // core.cpp:27-28 (lazy build inside cost_function)
    const bool table_ok = uploadTable();
    std::vector<double> xy;
    if (is_foreign) xy.swap(foreign); else new_frame->collectPoints(xy);
    ok = table_ok && ndtpso_host::check(ndtpso_align(ndtpso_host::device(), xy.data(), (uint32_t)(xy.size() / 2), g, dv, &abi, 0u, draws.data(),
                                                     ndtpso_host::score_mode(), pose, nullptr, nullptr), "align");
  }
  recordAlignOutcome(ok);
  return ok ? Vector3d(pose[0], pose[1], pose[2]) : guess;  // device fault: the initial guess, never a CPU estimate
}

double NDTFrame::cost(const Vector3d& trans, const NDTFrame* new_frame) {
  std::vector<double> foreign;
  const bool is_foreign = new_frame->dev() != dev();
  if (is_foreign) new_frame->collectPoints(foreign);
  ndtpso_host::Use use(dev());
  const double pose[3] = {trans.x(), trans.y(), trans.z()};
  double c = 0.;
  if (s_resident) {
    ndtpso_map* m = ensureMap();
    const DeviceScan scan(new_frame, is_foreign, foreign, "cost_function");
    if (ndtpso_host::check(ndtpso_map_cost(m, scan.pts, pose, 1, NDTPSO_SCORE_F64, &c), "cost_function"))  // builds if need be
      built = true;
    else
      c = 0.;
    return c;
  }
  if (!built) build();
  if (!uploadTable()) return 0.;
  std::vector<double> xy;
  if (is_foreign) xy.swap(foreign); else new_frame->collectPoints(xy);
  if (!ndtpso_host::check(ndtpso_cost_batch(ndtpso_host::device(), xy.data(), (uint32_t)(xy.size() / 2), pose, 1,
                                            NDTPSO_SCORE_F64, &c, nullptr), "cost_function"))
    return 0.;
  return c;
}

// reference: align, ndtframe.cpp:251-266.  The reference passes no config to pso_optimization (:257), so the
// frame's own PSOConfig is never used and every alignment runs the default 30 x 50.  That is what happens here
// too; NDTPSO_ALIGN_FRAME_CONFIG=1 in the environment makes align() honour the frame's PSOConfig instead.
namespace {
bool align_uses_frame_config() {
  static const bool frame_config = [] {
    const char* e = std::getenv("NDTPSO_ALIGN_FRAME_CONFIG");
    return e && e[0] == '1';
  }();
  return frame_config;
}
}  // namespace

Vector3d NDTFrame::nextDeviation() {
  const Vector3d deviation = s_iter < 2 ? Vector3d(.1, .1, 3.1415E-3) : Vector3d((s_pose_diff * 2.).array().abs());
  ++s_iter;
  return deviation;
}

Vector3d NDTFrame::recordAlignedPose(Vector3d pose) {
#if TRANSFORM_POSE_AFTER_ALIGN
  pose -= s_trans;
#endif
  s_pose_diff = pose - s_prev_pose;
  s_prev_pose = pose;
  return pose;
}

Vector3d NDTFrame::align(Vector3d initial_guess, const NDTFrame* const new_frame) {
  const Vector3d deviation = nextDeviation();
  return recordAlignedPose(optimize(initial_guess, new_frame, deviation, align_uses_frame_config() ? s_config.psoConfig : PSOConfig()));
}

// Several align() calls, the device work of independent ones in one launch (see ndtframe.h): align()'s own steps in request
// order, with ONE ndtpso_map_align_batch for a run of requests between the steps before the alignment and those after it.
void NDTFrame::alignBatch(NDTAlignRequest* reqs, size_t n) {
  if (!reqs) return;
  ndtpso_host::Ctx* const mine = ndtpso_host::thread_ctx();
  auto batchable = [&](const NDTAlignRequest& r) {
    if (!r.ref || !r.cur || align_uses_frame_config()) return false;  // (frames' own PSOConfigs: one cfg per launch)
    const NDTFrame* c = r.cur;
    return r.ref->s_resident && r.ref->dev() == mine && c->dev() == mine && c->s_resident && c->d_scan_ && !c->d_map_;
  };
  size_t i = 0;
  while (i < n) {
    size_t j = i;
    while (j < n && batchable(reqs[j])) {
      // The run ends before a request whose reference frame it has already seen (its deviation depends on the first result),
      // and before one that uses as reference a frame an earlier request aligns as scan, or the other way round: making the
      // reference's device map (ensureMap) turns such a frame's point list into a map, which sequential calls do between the two
      // alignments, not before both.
      bool again = false;
      for (size_t k = i; k < j && !again; ++k)
        again = reqs[k].ref == reqs[j].ref || reqs[k].cur == reqs[j].ref || reqs[k].ref == reqs[j].cur;
      if (again) break;
      ++j;
    }
    if (j - i < 2) {  // align() itself, in its place
      NDTAlignRequest& r = reqs[i];
      r.pose = r.ref->align(r.guess, r.cur);
      r.ok = r.ref->lastAlignOk();
      ++i;
      continue;
    }
    ndtpso_host::Use use(mine);
    const size_t cnt = j - i;
    const ndtpso_pso_config abi = to_abi(PSOConfig());  // (what align() passes on, ndtframe.cpp:257)
    const size_t n_draw = ndtpso_rand_draws(&abi);
    std::vector<ndtpso_map_align_job> jobs(cnt);
    std::vector<int32_t> draws(cnt * n_draw);
    std::memset(jobs.data(), 0, cnt * sizeof(ndtpso_map_align_job));
    bool no_map = false;
    for (size_t k = 0; k < cnt; ++k) {
      NDTAlignRequest& r = reqs[i + k];
      NDTFrame* f = r.ref;
      const Vector3d deviation = f->nextDeviation();
      ndtpso_map_align_job& job = jobs[k];
      job.map = f->ensureMap();
      no_map = no_map || !job.map;
      job.new_points = r.cur->d_scan_;
      ndtpso_host::draw_rand(&draws[k * n_draw], n_draw);  // drawn even if the device call fails (optimize)
      job.rand_table = &draws[k * n_draw];
      job.guess[0] = job.pose[0] = r.guess.x();
      job.guess[1] = job.pose[1] = r.guess.y();
      job.guess[2] = job.pose[2] = r.guess.z();
      job.deviation[0] = deviation.x();
      job.deviation[1] = deviation.y();
      job.deviation[2] = deviation.z();
    }
    int rc_call = NDTPSO_OK;
    if (no_map) {  // (a frame whose device map could not be made fails alone, as its align() would: one call each)
      for (size_t k = 0; k < cnt; ++k)
        jobs[k].rc = ndtpso_map_align(jobs[k].map, jobs[k].new_points, jobs[k].guess, jobs[k].deviation, &abi, 0u, jobs[k].rand_table,
                                      ndtpso_host::score_mode(), jobs[k].pose, nullptr, nullptr);
    } else {
      rc_call = ndtpso_map_align_batch(ndtpso_host::device(), jobs.data(), (uint32_t)cnt, &abi, ndtpso_host::score_mode());
    }
    bool some_job_failed = false;
    for (size_t k = 0; k < cnt; ++k) some_job_failed = some_job_failed || jobs[k].rc != NDTPSO_OK;
    for (size_t k = 0; k < cnt; ++k) {
      NDTAlignRequest& r = reqs[i + k];
      NDTFrame* f = r.ref;
      // (a call refused as a whole -- no device context, a HIP error before the launch -- failed every request)
      const int rc = (rc_call != NDTPSO_OK && !some_job_failed) ? rc_call : jobs[k].rc;
      const bool ok = ndtpso_host::check(rc, "align");
      f->recordAlignOutcome(ok);
      r.pose = f->recordAlignedPose(ok ? Vector3d(jobs[k].pose[0], jobs[k].pose[1], jobs[k].pose[2]) : r.guess);
      r.ok = ok;
    }
    i = j;
  }
}

// A pose lattice searched on the device, its best nodes refined in one launch (see ndtframe.h).
NDTRelocalizeResult NDTFrame::relocalize(const NDTFrame* new_frame, const Vector3d& origin, const Vector3d& step,
                                         const unsigned count[3], unsigned top_k) {
  const NDTRelocalizeResult failed{origin, 0., 0u, false};
  auto refuse = [&](int rc, const char* what) {
    ndtpso_host::check(rc, what);
    recordAlignOutcome(false);
    return failed;
  };
  if (!new_frame || !count) return refuse(NDTPSO_E_ARG, "relocalize: null argument");
  if (!s_resident) return refuse(NDTPSO_E_STATE, "relocalize: the frame is not resident");
  if (new_frame->dev() != dev()) return refuse(NDTPSO_E_ARG, "relocalize: a scan of another thread's context");
  ndtpso_host::Use use(dev());
  ndtpso_map* m = ensureMap();
  if (!m) return refuse(NDTPSO_E_STATE, "relocalize: no device map");
  std::vector<double> unused;
  const DeviceScan scan(new_frame, false, unused, "relocalize");
  ndtpso_lattice lat;
  std::memset(&lat, 0, sizeof(lat));
  for (int a = 0; a < 3; ++a) {
    lat.origin[a] = origin[a];
    lat.step[a] = step[a];
    lat.count[a] = count[a];
  }
  lat.top_k = top_k;
  ndtpso_lattice_hit hits[NDTPSO_SEARCH_MAX_TOP_K];
  uint32_t n_hits = 0;
  if (!ndtpso_host::check(ndtpso_map_search(m, scan.pts, &lat, ndtpso_host::score_mode(), hits, &n_hits, nullptr), "relocalize")) {
    recordAlignOutcome(false);
    return failed;
  }
  const ndtpso_pso_config abi = to_abi(align_uses_frame_config() ? s_config.psoConfig : PSOConfig());
  const size_t n_draw = ndtpso_rand_draws(&abi);
  std::vector<ndtpso_map_align_job> jobs(n_hits);
  std::vector<int32_t> draws(n_hits * n_draw);
  std::memset(jobs.data(), 0, jobs.size() * sizeof(ndtpso_map_align_job));
  const double first_call[3] = {.1, .1, 3.1415E-3};  // (nextDeviation's)
  for (uint32_t k = 0; k < n_hits; ++k) {
    ndtpso_map_align_job& job = jobs[k];
    job.map = m;
    job.new_points = scan.pts;
    ndtpso_host::draw_rand(&draws[k * n_draw], n_draw);  // drawn even if the device call fails (optimize)
    job.rand_table = &draws[k * n_draw];
    job.flags = 1u;  // cost wanted
    for (int a = 0; a < 3; ++a) {
      job.guess[a] = job.pose[a] = hits[k].pose[a];
      job.deviation[a] = count[a] > 1 ? step[a] / 2. : first_call[a];
    }
  }
  const int rc_call = ndtpso_map_align_batch(ndtpso_host::device(), jobs.data(), n_hits, &abi, ndtpso_host::score_mode());
  bool some_job_failed = false;
  for (uint32_t k = 0; k < n_hits; ++k) some_job_failed = some_job_failed || jobs[k].rc != NDTPSO_OK;
  // (a call refused as a whole failed every job, as in alignBatch)
  if (rc_call != NDTPSO_OK && !some_job_failed) return refuse(rc_call, "relocalize");
  int best = -1;
  for (uint32_t k = 0; k < n_hits; ++k)
    if (jobs[k].rc == NDTPSO_OK && (best < 0 || jobs[k].cost < jobs[(size_t)best].cost)) best = (int)k;
  if (best < 0) return refuse(rc_call != NDTPSO_OK ? rc_call : NDTPSO_E_HIP, "relocalize");
  Vector3d pose(jobs[(size_t)best].pose[0], jobs[(size_t)best].pose[1], jobs[(size_t)best].pose[2]);
#if TRANSFORM_POSE_AFTER_ALIGN
  pose -= s_trans;
#endif
  s_prev_pose = pose;
  s_pose_diff = Vector3d::Zero();
  s_iter = 0;
  recordAlignOutcome(true);
  return NDTRelocalizeResult{pose, jobs[(size_t)best].cost, n_hits, true};
}

// Several relocalize() calls (see ndtframe.h): the member's own steps per request, with ONE ndtpso_map_search_batch and ONE
// ndtpso_map_align_batch for a run of requests on different resident frames.
void NDTFrame::relocalizeBatch(NDTRelocalizeRequest* reqs, size_t n) {
  if (!reqs) return;
  ndtpso_host::Ctx* const mine = ndtpso_host::thread_ctx();
  auto batchable = [&](const NDTRelocalizeRequest& r) {
    if (!r.ref || !r.cur || align_uses_frame_config()) return false;  // (frames' own PSOConfigs: one cfg per launch)
    return r.ref->s_resident && r.ref->dev() == mine && r.cur->dev() == mine;
  };
  const double first_call[3] = {.1, .1, 3.1415E-3};  // (nextDeviation's)
  size_t i = 0;
  while (i < n) {
    size_t j = i;
    while (j < n && batchable(reqs[j])) {
      bool again = false;  // (as alignBatch: per frame the order of the steps is the member calls')
      for (size_t k = i; k < j && !again; ++k)
        again = reqs[k].ref == reqs[j].ref || reqs[k].cur == reqs[j].ref || reqs[k].ref == reqs[j].cur;
      if (again) break;
      ++j;
    }
    if (j - i < 2) {  // relocalize() itself, in its place
      NDTRelocalizeRequest& r = reqs[i];
      if (r.ref) {
        r.result = r.ref->relocalize(r.cur, r.origin, r.step, r.count, r.top_k);
      } else {
        ndtpso_host::check(NDTPSO_E_ARG, "relocalize: null argument");
        r.result = NDTRelocalizeResult{r.origin, 0., 0u, false};
      }
      ++i;
      continue;
    }
    ndtpso_host::Use use(mine);
    const size_t cnt = j - i;
    // ---- ONE search call over the run ----------------------------------------------------------------------------------------
    std::vector<int> rc(cnt, NDTPSO_OK);  // per request: what its relocalize() would have been refused with
    std::vector<const char*> what(cnt, "relocalize");
    std::vector<std::unique_ptr<DeviceScan>> scans(cnt);
    std::vector<ndtpso_map*> maps(cnt, nullptr);
    std::vector<ndtpso_map_search_job> sjobs;
    std::vector<size_t> sjob_req;
    std::vector<int> search_job(cnt, -1);  // a request's place in sjobs
    std::vector<ndtpso_lattice_hit> hits(cnt * NDTPSO_SEARCH_MAX_TOP_K);
    std::vector<double> unused;
    for (size_t k = 0; k < cnt; ++k) {
      NDTRelocalizeRequest& r = reqs[i + k];
      maps[k] = r.ref->ensureMap();
      if (!maps[k]) {
        rc[k] = NDTPSO_E_STATE;
        what[k] = "relocalize: no device map";
        continue;
      }
      scans[k].reset(new DeviceScan(r.cur, false, unused, "relocalize"));
      ndtpso_map_search_job job;
      std::memset(&job, 0, sizeof(job));
      job.map = maps[k];
      job.new_points = scans[k]->pts;
      for (int a = 0; a < 3; ++a) {
        job.lattice.origin[a] = r.origin[a];
        job.lattice.step[a] = r.step[a];
        job.lattice.count[a] = r.count[a];
      }
      job.lattice.top_k = r.top_k;
      job.hits = &hits[k * NDTPSO_SEARCH_MAX_TOP_K];
      search_job[k] = (int)sjobs.size();
      sjobs.push_back(job);
      sjob_req.push_back(k);
    }
    std::vector<uint32_t> n_hits(cnt, 0u);
    if (!sjobs.empty()) {
      const int rc_call = ndtpso_map_search_batch(ndtpso_host::device(), sjobs.data(), (uint32_t)sjobs.size(), ndtpso_host::score_mode(), nullptr);
      bool some_job_failed = false;
      for (const ndtpso_map_search_job& job : sjobs) some_job_failed = some_job_failed || job.rc != NDTPSO_OK;
      for (size_t q = 0; q < sjobs.size(); ++q) {
        // (a call refused as a whole failed every request)
        rc[sjob_req[q]] = (rc_call != NDTPSO_OK && !some_job_failed) ? rc_call : sjobs[q].rc;
        n_hits[sjob_req[q]] = rc[sjob_req[q]] == NDTPSO_OK ? sjobs[q].n_hits : 0u;
      }
    }
    // ---- the rand() tables, request by request in hit order; ONE refinement launch over all hits ---------------------------------
    const ndtpso_pso_config abi = to_abi(PSOConfig());  // (what align() passes on, ndtframe.cpp:257)
    const size_t n_draw = ndtpso_rand_draws(&abi);
    size_t total = 0;
    std::vector<size_t> first_job(cnt, 0);
    for (size_t k = 0; k < cnt; ++k) {
      first_job[k] = total;
      total += n_hits[k];
    }
    std::vector<ndtpso_map_align_job> jobs(total);
    std::vector<int32_t> draws(total * n_draw);
    if (total) std::memset(jobs.data(), 0, total * sizeof(ndtpso_map_align_job));
    for (size_t k = 0; k < cnt; ++k) {
      const NDTRelocalizeRequest& r = reqs[i + k];
      for (uint32_t h = 0; h < n_hits[k]; ++h) {
        const size_t at = first_job[k] + h;
        ndtpso_map_align_job& job = jobs[at];
        job.map = maps[k];
        job.new_points = scans[k]->pts;
        ndtpso_host::draw_rand(&draws[at * n_draw], n_draw);  // drawn even if the device call fails (optimize)
        job.rand_table = &draws[at * n_draw];
        job.flags = 1u;  // cost wanted
        for (int a = 0; a < 3; ++a) {
          job.guess[a] = job.pose[a] = hits[k * NDTPSO_SEARCH_MAX_TOP_K + h].pose[a];
          job.deviation[a] = r.count[a] > 1 ? r.step[a] / 2. : first_call[a];
        }
      }
    }
    int rc_align = NDTPSO_OK;
    bool some_align_failed = false;
    if (total) {
      rc_align = ndtpso_map_align_batch(ndtpso_host::device(), jobs.data(), (uint32_t)total, &abi, ndtpso_host::score_mode());
      for (const ndtpso_map_align_job& job : jobs) some_align_failed = some_align_failed || job.rc != NDTPSO_OK;
    }
    // ---- every frame's outcome, in request order ---------------------------------------------------------------------------------
    for (size_t k = 0; k < cnt; ++k) {
      NDTRelocalizeRequest& r = reqs[i + k];
      NDTFrame* f = r.ref;
      int best = -1;
      if (rc[k] == NDTPSO_OK) {
        if (rc_align != NDTPSO_OK && !some_align_failed) {  // (a call refused as a whole failed every job, as in alignBatch)
          rc[k] = rc_align;
        } else {
          for (uint32_t h = 0; h < n_hits[k]; ++h) {
            const ndtpso_map_align_job& job = jobs[first_job[k] + h];
            if (job.rc == NDTPSO_OK && (best < 0 || job.cost < jobs[first_job[k] + (size_t)best].cost)) best = (int)h;
          }
          if (best < 0) rc[k] = rc_align != NDTPSO_OK ? rc_align : NDTPSO_E_HIP;
        }
      }
      if (rc[k] != NDTPSO_OK) {
        // The shared search call leaves the context the text of its LAST refusal.  A request refused for its own arguments or plan
        // gets its own text back from the single call, which refuses it the same way before it enqueues anything.
        if (search_job[k] >= 0 && (rc[k] == NDTPSO_E_ARG || rc[k] == NDTPSO_E_CAPACITY) && sjobs[(size_t)search_job[k]].rc == rc[k]) {
          ndtpso_map_search_job& sj = sjobs[(size_t)search_job[k]];
          uint32_t none = 0;
          (void)ndtpso_map_search(sj.map, sj.new_points, &sj.lattice, ndtpso_host::score_mode(), sj.hits, &none, nullptr);
        }
        ndtpso_host::check(rc[k], what[k]);
        f->recordAlignOutcome(false);
        r.result = NDTRelocalizeResult{r.origin, 0., 0u, false};
        continue;
      }
      const ndtpso_map_align_job& won = jobs[first_job[k] + (size_t)best];
      Vector3d pose(won.pose[0], won.pose[1], won.pose[2]);
#if TRANSFORM_POSE_AFTER_ALIGN
      pose -= f->s_trans;
#endif
      f->s_prev_pose = pose;
      f->s_pose_diff = Vector3d::Zero();
      f->s_iter = 0;
      f->recordAlignOutcome(true);
      r.result = NDTRelocalizeResult{pose, won.cost, n_hits[k], true};
    }
    i = j;
  }
}

namespace {
// a device curvature as the drop-in returns it, with the covariance it stands for (host arithmetic, no device)
NDTCurvature curvature_result(const ndtpso_curvature& c) {
  NDTCurvature r;
  std::memset(static_cast<void*>(&r), 0, sizeof(r));
  r.cost = c.cost;
  r.gradient = Vector3d(c.gradient[0], c.gradient[1], c.gradient[2]);
  for (int i = 0; i < 6; ++i) r.hessian[i] = c.hessian[i];
  r.n_points = c.n_points;
  r.n_hit = c.n_hit;
  ndtpso_pose_covariance pc;
  (void)ndtpso_curvature_covariance(&c, &pc);  // (no null pointer here: it cannot fail)
  for (int i = 0; i < 9; ++i) r.covariance[i] = pc.cov[i];
  r.xy_major = pc.xy_major;
  r.xy_minor = pc.xy_minor;
  r.xy_angle = pc.xy_angle;
  r.definite = pc.definite != 0;
  r.ok = true;
  return r;
}
NDTCurvature curvature_failed() {
  NDTCurvature r;
  std::memset(static_cast<void*>(&r), 0, sizeof(r));
  r.gradient = Vector3d::Zero();
  return r;
}
}  // namespace

// Gradient, Hessian and covariance of the score at a pose (see ndtframe.h): cost()'s conventions, an observer.
NDTCurvature NDTFrame::curvature(const Vector3d& pose, const NDTFrame* new_frame) {
  if (!new_frame) {
    ndtpso_host::check(NDTPSO_E_ARG, "curvature: null argument");
    return curvature_failed();
  }
  if (!s_resident) {
    ndtpso_host::check(NDTPSO_E_STATE, "curvature: the frame is not resident");
    return curvature_failed();
  }
  std::vector<double> foreign;
  const bool is_foreign = new_frame->dev() != dev();
  if (is_foreign) new_frame->collectPoints(foreign);
  ndtpso_host::Use use(dev());
  ndtpso_map* m = ensureMap();
  if (!m) {
    ndtpso_host::check(NDTPSO_E_STATE, "curvature: no device map");
    return curvature_failed();
  }
  const DeviceScan scan(new_frame, is_foreign, foreign, "curvature");
  const double p[3] = {pose.x(), pose.y(), pose.z()};
  ndtpso_curvature c;
  std::memset(&c, 0, sizeof(c));
  if (!ndtpso_host::check(ndtpso_map_curvature(m, scan.pts, p, 1, &c), "curvature")) return curvature_failed();
  built = true;  // (the call built first if need be, as cost()'s)
  return curvature_result(c);
}

// Several curvature() calls (see ndtframe.h): ONE ndtpso_map_curvature_batch for a run of requests on resident frames of the
// calling thread's context.
void NDTFrame::curvatureBatch(NDTCurvatureRequest* reqs, size_t n) {
  if (!reqs) return;
  ndtpso_host::Ctx* const mine = ndtpso_host::thread_ctx();
  auto batchable = [&](const NDTCurvatureRequest& r) {
    return r.ref && r.cur && r.ref->s_resident && r.ref->dev() == mine && r.cur->dev() == mine;
  };
  size_t i = 0;
  while (i < n) {
    size_t j = i;
    while (j < n && batchable(reqs[j])) ++j;
    if (j - i < 2) {  // curvature() itself, in its place
      NDTCurvatureRequest& r = reqs[i];
      if (r.ref) {
        r.result = r.ref->curvature(r.pose, r.cur);
      } else {
        ndtpso_host::check(NDTPSO_E_ARG, "curvature: null argument");
        r.result = curvature_failed();
      }
      ++i;
      continue;
    }
    ndtpso_host::Use use(mine);
    const size_t cnt = j - i;
    std::vector<int> rc(cnt, NDTPSO_OK);
    std::vector<const char*> what(cnt, "curvature");
    std::vector<std::unique_ptr<DeviceScan>> scans(cnt);
    std::vector<ndtpso_map_curvature_job> jobs;
    std::vector<size_t> job_req;
    std::vector<double> poses(3 * cnt);
    std::vector<ndtpso_curvature> out(cnt);
    std::memset(out.data(), 0, cnt * sizeof(ndtpso_curvature));
    std::vector<double> unused;
    for (size_t k = 0; k < cnt; ++k) {
      NDTCurvatureRequest& r = reqs[i + k];
      ndtpso_map* m = r.ref->ensureMap();
      if (!m) {
        rc[k] = NDTPSO_E_STATE;
        what[k] = "curvature: no device map";
        continue;
      }
      scans[k].reset(new DeviceScan(r.cur, false, unused, "curvature"));
      for (int a = 0; a < 3; ++a) poses[3 * k + a] = r.pose[a];
      ndtpso_map_curvature_job job;
      std::memset(&job, 0, sizeof(job));
      job.map = m;
      job.new_points = scans[k]->pts;
      job.poses = &poses[3 * k];
      job.n_poses = 1;
      job.out = &out[k];
      jobs.push_back(job);
      job_req.push_back(k);
    }
    if (!jobs.empty()) {
      const int rc_call = ndtpso_map_curvature_batch(ndtpso_host::device(), jobs.data(), (uint32_t)jobs.size(), nullptr);
      bool some_job_failed = false;
      for (const ndtpso_map_curvature_job& job : jobs) some_job_failed = some_job_failed || job.rc != NDTPSO_OK;
      // (a call refused as a whole failed every request)
      for (size_t q = 0; q < jobs.size(); ++q) rc[job_req[q]] = (rc_call != NDTPSO_OK && !some_job_failed) ? rc_call : jobs[q].rc;
    }
    for (size_t k = 0; k < cnt; ++k) {  // every request's outcome, in request order
      NDTCurvatureRequest& r = reqs[i + k];
      if (rc[k] != NDTPSO_OK) {
        ndtpso_host::check(rc[k], what[k]);
        r.result = curvature_failed();
        continue;
      }
      r.ref->built = true;
      r.result = curvature_result(out[k]);
    }
    i = j;
  }
}

// ---- free space (see ndtframe.h): ndtpso_map_trace / ndtpso_map_get_nav_grid of the frame's device map ---------------------------
const char* NDTFrame::traceRefusal() const {
  if (!s_resident) return numOfCells >= (1u << 21) ? "a frame of 2^21 cells or more is kept on the host's side" : "the frame is not resident";
  if (numOfCells == 1 || (d_scan_ && !d_map_)) return "a one-cell scan frame holds no map";
  return nullptr;
}

ndtpso_map* NDTFrame::traceMap(const char* what) {
  auto refused = [&](const char* why) -> ndtpso_map* {
    ndtpso_host::check(NDTPSO_E_STATE, (std::string(what) + ": " + why).c_str());
    return nullptr;
  };
  if (const char* why = traceRefusal()) return refused(why);
  ndtpso_map* m = ensureMap();
  return m ? m : refused("no device map");
}

void NDTFrame::traceFreeSpace(const Vector3d& pose, const NDTFrame* new_frame) {
  if (!new_frame) {
    ndtpso_host::check(NDTPSO_E_ARG, "traceFreeSpace: null argument");
    return;
  }
  std::vector<double> foreign;
  const bool is_foreign = new_frame->dev() != dev();
  if (is_foreign && s_resident) new_frame->collectPoints(foreign);
  ndtpso_host::Use use(dev());
  ndtpso_map* m = traceMap("traceFreeSpace");
  if (!m) return;
  const DeviceScan scan(new_frame, is_foreign, foreign, "traceFreeSpace");
  const double p[3] = {pose.x(), pose.y(), pose.z()};
  ndtpso_host::check(ndtpso_map_trace(m, scan.pts, p), "traceFreeSpace");
}

bool NDTFrame::navGrid(std::vector<int8_t>& grid, unsigned& og_width, unsigned& og_height) {
  grid.clear();
  og_width = og_height = 0;
  ndtpso_host::Use use(dev());
  ndtpso_map* m = traceMap("navGrid");
  if (!m) return false;
  ndtpso_trace_info info;
  if (!ndtpso_host::check(ndtpso_map_get_trace_info(m, &info), "navGrid")) return false;
  grid.assign((size_t)info.width * info.height, (int8_t)-1);
  if (!ndtpso_host::check(ndtpso_map_get_nav_grid(m, grid.data(), grid.size()), "navGrid")) {
    grid.clear();
    return false;
  }
  og_width = info.width;
  og_height = info.height;
  return true;
}

bool NDTFrame::traceCounts(std::vector<uint32_t>& hits, std::vector<uint64_t>& passes) {
  hits.clear();
  passes.clear();
  ndtpso_host::Use use(dev());
  ndtpso_map* m = traceMap("traceCounts");
  if (!m) return false;
  ndtpso_trace_info info;
  if (!ndtpso_host::check(ndtpso_map_get_trace_info(m, &info), "traceCounts")) return false;
  const size_t n = (size_t)info.width * info.height;
  hits.assign(n, 0u);
  passes.assign(n, 0ull);
  if (!ndtpso_host::check(ndtpso_map_get_trace(m, hits.data(), passes.data(), n), "traceCounts")) {
    hits.clear();
    passes.clear();
    return false;
  }
  return true;
}

// Several loadLaser() calls (see ndtframe.h): the member's own steps per request, with ONE ndtpso_points_load_scans for a run of
// requests on per-scan frames.
void NDTFrame::loadLaserBatch(NDTLoadRequest* reqs, size_t n) {
  if (!reqs) return;
  ndtpso_host::Ctx* const mine = ndtpso_host::thread_ctx();
  auto batchable = [&](const NDTLoadRequest& r) {
    const NDTFrame* f = r.frame;
    if (!f || !r.laser_data || r.laser_data->empty()) return false;
    if (!f->s_resident || f->dev() != mine || f->numOfCells != 1 || f->d_map_) return false;
    const uint32_t cnt = (uint32_t)r.laser_data->size();
    return f->d_scan_ ? f->d_scan_upper_ + cnt <= f->d_scan_cap_ : true;  // (a first load sizes the buffer for the scan)
  };
  size_t i = 0;
  while (i < n) {
    size_t j = i;
    while (j < n && batchable(reqs[j])) {
      bool again = false;
      for (size_t k = i; k < j && !again; ++k) again = reqs[k].frame == reqs[j].frame;
      if (again) break;
      ++j;
    }
    if (j - i < 2) {  // loadLaser() itself, in its place
      const NDTLoadRequest& r = reqs[i];
      if (r.frame && r.laser_data) r.frame->loadLaser(*r.laser_data, r.min_angle, r.angle_increment, r.max_range);
      ++i;
      continue;
    }
    ndtpso_host::Use use(mine);
    std::vector<ndtpso_points_load_job> jobs;
    std::vector<NDTFrame*> owner;
    jobs.reserve(j - i);
    for (size_t k = i; k < j; ++k) {
      const NDTLoadRequest& r = reqs[k];
      NDTFrame* f = r.frame;
      const uint32_t cnt = (uint32_t)r.laser_data->size();
      f->built = false;
      if (!f->d_scan_) {
        f->d_scan_cap_ = std::max(kScanCapacity, cnt);
        f->d_scan_ = ndtpso_host::acquire_scan(f->d_scan_cap_);
        f->d_scan_upper_ = 0;
        if (!f->d_scan_) continue;  // no device memory: the scan is dropped (error recorded)
      }
      ndtpso_points_load_job job;
      std::memset(&job, 0, sizeof(job));
      job.pts = f->d_scan_;
      job.ranges = r.laser_data->data();
      job.geom = ndtpso_scan_geom{cnt, r.min_angle, r.angle_increment, r.max_range, f->s_config.laserIgnoreEpsilon};
      job.trans[0] = f->s_trans.x();
      job.trans[1] = f->s_trans.y();
      job.trans[2] = f->s_trans.z();
      job.clip = grid_of(*f);
      job.flags = 1u | 2u | (f->d_scan_upper_ > 0 ? 4u : 0u);
      jobs.push_back(job);
      owner.push_back(f);
    }
    if (!jobs.empty()) {
      const int rc_call = ndtpso_points_load_scans(ndtpso_host::device(), jobs.data(), (uint32_t)jobs.size());
      bool some_job_failed = false;
      for (const ndtpso_points_load_job& job : jobs) some_job_failed = some_job_failed || job.rc != NDTPSO_OK;
      for (size_t k = 0; k < jobs.size(); ++k)  // (a call refused as a whole failed every request)
        if (ndtpso_host::check((rc_call != NDTPSO_OK && !some_job_failed) ? rc_call : jobs[k].rc, "loadLaser"))
          owner[k]->d_scan_upper_ += jobs[k].geom.n_beams;
    }
    i = j;
  }
}

// Several update() calls (see ndtframe.h): the member's own steps per request, with ONE ndtpso_map_update_batch for a run of
// requests that merge device-resident scans into resident maps.
void NDTFrame::updateBatch(NDTUpdateRequest* reqs, size_t n) {
  if (!reqs) return;
  ndtpso_host::Ctx* const mine = ndtpso_host::thread_ctx();
  auto batchable = [&](const NDTUpdateRequest& r) {
    const NDTFrame* f = r.frame;
    const NDTFrame* c = r.new_frame;
    return f && c && f->s_resident && f->dev() == mine && c->dev() == mine && c->s_resident && c->d_scan_ && !c->d_map_;
  };
  size_t i = 0;
  while (i < n) {
    size_t j = i;
    while (j < n && batchable(reqs[j])) {
      bool again = false;
      for (size_t k = i; k < j && !again; ++k)
        again = reqs[k].frame == reqs[j].frame || reqs[k].new_frame == reqs[j].frame || reqs[k].frame == reqs[j].new_frame;
      if (again) break;
      ++j;
    }
    if (j - i < 2) {  // update() itself, in its place
      const NDTUpdateRequest& r = reqs[i];
      if (r.frame && r.new_frame) r.frame->update(r.trans, r.new_frame);
      ++i;
      continue;
    }
    ndtpso_host::Use use(mine);
    // update()'s steps per request; what each request has to record is recorded in request order behind the call
    enum { kRefused = -1, kNoMap = -2 };
    std::vector<ndtpso_map_update_job> jobs;
    std::vector<int> what(j - i);  // the request's job, or why it has none
    jobs.reserve(j - i);
    for (size_t k = i; k < j; ++k) {
      const NDTUpdateRequest& r = reqs[k];
      NDTFrame* f = r.frame;
      if (!f->s_last_align_ok || t_last_align_failed) {  // refused: see update()
        ++f->s_updates_refused;
        what[k - i] = kRefused;
        continue;
      }
      f->built = false;
      ndtpso_map* m = f->ensureMap();
      if (!m) {
        what[k - i] = kNoMap;
        continue;
      }
      ndtpso_map_update_job job;
      std::memset(&job, 0, sizeof(job));
      job.map = m;
      job.points = r.new_frame->d_scan_;
      job.pose[0] = r.trans.x();
      job.pose[1] = r.trans.y();
      job.pose[2] = r.trans.z();
      job.flags = 1u | ((f->s_iter > 0 && speculate_after_update()) ? 2u : 0u);
      what[k - i] = (int)jobs.size();
      jobs.push_back(job);
    }
    int rc_call = NDTPSO_OK;
    bool some_job_failed = false;
    if (!jobs.empty()) {
      rc_call = ndtpso_map_update_batch(ndtpso_host::device(), jobs.data(), (uint32_t)jobs.size());
      for (const ndtpso_map_update_job& job : jobs) some_job_failed = some_job_failed || job.rc != NDTPSO_OK;
    }
    for (size_t k = i; k < j; ++k) {
      const int w = what[k - i];
      if (w == kRefused)
        ndtpso_host::check(NDTPSO_E_STATE, kUpdateRefused);
      else if (w == kNoMap)
        ndtpso_host::check(ndtpso_map_mark_unbuilt(nullptr), "update");
      else
        ndtpso_host::check((rc_call != NDTPSO_OK && !some_job_failed) ? rc_call : jobs[(size_t)w].rc, "update");
    }
    // the flagged frames' scans through their occupancy grids (setTraceOnUpdate): ONE launch behind the shared update launches
    std::vector<ndtpso_map_trace_job> traces;
    for (size_t k = i; k < j; ++k) {
      const int w = what[k - i];
      if (w < 0 || !reqs[k].frame->s_trace_on_update) continue;
      if (const char* why = reqs[k].frame->traceRefusal()) {
        ndtpso_host::check(NDTPSO_E_STATE, (std::string("update: trace: ") + why).c_str());
        continue;
      }
      if (((rc_call != NDTPSO_OK && !some_job_failed) ? rc_call : jobs[(size_t)w].rc) != NDTPSO_OK) continue;  // (update() returns before its trace)
      ndtpso_map_trace_job t;
      std::memset(&t, 0, sizeof(t));
      t.map = jobs[(size_t)w].map;
      t.points = jobs[(size_t)w].points;
      std::memcpy(t.pose, jobs[(size_t)w].pose, sizeof(t.pose));
      traces.push_back(t);
    }
    if (!traces.empty()) {
      const int rc_trace = ndtpso_map_trace_batch(ndtpso_host::device(), traces.data(), (uint32_t)traces.size());
      bool some_trace_failed = false;
      for (const ndtpso_map_trace_job& t : traces) some_trace_failed = some_trace_failed || t.rc != NDTPSO_OK;
      for (const ndtpso_map_trace_job& t : traces)
        ndtpso_host::check((rc_trace != NDTPSO_OK && !some_trace_failed) ? rc_trace : t.rc, "update: trace");
    }
    i = j;
  }
}

// ---- bookkeeping / export members outside the accelerated path ---------------------------------------------

void NDTFrame::addPose(double timestamp, const Vector3d& pose, const Vector3d& odom) {
  s_timestamps.push_back(timestamp);
  s_poses.push_back(pose);
  s_odoms.push_back(odom);
}

// ---- save / load (see ndtframe.h): the C-ABI's map snapshot, followed by one section of host state ------------------------------
namespace {
constexpr char kFrameMagic[8] = {'N', 'D', 'T', 'F', 'R', 'A', 'M', 'E'};
constexpr uint32_t kFrameSectionVersion = 1;
struct FrameSectionHeader {
  char magic[8];
  uint32_t version, reserved;
  uint64_t bytes, checksum;  // of what follows this header: FNV-1a over its 64-bit words
};
struct FrameFixed {  // the section's fixed part; the pose, odometry (3 doubles each) and timestamp lists follow
  double trans[3], prev_pose[3], pose_diff[3], extent[4];
  double w, c1, c2, w_dumping;
  int32_t iterations, population, num_threads, iter;
  float laser_ignore_epsilon;
  uint32_t built, last_align_ok, reserved;
  uint64_t n_poses, n_odoms, n_timestamps;
};
static_assert(sizeof(FrameSectionHeader) == 32 && sizeof(FrameFixed) == 192, "frame file layout");

uint64_t fnv1a_words(const unsigned char* p, size_t bytes) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i + 8 <= bytes; i += 8) {
    uint64_t w;
    std::memcpy(&w, p + i, 8);
    h = (h ^ w) * 0x100000001b3ull;
  }
  return h;
}
bool save_refused(int rc, const char* what) {
  ndtpso_host::check(rc, what);
  return false;
}
NDTFrame* load_refused(int rc, const char* what) {
  ndtpso_host::check(rc, what);
  return nullptr;
}
}  // namespace

bool NDTFrame::save(const char* path) const {
  if (!path) return save_refused(NDTPSO_E_ARG, "save: null path");
  if (!s_resident)
    return save_refused(NDTPSO_E_STATE, numOfCells >= (1u << 21) ? "save: a frame of 2^21 cells or more is kept on the host's side and cannot be saved"
                                                                  : "save: the frame is not resident");
  if (d_scan_ && !d_map_) return save_refused(NDTPSO_E_STATE, "save: a one-cell scan frame holds no map");
  ndtpso_host::Use use(dev());
  ndtpso_map* m = const_cast<NDTFrame*>(this)->ensureMap();  // (a frame nothing was done to yet: an empty map)
  if (!m) return save_refused(NDTPSO_E_STATE, "save: no device map");
  uint64_t blob_bytes = 0;
  if (!ndtpso_host::check(ndtpso_map_snapshot_size(m, &blob_bytes), "save")) return false;
  FrameFixed fx;
  std::memset(&fx, 0, sizeof(fx));
  for (int a = 0; a < 3; ++a) {
    fx.trans[a] = s_trans[a];
    fx.prev_pose[a] = s_prev_pose[a];
    fx.pose_diff[a] = s_pose_diff[a];
  }
  fx.extent[0] = s_x_min;
  fx.extent[1] = s_x_max;
  fx.extent[2] = s_y_min;
  fx.extent[3] = s_y_max;
  fx.w = s_config.psoConfig.coeff.w;
  fx.c1 = s_config.psoConfig.coeff.c1;
  fx.c2 = s_config.psoConfig.coeff.c2;
  fx.w_dumping = s_config.psoConfig.coeff.w_dumping;
  fx.iterations = s_config.psoConfig.iterations;
  fx.population = s_config.psoConfig.populationSize;
  fx.num_threads = s_config.psoConfig.num_threads;
  fx.iter = s_iter;
  fx.laser_ignore_epsilon = s_config.laserIgnoreEpsilon;
  fx.built = built ? 1u : 0u;
  fx.last_align_ok = s_last_align_ok ? 1u : 0u;
  fx.n_poses = s_poses.size();
  fx.n_odoms = s_odoms.size();
  fx.n_timestamps = s_timestamps.size();
  const size_t section = sizeof(fx) + 24 * (s_poses.size() + s_odoms.size()) + 8 * s_timestamps.size();
  std::vector<unsigned char> file((size_t)blob_bytes + sizeof(FrameSectionHeader) + section);
  if (!ndtpso_host::check(ndtpso_map_snapshot(m, file.data(), blob_bytes, &blob_bytes), "save")) return false;
  unsigned char* at = file.data() + blob_bytes + sizeof(FrameSectionHeader);
  std::memcpy(at, &fx, sizeof(fx));
  at += sizeof(fx);
  for (const vector<Vector3d>* list : {&s_poses, &s_odoms})
    for (const Vector3d& v : *list) {
      const double xyz[3] = {v.x(), v.y(), v.z()};
      std::memcpy(at, xyz, 24);
      at += 24;
    }
  if (!s_timestamps.empty()) std::memcpy(at, s_timestamps.data(), 8 * s_timestamps.size());
  FrameSectionHeader sh;
  std::memset(&sh, 0, sizeof(sh));
  std::memcpy(sh.magic, kFrameMagic, 8);
  sh.version = kFrameSectionVersion;
  sh.bytes = section;
  sh.checksum = fnv1a_words(file.data() + blob_bytes + sizeof(sh), section);
  std::memcpy(file.data() + blob_bytes, &sh, sizeof(sh));
  // written beside the target and renamed over it: a reader never sees half a file
  const std::string tmp = std::string(path) + ".tmp";
  FILE* f = std::fopen(tmp.c_str(), "wb");
  if (!f) return save_refused(NDTPSO_E_ARG, "save: cannot create the file");
  const bool written = std::fwrite(file.data(), 1, file.size(), f) == file.size();
  const bool closed = std::fclose(f) == 0;
  if (!written || !closed || std::rename(tmp.c_str(), path) != 0) {
    std::remove(tmp.c_str());
    return save_refused(NDTPSO_E_ARG, "save: cannot write the file");
  }
  return true;
}

NDTFrame* NDTFrame::load(const char* path) {
  if (!path) return load_refused(NDTPSO_E_ARG, "load: null path");
  if (!ndtpso_host::resident_default()) return load_refused(NDTPSO_E_STATE, "load: frames are not resident (NDTPSO_RESIDENT=0)");
  std::vector<unsigned char> file;
  {
    FILE* f = std::fopen(path, "rb");
    if (!f) return load_refused(NDTPSO_E_ARG, "load: cannot open the file");
    unsigned char buf[1 << 16];
    for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;) file.insert(file.end(), buf, buf + n);
    std::fclose(f);
  }
  uint64_t blob_bytes = 0;
  if (file.size() >= NDTPSO_SNAPSHOT_BYTES_OFFSET + 8) std::memcpy(&blob_bytes, file.data() + NDTPSO_SNAPSHOT_BYTES_OFFSET, 8);
  ndtpso_snapshot_info info;
  if (blob_bytes > file.size() || ndtpso_snapshot_describe(file.data(), blob_bytes, &info) != NDTPSO_OK)
    return load_refused(NDTPSO_E_ARG, "load: the file does not begin with a valid map snapshot");
  FrameSectionHeader sh;
  FrameFixed fx;
  if (file.size() - blob_bytes < sizeof(sh) + sizeof(fx)) return load_refused(NDTPSO_E_ARG, "load: the host section is missing");
  std::memcpy(&sh, file.data() + blob_bytes, sizeof(sh));
  const unsigned char* section = file.data() + blob_bytes + sizeof(sh);
  if (std::memcmp(sh.magic, kFrameMagic, 8) != 0 || sh.version != kFrameSectionVersion || sh.bytes != file.size() - blob_bytes - sizeof(sh) ||
      sh.checksum != fnv1a_words(section, (size_t)sh.bytes))
    return load_refused(NDTPSO_E_ARG, "load: bad host section (magic, version, length or checksum)");
  std::memcpy(&fx, section, sizeof(fx));
  const uint64_t lists = (sh.bytes - sizeof(fx)) / 8;
  if (fx.n_poses > lists || fx.n_odoms > lists || fx.n_timestamps > lists ||
      sh.bytes != sizeof(fx) + 24 * (fx.n_poses + fx.n_odoms) + 8 * fx.n_timestamps)
    return load_refused(NDTPSO_E_ARG, "load: bad host section (list lengths)");
  NDTPSOConfig cfg;
  cfg.psoConfig.iterations = fx.iterations;
  cfg.psoConfig.populationSize = fx.population;
  cfg.psoConfig.num_threads = fx.num_threads;
  cfg.psoConfig.coeff.w = fx.w;
  cfg.psoConfig.coeff.c1 = fx.c1;
  cfg.psoConfig.coeff.c2 = fx.c2;
  cfg.psoConfig.coeff.w_dumping = fx.w_dumping;
  cfg.laserIgnoreEpsilon = fx.laser_ignore_epsilon;
  std::unique_ptr<NDTFrame> frame(new NDTFrame(Vector3d(fx.trans[0], fx.trans[1], fx.trans[2]), info.grid.width, info.grid.height,
                                               info.grid.cell_side, true, cfg, info.og_cell_size));
  if (!frame->s_resident) return load_refused(NDTPSO_E_STATE, "load: the frame is not resident");
  ndtpso_host::Use use(frame->dev());
  // (the pool ndtpso_map_create would have got, or twice what the saved map fills if that is more)
  const uint64_t pool = std::max<uint64_t>(map_pool_bytes(frame->numOfCells), 2 * 512 * info.n_chunks);
  if (!ndtpso_host::check(ndtpso_map_restore(ndtpso_host::device(), file.data(), blob_bytes, pool, &frame->d_map_), "load")) {
    frame->d_map_ = nullptr;
    return nullptr;
  }
  frame->s_prev_pose = Vector3d(fx.prev_pose[0], fx.prev_pose[1], fx.prev_pose[2]);
  frame->s_pose_diff = Vector3d(fx.pose_diff[0], fx.pose_diff[1], fx.pose_diff[2]);
  frame->s_x_min = fx.extent[0];
  frame->s_x_max = fx.extent[1];
  frame->s_y_min = fx.extent[2];
  frame->s_y_max = fx.extent[3];
  frame->s_iter = fx.iter;
  frame->built = fx.built != 0;
  frame->s_last_align_ok = fx.last_align_ok != 0;
  const unsigned char* at = section + sizeof(fx);
  for (vector<Vector3d>* list : {&frame->s_poses, &frame->s_odoms}) {
    const uint64_t n = list == &frame->s_poses ? fx.n_poses : fx.n_odoms;
    for (uint64_t k = 0; k < n; ++k, at += 24) {
      double xyz[3];
      std::memcpy(xyz, at, 24);
      list->push_back(Vector3d(xyz[0], xyz[1], xyz[2]));
    }
  }
  frame->s_timestamps.resize((size_t)fx.n_timestamps);
  if (fx.n_timestamps) std::memcpy(frame->s_timestamps.data(), at, 8 * (size_t)fx.n_timestamps);
  return frame.release();
}

void NDTFrame::resetCells() {
  ndtpso_host::Use use(dev());
  for (NDTCell& c : cells) c.reset();
  if (d_map_) ndtpso_host::check(ndtpso_map_reset(d_map_), "resetCells");
  if (d_scan_) {
    ndtpso_host::release_scan(d_scan_, d_scan_cap_);
    d_scan_ = nullptr;
    d_scan_upper_ = 0;
  }
}

// reference: transform, ndtframe.cpp:119-140 (never called by the node; re-bins every stored point)
void NDTFrame::transform(Vector3d trans) {
  ndtpso_host::Use use(dev());
  if (trans.isZero(1e-6)) return;
  if (s_resident) {
    std::vector<double> pts;
    residentPoints(false, pts);
    ndtpso_map* m = ensureMap();
    if (!ndtpso_host::check(ndtpso_map_clear(m), "transform")) return;  // fresh cells (ndtframe.cpp:123): not built
    const double t[3] = {trans.x(), trans.y(), trans.z()};
    if (!ndtpso_host::check(ndtpso_map_insert_host(m, pts.data(), (uint32_t)(pts.size() / 2), t), "transform")) {
      // the device refused the transformed points after the map was emptied: put the points back where they were
      // rather than leave an empty frame behind (the failure itself is on record, ndtpso_slam/status.h)
      ndtpso_host::check(ndtpso_map_insert_host(m, pts.data(), (uint32_t)(pts.size() / 2), nullptr), "transform (restore)");
    }
    built = false;
    return;
  }
  std::vector<double> xy;
  for (const NDTCell& c : cells) {  // cell order, slot order, insertion order (the loops of ndtframe.cpp:126-134)
    if (!c.win_) continue;
    for (auto& slot : c.win_->points)
      for (const Vector2d& p : slot) {
        xy.push_back(p.x());
        xy.push_back(p.y());
      }
  }
  for (uint32_t i : s_created) cells[i] = NDTCell();
  s_created.clear();
  const uint32_t n = (uint32_t)(xy.size() / 2);
  if (n) {
    std::vector<int32_t> idx(n);
    const double t[3] = {trans.x(), trans.y(), trans.z()};
    const ndtpso_grid grid = grid_of(*this);
    if (ndtpso_host::check(ndtpso_points_to_cells(ndtpso_host::device(), &grid, xy.data(), n, t, xy.data(), idx.data()), "transform"))
      append(xy.data(), idx.data(), n);
  }
  built = false;
}

// reference: dumpMap, ndtframe.cpp:268-422 -- <name>.pose.csv, <name>.map.csv, <name>.gnuplot, the map image and
// the occupancy-grid image, same file names and text formats.  The reference draws the images with OpenCV when it
// was found at build time; here they are always drawn (raster.h), so pixel-level equality with OpenCV's line and
// circle primitives is not claimed.  Shutdown-time export, not on the alignment path.
void NDTFrame::dumpMap(const char* filename, bool save_poses, bool save_points, bool save_image, short density
#if BUILD_OCCUPANCY_GRID
                       ,
                       bool save_occupancy_grid
#endif
) {
  using ndtpso_host::Raster;
  using ndtpso_host::Rgb;
  ndtpso_host::Use use(dev());
  FILE *poses = nullptr, *points = nullptr;
  char name[1280];
  if (save_poses) {
    std::snprintf(name, sizeof(name), "%s.pose.csv", filename);
    if ((poses = std::fopen(name, "w"))) std::fprintf(poses, "timestamp,xP,yP,thP,xO,yO,thO\n");
  }
  if (save_points) {
    std::snprintf(name, sizeof(name), "%s.map.csv", filename);
    if ((points = std::fopen(name, "w"))) std::fprintf(points, "x,y\n");
  }
  if ((save_poses && !poses) || (save_points && !points)) {  // ndtframe.cpp:294-297
    std::printf("%s: Cannot open files, cannot save!\n ", __func__);
    if (poses) std::fclose(poses);
    if (points) std::fclose(points);
    return;
  }

  const int size_x = width * density, size_y = height * density;  // density in pixels per metre
  Raster img(save_image ? size_x : 1, save_image ? size_y : 1, 3, 255);  // cv::Mat(rows = size_x, cols = size_y), :304
  if (save_image && density > 0)
    for (int i = 0; i < size_x; i += density) {  // one grid line per metre
      img.line(i, 0, i, size_y, Rgb{180, 180, 180});
      img.line(0, i, size_x, i, Rgb{180, 180, 180});
    }

  // every stored point, in cell order then window-slot order then insertion order (ndtframe.cpp:314-328)
  auto emit = [&](double x, double y) {
    if (save_image)
      img.circle(size_x / 2 + static_cast<int>(x * density), size_y / 2 - static_cast<int>(y * density), 1, Rgb{0, 0, 0});
    if (save_points) std::fprintf(points, "%.5f,%.5f\n", x, y);
  };
  if (s_resident) {
    std::vector<double> pts;
    residentPoints(false, pts);
    for (size_t i = 0; i + 1 < pts.size(); i += 2) emit(pts[i], pts[i + 1]);
  } else {
    for (const NDTCell& c : cells) {
      if (!c.win_) continue;
      for (const auto& slot : c.win_->points)
        for (const Vector2d& p : slot) emit(p.x(), p.y());
    }
  }

  int counter = 0;
  for (size_t i = 0; i < s_poses.size(); ++i) {  // ndtframe.cpp:331-350
    if (save_image) {
      const int x = size_x / 2 + static_cast<int>(s_poses[i].x() * density);
      const int y = size_y / 2 - static_cast<int>(s_poses[i].y() * density);
      const int dx = static_cast<int>(.5 * std::cos(-s_poses[i].z()) * density);
      const int dy = static_cast<int>(.5 * std::sin(-s_poses[i].z()) * density);
      if (counter == 0) img.line(x, y, x + dx, y + dy, Rgb{80, 40, 40});  // cv::Scalar is BGR
      img.circle(x, y, 2, Rgb{255, 0, 0});
      counter = (counter + 1) % 5;
    }
    // the reference guards the pose rows with save_points (:347); they go to the pose file, four columns
    if (save_points && poses)
      std::fprintf(poses, "%.6f,%.5f,%.5f,%.5f\n", s_timestamps[i], s_poses[i].x(), s_poses[i].y(), s_poses[i].z());
  }
  if (poses) std::fclose(poses);
  if (points) std::fclose(points);

  if (save_poses || save_points) {  // ndtframe.cpp:358-390
    std::snprintf(name, sizeof(name), "%s.gnuplot", filename);
    if (FILE* gp = std::fopen(name, "w")) {
      std::fprintf(gp, "set datafile separator ','\nset key autotitle columnhead\nset size ratio -1\nplot ");
      if (save_points)
        std::fprintf(gp, "'%s.map.csv' title 'Map' with points pointsize 0.2 pointtype 5 linecolor rgb '#555555'",
                     filename);
      if (save_poses)
        std::fprintf(gp,
                     ", \\\n'%s.pose.csv' using 2:3 title 'Pose (LiDAR)' with linespoints linewidth 0.7 "
                     "pointtype 6 pointsize 0.7 linecolor rgb '#ff0000'",
                     filename);
      std::fprintf(gp, "\npause 1000\n");
      std::fclose(gp);
    }
  }

  if (save_image) {  // ndtframe.cpp:393-398
    std::snprintf(name, sizeof(name), "%s-w%d-%dp%di-%dx%d-c%.2f-%dppm.png", filename, NDT_WINDOW_SIZE,
                  s_config.psoConfig.populationSize, s_config.psoConfig.iterations, width, height, cell_side, density);
    if (!img.writePng(name)) std::printf("%s: cannot write %s\n", __func__, name);
  }

#if BUILD_OCCUPANCY_GRID
  fetchOccupancy();
  const auto& g = s_occupancy_grid;
  if (save_occupancy_grid && g.cell_size > 0. && g.min_x_ind <= g.max_x_ind && g.min_y_ind <= g.max_y_ind) {
    // ndtframe.cpp:401-420.  The reference sizes the image (max - min) and then addresses row (max - min) and
    // column (max - min), one past the end; this image has the extra row and column instead.
    const uint32_t real_width = g.max_x_ind - g.min_x_ind, real_height = g.max_y_ind - g.min_y_ind;
    Raster og_img((int)real_height + 1, (int)real_width + 1, 1, 255);
    for (uint32_t i = g.min_x_ind; i <= g.max_x_ind; ++i)
      for (uint32_t j = g.min_y_ind; j <= g.max_y_ind; ++j) {
        const size_t ind = (size_t)i + (size_t)g.height * j;
        if (ind < g.og.size() && g.og[ind] > 0)
          og_img.put(int(i - g.min_x_ind), int(real_height - (j - g.min_y_ind)),
                     Rgb{uint8_t(255.0 - g.og[ind] * 2.55), 0, 0});
      }
    std::snprintf(name, sizeof(name), "%s-%dx%d-cell%.2fm-occupancy-grid.png", filename, g.width, g.height, g.cell_size);
    if (!og_img.writePng(name)) std::printf("%s: cannot write %s\n", __func__, name);
  }
#endif
}
