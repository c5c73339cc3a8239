// NDTFrame::setTraceOnUpdate / traceCounts / navGrid on the live sequence of NDTPSONode::scan_matcher_ (reference
// src/ndtpso_slam_node.cpp:177-244; node_replay.cpp): every scan the map takes in is also traced through its occupancy grid, at
// the pose it is merged at.
//
//   usage: trace_check [--host-trace | --no-trace] scans.bin frame_size cell_side og_cell_size iterations population seed prefix [robots]
//   (no option)     update() traces on the device (setTraceOnUpdate); with `robots` > 1 the fleet of node_fleet.cpp in lock step
//                   (one thread, one std::rand() stream drawn in robot order, loadLaserBatch / alignBatch / updateBatch; robot r
//                   replays the scans from r * (n_scans / R) on, cyclically): the traces of a step go out through updateBatch
//   --host-trace    what a caller had to do until now: after every update() the scan's points are downloaded (collectPoints:
//                   ndtpso_points_get) and the same rule is walked here on one CPU thread, with the device's sincos of the heading
//                   (ndtpso_device_math), and the nav grid is formed here from occupancyGrid() and those counters
//   --no-trace      no tracing at all (the pose log must not change)
//   prints per robot r and scan k   "pose r k x y theta"  (%.17g: node_replay's figures)
//   writes per robot r   <prefix>.<r>.hits (uint32), <prefix>.<r>.passes (uint64), <prefix>.<r>.nav (int8): og_width * og_height
//                        entries each, raw, og[x + og_height * y]   (--no-trace: no files)
//   usage: trace_check --refusals
//   the frames tracing refuses, each asked for traceFreeSpace(), an update() with setTraceOnUpdate(true), navGrid() and
//   traceCounts(): a one-cell per-scan frame, a frame of 2.25 M cells (300 m at 0.2 m: kept on the host's side), a frame without
//   an occupancy grid, one whose grid is not square and -- under NDTPSO_RESIDENT=0 -- an ordinary frame.  Prints per call
//   "refused <frame> <call> <errors recorded by it> <navGrid's / traceCounts' return, else -> <the recorded text>"; exits 0.
// TRACE_CHECK_TIMING=1: on stderr "replayed N scans in T ms (X ms per scan)" for the loop (files not counted) and, with --host-trace,
// "host trace Y us per scan" for the download and the walk alone (scripts/trace_ab.py).
// With no arguments it prints this usage and exits with code 2.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ndtpso_hip.h"
#include "ndtpso_slam/core.h"
#include "ndtpso_slam/ndtframe.h"
#include "ndtpso_slam/status.h"

static int usage(const char* exe) {
  std::fprintf(stderr,
               "usage: %s [--host-trace | --no-trace] scans.bin frame_size cell_side og_cell_size iterations population seed prefix [robots]\n",
               exe);
  return 2;
}

// The contract of ndtpso_map_trace (include/ndtpso_hip.h) on the host, one ray after the other.
struct HostTrace {
  double hw, hh, cs;
  uint32_t w, h;
  std::vector<uint32_t> hits;
  std::vector<uint64_t> passes;
  HostTrace(double width, double height, double og_cs)
      : hw(width / 2.), hh(height / 2.), cs(og_cs), w((uint32_t)std::ceil(width / og_cs)), h((uint32_t)std::ceil(height / og_cs)),
        hits((size_t)w * h, 0u), passes((size_t)w * h, 0ull) {}
  void pass(long cx, long cy) {
    const uint64_t at = (uint64_t)cx + (uint64_t)h * (uint64_t)cy;
    if (at < passes.size()) ++passes[at];
  }
  void hit(long cx, long cy) {
    const uint64_t at = (uint64_t)cx + (uint64_t)h * (uint64_t)cy;
    if (at < hits.size()) ++hits[at];
  }
  void ray(double ox, double oy, double ex, double ey) {
    if (!(std::fabs(ox) < hw && std::fabs(oy) < hh && std::fabs(ex) < hw && std::fabs(ey) < hh)) return;
    const double fx0 = (ox + hw) / cs, fy0 = (oy + hh) / cs, fx1 = (ex + hw) / cs, fy1 = (ey + hh) / cs;
    const long ix = (long)std::floor(fx0), iy = (long)std::floor(fy0), jx = (long)std::floor(fx1), jy = (long)std::floor(fy1);
    const double dx = fx1 - fx0, dy = fy1 - fy0;
    const long sx = jx > ix ? 1 : -1, sy = jy > iy ? 1 : -1, nx = std::labs(jx - ix), ny = std::labs(jy - iy);
    const double tdx = nx ? 1. / std::fabs(dx) : 0., tdy = ny ? 1. / std::fabs(dy) : 0.;
    const double tx0 = nx ? ((double)(sx > 0 ? ix + 1 : ix) - fx0) / dx : 0.;
    const double ty0 = ny ? ((double)(sy > 0 ? iy + 1 : iy) - fy0) / dy : 0.;
    long i = 0, j = 0, cx = ix, cy = iy;
    while (i < nx || j < ny) {
      pass(cx, cy);
      bool step_x = j == ny;
      if (i < nx && j < ny) {
        const double tx = tx0 + (double)i * tdx;  // (built with -ffp-contract=off: one multiplication, one addition)
        const double ty = ty0 + (double)j * tdy;
        step_x = tx <= ty;
      }
      if (step_x) {
        ++i;
        cx += sx;
      } else {
        ++j;
        cy += sy;
      }
    }
    hit(cx, cy);
  }
  void scan(const std::vector<double>& xy, const Vector3d& pose, ndtpso_ctx* math) {
    double th = pose.z(), sn = 0., cn = 1.;
    if (ndtpso_device_math(math, 2, &th, 1, &sn, &cn) != NDTPSO_OK) std::exit(1);
    for (size_t k = 0; k + 1 < xy.size(); k += 2) {
      const double x = xy[k], y = xy[k + 1];
      const double rx = x * cn - y * sn, ry = x * sn + y * cn;
      ray(pose.x(), pose.y(), rx + pose.x(), ry + pose.y());
    }
  }
};

static int refusals() {
  ndtpso_slam_device_init();
  NDTPSOConfig conf;
  const Vector3d zero = Vector3d::Zero();
  NDTFrame scan(zero, 20, 20, 20., false);
  const std::vector<float> ranges(64, 3.f);
  scan.loadLaser(ranges, -1.5f, 0.047f, 30.f);
  struct Case {
    const char* name;
    NDTFrame* frame;
  };
  NDTFrame one_cell(zero, 20, 20, 20., false, conf, 0.5), large(zero, 300, 300, 0.2, false, conf, 0.), no_grid(zero, 20, 20, 1., true, conf, 0.),
      wide(zero, 20, 10, 1., true, conf, 0.5), plain(zero, 20, 20, 1., true, conf, 0.5);
  const Case cases[] = {{"one-cell", &one_cell}, {"large", &large}, {"no-grid", &no_grid}, {"not-square", &wide}, {"plain", &plain}};
  for (const Case& c : cases) {
    std::vector<int8_t> nav;
    std::vector<uint32_t> hits;
    std::vector<uint64_t> passes;
    unsigned w = 0, h = 0;
    for (int call = 0; call < 4; ++call) {
      static const char* const names[4] = {"traceFreeSpace", "update", "navGrid", "traceCounts"};
      ndtpso_slam_clear_error();
      int ret = -1;
      if (call == 0) c.frame->traceFreeSpace(zero, &scan);
      if (call == 1) {
        c.frame->setTraceOnUpdate(true);
        c.frame->update(zero, &scan);
        c.frame->setTraceOnUpdate(false);
      }
      if (call == 2) ret = c.frame->navGrid(nav, w, h) ? 1 : 0;
      if (call == 3) ret = c.frame->traceCounts(hits, passes) ? 1 : 0;
      std::printf("refused %s %s %lu %d -> %s\n", c.name, names[call], ndtpso_slam_error_count(), ret, ndtpso_slam_last_error());
    }
  }
  return 0;
}

template <typename T>
static bool write_raw(const std::string& path, const std::vector<T>& v) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
  return std::fclose(f) == 0 && ok;
}

int main(int argc, char** argv) {
  int at = 1;
  bool host_trace = false, no_trace = false;
  if (argc == 2 && std::strcmp(argv[1], "--refusals") == 0) return refusals();
  if (argc > 1 && std::strcmp(argv[1], "--host-trace") == 0) host_trace = true, ++at;
  else if (argc > 1 && std::strcmp(argv[1], "--no-trace") == 0) no_trace = true, ++at;
  if (argc < at + 8) return usage(argv[0]);
  const char* path = argv[at];
  const unsigned short frame_size = (unsigned short)std::atoi(argv[at + 1]);
  const double cell_side = std::atof(argv[at + 2]);
  const double og_cs = std::atof(argv[at + 3]);
  NDTPSOConfig conf;
  conf.psoConfig.iterations = std::atoi(argv[at + 4]);
  conf.psoConfig.populationSize = std::atoi(argv[at + 5]);
  const unsigned seed = (unsigned)std::atoi(argv[at + 6]);
  const std::string prefix = argv[at + 7];
  const int R = argc > at + 8 ? std::max(1, std::atoi(argv[at + 8])) : 1;
  if (!(og_cs > 0.)) return usage(argv[0]);

  FILE* f = std::fopen(path, "rb");
  if (!f) return 2;
  int32_t n_scans = 0, n_beams = 0;
  float amin = 0, ainc = 0, rmax = 0;
  if (std::fread(&n_scans, 4, 1, f) != 1 || std::fread(&n_beams, 4, 1, f) != 1 || std::fread(&amin, 4, 1, f) != 1 ||
      std::fread(&ainc, 4, 1, f) != 1 || std::fread(&rmax, 4, 1, f) != 1 || n_scans < 1 || n_beams < 1)
    return 2;
  std::vector<float> all((size_t)n_scans * (size_t)n_beams);
  if (std::fread(all.data(), 4, all.size(), f) != all.size()) return 2;
  std::fclose(f);
  const int stride = std::max(1, n_scans / R);
  const bool fleet = R > 1;  // (one robot: the member calls of node_replay themselves)

  ndtpso_slam_device_init();  // before srand(): keep runtime start-up out of the rand() stream (node_replay)
  ndtpso_ctx* math = nullptr;  // --host-trace: the device's sincos, as any caller of the C-ABI gets it
  if (host_trace && ndtpso_ctx_create(0, &math) != NDTPSO_OK) return 1;
  std::srand(seed);
  const Vector3d initial_pose = Vector3d::Zero();
  std::vector<NDTFrame*> ref((size_t)R), cur((size_t)R);
  std::vector<HostTrace> host;
  std::vector<Vector3d> previous((size_t)R, initial_pose), current((size_t)R, initial_pose);
  for (int r = 0; r < R; ++r) {
    ref[(size_t)r] = new NDTFrame(Vector3d::Zero(), frame_size, frame_size, cell_side, true, conf, og_cs);  // :64-66
    cur[(size_t)r] = new NDTFrame(initial_pose, frame_size, frame_size, cell_side, false);                 // :73
    ref[(size_t)r]->setTraceOnUpdate(!host_trace && !no_trace);
    if (host_trace) host.emplace_back((double)frame_size, (double)frame_size, og_cs);
  }
  std::vector<std::vector<float>> ranges((size_t)R, std::vector<float>((size_t)n_beams));
  std::vector<NDTAlignRequest> reqs((size_t)R);
  std::vector<NDTLoadRequest> loads((size_t)R);
  std::vector<NDTUpdateRequest> updates((size_t)R);
  std::vector<double> xy;
  const bool timing = std::getenv("TRACE_CHECK_TIMING") != nullptr;
  double host_us = 0.;
  const auto t_begin = std::chrono::steady_clock::now();
  for (int k = 0; k < n_scans; ++k) {
    for (int r = 0; r < R; ++r) {
      const size_t s = (size_t)(((long long)r * stride + k) % n_scans);
      std::copy(all.begin() + s * (size_t)n_beams, all.begin() + (s + 1) * (size_t)n_beams, ranges[(size_t)r].begin());
      if (!fleet) cur[(size_t)r]->loadLaser(ranges[(size_t)r], amin, ainc, rmax);  // :186
      loads[(size_t)r] = NDTLoadRequest{cur[(size_t)r], &ranges[(size_t)r], amin, ainc, rmax};
    }
    if (fleet) NDTFrame::loadLaserBatch(loads.data(), (size_t)R);
    if (k > 0) {  // :188-194
      if (!fleet) {
        current[0] = ref[0]->align(previous[0], cur[0]);
      } else {
        for (int r = 0; r < R; ++r) reqs[(size_t)r] = NDTAlignRequest{ref[(size_t)r], cur[(size_t)r], previous[(size_t)r], initial_pose, false};
        NDTFrame::alignBatch(reqs.data(), (size_t)R);
        for (int r = 0; r < R; ++r) current[(size_t)r] = reqs[(size_t)r].pose;
      }
    }
    for (int r = 0; r < R; ++r) {
      previous[(size_t)r] = current[(size_t)r];
      if (!fleet) ref[(size_t)r]->update(current[(size_t)r], cur[(size_t)r]);  // :198
      updates[(size_t)r] = NDTUpdateRequest{ref[(size_t)r], current[(size_t)r], cur[(size_t)r]};
    }
    if (fleet) NDTFrame::updateBatch(updates.data(), (size_t)R);
    for (int r = 0; r < R; ++r) {
      if (host_trace) {
        const auto t0 = std::chrono::steady_clock::now();
        cur[(size_t)r]->collectPoints(xy);
        host[(size_t)r].scan(xy, current[(size_t)r], math);
        host_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
      }
      std::printf("pose %d %d %.17g %.17g %.17g\n", r, k, current[(size_t)r].x(), current[(size_t)r].y(), current[(size_t)r].z());
      delete cur[(size_t)r];  // :228-230
      cur[(size_t)r] = new NDTFrame(initial_pose, frame_size, frame_size, frame_size, false);
    }
  }
  if (timing) {
    {  // the updates and traces of the last scans are only enqueued: a synchronous export drains every robot's stream
      std::vector<int8_t> drained;
      unsigned w = 0, h = 0;
      for (int r = 0; r < R; ++r) ref[(size_t)r]->navGrid(drained, w, h);
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    std::fprintf(stderr, "replayed %d scans in %.3f ms (%.4f ms per scan)\n", n_scans * R, ms, ms / (n_scans * R));
    if (host_trace) std::fprintf(stderr, "host trace %.2f us per scan\n", host_us / (n_scans * R));
  }
  bool wrote = true;
  for (int r = 0; r < R && !no_trace; ++r) {
    std::vector<uint32_t> hits;
    std::vector<uint64_t> passes;
    std::vector<int8_t> nav;
    if (host_trace) {
      hits = host[(size_t)r].hits;
      passes = host[(size_t)r].passes;
      const std::vector<int8_t>& og = ref[(size_t)r]->occupancyGrid();
      nav.resize(hits.size());
      for (size_t i = 0; i < nav.size(); ++i) {
        const uint64_t h = hits[i], p = passes[i];
        const int8_t v = i < og.size() ? og[i] : (int8_t)0;
        nav[i] = v > 0 ? v : h + p == 0 ? (int8_t)-1 : (int8_t)((100 * h + (h + p) / 2) / (h + p));
      }
    } else {
      unsigned w = 0, h = 0;
      wrote = ref[(size_t)r]->traceCounts(hits, passes) && ref[(size_t)r]->navGrid(nav, w, h) && wrote;
    }
    const std::string base = prefix + "." + std::to_string(r);
    wrote = write_raw(base + ".hits", hits) && write_raw(base + ".passes", passes) && write_raw(base + ".nav", nav) && wrote;
  }
  for (int r = 0; r < R; ++r) {
    delete cur[(size_t)r];
    delete ref[(size_t)r];
  }
  if (math) ndtpso_ctx_destroy(math);
  return (ndtpso_slam_error_count() || !wrote) ? 1 : 0;
}
