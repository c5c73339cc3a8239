// R robots served by ONE host thread, in lock step: every robot runs the live sequence of NDTPSONode::scan_matcher_ (reference
// src/ndtpso_slam_node.cpp:177-244: loadLaser, align, update, a fresh one-cell per-scan frame) on frames of its own, and each
// phase of a step goes to the device for all R robots together -- NDTFrame::loadLaserBatch, alignBatch, updateBatch: a handful
// of launches per step -- instead of one robot after the other.
// Robot r replays the recorded scans from scan r * stride on, cyclically (stride = n_scans / R, NODE_FLEET_STRIDE overrides), so
// the R maps differ.  One thread, one std::rand() stream: srand(seed), drawn in robot order within a step -- so a fleet of one is
// `node_replay scans.bin ... seed`, and NODE_FLEET_SEQUENTIAL=1, which makes every call per robot (R x loadLaser, R x align,
// R x update), is the same computation without the shared launches.  NODE_FLEET_LOAD=calls / NODE_FLEET_UPDATE=calls keep the
// R member calls for that phase only (both: the step as it was before the load and update phases were batched).
//
//   usage: node_fleet scans.bin frame_size cell_side iterations population seed robots [out_prefix]
//   writes <out_prefix>.<r>.poses ("k x y theta" per scan, %.17g: node_replicas' format) and prints one JSON line: aggregate
//   scans per second, mean / p95 / max time per step, and the mean HOST time per phase of a step (load / align / update: load and
//   update only enqueue, so their share of the device's time shows up in the phase that next waits -- the alignment).
//   The first NODE_FLEET_WARM steps (default 10: maps and scan buffers get allocated) are replayed but not timed.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ndtpso_slam/core.h"
#include "ndtpso_slam/ndtframe.h"
#include "ndtpso_slam/status.h"

int main(int argc, char** argv) {
  if (argc < 8) {
    std::fprintf(stderr, "usage: %s scans.bin frame_size cell_side iterations population seed robots [out_prefix]\n", argv[0]);
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n_scans = 0, n_beams = 0;
  float amin = 0, ainc = 0, rmax = 0;
  if (std::fread(&n_scans, 4, 1, f) != 1 || std::fread(&n_beams, 4, 1, f) != 1 || std::fread(&amin, 4, 1, f) != 1 ||
      std::fread(&ainc, 4, 1, f) != 1 || std::fread(&rmax, 4, 1, f) != 1 || n_scans < 1 || n_beams < 1)
    return 2;
  std::vector<float> all((size_t)n_scans * (size_t)n_beams);
  if (std::fread(all.data(), 4, all.size(), f) != all.size()) return 2;
  std::fclose(f);
  const unsigned short frame_size = (unsigned short)std::atoi(argv[2]);
  const double cell_side = std::atof(argv[3]);
  NDTPSOConfig conf;
  conf.psoConfig.iterations = std::atoi(argv[4]);
  conf.psoConfig.populationSize = std::atoi(argv[5]);
  const unsigned seed = (unsigned)std::atoi(argv[6]);
  const int R = std::max(1, std::atoi(argv[7]));
  const char* prefix = argc > 8 ? argv[8] : nullptr;
  const int warm = std::min(n_scans - 1, std::getenv("NODE_FLEET_WARM") ? std::atoi(std::getenv("NODE_FLEET_WARM")) : 10);
  const int stride = std::getenv("NODE_FLEET_STRIDE") ? std::max(0, std::atoi(std::getenv("NODE_FLEET_STRIDE"))) : std::max(1, n_scans / R);
  const bool sequential = std::getenv("NODE_FLEET_SEQUENTIAL") && std::getenv("NODE_FLEET_SEQUENTIAL")[0] == '1';
  auto as_calls = [&](const char* name) {
    const char* e = std::getenv(name);
    return sequential || (e && std::string(e) == "calls");
  };
  const bool load_calls = as_calls("NODE_FLEET_LOAD"), update_calls = as_calls("NODE_FLEET_UPDATE");

  ndtpso_slam_device_init();  // before srand(): keep runtime start-up out of the rand() stream (node_replay)
  std::srand(seed);
  const Vector3d initial_pose = Vector3d::Zero();
  std::vector<NDTFrame*> ref((size_t)R), cur((size_t)R);
  std::vector<Vector3d> previous((size_t)R, initial_pose), current((size_t)R, initial_pose);
  std::vector<FILE*> out((size_t)R, nullptr);
  for (int r = 0; r < R; ++r) {
    ref[(size_t)r] = new NDTFrame(Vector3d::Zero(), frame_size, frame_size, cell_side, true, conf);  // :64-66
    cur[(size_t)r] = new NDTFrame(initial_pose, frame_size, frame_size, cell_side, false);           // :73
    if (prefix) out[(size_t)r] = std::fopen((std::string(prefix) + "." + std::to_string(r) + ".poses").c_str(), "w");
  }
  std::vector<std::vector<float>> ranges((size_t)R, std::vector<float>((size_t)n_beams));
  std::vector<NDTAlignRequest> reqs((size_t)R);
  std::vector<NDTLoadRequest> loads((size_t)R);
  std::vector<NDTUpdateRequest> updates((size_t)R);
  std::vector<double> step_ms;
  double phase_ms[3] = {0., 0., 0.};  // host time in load / align / update over the timed steps
  int failed = 0;
  std::chrono::steady_clock::time_point t_start{};
  for (int k = 0; k < n_scans; ++k) {
    if (k == warm) t_start = std::chrono::steady_clock::now();
    const auto t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < R; ++r) {
      const size_t s = (size_t)(((long long)r * stride + k) % n_scans);
      std::copy(all.begin() + s * (size_t)n_beams, all.begin() + (s + 1) * (size_t)n_beams, ranges[(size_t)r].begin());
      if (load_calls) cur[(size_t)r]->loadLaser(ranges[(size_t)r], amin, ainc, rmax);  // :186
      loads[(size_t)r] = NDTLoadRequest{cur[(size_t)r], &ranges[(size_t)r], amin, ainc, rmax};
    }
    if (!load_calls) NDTFrame::loadLaserBatch(loads.data(), (size_t)R);
    const auto t_loaded = std::chrono::steady_clock::now();
    if (k > 0) {  // :188-194
      if (sequential) {
        for (int r = 0; r < R; ++r) {
          current[(size_t)r] = ref[(size_t)r]->align(previous[(size_t)r], cur[(size_t)r]);
          if (!ref[(size_t)r]->lastAlignOk()) ++failed;
        }
      } else {
        for (int r = 0; r < R; ++r) reqs[(size_t)r] = NDTAlignRequest{ref[(size_t)r], cur[(size_t)r], previous[(size_t)r], initial_pose, false};
        NDTFrame::alignBatch(reqs.data(), (size_t)R);
        for (int r = 0; r < R; ++r) {
          current[(size_t)r] = reqs[(size_t)r].pose;
          if (!reqs[(size_t)r].ok) ++failed;
        }
      }
    }
    const auto t_aligned = std::chrono::steady_clock::now();
    for (int r = 0; r < R; ++r) {
      previous[(size_t)r] = current[(size_t)r];
      if (update_calls) ref[(size_t)r]->update(current[(size_t)r], cur[(size_t)r]);  // :198
      updates[(size_t)r] = NDTUpdateRequest{ref[(size_t)r], current[(size_t)r], cur[(size_t)r]};
    }
    if (!update_calls) NDTFrame::updateBatch(updates.data(), (size_t)R);
    const auto t1 = std::chrono::steady_clock::now();
    if (k >= warm && k > 0) {
      step_ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
      phase_ms[0] += std::chrono::duration<double, std::milli>(t_loaded - t0).count();
      phase_ms[1] += std::chrono::duration<double, std::milli>(t_aligned - t_loaded).count();
      phase_ms[2] += std::chrono::duration<double, std::milli>(t1 - t_aligned).count();
    }
    for (int r = 0; r < R; ++r) {
      if (out[(size_t)r])
        std::fprintf(out[(size_t)r], "%d %.17g %.17g %.17g\n", k, current[(size_t)r].x(), current[(size_t)r].y(), current[(size_t)r].z());
      delete cur[(size_t)r];  // :228-230
      cur[(size_t)r] = new NDTFrame(initial_pose, frame_size, frame_size, frame_size, false);
    }
  }
  const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
  for (int r = 0; r < R; ++r) {
    delete cur[(size_t)r];
    delete ref[(size_t)r];
    if (out[(size_t)r]) std::fclose(out[(size_t)r]);
  }
  std::sort(step_ms.begin(), step_ms.end());
  double mean = 0.;
  for (double v : step_ms) mean += v;
  mean /= (double)std::max<size_t>(step_ms.size(), 1);
  const double n_steps = (double)std::max<size_t>(step_ms.size(), 1);
  const double p95 = step_ms.empty() ? 0. : step_ms[(size_t)(0.95 * (double)(step_ms.size() - 1))];
  std::printf("{\"robots\": %d, \"sequential\": %d, \"timed_steps\": %d, \"wall_s\": %.6f, \"aggregate_scans_per_s\": %.1f, "
              "\"ms_per_step_mean\": %.4f, \"ms_per_step_p95\": %.4f, \"ms_per_step_max\": %.4f, \"failed_alignments\": %d, "
              "\"device_errors\": %lu, \"cluster_timeouts\": %lu, \"load\": \"%s\", \"update\": \"%s\", "
              "\"host_ms_load_mean\": %.4f, \"host_ms_align_mean\": %.4f, \"host_ms_update_mean\": %.4f, "
              "\"host_ms_note\": \"host time per phase of a step; load and update only enqueue\"}\n",
              R, sequential ? 1 : 0, n_scans - warm, wall, wall > 0. ? (double)R * (n_scans - warm) / wall : 0., mean, p95,
              step_ms.empty() ? 0. : step_ms.back(), failed, ndtpso_slam_error_count(), ndtpso_slam_cluster_timeouts(),
              load_calls ? "calls" : "batch", update_calls ? "calls" : "batch", phase_ms[0] / n_steps, phase_ms[1] / n_steps,
              phase_ms[2] / n_steps);
  return 0;
}
