// NDTFrame::curvature / curvatureBatch on the live sequence of NDTPSONode::scan_matcher_ (reference src/ndtpso_slam_node.cpp:
// 177-244; node_replay.cpp): after every align() the curvature of the score at the returned pose, between the alignment and the
// update of the map -- where a node would fill its message's covariance.
//
//   usage: curvature_check member scans.bin frame_size cell_side iterations population seed [robots [robot]]
//          curvature_check batch R scans.bin frame_size cell_side iterations population seed
//   member            one robot: node_replay's calls (loadLaser, align, update, a fresh one-cell per-scan frame), curvature() after
//                     every align().  With `robots` > 1: the fleet of `batch` below, the curvatures by member calls in robot order;
//                     `robot` prints that robot's lines only.
//   batch R           R robots in lock step as node_fleet.cpp runs them (one thread, one std::rand() stream drawn in robot order,
//                     loadLaserBatch / alignBatch / updateBatch; robot r replays the scans from r * (n_scans / R) on, cyclically),
//                     the R curvatures of a step through ONE curvatureBatch.
//   prints per robot r and scan k   "pose r k x y theta"  (%.17g: node_replay's figures)
//   and after every align()         "curv r k" + the pose and the curvature in hex (%a): x y theta, cost, gradient (3), Hessian
//                                   (xx xy xth yy yth thth) -- 13 doubles -- and n_points n_hit
// With no arguments it prints this usage and exits with code 2.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ndtpso_slam/core.h"
#include "ndtpso_slam/ndtframe.h"
#include "ndtpso_slam/status.h"

static int usage(const char* exe) {
  std::fprintf(stderr,
               "usage: %s member scans.bin frame_size cell_side iterations population seed [robots [robot]]\n"
               "       %s batch R scans.bin frame_size cell_side iterations population seed\n",
               exe, exe);
  return 2;
}

static void print_curvature(int r, int k, const Vector3d& pose, const NDTCurvature& c) {
  std::printf("curv %d %d %a %a %a %a %a %a %a", r, k, pose.x(), pose.y(), pose.z(), c.cost, c.gradient.x(), c.gradient.y(), c.gradient.z());
  for (int i = 0; i < 6; ++i) std::printf(" %a", c.hessian[i]);
  std::printf(" %u %u\n", c.n_points, c.n_hit);
}

int main(int argc, char** argv) {
  if (argc < 2) return usage(argv[0]);
  const bool batch = std::strcmp(argv[1], "batch") == 0;
  if (!batch && std::strcmp(argv[1], "member") != 0) return usage(argv[0]);
  int at = 2, R = 1, only = -1;
  if (batch) {
    if (argc < 9) return usage(argv[0]);
    R = std::max(1, std::atoi(argv[at++]));
  } else if (argc < 8) {
    return usage(argv[0]);
  }
  const char* path = argv[at];
  const unsigned short frame_size = (unsigned short)std::atoi(argv[at + 1]);
  const double cell_side = std::atof(argv[at + 2]);
  NDTPSOConfig conf;
  conf.psoConfig.iterations = std::atoi(argv[at + 3]);
  conf.psoConfig.populationSize = std::atoi(argv[at + 4]);
  const unsigned seed = (unsigned)std::atoi(argv[at + 5]);
  if (!batch && argc > at + 6) R = std::max(1, std::atoi(argv[at + 6]));
  if (!batch && argc > at + 7) only = std::atoi(argv[at + 7]);

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
  std::srand(seed);
  const Vector3d initial_pose = Vector3d::Zero();
  std::vector<NDTFrame*> ref((size_t)R), cur((size_t)R);
  std::vector<Vector3d> previous((size_t)R, initial_pose), current((size_t)R, initial_pose);
  for (int r = 0; r < R; ++r) {
    ref[(size_t)r] = new NDTFrame(Vector3d::Zero(), frame_size, frame_size, cell_side, true, conf);  // :64-66
    cur[(size_t)r] = new NDTFrame(initial_pose, frame_size, frame_size, cell_side, false);           // :73
  }
  std::vector<std::vector<float>> ranges((size_t)R, std::vector<float>((size_t)n_beams));
  std::vector<NDTAlignRequest> reqs((size_t)R);
  std::vector<NDTLoadRequest> loads((size_t)R);
  std::vector<NDTUpdateRequest> updates((size_t)R);
  std::vector<NDTCurvatureRequest> curvs((size_t)R);
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
      // the curvature at the pose the alignment returned, before the map takes the scan in
      for (int r = 0; r < R; ++r) {
        curvs[(size_t)r].ref = ref[(size_t)r];
        curvs[(size_t)r].cur = cur[(size_t)r];
        curvs[(size_t)r].pose = current[(size_t)r];
      }
      if (batch) {
        NDTFrame::curvatureBatch(curvs.data(), (size_t)R);
      } else {
        for (int r = 0; r < R; ++r) curvs[(size_t)r].result = ref[(size_t)r]->curvature(current[(size_t)r], cur[(size_t)r]);
      }
    }
    for (int r = 0; r < R; ++r) {
      previous[(size_t)r] = current[(size_t)r];
      if (!fleet) ref[(size_t)r]->update(current[(size_t)r], cur[(size_t)r]);  // :198
      updates[(size_t)r] = NDTUpdateRequest{ref[(size_t)r], current[(size_t)r], cur[(size_t)r]};
    }
    if (fleet) NDTFrame::updateBatch(updates.data(), (size_t)R);
    for (int r = 0; r < R; ++r) {
      if (only < 0 || only == r) {
        std::printf("pose %d %d %.17g %.17g %.17g\n", r, k, current[(size_t)r].x(), current[(size_t)r].y(), current[(size_t)r].z());
        if (k > 0) print_curvature(r, k, current[(size_t)r], curvs[(size_t)r].result);
      }
      delete cur[(size_t)r];  // :228-230
      cur[(size_t)r] = new NDTFrame(initial_pose, frame_size, frame_size, frame_size, false);
    }
  }
  for (int r = 0; r < R; ++r) {
    delete cur[(size_t)r];
    delete ref[(size_t)r];
  }
  return ndtpso_slam_error_count() ? 1 : 0;
}
