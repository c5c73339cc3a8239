// NDTFrame::relocalizeBatch against the member calls it stands for: R robots with maps of their own, built with update() from
// recorded scans at given poses, each with a query scan of the same file; all are relocalized -- in ONE relocalizeBatch call or
// by relocalize() robot after robot -- and every robot then makes one align() from its result, as a node would go on.
// Everything is printed as hex floats (%a), so a test compares bits.
//   usage: relocalize_fleet_check batch|member scans.bin seed R  <robot 0> <robot 1> ...
//     scans.bin   relocalize_check's format (node_replay's, see node_replay.cpp)
//     seed        srand() before the relocalizations (the PSO's random numbers, as the reference draws them): robot 0 draws first,
//                 so its result is relocalize_check's for the same seed
//     a robot     width height cell_side resident top_k query ox oy oth sx sy sth nx ny nth n_poses  scan0 x0 y0 th0  scan1 ...
//                 resident 0: the robot's map frame is made with NDTPSO_RESIDENT=0 (a request that cannot be served)
//   prints, per robot in order, relocalize_check's lines behind a line "robot <r>":
//            relocalize ok <0|1> hits <n> pose <x> <y> <th> cost <c>
//            align <x> <y> <th>                       (only after a successful relocalize)
//            errors <count recorded so far> refused <updates refused afterwards> last <text>     (only after a failure,
//                                                      followed by an update() with the returned pose)
//          then     rand <the first rand() behind the relocalizations: where they left the stream>
//          and a last line  errors <count recorded by the relocalizations> refused <updates refused, all robots> last <text>
//   The align() of robot r draws from srand(seed) advanced by the tables of r's own hits -- where the stream stands when r
//   relocalizes alone -- so that robot 0's lines are relocalize_check's, whichever robots follow it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "ndtpso_slam/core.h"
#include "ndtpso_slam/ndtframe.h"
#include "ndtpso_slam/status.h"

namespace {
struct Robot {
  unsigned short width = 0, height = 0;
  double cell_side = 0.;
  bool resident = true;
  unsigned top_k = 0;
  long query = 0;
  Vector3d origin{Vector3d::Zero()}, step{Vector3d::Zero()};
  unsigned count[3] = {0, 0, 0};
  std::vector<long> scan;
  std::vector<Vector3d> pose;
  std::unique_ptr<NDTFrame> map, cur;
};
}  // namespace

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const std::string path = argv[1];
  if (path != "batch" && path != "member") return 2;
  FILE* f = std::fopen(argv[2], "rb");
  if (!f) return 2;
  int32_t n_scans = 0, n_beams = 0;
  float amin = 0, ainc = 0, rmax = 0;
  if (std::fread(&n_scans, 4, 1, f) != 1 || std::fread(&n_beams, 4, 1, f) != 1 || std::fread(&amin, 4, 1, f) != 1 ||
      std::fread(&ainc, 4, 1, f) != 1 || std::fread(&rmax, 4, 1, f) != 1 || n_scans < 1 || n_beams < 1)
    return 2;
  std::vector<std::vector<float>> scans((size_t)n_scans, std::vector<float>((size_t)n_beams));
  for (auto& s : scans)
    if (std::fread(s.data(), 4, (size_t)n_beams, f) != (size_t)n_beams) return 2;
  std::fclose(f);
  const unsigned seed = (unsigned)std::strtoul(argv[3], nullptr, 10);
  const long n_robots = std::strtol(argv[4], nullptr, 10);
  if (n_robots < 1 || n_robots > 4096) return 2;
  std::vector<Robot> robots((size_t)n_robots);
  int at = 5;
  for (Robot& r : robots) {
    if (argc < at + 16) return 2;
    r.width = (unsigned short)std::atoi(argv[at]);
    r.height = (unsigned short)std::atoi(argv[at + 1]);
    r.cell_side = std::strtod(argv[at + 2], nullptr);
    r.resident = std::atoi(argv[at + 3]) != 0;
    r.top_k = (unsigned)std::strtoul(argv[at + 4], nullptr, 10);
    r.query = std::strtol(argv[at + 5], nullptr, 10);
    r.origin = Vector3d(std::strtod(argv[at + 6], nullptr), std::strtod(argv[at + 7], nullptr), std::strtod(argv[at + 8], nullptr));
    r.step = Vector3d(std::strtod(argv[at + 9], nullptr), std::strtod(argv[at + 10], nullptr), std::strtod(argv[at + 11], nullptr));
    for (int a = 0; a < 3; ++a) r.count[a] = (unsigned)std::strtoul(argv[at + 12 + a], nullptr, 10);
    const long n_poses = std::strtol(argv[at + 15], nullptr, 10);
    at += 16;
    if (n_poses < 0 || n_poses > n_scans || argc < at + 4 * n_poses || r.query < 0 || r.query >= n_scans) return 2;
    for (long m = 0; m < n_poses; ++m, at += 4) {
      r.scan.push_back(std::strtol(argv[at], nullptr, 10));
      if (r.scan.back() < 0 || r.scan.back() >= n_scans) return 2;
      r.pose.push_back(Vector3d(std::strtod(argv[at + 1], nullptr), std::strtod(argv[at + 2], nullptr), std::strtod(argv[at + 3], nullptr)));
    }
  }
  if (at != argc) return 2;

  const char* resident_env = std::getenv("NDTPSO_RESIDENT");
  const std::string resident_was = resident_env ? resident_env : "";
  for (Robot& r : robots) {
    const unsigned short side = r.width > r.height ? r.width : r.height;
    if (!r.resident) setenv("NDTPSO_RESIDENT", "0", 1);
    r.map.reset(new NDTFrame(Vector3d::Zero(), r.width, r.height, r.cell_side, true));
    if (!r.resident) {
      if (resident_env) setenv("NDTPSO_RESIDENT", resident_was.c_str(), 1); else unsetenv("NDTPSO_RESIDENT");
    }
    for (size_t m = 0; m < r.scan.size(); ++m) {
      NDTFrame scan(Vector3d::Zero(), r.width, r.height, side, false);
      scan.loadLaser(scans[(size_t)r.scan[m]], amin, ainc, rmax);
      r.map->update(r.pose[m], &scan);
    }
    r.cur.reset(new NDTFrame(Vector3d::Zero(), r.width, r.height, side, false));
    r.cur->loadLaser(scans[(size_t)r.query], amin, ainc, rmax);
  }

  const unsigned long errors_before = ndtpso_slam_error_count();
  std::vector<NDTRelocalizeRequest> reqs((size_t)n_robots);
  for (size_t k = 0; k < robots.size(); ++k) {
    Robot& r = robots[k];
    reqs[k].ref = r.map.get();
    reqs[k].cur = r.cur.get();
    reqs[k].origin = r.origin;
    reqs[k].step = r.step;
    std::memcpy(reqs[k].count, r.count, sizeof(r.count));
    reqs[k].top_k = r.top_k;
  }
  std::srand(seed);
  if (path == "batch") {
    NDTFrame::relocalizeBatch(reqs.data(), reqs.size());
  } else {
    for (NDTRelocalizeRequest& q : reqs) q.result = q.ref->relocalize(q.cur, q.origin, q.step, q.count, q.top_k);
  }
  const int next_rand = std::rand();  // where the relocalizations left the stream
  const unsigned long errors = ndtpso_slam_error_count() - errors_before;
  const std::string last = ndtpso_slam_last_error();

  const PSOConfig cfg;  // (what align() passes on)
  const size_t n_draw = 3 + 3 * (size_t)cfg.populationSize + 6 * (size_t)cfg.populationSize * (size_t)cfg.iterations;
  unsigned long refused = 0;
  for (size_t k = 0; k < robots.size(); ++k) {
    Robot& r = robots[k];
    const NDTRelocalizeResult& res = reqs[k].result;
    std::printf("robot %zu\n", k);
    std::printf("relocalize ok %d hits %u pose %a %a %a cost %a\n", res.ok ? 1 : 0, res.hits, res.pose.x(), res.pose.y(), res.pose.z(), res.cost);
    if (res.ok) {
      std::srand(seed);
      for (size_t d = 0; d < (size_t)res.hits * n_draw; ++d) (void)std::rand();
      const Vector3d next = r.map->align(res.pose, r.cur.get());
      std::printf("align %a %a %a\n", next.x(), next.y(), next.z());
    } else {
      r.map->update(res.pose, r.cur.get());
      std::printf("errors %lu refused %lu last %s\n", ndtpso_slam_error_count() - errors_before, r.map->updatesRefused(), ndtpso_slam_last_error());
    }
    refused += r.map->updatesRefused();
  }
  std::printf("rand %d\n", next_rand);
  std::printf("errors %lu refused %lu last %s\n", errors, refused, last.c_str());
  return 0;
}
