// NDTFrame::relocalize on a map built from recorded scans: the map is made with update() at given poses, the query scan is
// searched over a pose lattice and its best nodes refined, and one align() follows from the result, as a node would go on.
// Everything is printed as hex floats (%a), so a test compares bits.
//   usage: relocalize_check scans.bin width height cell_side seed top_k query ox oy oth sx sy sth nx ny nth  x0 y0 th0  x1 y1 th1 ...
//     scans.bin      node_replay's format (see node_replay.cpp); scan m is inserted at (xm, ym, thm), m = 0 .. number of poses - 1
//     query          index of the scan to relocalize
//     seed           srand() before relocalize (the PSO's random numbers, as the reference draws them)
//   prints   relocalize ok <0|1> hits <n> pose <x> <y> <th> cost <c>
//            align <x> <y> <th>                       (only after a successful relocalize)
//            errors <count recorded by the call> refused <updates refused afterwards> last <text>     (only after a failure,
//                                                      followed by an update() with the returned pose)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ndtpso_slam/core.h"
#include "ndtpso_slam/ndtframe.h"
#include "ndtpso_slam/status.h"

int main(int argc, char** argv) {
  if (argc < 17 || (argc - 17) % 3 != 0) return 2;
  FILE* f = std::fopen(argv[1], "rb");
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
  const unsigned short width = (unsigned short)std::atoi(argv[2]), height = (unsigned short)std::atoi(argv[3]);
  const double cell_side = std::strtod(argv[4], nullptr);
  const unsigned seed = (unsigned)std::strtoul(argv[5], nullptr, 10), top_k = (unsigned)std::strtoul(argv[6], nullptr, 10);
  const long query = std::strtol(argv[7], nullptr, 10);
  const Vector3d origin(std::strtod(argv[8], nullptr), std::strtod(argv[9], nullptr), std::strtod(argv[10], nullptr));
  const Vector3d step(std::strtod(argv[11], nullptr), std::strtod(argv[12], nullptr), std::strtod(argv[13], nullptr));
  const unsigned count[3] = {(unsigned)std::strtoul(argv[14], nullptr, 10), (unsigned)std::strtoul(argv[15], nullptr, 10),
                             (unsigned)std::strtoul(argv[16], nullptr, 10)};
  const int n_poses = (argc - 17) / 3;
  if (n_poses > n_scans || query < 0 || query >= n_scans) return 2;
  const unsigned short side = width > height ? width : height;

  NDTFrame map(Vector3d::Zero(), width, height, cell_side, true);
  for (int m = 0; m < n_poses; ++m) {
    NDTFrame scan(Vector3d::Zero(), width, height, side, false);
    scan.loadLaser(scans[(size_t)m], amin, ainc, rmax);
    map.update(Vector3d(std::strtod(argv[17 + 3 * m], nullptr), std::strtod(argv[18 + 3 * m], nullptr), std::strtod(argv[19 + 3 * m], nullptr)),
               &scan);
  }
  NDTFrame cur(Vector3d::Zero(), width, height, side, false);
  cur.loadLaser(scans[(size_t)query], amin, ainc, rmax);
  const unsigned long errors_before = ndtpso_slam_error_count();
  std::srand(seed);
  const NDTRelocalizeResult r = map.relocalize(&cur, origin, step, count, top_k);
  std::printf("relocalize ok %d hits %u pose %a %a %a cost %a\n", r.ok ? 1 : 0, r.hits, r.pose.x(), r.pose.y(), r.pose.z(), r.cost);
  if (r.ok) {
    const Vector3d next = map.align(r.pose, &cur);
    std::printf("align %a %a %a\n", next.x(), next.y(), next.z());
    return 0;
  }
  const unsigned long errors = ndtpso_slam_error_count() - errors_before;
  map.update(r.pose, &cur);
  std::printf("errors %lu refused %lu last %s\n", errors, map.updatesRefused(), ndtpso_slam_last_error());
  return 0;
}
