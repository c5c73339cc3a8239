// NDTFrame::save / NDTFrame::load across processes: the live sequence (loadLaser -> align -> update, node_replay's) run straight
// through, or cut in two by a file.  Every pose is printed as hex floats (%a), so a test compares bits.
//   usage: snapshot_check scans.bin frame_size cell_side seed0 straight N        scans 0 .. N-1 in one process
//          snapshot_check scans.bin frame_size cell_side seed0 save N FILE       scans 0 .. N-1, then save the reference frame to FILE
//          snapshot_check scans.bin frame_size cell_side seed0 resume FILE N     load FILE (saved by `save N/2 FILE`) and run scans
//                                                                                N/2 .. N-1 from the pose the loaded frame tracks from
//     scans.bin   node_replay's format (see node_replay.cpp)
//     seed0       ndtpso_slam_thread_srand(seed0 + k) before scan k: no state of the random stream crosses the save
//   prints   pose <k> <x> <y> <th>           per scan
//            saved <0|1> errors <count> last <text>     (save)
//            loaded 0 errors <count> last <text>    (resume, when the file is refused; exit status 1)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "ndtpso_slam/core.h"
#include "ndtpso_slam/ndtframe.h"
#include "ndtpso_slam/status.h"

int main(int argc, char** argv) {
  if (argc < 7) return 2;
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
  const unsigned short frame_size = (unsigned short)std::atoi(argv[2]);
  const double cell_side = std::strtod(argv[3], nullptr);
  const unsigned seed0 = (unsigned)std::strtoul(argv[4], nullptr, 10);
  const char* mode = argv[5];
  const bool straight = !std::strcmp(mode, "straight"), save = !std::strcmp(mode, "save"), resume = !std::strcmp(mode, "resume");
  if (!(straight || save || resume) || ((save || resume) && argc < 8)) return 2;
  const int n = std::atoi(resume ? argv[7] : argv[6]);
  const char* file = save ? argv[7] : resume ? argv[6] : nullptr;
  if (n < 1 || n > n_scans) return 2;

  ndtpso_slam_device_init();
  std::unique_ptr<NDTFrame> ref;
  int first = 0;
  Vector3d previous_pose = Vector3d::Zero();
  if (resume) {
    ref.reset(NDTFrame::load(file));
    if (!ref) {
      std::printf("loaded 0 errors %lu last %s\n", ndtpso_slam_error_count(), ndtpso_slam_last_error());
      return 1;
    }
    previous_pose = ref->lastPose();
  } else {
    ref.reset(new NDTFrame(Vector3d::Zero(), frame_size, frame_size, cell_side, true));
  }
  if (resume) first = n / 2;  // (the file was saved after the first half)
  for (int k = first; k < n; ++k) {
    ndtpso_slam_thread_srand(seed0 + (unsigned)k);
    NDTFrame current(Vector3d::Zero(), frame_size, frame_size, k == 0 ? cell_side : (double)frame_size, false);
    current.loadLaser(scans[(size_t)k], amin, ainc, rmax);
    const Vector3d pose = k == 0 ? previous_pose : ref->align(previous_pose, &current);
    previous_pose = pose;
    ref->update(pose, &current);
    ref->addPose(0.025 * k, pose);
    std::printf("pose %d %a %a %a\n", k, pose.x(), pose.y(), pose.z());
  }
  if (save) {
    const unsigned long before = ndtpso_slam_error_count();
    const bool ok = ref->save(file);
    std::printf("saved %d errors %lu last %s\n", ok ? 1 : 0, ndtpso_slam_error_count() - before, ok ? "" : ndtpso_slam_last_error());
  }
  return 0;
}
