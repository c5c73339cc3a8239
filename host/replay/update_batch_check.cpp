// NDTFrame::loadLaserBatch / updateBatch against the member calls they stand for: the same sequence is driven twice on twin
// sets of frames -- once through the batch entries, once through loadLaser() / update() in request order -- and everything a
// caller can observe is printed with full precision and compared: created / built / mean per frame after syncHostView(),
// `built`, updatesRefused(), the error count, and the pose of a following align().  The requests cover the batchable case
// (resident maps, device-resident per-scan frames), a frame that owns a map used as the "scan", a frame repeated in one call, a
// frame of another thread's context and requests that follow a failed align (refused).
//   usage: update_batch_check scans.bin       (file format: see node_replay.cpp; needs >= 6 scans)   prints OK, exits 0
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "ndtpso_slam/core.h"
#include "ndtpso_slam/ndtframe.h"

namespace {
std::vector<std::vector<float>> g_scans;
float g_amin = 0, g_ainc = 0, g_rmax = 0;

void note(std::string& log, const char* tag, NDTFrame& f) {
  f.syncHostView();
  unsigned created = 0, built = 0;
  double sx = 0., sy = 0.;
  for (const NDTCell& c : f.cells) {
    created += c.created ? 1u : 0u;
    if (c.built) {
      ++built;
      sx += c.mean.x();
      sy += c.mean.y();
    }
  }
  char line[256];
  std::snprintf(line, sizeof(line), "%s created %u built %u mean_sum %.17g %.17g flag %d refused %lu\n", tag, created, built, sx, sy,
                f.built ? 1 : 0, f.updatesRefused());
  log += line;
}

void note_pose(std::string& log, const char* tag, const Vector3d& p) {
  char line[160];
  std::snprintf(line, sizeof(line), "%s %.17g %.17g %.17g\n", tag, p.x(), p.y(), p.z());
  log += line;
}

using Frame = std::unique_ptr<NDTFrame>;
Frame scan_frame() { return Frame(new NDTFrame(Vector3d::Zero(), 60, 60, 60, false)); }

std::string drive(bool batch) {
  std::string log;
  std::srand(5);
  constexpr int R = 3;
  std::vector<Frame> ref, cur;
  for (int r = 0; r < R; ++r) ref.emplace_back(new NDTFrame(Vector3d::Zero(), 60, 60, r == 1 ? 0.25 : 0.5, true));
  std::vector<Vector3d> pose((size_t)R, Vector3d::Zero());
  auto load = [&](std::vector<NDTLoadRequest> reqs) {
    if (batch) {
      NDTFrame::loadLaserBatch(reqs.data(), reqs.size());
    } else {
      for (NDTLoadRequest& q : reqs) q.frame->loadLaser(*q.laser_data, q.min_angle, q.angle_increment, q.max_range);
    }
  };
  auto update = [&](std::vector<NDTUpdateRequest> reqs) {
    if (batch) {
      NDTFrame::updateBatch(reqs.data(), reqs.size());
    } else {
      for (NDTUpdateRequest& q : reqs) q.frame->update(q.trans, q.new_frame);
    }
  };
  auto load_req = [&](NDTFrame* f, size_t s) { return NDTLoadRequest{f, &g_scans[s % g_scans.size()], g_amin, g_ainc, g_rmax}; };

  // ---- batchable requests: the live sequence of three robots, four steps -------------------------------------------------
  for (int k = 0; k < 4; ++k) {
    cur.clear();
    for (int r = 0; r < R; ++r) cur.push_back(scan_frame());
    load({load_req(cur[0].get(), (size_t)k), load_req(cur[1].get(), (size_t)k + 1), load_req(cur[2].get(), (size_t)k + 2)});
    if (k > 0)
      for (int r = 0; r < R; ++r) pose[(size_t)r] = ref[(size_t)r]->align(pose[(size_t)r], cur[(size_t)r].get());
    update({{ref[0].get(), pose[0], cur[0].get()}, {ref[1].get(), pose[1], cur[1].get()}, {ref[2].get(), pose[2], cur[2].get()}});
  }
  for (int r = 0; r < R; ++r) note_pose(log, "pose after the live steps", pose[(size_t)r]);
  for (int r = 0; r < R; ++r) note(log, "map after the live steps", *ref[(size_t)r]);

  // ---- a second load into a frame, and one frame twice in a call -------------------------------------------------------
  cur.clear();
  for (int r = 0; r < R; ++r) cur.push_back(scan_frame());
  cur[1]->setTrans(Vector3d(0.2, -0.1, 0.02));
  load({load_req(cur[0].get(), 0), load_req(cur[1].get(), 1), load_req(cur[2].get(), 2), load_req(cur[1].get(), 3)});
  for (int r = 0; r < R; ++r) note(log, "scan frame", *cur[(size_t)r]);
  // ---- a map twice in one call; a frame that owns a map as the "scan" (its points travel through the host) ---------------------
  NDTFrame owner(Vector3d::Zero(), 60, 60, 0.5, true);
  owner.loadLaser(g_scans[4 % g_scans.size()], g_amin, g_ainc, g_rmax);
  update({{ref[0].get(), Vector3d(0.1, 0.0, 0.01), cur[0].get()},
          {ref[1].get(), Vector3d(0.0, 0.1, -0.01), cur[1].get()},
          {ref[0].get(), Vector3d(-0.1, 0.05, 0.02), cur[2].get()},
          {ref[2].get(), Vector3d(0.05, 0.05, 0.0), &owner},
          {ref[1].get(), Vector3d(0.02, 0.0, 0.0), cur[0].get()}});
  for (int r = 0; r < R; ++r) note(log, "map after repeats", *ref[(size_t)r]);

  // ---- a frame of another thread's context -----------------------------------------------------------------------------------
  Frame far = scan_frame();
  Frame far2 = scan_frame();
  std::thread([&] {
    far->loadLaser(g_scans[5 % g_scans.size()], g_amin, g_ainc, g_rmax);
    far2->loadLaser(g_scans[0], g_amin, g_ainc, g_rmax);  // (bound to that thread's context; loaded again below from this one)
  }).join();
  cur.clear();
  for (int r = 0; r < R; ++r) cur.push_back(scan_frame());
  load({load_req(cur[0].get(), 1), load_req(far2.get(), 2), load_req(cur[1].get(), 3), load_req(cur[2].get(), 4)});
  update({{ref[0].get(), Vector3d(0.0, 0.0, 0.0), cur[0].get()},
          {ref[1].get(), Vector3d(0.1, 0.1, 0.0), far.get()},
          {ref[2].get(), Vector3d(0.0, -0.1, 0.0), cur[2].get()},
          {ref[0].get(), Vector3d(0.03, 0.0, 0.0), far2.get()}});
  for (int r = 0; r < R; ++r) note(log, "map after a foreign frame", *ref[(size_t)r]);

  // ---- requests that follow a failed align: refused, counted, recorded ---------------------------------------------------
  PSOConfig bad;
  bad.populationSize = 0;  // refused by the device library before anything is enqueued
  const unsigned long errors_before = ndtpso_slam_error_count();
  const Vector3d unrefined = ref[1]->optimize(Vector3d(0.3, 0.2, 0.1), cur[1].get(), Vector3d(.1, .1, 3.1415E-3), bad);
  note_pose(log, "failed align returns its guess", unrefined);
  update({{ref[0].get(), pose[0], cur[0].get()}, {ref[1].get(), pose[1], cur[1].get()}, {ref[2].get(), pose[2], cur[2].get()}});
  char line[96];
  std::snprintf(line, sizeof(line), "errors recorded %lu\n", ndtpso_slam_error_count() - errors_before);
  log += line;
  for (int r = 0; r < R; ++r) note(log, "map after refused updates", *ref[(size_t)r]);
  for (int r = 0; r < R; ++r) {  // the next successful align clears the condition
    pose[(size_t)r] = ref[(size_t)r]->align(pose[(size_t)r], cur[(size_t)r].get());
    note_pose(log, "align after all that", pose[(size_t)r]);
  }
  update({{ref[0].get(), pose[0], cur[0].get()}, {ref[1].get(), pose[1], cur[1].get()}, {ref[2].get(), pose[2], cur[2].get()}});
  for (int r = 0; r < R; ++r) note(log, "map at the end", *ref[(size_t)r]);
  return log;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n_scans = 0, n_beams = 0;
  if (std::fread(&n_scans, 4, 1, f) != 1 || std::fread(&n_beams, 4, 1, f) != 1 || std::fread(&g_amin, 4, 1, f) != 1 ||
      std::fread(&g_ainc, 4, 1, f) != 1 || std::fread(&g_rmax, 4, 1, f) != 1 || n_scans < 6)
    return 2;
  g_scans.assign((size_t)n_scans, std::vector<float>((size_t)n_beams));
  for (auto& s : g_scans)
    if (std::fread(s.data(), 4, (size_t)n_beams, f) != (size_t)n_beams) return 2;
  std::fclose(f);
  ndtpso_slam_device_init();
  const std::string batched = drive(true), calls = drive(false);
  if (batched != calls) {
    std::printf("MISMATCH\n---- batch entries ----\n%s---- member calls ----\n%s", batched.c_str(), calls.c_str());
    return 1;
  }
  std::fputs(batched.c_str(), stdout);
  std::printf("OK\n");
  return 0;
}
