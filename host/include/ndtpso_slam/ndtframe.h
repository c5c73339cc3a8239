// NDTFrame of the MI355X build of libndtpso_slam.
//
// Source-compatible with the reference's include/ndtpso_slam/ndtframe.h:12-72 -- same constructor
// arguments, same public data members, same methods -- so ndtpso_slam_node.cpp (call sites :64-78, 110,
// 155, 167, 186, 194, 198, 202, 206, 229-230) builds against it unchanged.  The frame keeps the points
// and the window state; every number is produced on the GPU through the C-ABI in include/ndtpso_hip.h:
//   loadLaser -> ndtpso_scan_to_cells                               update -> ndtpso_points_to_cells
//   build     -> ndtpso_cells_build_windowed (+ ndtpso_occupancy_values) align  -> ndtpso_ref_set_cells + ndtpso_align
#ifndef NDTPSO_SLAM_AMD_NDTFRAME_H
#define NDTPSO_SLAM_AMD_NDTFRAME_H

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "ndtpso_slam/ndtcell.h"

using namespace Eigen;
using std::vector;

struct ndtpso_points;  // device-resident scan (include/ndtpso_hip.h)
struct ndtpso_map;     // device-resident map

// ndtpso_slam_device_init(): creates the process-wide device context now instead of at the first frame operation
// (optional).  Call it before srand() when the std::rand() stream must be reproducible: runtime start-up may itself
// call rand().  ndtpso_slam_last_error() / ndtpso_slam_error_count(): what a failed (skipped) device call left behind.
#include "ndtpso_slam/status.h"

namespace ndtpso_host {
struct Ctx;
}

class NDTFrame;
// One request of NDTFrame::alignBatch (not in the reference): pose = ref->align(guess, cur), ok = ref->lastAlignOk() after it.
struct NDTAlignRequest {
  NDTFrame* ref;
  const NDTFrame* cur;
  Vector3d guess;
  Vector3d pose;  // out
  bool ok;        // out
};

// What NDTFrame::relocalize returns (not in the reference): the refined pose of lowest cost and that cost, the lattice hits that
// were refined, and whether the device did it (false: `pose` is the lattice's origin, the error is recorded, status.h).
struct NDTRelocalizeResult {
  Vector3d pose;
  double cost;
  unsigned hits;
  bool ok;
};

// One request of NDTFrame::relocalizeBatch (not in the reference): result = ref->relocalize(cur, origin, step, count, top_k).
struct NDTRelocalizeRequest {
  NDTFrame* ref;
  const NDTFrame* cur;
  Vector3d origin, step;
  unsigned count[3];
  unsigned top_k;
  NDTRelocalizeResult result;  // out
};

// What NDTFrame::curvature returns (not in the reference): the score at a pose with its gradient and Hessian (xx, xy, xth, yy, yth,
// thth), the pose covariance they stand for -- the plain inverse Hessian, row-major: a relative measure, the caller owns the
// scale factor for their sensor's noise -- and the principal axes of its translational block.  definite: the Hessian is
// positive definite (else covariance and the xy fields are zeros: a saddle, no overlap, a NaN).  ok: the device did it (false:
// everything zero, the error is recorded, status.h).
struct NDTCurvature {
  double cost;
  Vector3d gradient;
  double hessian[6];
  double covariance[9];
  double xy_major, xy_minor, xy_angle;
  unsigned n_points, n_hit;
  bool definite, ok;
};

// One request of NDTFrame::curvatureBatch (not in the reference): result = ref->curvature(pose, cur).
struct NDTCurvatureRequest {
  NDTFrame* ref;
  const NDTFrame* cur;
  Vector3d pose;
  NDTCurvature result;  // out
};

// One request of NDTFrame::loadLaserBatch (not in the reference): frame->loadLaser(*laser_data, min_angle, angle_increment, max_range).
struct NDTLoadRequest {
  NDTFrame* frame;
  const vector<float>* laser_data;
  float min_angle, angle_increment, max_range;
};
// One request of NDTFrame::updateBatch (not in the reference): frame->update(trans, new_frame).
struct NDTUpdateRequest {
  NDTFrame* frame;
  Vector3d trans;
  NDTFrame* new_frame;
};

class NDTFrame {
 public:
  uint16_t width, height, widthNumOfCells, heightNumOfCells;
  vector<NDTCell> cells;
  bool built;
  unsigned int numOfCells;
  double cell_side;

  NDTFrame(Vector3d trans, unsigned short width = 20, unsigned short height = 20, double cell_side = 1.0,
           bool calculate_cells_params = true, NDTPSOConfig config = NDTPSOConfig()
#if BUILD_OCCUPANCY_GRID
               ,
           double occupancy_grid_cell_size = .0
#endif
  );

  ~NDTFrame();
  NDTFrame(const NDTFrame&) = delete;  // a frame owns device state (the reference's frames are never copied either)
  NDTFrame& operator=(const NDTFrame&) = delete;

  void loadLaser(const vector<float>& laser_data, const float& min_angle, const float& angle_increment,
                 const float& max_range);
  void update(Vector3d trans, NDTFrame* new_frame);
  void addPoint(Vector2d& point);
  inline void setTrans(Vector3d trans) { s_trans = std::move(trans); }
  void transform(Vector3d trans);
  void build();
  int getCellIndex(Vector2d point, int grid_width, double cell_side);
  Vector3d align(Vector3d initial_guess, const NDTFrame* const new_frame);
  void dumpMap(const char* filename, bool save_poses = true, bool save_points = true, bool save_image = true,
               short density = 50
#if BUILD_OCCUPANCY_GRID
               ,
               bool save_occupancy_grid = true
#endif
  );
  void addPose(double timestamp, const Vector3d& pose, const Vector3d& odom = Vector3d::Zero());
  void resetCells();

  // ---- additions of this build (not in the reference) ----
  // BASELINE.json's north star names an `addScan()`; the reference has no such method -- its ingest is loadLaser() into
  // a per-scan frame followed by update() of the map with that frame at the estimated pose (ndtpso_slam_node.cpp:186,
  // 194-198).  addScan() is that pair in one call: the scan, taken at `pose` in this frame's coordinates, is merged
  // into this frame.  Equivalent to { NDTFrame f(Vector3d::Zero(), width, height, max(width, height), false, config());
  // f.loadLaser(...); update(pose, &f); } -- same points, same order, same bits.
  void addScan(const Vector3d& pose, const vector<float>& laser_data, const float& min_angle, const float& angle_increment,
               const float& max_range);
  // Several align() calls at once: observably identical to reqs[i].pose = reqs[i].ref->align(reqs[i].guess, reqs[i].cur) for
  // i = 0 .. n - 1 in that order -- the same deviation rule per frame, the same PSOConfig, the std::rand() stream drawn in request
  // order, `built` / lastAlignOk() / the refusal of update() after a failure as those calls would leave them, a failed request
  // returning its guess -- but consecutive requests on DIFFERENT resident reference frames of the calling thread's device context,
  // with device-resident scans, share one launch (ndtpso_map_align_batch, include/ndtpso_hip.h): R robots served by one host
  // thread.  A reference frame that appears a second time closes the current launch (its deviation depends on the first
  // result), and so does a frame that one request aligns against and another aligns as scan; any other request takes align() itself, in its place.  The reference aligns one scan at a time
  // (ndtpso_slam_node.cpp:182-194).
  static void alignBatch(NDTAlignRequest* reqs, size_t n);
  // Where in this frame was `new_frame` taken, when no guess within align()'s +-0.1 m / +-3 mrad (ndtframe.cpp:253) is known: a
  // robot switched on inside a known map, a lost track, a loop closure.  The scan is scored at every node of the pose lattice
  // origin + (i, j, k) * step, i < count[0], j < count[1], k < count[2] (ndtpso_map_search, include/ndtpso_hip.h, in the
  // library's score mode); each of the best top_k nodes (1 .. 64), in hit order, is then refined by pso_optimization from the node
  // with a deviation of step / 2 per axis (on an axis of one node: align()'s first-call deviation on that axis), the configuration
  // align() would use and one table of the thread's rand() stream each, all in ONE launch (ndtpso_map_align_batch); the refined
  // pose of lowest cost is returned, ties to the earlier hit.  The frame then tracks from there as a fresh one would: the next
  // two align() calls use the first-call deviation.  On failure -- a frame that is not resident, a scan of another thread's
  // context, a device call that fails -- the result is {origin, 0, 0, false}, the error is recorded (ndtpso_slam/status.h), a
  // following update() is refused as after a failed align(), and the tracking state is untouched.  The rand() tables are drawn
  // once the hits are known, even if the refinement then fails (as optimize() draws).
  NDTRelocalizeResult relocalize(const NDTFrame* new_frame, const Vector3d& origin, const Vector3d& step, const unsigned count[3],
                                 unsigned top_k);
  // Several relocalize() calls at once -- the R robots one host thread serves, switched on together or lost together: observably
  // identical to reqs[i].result = reqs[i].ref->relocalize(reqs[i].cur, origin, step, count, top_k) for i = 0 .. n - 1 in that order
  // -- the results, the std::rand() stream (a request's tables are drawn in hit order, request by request; a request whose search
  // fails draws nothing), lastAlignOk(), the refusal of a following update() after a failure, the errors recorded (count, call
  // site, code; the text too where a request is refused for its own lattice or plan -- after a device failure inside a shared call
  // every request it failed carries that call's text) -- but consecutive
  // requests on DIFFERENT resident frames of the calling thread's device context share ONE lattice search call
  // (ndtpso_map_search_batch, include/ndtpso_hip.h) and ONE refinement launch over all hits of all of them
  // (ndtpso_map_align_batch).  A frame that appears a second time, as map or as scan, closes the run; a request that cannot be
  // batched (a null pointer, a frame that is not resident, a scan of another thread's context, frames' own PSOConfigs) is the
  // member call itself, in its place, so the stream order is kept.
  static void relocalizeBatch(NDTRelocalizeRequest* reqs, size_t n);
  // How well is `pose` constrained: cost_function (core.cpp:26-48) with normalDistribution (ndtcell.cpp:70-78) differentiated once
  // and twice by the pose, on the device in fp64 (ndtpso_map_curvature, include/ndtpso_hip.h), and the inverse Hessian as pose
  // covariance.  `pose` is in the convention align() returns and cost() takes; cost is cost(pose, new_frame) bit for bit.  The
  // conventions are cost()'s: a resident frame, the scan as a device-resident point list (a scan of another thread's context
  // goes through the host), the frame built first if need be -- `built` is the only state that changes.  It is an observer: it
  // draws nothing from std::rand() and leaves the tracking state, lastAlignOk() and the refusal of update() as they are.  On a
  // frame that is not resident, or when a device call fails, the result is all zeros with ok = false and the error is recorded
  // (ndtpso_slam/status.h); it never aborts.
  NDTCurvature curvature(const Vector3d& pose, const NDTFrame* new_frame);
  // Several curvature() calls at once: observably the member calls in request order, but consecutive requests on resident frames
  // of the calling thread's device context go out as ONE ndtpso_map_curvature_batch.  Maps and scans may repeat freely (nothing
  // depends on an earlier result); a request that cannot join takes the member call, in its place.
  static void curvatureBatch(NDTCurvatureRequest* reqs, size_t n);
  // Free space (not in the reference, whose occupancy grid knows occupied and nothing else): every beam of new_frame's scan,
  // taken at `pose` (the convention of align()'s result and update()'s argument), is walked from the sensor to its end point
  // through this frame's occupancy grid on the device (ndtpso_map_trace, include/ndtpso_hip.h); the cells it crosses count as
  // seen through, its last cell as hit.  Only enqueued, as update() is.  An observer: it draws nothing from std::rand(), leaves
  // the tracking state, `built`, lastAlignOk() and a pending speculative build as they are, and no later align / cost / update
  // changes by a bit.  Refused, with the error recorded (ndtpso_slam/status.h) as save() records its refusals: a frame that is
  // not resident (NDTPSO_RESIDENT=0, 2^21 cells or more), a one-cell per-scan frame, a frame without an occupancy grid or
  // with one that is not square.
  void traceFreeSpace(const Vector3d& pose, const NDTFrame* new_frame);
  // update(trans, new_frame) then also traces the same scan at `trans`: one more launch on the same stream.  updateBatch traces
  // the flagged frames of a shared run through ONE ndtpso_map_trace_batch behind the shared update launches (so a run's trace
  // errors, if any, are recorded behind ALL its update errors, where the member calls would record update k, trace k, update k + 1:
  // the count is the same, the last error may be another).
  void setTraceOnUpdate(bool on) { s_trace_on_update = on; }
  bool traceOnUpdate() const { return s_trace_on_update; }
  // The three-state grid a planner wants, as nav_msgs/OccupancyGrid counts: -1 unknown, 0 .. 100 occupied, og[x + height * y] as
  // occupancyGrid() stores it -- the reference's value where that is > 0, else the share of the beams that ended in the cell
  // (0: only ever seen through).  Formed on the device (ndtpso_map_get_nav_grid); settles the frame as occupancyGrid() does.
  // false, with the error recorded, where traceFreeSpace() refuses.
  bool navGrid(std::vector<int8_t>& grid, unsigned& og_width, unsigned& og_height);
  // the raw counters behind it, addressed alike (ndtpso_map_get_trace): beams that ended in the cell, beams that went through
  bool traceCounts(std::vector<uint32_t>& hits, std::vector<uint64_t>& passes);
  // Several loadLaser() / update() calls at once: observably identical to the member calls in request order -- `built`, the
  // refusal of an update() after a failed align() with its count (updatesRefused()) and recorded error, the rule for the
  // speculative build, every error recorded as the member call records it -- but consecutive requests that qualify share their
  // launches (ndtpso_points_load_scans, ndtpso_map_update_batch, include/ndtpso_hip.h): one launch for the R scan loads of a
  // fleet step, three for its R map updates.  A request qualifies when its frame is resident and lives in the calling thread's
  // device context and, for a load, is a one-cell per-scan frame without a map and with room in its scan buffer; for an update,
  // when the new frame is such a device-resident point list.  A frame that appears a second time in a run -- or as map in one
  // request and as scan in another -- closes the run; every other request is the member call itself, in its place.
  static void loadLaserBatch(NDTLoadRequest* reqs, size_t n);
  static void updateBatch(NDTUpdateRequest* reqs, size_t n);
  // A map outlives its process (not in the reference, whose dumpMap writes a plot nothing reads back).  save() writes this frame
  // to `path`: the device map's snapshot (ndtpso_map_snapshot, include/ndtpso_hip.h: cells, sliding windows, stored points,
  // occupancy grid -- everything later results depend on) followed by one section of host state with its own length and
  // checksum: s_trans, the tracking state align() goes by (previous pose, pose difference, alignments counted, so a loaded
  // frame's next align() uses the deviation the original's would have used), the frame's NDTPSOConfig, the pose / odometry /
  // timestamp lists of addPose(), the four extents, `built` and lastAlignOk().  A pending speculative build is put back first,
  // as by every export; the frame goes on afterwards as if it had not been saved.  The file is written as `path`.tmp and renamed.
  // load() makes a new frame from such a file in the CALLING thread's device context (the caller deletes it): every later
  // loadLaser / align / update / relocalize / build / dumpMap on it gives, bit for bit, what it would have given on the original.
  // The std::rand() stream is the caller's and is not saved: a process that wants the random numbers the original would have
  // drawn next seeds for them itself (srand(), ndtpso_slam_thread_srand()).
  // Only resident frames that are maps can be saved: with NDTPSO_RESIDENT=0, on a one-cell per-scan frame (a point list, no map)
  // and on a frame of 2^21 cells or more (kept on the host's side of the C-ABI, see the constructor) save() returns false and
  // records the error (ndtpso_slam/status.h); load() returns nullptr and records the error when the file cannot be read, fails
  // a check (magic, version, constants, counts, checksums of either part) or the device refuses it.  Nothing is left allocated.
  bool save(const char* path) const;
  static NDTFrame* load(const char* path);
  // the pose the frame tracks from: what its last align() or relocalize() returned (zero before the first) -- where a loaded
  // frame's caller takes up the sequence
  Vector3d lastPose() const { return s_prev_pose; }
  // new-frame points in the order cost_function visits them (cells, then insertion; core.cpp:33-36)
  void collectPoints(std::vector<double>& xy) const;
  const NDTPSOConfig& config() const { return s_config; }
  // Resident mode (default; NDTPSO_RESIDENT=0 turns it off): the points, the sliding windows, the occupancy grid and
  // the alignment table of this frame live on the GPU and `cells` is not maintained while the frame is used.
  // syncHostView() refreshes created / built / mean of every cell from the device.
  bool resident() const { return s_resident; }
  void syncHostView();
#if BUILD_OCCUPANCY_GRID
  // the occupancy grid as the reference stores it (og[x + height * y]) and its extent {min_x, max_x, min_y, max_y}
  const vector<int8_t>& occupancyGrid(uint32_t* og_width = nullptr, uint32_t* og_height = nullptr,
                                      uint32_t extent[4] = nullptr) const;
#endif
  // false when the last align() / pso_optimization against this frame could not run on the device and returned its
  // initial guess unrefined (the reference's API has no error channel; see also ndtpso_slam/status.h).  A caller that
  // is about to update() the map with that pose can look first.
  bool lastAlignOk() const { return s_last_align_ok; }
  // pso_optimization against this frame (used by align() and by the free function in core.h)
  Vector3d optimize(const Vector3d& guess, const NDTFrame* new_frame, const Vector3d& deviation, const PSOConfig& cfg);
  double cost(const Vector3d& trans, const NDTFrame* new_frame);

 private:
  Vector3d s_trans{Vector3d::Zero()}, s_prev_pose{Vector3d::Zero()}, s_pose_diff{Vector3d::Zero()};
  vector<Vector3d> s_poses, s_odoms;
  vector<double> s_timestamps;
  double s_x_min, s_x_max, s_y_min, s_y_max;
  NDTPSOConfig s_config;
  int s_iter{0};
#if BUILD_OCCUPANCY_GRID
  mutable struct {  // reference: s_occupancy_grid, ndtframe.h:22-29
    uint32_t count{0}, width{0}, height{0}, max_x_ind{0}, max_y_ind{0}, min_x_ind{UINT32_MAX}, min_y_ind{UINT32_MAX};
    double cell_size{0.};
    vector<int8_t> og;
  } s_occupancy_grid;
  void rasteriseOccupancy();
  void fetchOccupancy() const;  // resident mode: device -> s_occupancy_grid
#endif
  std::vector<uint32_t> s_created;  // indices of created cells, in creation order
  bool s_table_dirty{true};         // the device reference table must be re-uploaded before the next align
  bool s_last_align_ok{true};
  bool s_trace_on_update{false};
  const char* traceRefusal() const;        // why this frame cannot be traced (not resident, a one-cell scan frame), or nullptr
  ndtpso_map* traceMap(const char* what);  // the map traceFreeSpace / navGrid work on, or nullptr with the refusal recorded
  void append(const double* xy, const int32_t* idx, uint32_t n);
  bool uploadTable();  // false: the device refused the table (error recorded, see status.h)
  // what align() does around its alignment, step by step (alignBatch does the same steps around a shared launch)
  Vector3d nextDeviation();                 // the search range of this frame's next alignment; counts it
  void recordAlignOutcome(bool ok);         // built, lastAlignOk(), the refusal of update() after a failure
  Vector3d recordAlignedPose(Vector3d pose);  // the pose align() returns; s_pose_diff / s_prev_pose follow it
  struct DeviceScan;  // a new frame's points as an ndtpso_points (ndtframe.cpp)
  // resident mode
  bool s_resident{false};
  ndtpso_points* d_scan_{nullptr};  // a one-cell frame that only ever had scans loaded: its point list
  ndtpso_map* d_map_{nullptr};      // everything else
  uint32_t d_scan_upper_{0};        // upper bound of the points in d_scan_
  uint32_t d_scan_cap_{0};
  ndtpso_map* ensureMap();
  void residentPoints(bool slot0_only, std::vector<double>& xy) const;
  // the device context this frame lives in: the calling thread's at the frame's first device operation, then for good
  // (host/src/device.h: one context per host thread; every device-touching member locks and uses this one)
  mutable ndtpso_host::Ctx* s_dev{nullptr};
  ndtpso_host::Ctx* dev() const;
  unsigned long s_updates_refused{0};

 public:
  // update() calls refused because the frame's last align() had failed on the device (see update()); not in the reference
  unsigned long updatesRefused() const { return s_updates_refused; }
};

#endif
