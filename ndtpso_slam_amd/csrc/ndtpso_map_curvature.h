// ndtpso_map_curvature.h -- the kernel's side of ndtpso_map_curvature / ndtpso_map_curvature_batch (ndtpso_map_curvature.inc): the
// descriptor of one job of a launch and the host function through which the rest of the library reaches the kernel, which is a
// translation unit of its own (ndtpso_map_curvature.hip) for the reason ndtpso_map_search.hip is one: nothing the kernels of the
// existing entries are compiled from changes.  Included behind ndtpso_device_common.inc (Layout) by both units.
#ifndef NDTPSO_MAP_CURVATURE_H
#define NDTPSO_MAP_CURVATURE_H

// What the kernel writes per pose: ndtpso_curvature (include/ndtpso_hip.h), field for field.
struct alignas(16) CurvatureOut {
  double cost, gradient[3], hessian[6];
  uint32_t n_points, n_hit, path, reserved;
};
static_assert(sizeof(CurvatureOut) == sizeof(ndtpso_curvature), "the kernel writes ndtpso_curvature records");

// One job of a launch: a map's table, a scan, a list of poses (device memory, three doubles each) and where their records go.
// The host writes a table of these into a pinned staging block; the kernel reads its entry in place, with wave-uniform loads.
// A launch has `n_shares` SHARES, dealt as ndtpso_map_search_jobs.h describes: a job owns `share` consecutive ones from `share0`
// on, share s of a job takes the poses s * 8 + w, (s + share) * 8 + w, ... for wave w of its eight; workgroup b takes the shares
// b, b + grid, ...  A workgroup stages a job's table and scan once per share.
struct alignas(16) CurvatureJob {
  const unsigned char* image;
  const double2* xy;
  const double* poses;
  CurvatureOut* out;
  ndtpso::GridP g;
  ndtpso::WinP wn;
  Layout L;
  ndtpso::DenseP dn;
  int n;
  uint32_t n_poses, share0, share;
};
static_assert(sizeof(CurvatureJob) % 16 == 0, "job descriptors are read with wide uniform loads");

constexpr unsigned kCurvatureThreads = 512;  // (eight waves: see k_curvature_jobs)

// path: the fp64 plan's (Plan::path: 0, 1, 4, 5).  `jobs`: CurvatureJob[] of that plan, `share_job`: the job of every share; both
// readable by the device.  lds_bytes: the largest job's.
__attribute__((visibility("hidden"))) hipError_t curvature_jobs_launch(int path, unsigned grid, int lds_bytes, hipStream_t stream,
                                                                       const void* jobs, const uint32_t* share_job, uint32_t n_shares);

#endif
