// ndtpso_map_jobs.h -- the job kernels' side of ndtpso_points_load_scans and ndtpso_map_update_batch (ndtpso_map_update.inc):
// the descriptors of one job and the host functions through which the rest of the library reaches the four job kernels, which
// are a translation unit of their own (ndtpso_map_jobs.hip), as k_align_jobs is and for the same reason: nothing the kernels of
// the single calls are compiled from changes.  Included behind ndtpso_map_device.inc (MapP, MapUndo, MapHeader) by both units.
#ifndef NDTPSO_MAP_JOBS_H
#define NDTPSO_MAP_JOBS_H

// One scan load of a launch of several: k_scan_to_resident's kernel arguments.  The host writes a table of these into a pinned
// staging slot, and all the jobs' ranges behind it in the same slot; the kernel reads both in place.
struct alignas(16) ScanLoadJob {
  const float* ranges;
  const double2* dirs;
  double2* out_xy;
  uint32_t* n_io;
  double tc, ts, ttx, tty, clip_hw, clip_hh;
  ScanP sp;
  int do_trans, append, capacity;
};

// One map update of a launch of several: what k_map_insert takes, and for a job that builds afterwards what k_map_build and
// k_map_pack take (`undo`, `image`, `mirror`, `seq`, and the bitmap words the job's OWN single launch would have had LDS for).
struct alignas(16) MapUpdateJob {
  MapP m;
  const double2* pts;
  const uint32_t* n_ptr;
  MapUndo* undo;
  unsigned char* image;
  MapHeader* mirror;
  double tc, ts, ttx, tty;
  int n, do_trans, cap_words;
  uint32_t seq;
};

// `jobs`: a table of n descriptors, readable by the device.  build: `blocks_x` workgroups of 32 lanes per job, the largest
// job's count (a job with fewer created cells leaves through the body's own `t >= n_created`).  pack: `lds_bytes` is the
// largest job's.
__attribute__((visibility("hidden"))) hipError_t map_jobs_allow_big_lds();
__attribute__((visibility("hidden"))) void scan_jobs_launch(hipStream_t stream, const void* jobs, unsigned n);
__attribute__((visibility("hidden"))) void map_insert_jobs_launch(hipStream_t stream, const void* jobs, unsigned n);
__attribute__((visibility("hidden"))) void map_build_jobs_launch(hipStream_t stream, const void* jobs, unsigned n, unsigned blocks_x);
__attribute__((visibility("hidden"))) void map_pack_jobs_launch(hipStream_t stream, const void* jobs, unsigned n, int lds_bytes);

#endif
