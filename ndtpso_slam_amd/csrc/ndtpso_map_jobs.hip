// ndtpso_map_jobs.hip -- the scan loads and map updates of several single calls in one launch each (ndtpso_points_load_scans,
// ndtpso_map_update_batch): a fleet step's R x (k_scan_to_resident, k_map_insert, k_map_build, k_map_pack) become four
// launches.  Every kernel here is the single call's body (ndtpso_map_device.inc), run once per entry of a job table that lies in
// a pinned staging slot: the entry is wave-uniform and read once, ahead of the body's first store, so its fields sit in SGPRs as
// the single kernel's arguments do.  The maps of a launch are independent -- cells, windows, pool and header are per map -- so
// the workgroups of different jobs share nothing.  A translation unit of its own, as ndtpso_align_jobs.hip is.
#include "ndtpso_kernels.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "../../include/ndtpso_hip.h"

#include "ndtpso_device_common.inc"
#include "ndtpso_map_device.inc"
#include "ndtpso_map_jobs.h"

// workgroup j: k_scan_to_resident for job j
__global__ void __launch_bounds__(1024)
k_scans_to_resident_jobs(const ScanLoadJob* __restrict__ jobs) {
  const ScanLoadJob* __restrict__ job = jobs + blockIdx.x;
  const ScanP sp = job->sp;
  scan_to_resident_wg(job->ranges, sp, job->dirs, job->do_trans, job->tc, job->ts, job->ttx, job->tty, job->clip_hw, job->clip_hh,
                      job->out_xy, job->n_io, job->append, job->capacity);
}

// workgroup j: k_map_insert for job j (the same 1024 threads, the same static LDS, the same tile loop)
__global__ void __launch_bounds__(kInsertThreads)
k_map_insert_jobs(const MapUpdateJob* __restrict__ jobs) {
  const MapUpdateJob* __restrict__ job = jobs + blockIdx.x;
  const MapP m = job->m;
  map_insert_wg(m, job->pts, job->n, job->n_ptr, job->do_trans, job->tc, job->ts, job->ttx, job->tty);
}

// row j of the grid: k_map_build over job j's created cells, in the single launch's workgroups of 32 lanes (map_enqueue_cells
// says why 32).  The row is as long as the launch's largest job needs; the others' spare workgroups leave at once.
__global__ void __launch_bounds__(256)
k_map_build_jobs(const MapUpdateJob* __restrict__ jobs) {
  const MapUpdateJob* __restrict__ job = jobs + blockIdx.y;
  const MapP m = job->m;
  map_build_cell(m, job->undo, blockIdx.x * blockDim.x + threadIdx.x);
}

// workgroup j: k_map_pack for job j.  cap_words is the job's own, so a job assembles its bitmap in LDS or in the image exactly
// when its single call would, whatever LDS the launch was given for its largest job.
__global__ void __launch_bounds__(1024)
k_map_pack_jobs(const MapUpdateJob* __restrict__ jobs) {
  const MapUpdateJob* __restrict__ job = jobs + blockIdx.x;
  const MapP m = job->m;
  map_pack_wg(m, job->image, job->mirror, job->seq, job->cap_words);
}

hipError_t map_jobs_allow_big_lds() {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(k_map_pack_jobs), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
}

void scan_jobs_launch(hipStream_t stream, const void* jobs, unsigned n) {
  hipLaunchKernelGGL(k_scans_to_resident_jobs, dim3(n), dim3(1024), kCtrlBytes, stream, static_cast<const ScanLoadJob*>(jobs));
}

void map_insert_jobs_launch(hipStream_t stream, const void* jobs, unsigned n) {
  hipLaunchKernelGGL(k_map_insert_jobs, dim3(n), dim3(kInsertThreads), 0, stream, static_cast<const MapUpdateJob*>(jobs));
}

void map_build_jobs_launch(hipStream_t stream, const void* jobs, unsigned n, unsigned blocks_x) {
  hipLaunchKernelGGL(k_map_build_jobs, dim3(blocks_x, n), dim3(32), 0, stream, static_cast<const MapUpdateJob*>(jobs));
}

void map_pack_jobs_launch(hipStream_t stream, const void* jobs, unsigned n, int lds_bytes) {
  hipLaunchKernelGGL(k_map_pack_jobs, dim3(n), dim3(1024), lds_bytes, stream, static_cast<const MapUpdateJob*>(jobs));
}
