// ndtpso_align_jobs.hip -- k_align_jobs: the alignments of several ndtpso_map_align calls in one launch (ndtpso_map_align_batch).
// A translation unit of its own: k_align_jobs<M, P, C, A> calls the very instantiations of pso_run_wg that its twin k_align<M, P, C, A>
// calls, and in one module the second caller moved the first one's code (two instructions of k_align<0, 2, false, true>: a
// sign extension the compiler could no longer fold) -- here nothing the existing kernels are compiled from changes.
#include "ndtpso_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "../../include/ndtpso_hip.h"

#include "ndtpso_device_common.inc"
#include "ndtpso_align_jobs.h"

// Job j of the launch by workgroup j (CLUSTER = false) or by cluster j of cl.K workgroups, placed as the fused pairs kernel
// places its clusters (ndtpso_pairs_body.inc).  The descriptor is wave-uniform and read once, before the kernel's first store:
// uniform loads into SGPRs, so the jobs' differing grids, windows and layouts cost the PSO's loop no VGPRs.  Then k_align's text.
template <int MODE, int PATH, bool CLUSTER, bool ARB = false>
__global__ void __launch_bounds__(CLUSTER ? kClusterMaxThreads : 1024)
k_align_jobs(const AlignJob* __restrict__ jobs, PsoP ps, ClusterP cl, int table_vec) {
  size_t j = blockIdx.x;
  if constexpr (CLUSTER) {
    if (!cluster_place(cl, &j, &cl.rank)) return;
    cl.xc += j * (2 * (size_t)cl.stride + (size_t)round_up(cl.K, 8));  // two slot buffers + the workgroups' heartbeats
  } else {
    cl.rank = 0;
  }
  const AlignJob* __restrict__ job = jobs + j;
  const unsigned char* __restrict__ image = job->image;
  const double2* __restrict__ xy = job->xy;
  int n = job->n;
  const uint32_t* __restrict__ n_ptr = job->n_ptr;
  GridP g = job->g;
  WinP wn = job->wn;
  const Layout L = job->L;
  DenseP dn = job->dn;
  const double* __restrict__ guess = job->guess;
  const double* __restrict__ dev = guess + 3;
  const uint32_t seed = job->seed;
  const int32_t* __restrict__ table = nullptr;  // (tables travel through the staging slot only)
  unsigned char* __restrict__ ws = nullptr;     // (swarms kept in HBM take the single path)
  double* __restrict__ out_pose = job->out;
  double* __restrict__ out_cost = job->want_cost ? out_pose + 3 : nullptr;
  AlignStats* __restrict__ stats = reinterpret_cast<AlignStats*>(out_pose + 4);
  double* __restrict__ mirror = job->mirror;
  const int4* __restrict__ table_src = job->table_src;
  int4* __restrict__ table_dst = job->table_dst;
  const uint32_t* __restrict__ late_hdr = job->late_hdr;
  const int late_table_cap = job->late_table_cap, late_rec_cap = job->late_rec_cap;
  const uint32_t seq = job->seq;
  if constexpr (CLUSTER) {
    cl.spec_off = job->spec_off;  // (behind the job's own layout)
    cl.spec = cl.spec_off >= 0 ? reinterpret_cast<double*>(g_lds + cl.spec_off) : nullptr;
  }
#include "ndtpso_align_body.inc"
}

hipError_t align_jobs_allow_big_lds() {
  hipError_t e = hipSuccess;
#define NDTPSO_JOBS_BIG(...)                                                                                    \
  if (e == hipSuccess)                                                                                          \
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_align_jobs<__VA_ARGS__>), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds)
  NDTPSO_JOBS_BIG(kScoreF32, 2, false, false);
  NDTPSO_JOBS_BIG(kScoreF32, 2, true, false);
  NDTPSO_JOBS_BIG(kScoreF32, 2, false, true);
  NDTPSO_JOBS_BIG(kScoreF32, 2, true, true);
  NDTPSO_JOBS_BIG(kScoreF64, 1, false, false);
  NDTPSO_JOBS_BIG(kScoreF64, 1, true, false);
#undef NDTPSO_JOBS_BIG
  return e;
}

void align_jobs_launch(int kind, bool cluster, unsigned grid, unsigned threads, int lds_bytes, hipStream_t stream, const void* jobs,
                       const PsoP& ps, const ClusterP& cl, int table_vec) {
  const AlignJob* d_jobs = static_cast<const AlignJob*>(jobs);
#define NDTPSO_JOBS_LAUNCH(...) \
  hipLaunchKernelGGL((k_align_jobs<__VA_ARGS__>), dim3(grid), dim3(threads), lds_bytes, stream, d_jobs, ps, cl, table_vec)
  if (kind == 0) {
    if (cluster) NDTPSO_JOBS_LAUNCH(kScoreF32, 2, true, false); else NDTPSO_JOBS_LAUNCH(kScoreF32, 2, false, false);
  } else if (kind == 1) {
    if (cluster) NDTPSO_JOBS_LAUNCH(kScoreF32, 2, true, true); else NDTPSO_JOBS_LAUNCH(kScoreF32, 2, false, true);
  } else {
    if (cluster) NDTPSO_JOBS_LAUNCH(kScoreF64, 1, true, false); else NDTPSO_JOBS_LAUNCH(kScoreF64, 1, false, false);
  }
#undef NDTPSO_JOBS_LAUNCH
}
