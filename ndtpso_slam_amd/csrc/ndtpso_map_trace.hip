// ndtpso_map_trace.hip -- the kernels of ndtpso_map_trace, ndtpso_map_trace_batch and ndtpso_map_get_nav_grid: every beam of a
// scan walked through the map's occupancy grid, the cells it crosses counted as seen through and its last cell as hit.  The
// reference has no counterpart (its grid knows occupied and nothing else).  A translation unit of its own, as the search and
// curvature kernels are: nothing the kernels of the existing entries are compiled from changes.
//
// The traversal is the one include/ndtpso_hip.h states: the cells are the staircase that merges the x-crossings
// tx_i = tx0 + (double)i * tdx and the y-crossings ty_j = ty0 + (double)j * tdy, x first on a tie.  The crossing times are closed
// forms of the ray, not running sums, so the order of the steps is a pure function of the ray.  One lane walks one ray:
// neighbouring beams end on the same wall, so the walks of a wave have similar lengths.  Every add is an integer atomic whose
// result is not used (no wait for a return), so the counters do not depend on the order of rays, jobs or launches.  The first
// cell of every ray of a job is the origin's: a workgroup counts its rays that go on from there and adds them with ONE atomic
// (AGG) instead of 256 on one address -- the same sum.  Totals and extent are gathered in LDS and leave with one atomic each
// per workgroup.  No workgroup waits for another.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ndtpso_map_trace.h"

namespace {

template <bool AGG>
__global__ void __launch_bounds__(kTraceThreads)
k_trace_jobs(const TraceJob* __restrict__ jobs) {
  const TraceJob* __restrict__ job = jobs + blockIdx.x;
  const uint32_t n = min(*job->n_ptr, job->n);
  if (blockIdx.y * kTraceThreads >= n) return;  // (uniform: a spare workgroup of a short job)
  __shared__ uint32_t s_cnt[4];                 // rays traced, rays skipped, steps, rays that leave the origin's cell
  __shared__ uint32_t s_ext[4];                 // min ox, max ox, min oy, max oy
  if (threadIdx.x < 4) {
    s_cnt[threadIdx.x] = 0u;
    s_ext[threadIdx.x] = (threadIdx.x & 1u) ? 0u : UINT32_MAX;
  }
  __syncthreads();

  const double hw = job->hw, hh = job->hh, cs = job->cs;
  const double ox = job->tx, oy = job->ty;
  const uint32_t H = job->og_height, count = job->og_count;
  uint32_t* __restrict__ hits = job->hits;
  unsigned long long* __restrict__ passes = job->passes;
  const bool origin_in = (int)(fabs(ox) < hw) & (int)(fabs(oy) < hh);
  const double fx0 = (ox + hw) / cs, fy0 = (oy + hh) / cs;
  const int ix = (int)floor(fx0), iy = (int)floor(fy0);

  const uint32_t r = blockIdx.y * kTraceThreads + threadIdx.x;
  if (r < n) {
    double sn, cn;
    sincos(job->theta, &sn, &cn);
    const double2 p = job->xy[r];
    // transform_point's rounding (core.h:28-31), no fused operation
    const double ex = __dadd_rn(__dadd_rn(__dmul_rn(p.x, cn), -__dmul_rn(p.y, sn)), ox);
    const double ey = __dadd_rn(__dadd_rn(__dmul_rn(p.x, sn), __dmul_rn(p.y, cn)), oy);
    const bool end_in = (int)(fabs(ex) < hw) & (int)(fabs(ey) < hh);
    if (!(origin_in && end_in)) {
      atomicAdd(&s_cnt[1], 1u);
    } else {
      const double fx1 = (ex + hw) / cs, fy1 = (ey + hh) / cs;
      const int jx = (int)floor(fx1), jy = (int)floor(fy1);
      const double dx = fx1 - fx0, dy = fy1 - fy0;
      const int sx = jx > ix ? 1 : -1, sy = jy > iy ? 1 : -1;
      const int nx = abs(jx - ix), ny = abs(jy - iy);
      const double tdx = nx ? 1. / fabs(dx) : 0.;
      const double tdy = ny ? 1. / fabs(dy) : 0.;
      const double tx0 = nx ? ((double)(sx > 0 ? ix + 1 : ix) - fx0) / dx : 0.;
      const double ty0 = ny ? ((double)(sy > 0 ? iy + 1 : iy) - fy0) / dy : 0.;
      atomicAdd(&s_cnt[0], 1u);
      atomicAdd(&s_cnt[2], (uint32_t)(nx + ny));
      atomicMin(&s_ext[0], (uint32_t)min(ix, jx));
      atomicMax(&s_ext[1], (uint32_t)max(ix, jx));
      atomicMin(&s_ext[2], (uint32_t)min(iy, jy));
      atomicMax(&s_ext[3], (uint32_t)max(iy, jy));
      int i = 0, j = 0, cx = ix, cy = iy;
      if (AGG && nx + ny > 0) atomicAdd(&s_cnt[3], 1u);
      while (i < nx || j < ny) {
        if (!(AGG && i + j == 0)) {
          const unsigned long long at = (unsigned long long)cx + (unsigned long long)H * (unsigned long long)cy;
          if (at < count) atomicAdd(&passes[at], 1ull);
        }
        bool step_x = j == ny;
        if (i < nx && j < ny) {
          const double tx = __dadd_rn(tx0, __dmul_rn((double)i, tdx));
          const double ty = __dadd_rn(ty0, __dmul_rn((double)j, tdy));
          step_x = tx <= ty;
        }
        if (step_x) {
          ++i;
          cx += sx;
        } else {
          ++j;
          cy += sy;
        }
      }
      const unsigned long long at = (unsigned long long)cx + (unsigned long long)H * (unsigned long long)cy;
      if (at < count) atomicAdd(&hits[at], 1u);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    TraceTotals* __restrict__ tot = job->tot;
    if (s_cnt[1]) atomicAdd(&tot->n_skipped, (unsigned long long)s_cnt[1]);
    if (s_cnt[0]) {
      atomicAdd(&tot->n_rays, (unsigned long long)s_cnt[0]);
      if (s_cnt[2]) atomicAdd(&tot->n_steps, (unsigned long long)s_cnt[2]);
      atomicMin(&tot->min_x, s_ext[0]);
      atomicMax(&tot->max_x, s_ext[1]);
      atomicMin(&tot->min_y, s_ext[2]);
      atomicMax(&tot->max_y, s_ext[3]);
      if (AGG && s_cnt[3]) {
        const unsigned long long at = (unsigned long long)ix + (unsigned long long)H * (unsigned long long)iy;
        if (at < count) atomicAdd(&passes[at], (unsigned long long)s_cnt[3]);
      }
    }
  }
}

// ndtpso_map_get_nav_grid's rule, one entry per thread
__global__ void __launch_bounds__(256)
k_nav_grid(const unsigned long long* __restrict__ og_key, const uint32_t* __restrict__ hits,
           const unsigned long long* __restrict__ passes, uint32_t og_count, int8_t* __restrict__ grid) {
  const uint32_t at = blockIdx.x * blockDim.x + threadIdx.x;
  if (at >= og_count) return;
  const int8_t v = (int8_t)(uint8_t)(og_key[at] & 0xffull);  // the byte ndtpso_map_get_occupancy returns
  int8_t out = v;
  if (!(v > 0)) {
    const unsigned long long h = hits ? (unsigned long long)hits[at] : 0ull, p = hits ? passes[at] : 0ull;
    out = h + p == 0ull ? (int8_t)-1 : (int8_t)((100ull * h + (h + p) / 2ull) / (h + p));
  }
  grid[at] = out;
}

}  // namespace

hipError_t trace_jobs_launch(hipStream_t stream, const void* jobs, unsigned n_jobs, unsigned blocks_y, int aggregate) {
  const dim3 grid(n_jobs, blocks_y), block(kTraceThreads);
  if (aggregate)
    hipLaunchKernelGGL(k_trace_jobs<true>, grid, block, 0, stream, static_cast<const TraceJob*>(jobs));
  else
    hipLaunchKernelGGL(k_trace_jobs<false>, grid, block, 0, stream, static_cast<const TraceJob*>(jobs));
  return hipGetLastError();
}

hipError_t nav_grid_launch(hipStream_t stream, const unsigned long long* og_key, const uint32_t* hits, const unsigned long long* passes,
                           uint32_t og_count, int8_t* grid) {
  hipLaunchKernelGGL(k_nav_grid, dim3((og_count + 255u) / 256u), dim3(256), 0, stream, og_key, hits, passes, og_count, grid);
  return hipGetLastError();
}
