// ndtpso_map_search_jobs.hip -- the kernels of ndtpso_map_search_batch: the lattices of several ndtpso_map_search calls in shared
// launches.  A translation unit of its own, as ndtpso_align_jobs.hip is: nothing the kernels of the existing entries are compiled
// from changes.
//
// Every kernel here is its single twin with its inputs in a table: k_lattice_sweep_jobs walks the items of k_lattice_sweep
// (ndtpso_map_search.hip) -- one heading, a slab of its translations, one wave per node with the same trips, lane accumulators and
// wave sum, so a node's cost is the single sweep's bit for bit whichever workgroup scores it --, k_lattice_select_jobs keeps
// k_lattice_select's order (search_key_less), k_lattice_collect_jobs forms the threshold the host forms, and k_lattice_cost_jobs
// is k_cost_batch's fp64 score (ndtpso_hip.hip) over the collected nodes.
#include "ndtpso_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "../../include/ndtpso_hip.h"

#include "ndtpso_device_common.inc"
#include "ndtpso_map_search.h"
#include "ndtpso_map_search_jobs.h"

template <int MODE, int PATH>
__global__ void __launch_bounds__(1024)
k_lattice_sweep_jobs(const SweepJob* __restrict__ jobs, const uint32_t* __restrict__ share_job, uint32_t n_shares) {
  const uint32_t n_waves = blockDim.x >> 6;
  bool staged = false;
  for (uint32_t s = blockIdx.x; s < n_shares; s += gridDim.x) {
    // the descriptor is wave-uniform: uniform loads into SGPRs, as k_align_jobs reads its own
    const SweepJob* __restrict__ job = jobs + share_job[s];
    const uint32_t first_item = s - job->share0, item_step = job->share;
    const LatticeP lat = job->lat;
    if (first_item >= lat.n_items) continue;  // (uniform)
    const unsigned char* __restrict__ image = job->image;
    const double2* __restrict__ xy = job->xy;
    double* __restrict__ costs = job->costs;
    const GridP g = job->g;
    const WinP wn = job->wn;
    const Layout L = job->L;
    const DenseP dn = job->dn;
    const int n = job->n, n_pad = round_up(n, kPointPad);
    const uint32_t nxy = lat.nx * lat.ny;
    double2* pts = reinterpret_cast<double2*>(g_lds + L.pts_off);
    if (staged) __syncthreads();  // the previous share's last reads of its table and points
    staged = true;
    stage_image<MODE, PATH>(image, g, wn, L, dn);
    const EvalCtx E = PATH >= 4 ? make_eval_ctx_global(g, wn, dn, image) : make_eval_ctx(g, wn, L, dn);
    for (uint32_t item = first_item; item < lat.n_items; item += item_step) {
      const uint32_t k = item / lat.slabs, slab = item - k * lat.slabs;
      const double th = lat.oth + (double)k * lat.sth;
      double sn, cn;
      sincos(th, &sn, &cn);
      __syncthreads();  // the staging above, or the previous item's last read of the points
      for (int i = threadIdx.x; i < n_pad; i += blockDim.x) {
        // (the padding is pad_points_wg's sentinel, turned like a point: what the cost kernel's trips make of it)
        const double2 p = i < n ? xy[i] : make_double2(1e6, 1e6);
        pts[i] = make_double2(p.x * cn - p.y * sn, p.x * sn + p.y * cn);
      }
      __syncthreads();
      const uint32_t first = slab * lat.slab, last = min(first + lat.slab, nxy);
      for (uint32_t q = first + (uint32_t)wave_id(); q < last; q += n_waves) {
        const uint32_t j = q / lat.nx, i = q - j * lat.nx;
        const double tx = uniform_f64(lat.ox + (double)i * lat.sx), ty = uniform_f64(lat.oy + (double)j * lat.sy);
        double cost;
        if constexpr (PATH == 2)
          cost = eval_pose_wave_dense<false, false, false, true>(E.g, E.dn, E.lds0, pts, n, 1., 0., tx, ty, nullptr);
        else
          cost = eval_pose_wave_t<MODE, (PATH & 3) == 1, false, false, true>(E.g, E.wn, E.T, pts, n, 1., 0., tx, ty, nullptr);
        if (lane_id() == 0) costs[(size_t)k * nxy + q] = cost;
      }
    }
  }
}

// The exact mode's rescoring: k_cost_batch's fp64 score (ndtpso_hip.hip: the scan staged as it is, one wave per pose, the same
// function with the same arguments -- so a cost is ndtpso_map_cost's bit for bit) with its inputs in the table, over the nodes
// that k_lattice_collect_jobs listed in this call: node cand[e] into out[e] = {cost, node}, the pose from the descriptor
// (origin + (double)i * step: one multiplication, one addition).  Share s of a job takes the candidates s, s + share, ... wave by
// wave.  A list that the host will not use (a NaN cost counted, more candidates than cand_cap) is skipped.
constexpr unsigned kCostJobsThreads = 512;  // (eight waves: with sixteen the division forms spill 32 bytes a lane, and candidates are few)
template <int PATH>
__global__ void __launch_bounds__(kCostJobsThreads)
k_lattice_cost_jobs(const SweepJob* __restrict__ jobs, const uint32_t* __restrict__ share_job, uint32_t n_shares) {
  const uint32_t n_waves = blockDim.x >> 6;
  bool staged = false;
  for (uint32_t s = blockIdx.x; s < n_shares; s += gridDim.x) {
    const SweepJob* __restrict__ job = jobs + share_job[s];
    const uint32_t* __restrict__ hdr = job->cand_hdr;
    const uint32_t n_cand = (uint32_t)__builtin_amdgcn_readfirstlane((int)hdr[0]);
    const uint32_t n_nan = (uint32_t)__builtin_amdgcn_readfirstlane((int)hdr[1]);
    const uint32_t first = (s - job->share0) * n_waves, step = job->share * n_waves;
    if (n_nan != 0 || n_cand > job->cand_cap || first >= n_cand) continue;  // (uniform)
    const uint32_t* __restrict__ cand = job->cand;
    SearchKey* __restrict__ out = job->out;
    const LatticeP lat = job->lat;
    const unsigned char* __restrict__ image = job->image;
    const double2* __restrict__ xy = job->xy;
    const GridP g = job->g;
    const WinP wn = job->wn;
    const Layout L = job->L;
    const DenseP dn = job->dn;
    const int n = job->n;
    const uint32_t nxy = lat.nx * lat.ny;
    double2* pts = reinterpret_cast<double2*>(g_lds + L.pts_off);
    if (staged) __syncthreads();  // the previous share's last reads of its table and points
    staged = true;
    stage_image<kScoreF64, PATH>(image, g, wn, L, dn);
    copy16(pts, xy, n * 16);
    pad_points_wg(pts, n);
    __syncthreads();
    const EvalCtx E = PATH >= 4 ? make_eval_ctx_global(g, wn, dn, image) : make_eval_ctx(g, wn, L, dn);
    for (uint32_t e = first + (uint32_t)wave_id(); e < n_cand; e += step) {
      const uint32_t node = (uint32_t)__builtin_amdgcn_readfirstlane((int)cand[e]);
      const uint32_t k = node / nxy, q = node - k * nxy, j = q / lat.nx, i = q - j * lat.nx;
      const double th = lat.oth + (double)k * lat.sth;
      double sn, cn;
      sincos(th, &sn, &cn);
      const double tx = lat.ox + (double)i * lat.sx, ty = lat.oy + (double)j * lat.sy;
      const double cost = eval_pose_wave_t<kScoreF64, (PATH & 3) == 1, false>(E.g, E.wn, E.T, pts, n, cn, sn, tx, ty, nullptr);
      if (lane_id() == 0) out[e] = SearchKey{cost, node, 1u};
    }
  }
}

// Workgroup b: the best k keys of part b, in order: k rounds of "the smallest key behind the last one taken" (k_lattice_select).
// KEYS: the part is a list of keys (the merge of a job's first-stage lists), else costs with the node's number as index.
template <bool KEYS>
__global__ void __launch_bounds__(kSelectThreads)
k_lattice_select_jobs(const double* __restrict__ costs, const SearchKey* keys, const SelectPart* __restrict__ parts, SearchKey* out) {
  __shared__ double s_cost[kSelectThreads / 64];
  __shared__ uint32_t s_index[kSelectThreads / 64], s_ok[kSelectThreads / 64];
  __shared__ SearchKey s_best;
  const SelectPart part = parts[blockIdx.x];
  const uint32_t lo = part.lo, hi = part.hi, k = part.k;
  const size_t src = part.src, dst = part.out;
  const uint32_t n_waves = blockDim.x >> 6;
  double last_c = 0.;
  uint32_t last_i = 0;
  bool have_last = false;
  for (uint32_t r = 0; r < k; ++r) {
    double bc = 0.;
    uint32_t bi = 0;
    bool ok = false;
    for (uint32_t e = lo + threadIdx.x; e < hi; e += blockDim.x) {
      double c;
      uint32_t i;
      if constexpr (KEYS) {
        const SearchKey q = keys[src + e];
        if (!q.valid) continue;
        c = q.cost;
        i = q.index;
      } else {
        c = costs[src + e];
        i = e;
      }
      if (have_last && !search_key_less(last_c, last_i, c, i)) continue;
      if (!ok || search_key_less(c, i, bc, bi)) {
        bc = c;
        bi = i;
        ok = true;
      }
    }
    for (int off = 32; off; off >>= 1) {
      const double oc = __shfl_xor(bc, off);
      const uint32_t oi = (uint32_t)__shfl_xor((int)bi, off);
      const bool ook = __shfl_xor((int)ok, off) != 0;
      if (ook && (!ok || search_key_less(oc, oi, bc, bi))) {
        bc = oc;
        bi = oi;
        ok = true;
      }
    }
    if (lane_id() == 0) {
      s_cost[wave_id()] = bc;
      s_index[wave_id()] = bi;
      s_ok[wave_id()] = ok ? 1u : 0u;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      SearchKey b{0., 0u, 0u};
      for (uint32_t w = 0; w < n_waves; ++w)
        if (s_ok[w] && (!b.valid || search_key_less(s_cost[w], s_index[w], b.cost, b.index))) b = SearchKey{s_cost[w], s_index[w], 1u};
      s_best = b;
      out[dst + r] = b;
    }
    __syncthreads();
    const SearchKey b = s_best;
    if (!b.valid) {  // (uniform) the part is exhausted: the rest of the list is empty
      if (threadIdx.x == 0)
        for (uint32_t rr = r + 1; rr < k; ++rr) out[dst + rr] = SearchKey{0., 0u, 0u};
      return;
    }
    last_c = b.cost;
    last_i = b.index;
    have_last = true;
  }
}

// The exact mode's candidates, part by part of the first selection stage: every node of the part whose fp32 cost is at most the
// job's threshold, and how many of its costs are NaN.  The threshold is the host's: one multiplication, one addition (this unit
// is compiled without contraction, like the host code) of the job's K-th key -- the second selection stage has written it.
__global__ void __launch_bounds__(256)
k_lattice_collect_jobs(const double* __restrict__ costs, const SearchKey* __restrict__ keys, const SelectPart* __restrict__ parts,
                       const CollectJob* __restrict__ jobs, uint32_t* __restrict__ cand) {
  const SelectPart part = parts[blockIdx.x];
  const CollectJob cj = jobs[part.job];
  const double c32_k = keys[cj.kth].cost;
  if (c32_k != c32_k || c32_k > -kTinyCost) return;  // (uniform) the host rules the job a fallback from the key itself
  const double slack = kArbAbsPerPoint * (double)cj.n_points;
  const double thresh = c32_k + slack;
  uint32_t* __restrict__ hdr = cand + cj.hdr;
  uint32_t* __restrict__ out = cand + cj.list;
  for (uint32_t e = part.lo + threadIdx.x; e < part.hi; e += blockDim.x) {
    const double c = costs[(size_t)part.src + e];
    if (c != c) {
      atomicAdd(hdr + 1, 1u);
    } else if (c <= thresh) {
      const uint32_t at = atomicAdd(hdr, 1u);
      if (at < cj.cap) out[at] = e;
    }
  }
}

hipError_t search_jobs_sweep_launch(int mode, int path, unsigned grid, int lds_bytes, hipStream_t stream, const void* jobs,
                                    const uint32_t* share_job, uint32_t n_shares) {
  const SweepJob* d_jobs = static_cast<const SweepJob*>(jobs);
  hipError_t e = hipSuccess;
#define NDTPSO_JOBS_KERNEL(THREADS, ...)                                                                                             \
  do {                                                                                                                       \
    /* (per launch, as the single sweep: the attribute is the current device's) */                                          \
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(__VA_ARGS__), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds); \
    if (e == hipSuccess) hipLaunchKernelGGL((__VA_ARGS__), dim3(grid), dim3(THREADS), lds_bytes, stream, d_jobs, share_job, n_shares); \
  } while (0)
  if (mode == kScoreF32) {
    switch (path) {
      case 2: NDTPSO_JOBS_KERNEL(1024, k_lattice_sweep_jobs<kScoreF32, 2>); break;
      case 1: NDTPSO_JOBS_KERNEL(1024, k_lattice_sweep_jobs<kScoreF32, 1>); break;
      case 4: NDTPSO_JOBS_KERNEL(1024, k_lattice_sweep_jobs<kScoreF32, 4>); break;
      case 5: NDTPSO_JOBS_KERNEL(1024, k_lattice_sweep_jobs<kScoreF32, 5>); break;
      default: NDTPSO_JOBS_KERNEL(1024, k_lattice_sweep_jobs<kScoreF32, 0>);
    }
  } else {
    switch (path) {
      case 1: NDTPSO_JOBS_KERNEL(1024, k_lattice_sweep_jobs<kScoreF64, 1>); break;
      case 4: NDTPSO_JOBS_KERNEL(1024, k_lattice_sweep_jobs<kScoreF64, 4>); break;
      case 5: NDTPSO_JOBS_KERNEL(1024, k_lattice_sweep_jobs<kScoreF64, 5>); break;
      default: NDTPSO_JOBS_KERNEL(1024, k_lattice_sweep_jobs<kScoreF64, 0>);
    }
  }
  return e != hipSuccess ? e : hipGetLastError();
}

hipError_t search_jobs_cost_launch(int path, unsigned grid, int lds_bytes, hipStream_t stream, const void* jobs, const uint32_t* share_job,
                                   uint32_t n_shares) {
  const SweepJob* d_jobs = static_cast<const SweepJob*>(jobs);
  hipError_t e = hipSuccess;
  switch (path) {
    case 1: NDTPSO_JOBS_KERNEL(kCostJobsThreads, k_lattice_cost_jobs<1>); break;
    case 4: NDTPSO_JOBS_KERNEL(kCostJobsThreads, k_lattice_cost_jobs<4>); break;
    case 5: NDTPSO_JOBS_KERNEL(kCostJobsThreads, k_lattice_cost_jobs<5>); break;
    default: NDTPSO_JOBS_KERNEL(kCostJobsThreads, k_lattice_cost_jobs<0>);
  }
#undef NDTPSO_JOBS_KERNEL
  return e != hipSuccess ? e : hipGetLastError();
}

hipError_t search_jobs_select_launch(hipStream_t stream, const double* costs, void* keys, const void* first, uint32_t n_first,
                                     const void* second, uint32_t n_second) {
  SearchKey* d_keys = static_cast<SearchKey*>(keys);
  hipLaunchKernelGGL((k_lattice_select_jobs<false>), dim3(n_first), dim3(kSelectThreads), 0, stream, costs, (const SearchKey*)nullptr,
                     static_cast<const SelectPart*>(first), d_keys);
  hipLaunchKernelGGL((k_lattice_select_jobs<true>), dim3(n_second), dim3(kSelectThreads), 0, stream, (const double*)nullptr,
                     (const SearchKey*)d_keys, static_cast<const SelectPart*>(second), d_keys);
  return hipGetLastError();
}

hipError_t search_jobs_collect_launch(hipStream_t stream, const double* costs, const void* keys, const void* parts, uint32_t n_parts,
                                      const void* jobs, uint32_t* cand) {
  hipLaunchKernelGGL(k_lattice_collect_jobs, dim3(n_parts), dim3(256), 0, stream, costs, static_cast<const SearchKey*>(keys),
                     static_cast<const SelectPart*>(parts), static_cast<const CollectJob*>(jobs), cand);
  return hipGetLastError();
}
