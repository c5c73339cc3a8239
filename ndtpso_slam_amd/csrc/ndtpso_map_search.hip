// ndtpso_map_search.hip -- the kernels of ndtpso_map_search: cost_function (core.cpp:26-48) at every node of a pose lattice
// against a resident map, and the best K nodes picked on the device.  A translation unit of its own, as the job kernels are:
// nothing the kernels of the existing entries are compiled from changes.
//
// The sweep is k_cost_batch (same staging, same trips, one wave per pose, same lane accumulators and wave sum) with the lattice's
// structure taken out of the loop: a workgroup takes one heading at a time, computes its sincos once, turns the whole scan once
// into LDS -- fl(fl(x c) - fl(y s)), fl(fl(x s) + fl(y c)), the reference's own intermediate values (core.h:28-31) -- and its waves
// then walk the translations of that heading: per point and node the transform is two additions (the trips' PREROT form).  In
// the fp64 score every term is the cost kernel's bit for bit.  Node poses come from the descriptor (LatticeP), wave-uniform.
#include "ndtpso_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "../../include/ndtpso_hip.h"

#include "ndtpso_device_common.inc"
#include "ndtpso_map_search.h"

template <int MODE, int PATH>
__global__ void __launch_bounds__(1024)
k_lattice_sweep(SweepArgs a) {
  double2* pts = reinterpret_cast<double2*>(g_lds + a.L.pts_off);
  stage_image<MODE, PATH>(a.image, a.g, a.wn, a.L, a.dn);
  const EvalCtx E = PATH >= 4 ? make_eval_ctx_global(a.g, a.wn, a.dn, a.image) : make_eval_ctx(a.g, a.wn, a.L, a.dn);
  const LatticeP lat = a.lat;
  const int n = a.n, n_pad = round_up(n, kPointPad);
  const uint32_t n_waves = blockDim.x >> 6, nxy = lat.nx * lat.ny;
  for (uint32_t item = blockIdx.x; item < lat.n_items; item += gridDim.x) {
    const uint32_t k = item / lat.slabs, slab = item - k * lat.slabs;
    const double th = lat.oth + (double)k * lat.sth;
    double sn, cn;
    sincos(th, &sn, &cn);
    __syncthreads();  // the staging above, or the previous item's last read of the points
    for (int i = threadIdx.x; i < n_pad; i += blockDim.x) {
      // (the padding is pad_points_wg's sentinel, turned like a point: what the cost kernel's trips make of it)
      const double2 p = i < n ? a.xy[i] : make_double2(1e6, 1e6);
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
      if (lane_id() == 0) a.costs[(size_t)k * nxy + q] = cost;
    }
  }
}

// Workgroup b: the best k keys of its part [b * per_wg, (b + 1) * per_wg) of the input, in order, into out[b * k ...]: k rounds of
// "the smallest key behind the last one taken".  KEYS: the input is a list of keys (the merge of the first stage's lists), else
// costs[] with the position as index.
template <bool KEYS>
__global__ void __launch_bounds__(kSelectThreads)
k_lattice_select(const double* __restrict__ costs, const SearchKey* __restrict__ keys, uint32_t n, uint32_t per_wg, uint32_t k,
                 SearchKey* __restrict__ out) {
  __shared__ double s_cost[kSelectThreads / 64];
  __shared__ uint32_t s_index[kSelectThreads / 64], s_ok[kSelectThreads / 64];
  __shared__ SearchKey s_best;
  const uint32_t lo = blockIdx.x * per_wg, hi = min(n, lo + per_wg);
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
        const SearchKey q = keys[e];
        if (!q.valid) continue;
        c = q.cost;
        i = q.index;
      } else {
        c = costs[e];
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
      out[(size_t)blockIdx.x * k + r] = b;
    }
    __syncthreads();
    const SearchKey b = s_best;
    if (!b.valid) {  // (uniform) the part is exhausted: the rest of the list is empty
      if (threadIdx.x == 0)
        for (uint32_t rr = r + 1; rr < k; ++rr) out[(size_t)blockIdx.x * k + rr] = SearchKey{0., 0u, 0u};
      return;
    }
    last_c = b.cost;
    last_i = b.index;
    have_last = true;
  }
}

// the exact mode's candidates: every node whose fp32 cost is at most `thresh`, and how many costs are NaN
__global__ void __launch_bounds__(256)
k_lattice_collect(const double* __restrict__ costs, uint32_t n, double thresh, uint32_t cap, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double c = costs[i];
  if (c != c) {
    atomicAdd(out + 1, 1u);
  } else if (c <= thresh) {
    const uint32_t at = atomicAdd(out, 1u);
    if (at < cap) out[2 + at] = i;
  }
}

hipError_t search_sweep_launch(int mode, int path, unsigned grid, int lds_bytes, hipStream_t stream, const void* args) {
  const SweepArgs& a = *static_cast<const SweepArgs*>(args);
  hipError_t e = hipSuccess;
#define NDTPSO_SWEEP(MODE, PATH)                                                                                                  \
  do {                                                                                                                            \
    /* (per launch: the attribute is the current device's, and a search is no per-scan call) */                                  \
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_lattice_sweep<MODE, PATH>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                            kMaxLds);                                                                                             \
    if (e == hipSuccess) hipLaunchKernelGGL((k_lattice_sweep<MODE, PATH>), dim3(grid), dim3(1024), lds_bytes, stream, a);         \
  } while (0)
  if (mode == kScoreF32) {
    switch (path) {
      case 2: NDTPSO_SWEEP(kScoreF32, 2); break;
      case 1: NDTPSO_SWEEP(kScoreF32, 1); break;
      case 4: NDTPSO_SWEEP(kScoreF32, 4); break;
      case 5: NDTPSO_SWEEP(kScoreF32, 5); break;
      default: NDTPSO_SWEEP(kScoreF32, 0);
    }
  } else {
    switch (path) {
      case 1: NDTPSO_SWEEP(kScoreF64, 1); break;
      case 4: NDTPSO_SWEEP(kScoreF64, 4); break;
      case 5: NDTPSO_SWEEP(kScoreF64, 5); break;
      default: NDTPSO_SWEEP(kScoreF64, 0);
    }
  }
#undef NDTPSO_SWEEP
  return e != hipSuccess ? e : hipGetLastError();
}

hipError_t search_select_launch(hipStream_t stream, const double* costs, uint32_t n, uint32_t k, uint32_t lists, uint32_t per_wg,
                                void* partial, void* out) {
  hipLaunchKernelGGL((k_lattice_select<false>), dim3(lists), dim3(kSelectThreads), 0, stream, costs, (const SearchKey*)nullptr, n,
                     per_wg, k, static_cast<SearchKey*>(partial));
  hipLaunchKernelGGL((k_lattice_select<true>), dim3(1), dim3(kSelectThreads), 0, stream, (const double*)nullptr,
                     static_cast<const SearchKey*>(partial), lists * k, lists * k, k, static_cast<SearchKey*>(out));
  return hipGetLastError();
}

hipError_t search_collect_launch(hipStream_t stream, const double* costs, uint32_t n, double thresh, uint32_t cap, uint32_t* out) {
  hipLaunchKernelGGL(k_lattice_collect, dim3((n + 255) / 256), dim3(256), 0, stream, costs, n, thresh, cap, out);
  return hipGetLastError();
}
