// ndtpso_map_search.h -- the kernels' side of ndtpso_map_search (ndtpso_map_search.inc): the arguments of a lattice sweep, the
// keys of the selection, and the host functions through which the rest of the library reaches the kernels, which are a
// translation unit of their own (ndtpso_map_search.hip), as the job kernels are and for the same reason: nothing the kernels of
// the existing entries are compiled from changes.  Included behind ndtpso_device_common.inc (Layout) by both units.
#ifndef NDTPSO_MAP_SEARCH_H
#define NDTPSO_MAP_SEARCH_H

// A pose lattice as the sweep walks it.  Node (i, j, k) is number (k * ny + j) * nx + i and lies at origin + (double)i * step per
// axis: one multiplication, one addition, no FMA (the library is compiled without contraction).  A workgroup takes ITEMS: one
// heading k and a slab of `slab` consecutive (i, j) translations of it; `slabs` items per heading.
struct LatticeP {
  double ox, oy, oth, sx, sy, sth;
  uint32_t nx, ny, nth;
  uint32_t slab, slabs, n_items;
};

// k_lattice_sweep's arguments (passed by value: wave-uniform, in SGPRs)
struct SweepArgs {
  const unsigned char* image;
  const double2* xy;
  double* costs;  // one per node, in device memory
  ndtpso::GridP g;
  ndtpso::WinP wn;
  Layout L;
  ndtpso::DenseP dn;
  LatticeP lat;
  int n;
};

// One entry of a best-K list: ascending cost, ties by ascending index, a NaN behind every number (search_key_less).
// valid == 0: the list had fewer entries.
struct alignas(16) SearchKey {
  double cost;
  uint32_t index, valid;
};

// The order of the hits: ascending cost by value (-0. and +0. tie), ties by ascending index, a NaN behind every number and NaNs
// among themselves by index.  A strict total order on (cost, index) for distinct indices, so the best K of a set are the best K
// of the union of its parts' best K, however the parts were cut.  One text for the single kernels and the job kernels.
__device__ __forceinline__ bool search_key_less(double a, uint32_t ai, double b, uint32_t bi) {
  const bool an = a != a, bn = b != b;
  if (an || bn) return an == bn ? ai < bi : bn;
  return a < b || (a == b && ai < bi);
}

constexpr uint32_t kSelectThreads = 1024;
constexpr uint32_t kSelectMinPerWg = 4096;   // nodes per workgroup of the first selection stage, at least
constexpr uint32_t kSelectMaxLists = 1024;   // ... and at most this many workgroups (lists the last stage merges)

// mode: kScoreF32 / kScoreF64; path: Plan::path (0, 1, 4, 5; fp32 also 2).  `args`: SweepArgs.
__attribute__((visibility("hidden"))) hipError_t search_sweep_launch(int mode, int path, unsigned grid, int lds_bytes, hipStream_t stream,
                                                                     const void* args);
// the best k of costs[0 .. n) into out[0 .. k): `lists` workgroups of `per_wg` nodes each into lists x k keys at `partial`, then one
// workgroup merges them.  The result does not depend on lists / per_wg.
__attribute__((visibility("hidden"))) hipError_t search_select_launch(hipStream_t stream, const double* costs, uint32_t n, uint32_t k,
                                                                      uint32_t lists, uint32_t per_wg, void* partial, void* out);
// EXACT: out[0] = number of nodes with cost <= thresh, out[1] = number of NaN costs, out[2 ..] = the first `cap` such nodes in
// no particular order.  out[0 .. 2) must be zero before the launch.
__attribute__((visibility("hidden"))) hipError_t search_collect_launch(hipStream_t stream, const double* costs, uint32_t n, double thresh,
                                                                       uint32_t cap, uint32_t* out);

#endif
