// ndtpso_map_snapshot.hip -- the kernels of ndtpso_map_snapshot and ndtpso_map_restore: a resident map's primary state gathered
// into one contiguous blob in device memory, and scattered back into a freshly cleared map.  A translation unit of its own, as the
// job and search kernels are: nothing the kernels of the existing entries are compiled from changes.
//
// A wave takes one created cell.  Its 100 window slots are looked at by the lanes in two passes (slots 0-63, 64-99); a slot is in
// the blob if anything about it differs from what map_clear leaves (a length, a window count, any bit of the window sum or
// covariance).  Where things go is decided by prefix sums in the blob's fixed order -- created order, slot order, chain order --
// never by an atomic whose outcome depends on scheduling: the same map state gives the same bytes.  (The one atomic here adds
// integers into a total, which has one value whatever the order.)
// A slot's points are a chain of 512-byte chunks (ndtpso_map_device.inc): the walk is a sequence of dependent loads, as in
// k_map_build, so each half wave walks its own chains -- even slots the lower half, odd slots the upper -- and copies a chunk with
// one 16-byte load per lane while the link to the next chunk is already in flight.
#include "ndtpso_kernels.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "../../include/ndtpso_hip.h"

#include "ndtpso_device_common.inc"
#include "ndtpso_map_device.inc"
#include "ndtpso_map_snapshot.h"

namespace {

constexpr int kSnapWaves = 4;  // cells per workgroup
constexpr int kSnapThreads = kSnapWaves * kWave;

__device__ __forceinline__ bool snap_mask_bit(const uint32_t mask[4], int s) { return (mask[s >> 5] >> (s & 31)) & 1u; }

__device__ __forceinline__ int snap_rank(const uint32_t mask[4], int s) {  // used slots of the cell before slot s
  int r = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    if (w < (s >> 5)) r += __popc(mask[w]);
    if (w == (s >> 5)) r += __popc(mask[w] & ((1u << (s & 31)) - 1u));
  }
  return r;
}

__device__ __forceinline__ unsigned wave_inclusive_sum(unsigned v) {
  const int lane = lane_id();
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const unsigned t = (unsigned)__shfl_up((int)v, d, kWave);
    if (lane >= d) v += t;
  }
  return v;
}

__device__ __forceinline__ int chunks_of(int len) { return len > 0 ? (len + kChunk - 1) / kChunk : 0; }

// does slot `slot` hold anything map_clear does not leave?  (bits, not values: a -0. in a window sum is state)
__device__ __forceinline__ bool slot_used(const MapP& m, size_t slot, int len) {
  const unsigned long long* s = reinterpret_cast<const unsigned long long*>(m.win_sum + slot);
  const unsigned long long* c = reinterpret_cast<const unsigned long long*>(m.win_cov + slot);
  return len != 0 || m.win_count[slot] != 0 || (s[0] | s[1] | c[0] | c[1] | c[2] | c[3]) != 0ull;
}

// entry i of the occupancy box <-> its place in the map's key array (the reference's og[x + height * y], which k_map_occupancy
// keeps); a place beyond the array (the write the reference makes out of bounds and k_map_occupancy drops) holds nothing
__device__ __forceinline__ size_t og_place(const SnapOgP& og, size_t i) {
  const size_t r = i / og.w, c = i - r * og.w;
  return ((size_t)og.x0 + c) + (size_t)og.og_height * ((size_t)og.y0 + r);
}

}  // namespace

// ---- count: per created cell the used-slot mask, the number of used slots and the number of chunks -----------------------------
__global__ void __launch_bounds__(kSnapThreads)
k_snapshot_count(MapP m, unsigned n_created, SnapCellIndex* __restrict__ index, unsigned long long* __restrict__ totals) {
  const unsigned t = blockIdx.x * kSnapWaves + wave_id();
  if (t >= n_created) return;  // (wave-uniform)
  const int lane = lane_id();
  const int ci = m.created[t];
  uint32_t mask[4];
  unsigned n_chunks = 0, n_points = 0;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int s = pass * kWave + lane;
    bool used = false;
    if (s < kWinSlots) {
      const size_t slot = (size_t)ci * kWinSlots + s;
      const int len = m.slot_len[slot];
      used = slot_used(m, slot, len);
      n_chunks += (unsigned)chunks_of(len);
      n_points += (unsigned)max(len, 0);
    }
    const unsigned long long b = __ballot(used);
    mask[2 * pass] = (uint32_t)b;
    mask[2 * pass + 1] = (uint32_t)(b >> 32);
  }
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) {
    n_chunks += (unsigned)__shfl_xor((int)n_chunks, d, kWave);
    n_points += (unsigned)__shfl_xor((int)n_points, d, kWave);
  }
  if (lane == 0) {
    SnapCellIndex ix;
#pragma unroll
    for (int w = 0; w < 4; ++w) ix.mask[w] = mask[w];
    ix.slot_base = (unsigned long long)(__popc(mask[0]) + __popc(mask[1]) + __popc(mask[2]) + __popc(mask[3]));
    ix.chunk_base = n_chunks;
    index[t] = ix;
    atomicAdd(&totals[2], (unsigned long long)n_points);
  }
}

// ---- offsets: the exclusive scan of the two counts over the created list, one workgroup, tile after tile with a carry ------------
// (a frame has fewer than 2^21 cells: at most 2048 tiles.  A tile's sums fit 32 bits -- 1024 cells of at most 100 slots, and the
// pool holds fewer than 2^31 chunks --, the carry is 64 bits wide.)
__global__ void __launch_bounds__(1024)
k_snapshot_scan(unsigned n_created, SnapCellIndex* __restrict__ index, unsigned long long* __restrict__ totals) {
  __shared__ unsigned s_slots[1024 / kWave], s_chunks[1024 / kWave];
  __shared__ unsigned long long s_carry[2];
  const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
  if (tid == 0) s_carry[0] = s_carry[1] = 0ull;
  __syncthreads();
  for (unsigned base = 0; base < n_created; base += 1024) {
    const unsigned i = base + (unsigned)tid;
    const bool live = i < n_created;
    const unsigned a = live ? (unsigned)index[i].slot_base : 0u, b = live ? (unsigned)index[i].chunk_base : 0u;
    const unsigned ia = wave_inclusive_sum(a), ib = wave_inclusive_sum(b);
    if (lane == kWave - 1) {
      s_slots[wave] = ia;
      s_chunks[wave] = ib;
    }
    __syncthreads();
    unsigned wa = 0, wb = 0;
    for (int w = 0; w < wave; ++w) {
      wa += s_slots[w];
      wb += s_chunks[w];
    }
    const unsigned long long ca = s_carry[0], cb = s_carry[1];
    if (live) {
      index[i].slot_base = ca + wa + (ia - a);
      index[i].chunk_base = cb + wb + (ib - b);
    }
    __syncthreads();  // every thread has read the carry and the waves' sums
    if (tid == 1023) {
      s_carry[0] = ca + wa + ia;
      s_carry[1] = cb + wb + ib;
    }
    __syncthreads();
  }
  if (tid == 0) {
    totals[0] = s_carry[0];
    totals[1] = s_carry[1];
  }
}

// ---- gather: map -> blob ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSnapThreads)
k_snapshot_gather(MapP m, unsigned n_created, const SnapCellIndex* __restrict__ index, SnapBlobP b, SnapOgP og) {
  __shared__ int s_head[kSnapWaves][kWinSlots], s_len[kSnapWaves][kWinSlots];
  __shared__ unsigned s_first[kSnapWaves][kWinSlots];  // a slot's first chunk, counted from the cell's chunk_base
  const int lane = lane_id(), w = wave_id();
  const unsigned t = blockIdx.x * kSnapWaves + w;
  const bool live = t < n_created;  // (wave-uniform)
  SnapCellIndex ix{};
  if (live) {
    const int ci = m.created[t];
    ix = index[t];
    if (lane == 0) {
      b.created[t] = ci;
      b.index[t] = ix;
    }
    if (lane < (int)(sizeof(MapCell) / 16))
      reinterpret_cast<uint4*>(b.cells + t)[lane] = reinterpret_cast<const uint4*>(m.cell + ci)[lane];
    unsigned run = 0;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int s = pass * kWave + lane;
      const bool used = s < kWinSlots && snap_mask_bit(ix.mask, s);
      int len = 0, head = -1;
      if (used) {
        const size_t slot = (size_t)ci * kWinSlots + s, k = (size_t)ix.slot_base + (size_t)snap_rank(ix.mask, s);
        len = m.slot_len[slot];
        head = m.slot_head[slot];
        b.win_sum[k] = m.win_sum[slot];
        b.win_cov[k] = m.win_cov[slot];
        b.win_count[k] = m.win_count[slot];
        b.slot_len[k] = len;
      }
      const unsigned nch = (unsigned)chunks_of(len), incl = wave_inclusive_sum(nch);
      if (s < kWinSlots) {
        s_head[w][s] = head;
        s_len[w][s] = len;
        s_first[w][s] = run + (incl - nch);
      }
      run += (unsigned)__shfl((int)incl, kWave - 1, kWave);
    }
  }
  __syncthreads();
  if (live) {
    const int half = lane >> 5, l = lane & (kChunk - 1);
    static_assert(kChunk * 2 == kWave, "a half wave copies a chunk");
    for (int s = half; s < kWinSlots; s += 2) {
      int left = s_len[w][s];
      if (left <= 0) continue;
      const size_t out = (size_t)ix.chunk_base + s_first[w][s];
      const int n = chunks_of(left);
      int ch = s_head[w][s];
      for (int k = 0; k < n && (unsigned)ch < (unsigned)m.pool_chunks; ++k) {
        const int nx = m.chunk_next[ch];  // in flight together with the chunk's points
        double2 v = m.chunk_pts[(size_t)ch * kChunk + l];
        if (l >= left) v = make_double2(0., 0.);  // what lies behind a chain's last point is no state
        b.chunks[(out + (size_t)k) * kChunk + l] = v;
        left -= kChunk;
        ch = nx;
      }
    }
  }
  // the occupancy keys of the box.  k_map_occupancy widens the box (atomicMin / atomicMax on the header) in the same thread that
  // writes a key, so no key outside the box was ever written: what map_clear left there is all there is.
  const size_t n_og = (size_t)og.w * og.h, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_og; i += stride) {
    const size_t at = og_place(og, i);
    b.og[i] = at < og.og_count ? og.og_key[at] : 0ull;
  }
}

// ---- scatter: blob -> a map that map_clear has just left --------------------------------------------------------------------------
// Slots the blob does not hold keep map_clear's values (0 for the counts, -1 for heads and tails).  Chunks are numbered as the
// blob stores them: the cell's chunk_base plus the slot's place, consecutive along a chain, -1 behind its last one.
__global__ void __launch_bounds__(kSnapThreads)
k_restore_scatter(MapP m, unsigned n_created, SnapBlobP b, SnapOgP og) {
  __shared__ int s_len[kSnapWaves][kWinSlots];
  __shared__ unsigned s_first[kSnapWaves][kWinSlots];
  const int lane = lane_id(), w = wave_id();
  const unsigned t = blockIdx.x * kSnapWaves + w;
  const bool live = t < n_created;
  SnapCellIndex ix{};
  if (live) {
    const int ci = b.created[t];
    ix = b.index[t];
    if (lane == 0) m.created[t] = ci;
    if (lane < (int)(sizeof(MapCell) / 16))
      reinterpret_cast<uint4*>(m.cell + ci)[lane] = reinterpret_cast<const uint4*>(b.cells + t)[lane];
    unsigned run = 0;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int s = pass * kWave + lane;
      const bool used = s < kWinSlots && snap_mask_bit(ix.mask, s);
      int len = 0;
      size_t slot = 0;
      if (used) {
        const size_t k = (size_t)ix.slot_base + (size_t)snap_rank(ix.mask, s);
        slot = (size_t)ci * kWinSlots + s;
        len = b.slot_len[k];
        m.win_sum[slot] = b.win_sum[k];
        m.win_cov[slot] = b.win_cov[k];
        m.win_count[slot] = b.win_count[k];
        m.slot_len[slot] = len;
      }
      const unsigned nch = (unsigned)chunks_of(len), incl = wave_inclusive_sum(nch), first = run + (incl - nch);
      if (used && nch) {
        m.slot_head[slot] = (int)((unsigned)ix.chunk_base + first);
        m.slot_tail[slot] = (int)((unsigned)ix.chunk_base + first + nch - 1u);
      }
      if (s < kWinSlots) {
        s_len[w][s] = len;
        s_first[w][s] = first;
      }
      run += (unsigned)__shfl((int)incl, kWave - 1, kWave);
    }
  }
  __syncthreads();
  if (live) {
    const int half = lane >> 5, l = lane & (kChunk - 1);
    for (int s = half; s < kWinSlots; s += 2) {
      const int n = chunks_of(s_len[w][s]);
      const size_t first = (size_t)ix.chunk_base + s_first[w][s];
      for (int k = 0; k < n; ++k) {
        const size_t id = first + (size_t)k;
        m.chunk_pts[id * kChunk + l] = b.chunks[id * kChunk + l];
        if (l == 0) m.chunk_next[id] = k + 1 < n ? (int)id + 1 : -1;
      }
    }
  }
  const size_t n_og = (size_t)og.w * og.h, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_og; i += stride) {
    const size_t at = og_place(og, i);
    if (at < og.og_count) og.og_key[at] = b.og[i];
  }
}

namespace {
unsigned snap_blocks(unsigned n_created) { return (n_created + kSnapWaves - 1) / kSnapWaves; }
}  // namespace

void snapshot_count_launch(hipStream_t stream, const void* map_p, unsigned n_created, SnapCellIndex* index, unsigned long long* totals) {
  hipLaunchKernelGGL(k_snapshot_count, dim3(snap_blocks(n_created)), dim3(kSnapThreads), 0, stream, *static_cast<const MapP*>(map_p), n_created, index, totals);
}

void snapshot_scan_launch(hipStream_t stream, unsigned n_created, SnapCellIndex* index, unsigned long long* totals) {
  hipLaunchKernelGGL(k_snapshot_scan, dim3(1), dim3(1024), 0, stream, n_created, index, totals);
}

void snapshot_gather_launch(hipStream_t stream, const void* map_p, unsigned n_created, const SnapCellIndex* index, const SnapBlobP& blob,
                            const SnapOgP& og) {
  hipLaunchKernelGGL(k_snapshot_gather, dim3(snap_blocks(n_created)), dim3(kSnapThreads), 0, stream, *static_cast<const MapP*>(map_p), n_created, index, blob, og);
}

void restore_scatter_launch(hipStream_t stream, const void* map_p, unsigned n_created, const SnapBlobP& blob, const SnapOgP& og) {
  hipLaunchKernelGGL(k_restore_scatter, dim3(snap_blocks(n_created)), dim3(kSnapThreads), 0, stream, *static_cast<const MapP*>(map_p), n_created, blob, og);
}
