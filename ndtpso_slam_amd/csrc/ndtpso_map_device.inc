// ndtpso_map_device.inc -- the device side of the resident map (ndtpso_map.inc): its structures and the bodies of the four
// kernels of a live step -- scan -> resident points, insert, build, pack -- as __device__ functions.  Two translation units
// include it: ndtpso_hip.hip wraps each body in the kernel of the single calls (k_scan_to_resident, k_map_insert, k_map_build,
// k_map_pack), ndtpso_map_jobs.hip in the kernel that runs it once per job of a table (ndtpso_points_load_scans,
// ndtpso_map_update_batch).  The bit-for-bit rules -- insertion order inside a cell, the running-sum order, WINDOW_ADD, the
// eigenvalue form of the covariance inverse -- are stated here once.  Behind ndtpso_device_common.inc.

namespace {

constexpr int kWinSlots = NDTPSO_WINDOW_SIZE;          // NDT_WINDOW_SIZE, config.h:8
constexpr int kRotateAfter = NDTPSO_MAX_POINTS_PER_CELL;  // NDT_MAX_POINTS_PER_CELL, config.h:5
constexpr int kChunk = 32;                             // points per pool chunk (512 B)
constexpr int kInsertThreads = 1024, kInsertTile = 2048;  // the insert's workgroup; points one pass handles (two per thread)

constexpr int kCellCreated = 1, kCellBuilt = 2;
constexpr int kSpecSeqWord = 32;  // ndtpso_map::spec_hdr: the header, and at this 32-bit word the number of the build it belongs to
constexpr uint32_t kMapPoolExhausted = 1u, kMapOgOutside = 2u;

struct MapCell {
  double4 global_cov;  // s_global_covar_sum, row-major
  double4 icov;        // s_inv_covar, row-major
  double2 cur_sum;     // s_current_partial_sum
  double2 global_sum;  // s_global_sum
  double2 mean;
  int cur_count, cur_id, global_count, flags;
};
static_assert(sizeof(MapCell) == 128, "MapCell layout");

struct MapHeader {  // lives on the device; mirrored to the host when a decision needs it
  uint32_t n_created, n_built, status, n_words;
  int32_t x0, x1, y0, y1;                          // bounding box of the built cells (cell coordinates)
  uint32_t og_min_x, og_max_x, og_min_y, og_max_y;  // s_occupancy_grid.{min,max}_{x,y}_ind
  int32_t pool_bump, pool_free;
  unsigned long long n_points;                     // points ever inserted
};
static_assert(sizeof(MapHeader) == sizeof(ndtpso_map_info), "map info ABI");

struct MapP {
  GridP g;
  int n_cells, pool_chunks;
  MapCell* cell;
  double2* win_sum;
  double4* win_cov;
  int* win_count;
  int* slot_head;
  int* slot_tail;
  int* slot_len;
  double2* chunk_pts;
  int* chunk_next;
  int* free_list;
  int* created;
  MapHeader* hdr;
};

// ---- chunk pool ----------------------------------------------------------------------------------------------
// Within one kernel phase only pushes or only pops happen (a workgroup barrier separates them), so the free
// stack needs no ABA protection.
__device__ inline void pool_push(const MapP& m, int chunk) { m.free_list[atomicAdd(&m.hdr->pool_free, 1)] = chunk; }
__device__ inline int pool_pop(const MapP& m) {
  const int t = atomicSub(&m.hdr->pool_free, 1);
  if (t > 0) return m.free_list[t - 1];
  atomicAdd(&m.hdr->pool_free, 1);
  const int c = atomicAdd(&m.hdr->pool_bump, 1);
  if (c < m.pool_chunks) return c;
  atomicOr(&m.hdr->status, kMapPoolExhausted);
  return -1;
}

}  // namespace

// ---- insert: NDTFrame::update / loadLaser / addPoint into the resident map --------------------------------------
// One workgroup; points go through in tiles of 2048, in order, two per thread (a 1081-beam scan is one tile: a tile is
// a chain of five dependent round trips to memory whatever its size, and the second tile of 57 points cost as much as the
// first).  A tile is sorted by (cell, input position) in LDS (bitonic, the input position in the key keeps insertion
// order inside a cell), which turns every touched cell into a run: the run's head owns the cell (slot reset, running
// sum in input order, counters), every point knows its rank and writes itself into the slot's chunk chain in parallel,
// the first point of every new chunk allocates and links it.
// Insertion order inside a cell is the input order, as the reference's push_back gives it, and the running slot sum
// adds the points one after the other in that order, so the statistics are the reference's bit for bit.
// Thread t holds the sort positions 2t and 2t + 1: the network's last stage of every merge (partner distance 1) is a
// compare-exchange inside the thread, the others exchange both keys with thread t ^ (j / 2) -- by shuffle inside a wave,
// through LDS across waves.
__device__ inline int block_exclusive_max(int v, int* s_wave) {  // max of v over the threads before this one (0: none)
  const int lane = lane_id(), wave = wave_id(), n_waves = blockDim.x >> 6;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const int t = __shfl_up(v, d, kWave);
    if (lane >= d) v = max(v, t);
  }
  if (lane == kWave - 1) s_wave[wave] = v;
  int excl = __shfl_up(v, 1, kWave);
  if (lane == 0) excl = 0;
  __syncthreads();
  int carry = 0;
  for (int w = 0; w < n_waves; ++w)
    if (w < wave) carry = max(carry, s_wave[w]);
  __syncthreads();
  return max(excl, carry);
}

__device__ __forceinline__ void
map_insert_wg(const MapP& m, const double2* __restrict__ pts, int n, const uint32_t* __restrict__ n_ptr, int do_trans,
              double tc, double ts, double ttx, double tty) {
  __shared__ double2 s_p[kInsertTile];   // transformed points, input order
  __shared__ uint32_t s_sort[kInsertTile];
  __shared__ int s_total[kInsertTile];   // run length, stored at the run's start
  __shared__ int s_chunk[kInsertTile];   // chunk allocated by the point at this sorted position
  __shared__ int s_wave[kInsertThreads / kWave];
  constexpr uint32_t kInvalid = 0xFFFFFFFFu;
  constexpr uint32_t kPosMask = (uint32_t)kInsertTile - 1u;
  constexpr int kPosBits = 11;
  static_assert((1 << kPosBits) == kInsertTile, "sort key layout");
  if (n_ptr) n = min((int)*n_ptr, n);
  const int tid = threadIdx.x;
  const int e0 = 2 * tid;  // this thread's sort positions: e0, e0 + 1
#ifdef NDTPSO_PROFILE_INSERT
  unsigned long long it_[8]; int itn_ = 0;
#define IT_MARK() do { __syncthreads(); if (itn_ < 8) it_[itn_++] = wall_clock64(); } while (0)
#else
#define IT_MARK() do { } while (0)
#endif
  IT_MARK();
  for (int base = 0; base < n; base += kInsertTile) {
    const int cnt = min(kInsertTile, n - base);
    uint32_t key[2] = {kInvalid, kInvalid};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = e0 + h;  // input position inside the tile
      if (i < cnt) {
        double2 p = pts[base + i];
        if (do_trans) {  // transform_point, core.h:28-31
          const double x = p.x * tc - p.y * ts + ttx;
          const double y = p.x * ts + p.y * tc + tty;
          p.x = x;
          p.y = y;
        }
        int ix, iy;
        if (point_cell(m.g, p, ix, iy)) key[h] = ((uint32_t)(ix + m.g.W * iy) << kPosBits) | (uint32_t)i;
        s_p[i] = p;
      }
    }
    IT_MARK();
    int xstep = 0;
    int sort_n = 2 * kWave;  // the invalid keys of the unused tail sort last on their own: sort only the tile's extent
    while (sort_n < cnt) sort_n <<= 1;
    for (int k = 2; k <= sort_n; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        if (j == 1) {  // partner inside the thread
          const bool asc = (e0 & k) == 0;
          const uint32_t lo = min(key[0], key[1]), hi = max(key[0], key[1]);
          key[0] = asc ? lo : hi;
          key[1] = asc ? hi : lo;
          continue;
        }
        const int jj = j >> 1;  // partner thread distance
        uint32_t other[2];
        if (jj >= kWave) {  // across waves: through LDS, two buffers in turn (s_total and s_chunk are idle during the sort), so
                            // that one barrier per step is enough -- a buffer is written again two barriers after it was read
          uint32_t* xb = reinterpret_cast<uint32_t*>((xstep++ & 1) ? s_chunk : s_total);
          xb[e0] = key[0];
          xb[e0 + 1] = key[1];
          __syncthreads();
          other[0] = xb[2 * (tid ^ jj)];
          other[1] = xb[2 * (tid ^ jj) + 1];
        } else {
          other[0] = (uint32_t)__shfl_xor((int)key[0], jj, kWave);
          other[1] = (uint32_t)__shfl_xor((int)key[1], jj, kWave);
        }
        const bool keep_min = ((tid & jj) == 0) == ((e0 & k) == 0);  // lower index of an ascending run, or upper of a descending one
        key[0] = keep_min ? min(key[0], other[0]) : max(key[0], other[0]);
        key[1] = keep_min ? min(key[1], other[1]) : max(key[1], other[1]);
      }
    s_sort[e0] = key[0];
    s_sort[e0 + 1] = key[1];
    __syncthreads();
    IT_MARK();
    const uint32_t before0 = tid > 0 ? s_sort[e0 - 1] : kInvalid;
    const uint32_t after1 = e0 + 2 < kInsertTile ? s_sort[e0 + 2] : kInvalid;
    bool valid[2], is_head[2], is_tail[2];
    int cell[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint32_t before = h ? key[0] : before0, after = h ? after1 : key[1];
      valid[h] = key[h] != kInvalid;
      cell[h] = (int)(key[h] >> kPosBits);
      is_head[h] = valid[h] && ((e0 + h) == 0 || before == kInvalid || (int)(before >> kPosBits) != cell[h]);
      is_tail[h] = valid[h] && (after == kInvalid || (int)(after >> kPosBits) != cell[h]);
    }
    // start of the run each position belongs to: running maximum of the heads' positions
    const int hv0 = is_head[0] ? e0 : 0, hv1 = is_head[1] ? e0 + 1 : 0;
    const int carry = block_exclusive_max(max(hv0, hv1), s_wave);
    int start[2];
    start[0] = max(carry, hv0);
    start[1] = max(start[0], hv1);
    double2 p[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      p[h] = valid[h] ? s_p[key[h] & kPosMask] : make_double2(0., 0.);
      if (is_tail[h]) s_total[start[h]] = e0 + h - start[h] + 1;
    }
    __syncthreads();
    int total[2] = {0, 0}, slot[2] = {0, 0}, len0[2] = {0, 0}, tail0[2] = {-1, -1};
    bool reset[2] = {false, false};
    double2 head_sum[2];  // a run's head reads what it will update (running sum, count, flags) here, with the rest
    int head_count[2], head_flags[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      head_sum[h] = make_double2(0., 0.);
      head_count[h] = head_flags[h] = 0;
      if (!valid[h]) continue;
      total[h] = s_total[start[h]];
      const MapCell& c = m.cell[cell[h]];
      const int cur_id = c.cur_id;
      head_count[h] = c.cur_count;
      if (is_head[h]) {
        head_sum[h] = c.cur_sum;
        head_flags[h] = c.flags;
      }
      reset[h] = head_count[h] == 0;  // NDTCell::addPoint's slot reset, ndtcell.cpp:22-27
      slot[h] = cell[h] * kWinSlots + cur_id;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (!valid[h]) continue;
      if (!reset[h]) {
        len0[h] = m.slot_len[slot[h]];
        tail0[h] = m.slot_tail[slot[h]];
      } else if (is_head[h]) {  // the slot's old chunks go back to the pool
        for (int c = m.slot_head[slot[h]]; c >= 0;) {
          const int nx = m.chunk_next[c];
          pool_push(m, c);
          c = nx;
        }
        m.slot_head[slot[h]] = -1;
      }
    }
    __syncthreads();  // pushes before pops; every reader of slot_len / slot_tail before their update
    IT_MARK();
    int pos[2];
    bool leader[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      pos[h] = len0[h] + (e0 + h - start[h]);
      leader[h] = valid[h] && (pos[h] % kChunk) == 0;  // first point of a new chunk
      if (leader[h]) {
        const int ch = pool_pop(m);
        s_chunk[e0 + h] = ch;
        if (ch >= 0) m.chunk_next[ch] = -1;
      }
    }
    __syncthreads();
    IT_MARK();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (!valid[h]) continue;
      const int e = e0 + h;
      const bool in_old_tail = pos[h] - (pos[h] % kChunk) < len0[h];  // the partly filled chunk the slot already ends in
      const int ch = in_old_tail ? tail0[h] : s_chunk[e - (pos[h] % kChunk)];
      if (ch >= 0) m.chunk_pts[(size_t)ch * kChunk + (pos[h] % kChunk)] = p[h];
      if (leader[h] && ch >= 0) {
        if (pos[h] == 0) {
          m.slot_head[slot[h]] = ch;
        } else {
          const int prev = (pos[h] - kChunk >= len0[h]) ? s_chunk[e - kChunk] : tail0[h];
          if (prev >= 0) m.chunk_next[prev] = ch;
        }
      }
      if (is_tail[h]) {
        m.slot_tail[slot[h]] = ch;
        m.slot_len[slot[h]] = len0[h] + total[h];
      }
      if (is_head[h]) {  // (only this thread touches the cell's record during the insert)
        double2 sum = head_sum[h];
        for (int r = 0; r < total[h]; ++r) {  // s_current_partial_sum += point, ndtcell.cpp:30
          const double2 q = s_p[s_sort[start[h] + r] & kPosMask];
          sum.x += q.x;
          sum.y += q.y;
        }
        MapCell& c = m.cell[cell[h]];
        c.cur_sum = sum;
        c.cur_count = head_count[h] + total[h];
        if (!(head_flags[h] & kCellCreated)) m.created[atomicAdd(&m.hdr->n_created, 1u)] = cell[h];
        c.flags = (head_flags[h] | kCellCreated) & ~kCellBuilt;  // ndtcell.cpp:32-33
        atomicAdd(&m.hdr->n_points, (unsigned long long)total[h]);
      }
    }
    __syncthreads();
    IT_MARK();
#ifdef NDTPSO_PROFILE_INSERT
    if (tid == 0) printf("insert (us): load %.2f sort %.2f lookup %.2f pop %.2f write %.2f  n %d\n", (it_[1]-it_[0])*0.01, (it_[2]-it_[1])*0.01, (it_[3]-it_[2])*0.01, (it_[4]-it_[3])*0.01, (it_[5]-it_[4])*0.01, cnt);
#endif
  }
}

// ---- build: NDTCell::build on every created cell (ndtframe.cpp:73-77), one thread per cell ---------------------------
// undo != nullptr: a SPECULATIVE build (see ndtpso_map_speculate_build) -- everything the build overwrites is logged
// first, so that k_map_undo can put the map back as if the build had not happened yet.
struct MapUndo {
  MapCell cell;  // the cell before the build
  double4 win_cov;
  double2 win_sum;
  int win_count, slot;  // the window terms of the slot the build replaces
  int pad[2];
};
static_assert(sizeof(MapUndo) == 192, "MapUndo layout");

__device__ __forceinline__ void
map_build_cell(const MapP& m, MapUndo* __restrict__ undo, unsigned t) {  // t: the thread's place in the list of created cells
  if (t >= m.hdr->n_created) return;
  const int ci = m.created[t];
  MapCell c = m.cell[ci];
  const int slot = ci * kWinSlots + c.cur_id;
  if (undo) {
    MapUndo u;
    u.cell = c;
    u.win_cov = m.win_cov[slot];
    u.win_sum = m.win_sum[slot];
    u.win_count = m.win_count[slot];
    u.slot = slot;
    u.pad[0] = u.pad[1] = 0;
    undo[t] = u;
  }
  // WINDOW_ADD (ndtcell.h:13-15): global = (global + partial) - partials[idx]; partials[idx] = partial
  const double2 ws = m.win_sum[slot];
  c.global_sum.x = (c.global_sum.x + c.cur_sum.x) - ws.x;
  c.global_sum.y = (c.global_sum.y + c.cur_sum.y) - ws.y;
  m.win_sum[slot] = c.cur_sum;
  c.global_count = (c.global_count + c.cur_count) - m.win_count[slot];
  m.win_count[slot] = c.cur_count;
  if (c.global_count > 2) {
    const double mx = c.global_sum.x / (double)c.global_count;  // ndtcell.cpp:44
    const double my = c.global_sum.y / (double)c.global_count;
    double c00 = 0., c01 = 0., c10 = 0., c11 = 0.;
    int left = m.slot_len[slot];
    const double4 wc = m.win_cov[slot];  // ndtcell.cpp:54-55 (asked for ahead of the chain of loads below)
    for (int ch = m.slot_head[slot]; ch >= 0 && left > 0;) {  // ndtcell.cpp:49-52
      const int nx = m.chunk_next[ch];  // in flight together with the chunk's points
      const double2* p = m.chunk_pts + (size_t)ch * kChunk;
      const int k = min(left, kChunk);
      for (int i = 0; i < k; ++i) {
        const double d0 = p[i].x - mx, d1 = p[i].y - my;
        c00 += d0 * d0;
        c01 += d0 * d1;
        c10 += d1 * d0;
        c11 += d1 * d1;
      }
      left -= k;
      ch = nx;
    }
    c.global_cov.x = (c.global_cov.x + c00) - wc.x;
    c.global_cov.y = (c.global_cov.y + c01) - wc.y;
    c.global_cov.z = (c.global_cov.z + c10) - wc.z;
    c.global_cov.w = (c.global_cov.w + c11) - wc.w;
    m.win_cov[slot] = make_double4(c00, c01, c10, c11);
    // s_calc_covar_inverse, ndtcell.cpp:93-111 (eigenvalues as Eigen's EigenSolver computes them, as k_cells_build_windowed)
    const double nn = (double)c.global_count;
    const double v00 = c.global_cov.x / nn, v01 = c.global_cov.y / nn;
    const double v10 = c.global_cov.z / nn, v11 = c.global_cov.w / nn;
    double inv[4];
    covar_inverse_eigen(v00, v01, v10, v11, inv);
    c.mean = make_double2(mx, my);
    c.icov = make_double4(inv[0], inv[1], inv[2], inv[3]);
    c.flags |= kCellBuilt;
  }
  if (c.cur_count > kRotateAfter) {  // ndtcell.cpp:61-65
    c.cur_id = (c.cur_id + 1) % kWinSlots;
    c.cur_count = 0;
    c.cur_sum = make_double2(0., 0.);
  }
  m.cell[ci] = c;
}

// ---- pack: built cells -> the alignment table image (same layout ndtpso_ref_set_cells produces) ------------------
// One workgroup; the bitmap of the bounding box is assembled in LDS.
__device__ __forceinline__ void
map_pack_wg(const MapP& m, unsigned char* __restrict__ image, MapHeader* __restrict__ mirror, uint32_t seq, int cap_words) {
  int* box = lds_cnt(0);  // {min x, max x, min y, max y}
  uint2* bm = reinterpret_cast<uint2*>(g_lds + kCtrlBytes);
  const int tid = threadIdx.x;
  const int n_created = (int)m.hdr->n_created;
  MapHeader hdr0{};  // (thread 0: the header's other fields for the host's copy at the end, asked for now)
  if (tid == 0) {
    if (mirror) hdr0 = *m.hdr;
    box[0] = box[2] = INT_MAX;
    box[1] = box[3] = -1;
  }
  __syncthreads();
  {  // bounding box of the built cells: per thread, then per wave (64 lanes on one LDS word serialise), then four atomics a wave
    int bx0 = INT_MAX, bx1 = -1, by0 = INT_MAX, by1 = -1;
    for (int t = tid; t < n_created; t += blockDim.x) {
      const int ci = m.created[t];
      if (m.cell[ci].flags & kCellBuilt) {
        const int ix = ci % m.g.W, iy = ci / m.g.W;
        bx0 = min(bx0, ix);
        bx1 = max(bx1, ix);
        by0 = min(by0, iy);
        by1 = max(by1, iy);
      }
    }
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
      bx0 = min(bx0, __shfl_xor(bx0, d, kWave));
      bx1 = max(bx1, __shfl_xor(bx1, d, kWave));
      by0 = min(by0, __shfl_xor(by0, d, kWave));
      by1 = max(by1, __shfl_xor(by1, d, kWave));
    }
    if (lane_id() == 0 && bx1 >= 0) {
      atomicMin(&box[0], bx0);
      atomicMax(&box[1], bx1);
      atomicMin(&box[2], by0);
      atomicMax(&box[3], by1);
    }
  }
  __syncthreads();
  const bool any = box[1] >= 0;
  const int x0 = any ? box[0] : 0, x1 = any ? box[1] : 0, y0 = any ? box[2] : 0, y1 = any ? box[3] : 0;
  const int w = x1 - x0 + 1, h = y1 - y0 + 1, n_words = (w * h + 31) / 32;
  // A box beyond what LDS holds (~650 000 cells: a robot that has covered 200 m x 200 m at 0.25 m cells) is assembled in the
  // image itself: the same steps through HBM -- global atomics, wave 0's two sweeps over the words -- a millisecond where LDS
  // takes 20 us, and only then (until round 6 such a frame was refused)
  uint2* g_bm = reinterpret_cast<uint2*>(image + kImageHeaderBytes);
  const bool in_image = n_words > cap_words;  // (uniform)
  if (in_image) bm = g_bm;
  for (int i = tid; i < n_words; i += blockDim.x) bm[i] = make_uint2(0u, 0u);
  __syncthreads();
  for (int t = tid; t < n_created; t += blockDim.x) {
    const int ci = m.created[t];
    if (m.cell[ci].flags & kCellBuilt) {
      const int k = (ci / m.g.W - y0) * w + (ci % m.g.W - x0);
      atomicOr(&bm[k >> 5].x, 1u << (k & 31));
    }
  }
  __syncthreads();
  uint32_t* total = reinterpret_cast<uint32_t*>(box + 8);
  if (wave_id() == 0) prefix_words_wave0(bm, n_words, total);
  __syncthreads();
  const int n_built = (int)*total, cap = max(n_built, 1);
  double2* t_mean = reinterpret_cast<double2*>(image + image_mean_offset(n_words));
  double2* t_ab = reinterpret_cast<double2*>(image + image_ab_offset(n_words, cap));
  double2* t_cd = reinterpret_cast<double2*>(image + image_cd_offset(n_words, cap));
  float4* t_chol = reinterpret_cast<float4*>(image + image_chol_offset(n_words, cap));
  for (int t = tid; t < n_created; t += blockDim.x) {
    const int ci = m.created[t];
    const MapCell& c = m.cell[ci];
    if (!(c.flags & kCellBuilt)) continue;
    const int k = (ci / m.g.W - y0) * w + (ci % m.g.W - x0);
    const uint2 e = bm[k >> 5];
    const int s = (int)e.y + __popc(e.x & ((1u << (k & 31)) - 1u));
    t_mean[s] = c.mean;
    t_ab[s] = make_double2(c.icov.x, c.icov.y);
    t_cd[s] = make_double2(c.icov.z, c.icov.w);
    float l[4];
    make_chol(c.icov.x, c.icov.y, c.icov.z, c.icov.w, l);
    t_chol[s] = make_float4(l[0], l[1], l[2], l[3]);
  }
  if (!in_image)
    for (int i = tid; i < n_words; i += blockDim.x) g_bm[i] = bm[i];
  if (tid == 0) {
    ImageHeader* ih = reinterpret_cast<ImageHeader*>(image);
    ih->n_built = (uint32_t)n_built;
    ih->n_created = (uint32_t)n_created;
    ih->status = 0;
    m.hdr->n_built = (uint32_t)n_built;
    m.hdr->n_words = (uint32_t)n_words;
    m.hdr->x0 = x0;
    m.hdr->x1 = x1;
    m.hdr->y0 = y0;
    m.hdr->y1 = y1;
    if (mirror) {  // the host's pinned copy of the header (a build ahead of time): written from here, no copy operation
      MapHeader hh = hdr0;
      hh.n_built = (uint32_t)n_built;
      hh.n_words = (uint32_t)n_words;
      hh.x0 = x0;
      hh.x1 = x1;
      hh.y0 = y0;
      hh.y1 = y1;
      *mirror = hh;
      publish_pinned_word(reinterpret_cast<uint32_t*>(mirror) + kSpecSeqWord, seq);  // polled by the host (wait_pinned_word)
    }
  }
}

// scan -> points of a resident scan (NDTFrame::loadLaser into the node's one-cell frame), appending at *n_io
__device__ __forceinline__ void
scan_to_resident_wg(const float* __restrict__ ranges, const ScanP& sp, const double2* __restrict__ dirs, int do_trans, double tc, double ts,
                    double ttx, double tty, double clip_hw, double clip_hh, double2* __restrict__ out_xy, uint32_t* __restrict__ n_io,
                    int append, int capacity) {
  const int old_n = append ? (int)*n_io : 0;
  __syncthreads();
  if (old_n + sp.n_beams > capacity) return;  // host checked the upper bound; never taken
  const int n = scan_to_points_wg<true>(ranges, sp, dirs, do_trans != 0, tc, ts, ttx, tty, out_xy + old_n, lds_cnt(0), clip_hw,
                                  clip_hh);
  if (threadIdx.x == 0) *n_io = (uint32_t)(old_n + n);
}
