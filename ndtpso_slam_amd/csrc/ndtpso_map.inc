// ndtpso_map.inc -- the device-resident reference frame (SURVEY 8 f-2 / f-3): NDTFrame's cells with their sliding
// windows live in HBM, scans are ingested, inserted, built and aligned against without the host touching a point.
// Included at the end of ndtpso_hip.hip (same translation unit: shares the context, the planner and k_align).
//
// Reference behaviour restated here (lib/ndtpso_slam/..):
//   NDTCell::addPoint   ndtcell.cpp:21-34    insert: slot reset on the first point after a rotation, running slot sum
//   NDTCell::build      ndtcell.cpp:36-68    build: WINDOW_ADD of sum / count / covariance, rotation after > 50 points
//   s_calc_covar_inverse ndtcell.cpp:93-111
//   NDTFrame::addPoint  ndtframe.cpp:215-235, getCellIndex :240-249, update :187-198, build :68-117 (occupancy :79-112)
//
// HBM layout (SoA over the W x H cells of the frame; sized for the whole frame up front -- 5.3 KB per cell):
//   cell[c]                MapCell, 128 B: running slot sum, window totals, mean, inverse covariance, counters
//   win_sum/cov/count      [c * 100 + slot]: the window's partial terms (s_partial_sums / covars / counts)
//   slot_head/tail/len     [c * 100 + slot]: the slot's point vector = a chain of 32-point chunks
//   chunk_pts, chunk_next  chunk pool: bump allocation + a free stack refilled when a slot is reset
//   created[]              indices of created cells (creation order; every per-cell pass runs over this list)
//   image                  the alignment table (bitmap words + records of the BUILT cells), rebuilt by pack
//   og_key[]               occupancy grid: (build number, cell, int8 value) keys, atomicMax = "the later write wins"

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

__global__ void __launch_bounds__(kInsertThreads)
k_map_insert(MapP m, const double2* __restrict__ pts, int n, const uint32_t* __restrict__ n_ptr, int do_trans,
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

// ---- NDTFrame::resetCells (ndtframe.cpp:208-212): NDTCell::reset (ndtcell.cpp:80-91) on every created cell -------------
// The running sums, the counts and the point vectors are cleared; the window's partial terms, created / built, the
// mean and the inverse covariance are not (so a cell that was built stays in the alignment table until it is touched).
__global__ void __launch_bounds__(256)
k_map_reset_cells(MapP m) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m.hdr->n_created) return;
  const int ci = m.created[t];
  for (int s = 0; s < kWinSlots; ++s) {
    const int slot = ci * kWinSlots + s;
    for (int c = m.slot_head[slot]; c >= 0;) {
      const int nx = m.chunk_next[c];
      pool_push(m, c);
      c = nx;
    }
    m.slot_head[slot] = -1;
    m.slot_tail[slot] = -1;
    m.slot_len[slot] = 0;
  }
  MapCell c = m.cell[ci];
  c.cur_sum = make_double2(0., 0.);
  c.global_sum = make_double2(0., 0.);
  c.global_cov = make_double4(0., 0., 0., 0.);
  c.cur_count = 0;
  c.global_count = 0;
  c.cur_id = 0;
  m.cell[ci] = c;
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

__global__ void __launch_bounds__(256)
k_map_build(MapP m, MapUndo* __restrict__ undo) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
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

__global__ void __launch_bounds__(256)
k_map_undo(MapP m, const MapUndo* __restrict__ undo) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m.hdr->n_created) return;
  const MapUndo u = undo[t];
  m.cell[m.created[t]] = u.cell;
  m.win_cov[u.slot] = u.win_cov;
  m.win_sum[u.slot] = u.win_sum;
  m.win_count[u.slot] = u.win_count;
}

// ---- occupancy grid of build() (ndtframe.cpp:79-112): one thread per (created cell, sub-cell) ----------------------
// The reference writes og[x + height * y] for ascending cell index, so of two cells that map to one entry (only
// possible when W != H, through row = index / heightNumOfCells) the higher index wins, and a later build overwrites
// an earlier one.  The key (build number, cell, value) under atomicMax reproduces both.
__global__ void __launch_bounds__(256)
k_map_occupancy(MapP m, int per_cell, double og_cs, unsigned og_height, unsigned og_count, unsigned long long build_no,
                unsigned long long* __restrict__ og_key) {
  const int kk2 = per_cell * per_cell;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)m.hdr->n_created * kk2) return;
  const int ci = m.created[t / kk2];
  const MapCell& c = m.cell[ci];
  if (!(c.flags & kCellBuilt)) return;  // normalDistribution of an un-built cell is 0 (ndtcell.cpp:70-78)
  const int r = (int)(t % kk2), j = r / per_cell, k = r % per_cell;
  const unsigned cx = (unsigned)ci % (unsigned)m.g.W, cy = (unsigned)ci / (unsigned)m.g.H;  // sic (ndtframe.cpp:81)
  const unsigned ox = cx * (unsigned)per_cell + (unsigned)j, oy = cy * (unsigned)per_cell + (unsigned)k;
  const double x_c = ((double)ox * og_cs + og_cs / 2.) - m.g.hw;
  const double y_c = ((double)oy * og_cs + og_cs / 2.) - m.g.hh;
  const double d0 = x_c - c.mean.x, d1 = y_c - c.mean.y;
  const double r0 = d0 * c.icov.x + d1 * c.icov.z;
  const double r1 = d0 * c.icov.y + d1 * c.icov.w;
  const double p = exp(-(r0 * d0 + r1 * d1) / 2.);
  if (!(p > 0.)) return;
  atomicMin(&m.hdr->og_min_x, ox);
  atomicMax(&m.hdr->og_max_x, ox);
  atomicMin(&m.hdr->og_min_y, oy);
  atomicMax(&m.hdr->og_max_y, oy);
  const size_t at = (size_t)ox + (size_t)og_height * oy;
  if (at >= og_count) {  // the reference writes out of bounds here
    atomicOr(&m.hdr->status, kMapOgOutside);
    return;
  }
  const unsigned long long key = (build_no << 40) | ((unsigned long long)(unsigned)ci << 8) |
                                 (unsigned long long)(uint8_t)x86_int8_of(p * 100.);
  atomicMax(&og_key[at], key);
}

// ---- pack: built cells -> the alignment table image (same layout ndtpso_ref_set_cells produces) ------------------
// One workgroup; the bitmap of the bounding box is assembled in LDS.
__global__ void __launch_bounds__(1024)
k_map_pack(MapP m, unsigned char* __restrict__ image, MapHeader* __restrict__ mirror, uint32_t seq, int cap_words) {
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
__global__ void __launch_bounds__(1024)
k_scan_to_resident(const float* __restrict__ ranges, ScanP sp, const double2* __restrict__ dirs, int do_trans, double tc, double ts, double ttx,
                   double tty, double clip_hw, double clip_hh, double2* __restrict__ out_xy, uint32_t* __restrict__ n_io,
                   int append, int capacity) {
  const int old_n = append ? (int)*n_io : 0;
  __syncthreads();
  if (old_n + sp.n_beams > capacity) return;  // host checked the upper bound; never taken
  const int n = scan_to_points_wg<true>(ranges, sp, dirs, do_trans != 0, tc, ts, ttx, tty, out_xy + old_n, lds_cnt(0), clip_hw,
                                  clip_hh);
  if (threadIdx.x == 0) *n_io = (uint32_t)(old_n + n);
}

// =====================================================================================================================
// host side
// =====================================================================================================================

struct ndtpso_points {
  ndtpso_ctx* ctx = nullptr;
  DevBuf xy, n_dev, ranges;
  uint32_t capacity = 0;
  uint32_t n_upper = 0;  // host-side upper bound of the device-side count
};

struct ndtpso_map {
  ndtpso_ctx* ctx = nullptr;
  ndtpso_grid grid{};
  MapP p{};
  DevBuf cell, win_sum, win_cov, win_count, slot_head, slot_tail, slot_len, chunk_pts, chunk_next, free_list, created,
      hdr, image, og_key, stage;
  double og_cell_size = 0.;
  uint32_t og_width = 0, og_height = 0, og_count = 0;
  int n_words_max = 0;
  bool built = false;          // NDTFrame::built: false after an insert until the next build
  // A speculative build is in flight or done (ndtpso_map_speculate_build): cells built and table packed ahead of the
  // alignment that will want them, undo log kept, occupancy grid not yet touched.  align / build commit it; anything
  // else (insert, reset, exports) first puts the map back.
  bool spec = false;
  DevBuf undo;
  MapHeader* spec_hdr = nullptr;  // pinned: the header as of the speculative build, written by the pack kernel itself
  uint32_t spec_seq = 0;          // number of that build (kSpecSeqWord)
  unsigned long long builds = 0;
  unsigned long long points_upper = 0;  // upper bound of the points ever inserted (bounds n_created)
  unsigned long long chunks_bound = 0;  // upper bound of the pool chunks in use (a point opens at most one)
  MapHeader host_hdr{};
  // late window binding (ndtpso_map_align): points_upper when the latest build was enqueued, the same figure for the
  // build whose header host_hdr holds (ULLONG_MAX: not known) -- the built cells can have grown by at most the
  // difference --, and for the build before a speculative one
  unsigned long long build_pts = 0, known_pts = ~0ull, spec_prev_pts = 0;
  unsigned long long late_aligned = 0, late_fallbacks = 0;  // diagnostics (NDTPSO_LOG_LATE)
};

namespace {

void map_release(ndtpso_map* m) {
  for (DevBuf* b : {&m->cell, &m->win_sum, &m->win_cov, &m->win_count, &m->slot_head, &m->slot_tail, &m->slot_len,
                    &m->chunk_pts, &m->chunk_next, &m->free_list, &m->created, &m->hdr, &m->image, &m->og_key, &m->stage,
                    &m->undo})
    b->release();
  if (m->spec_hdr) (void)hipHostFree(m->spec_hdr);
  m->spec_hdr = nullptr;
}

int map_clear(ndtpso_map* m) {  // the state of a freshly constructed frame
  ndtpso_ctx* c = m->ctx;
  const size_t nc = (size_t)m->p.n_cells, ns = nc * kWinSlots;
  HIP_TRY(c, hipMemsetAsync(m->cell.p, 0, nc * sizeof(MapCell), c->stream));
  HIP_TRY(c, hipMemsetAsync(m->win_sum.p, 0, ns * 16, c->stream));
  HIP_TRY(c, hipMemsetAsync(m->win_cov.p, 0, ns * 32, c->stream));
  HIP_TRY(c, hipMemsetAsync(m->win_count.p, 0, ns * 4, c->stream));
  HIP_TRY(c, hipMemsetAsync(m->slot_head.p, 0xff, ns * 4, c->stream));
  HIP_TRY(c, hipMemsetAsync(m->slot_tail.p, 0xff, ns * 4, c->stream));
  HIP_TRY(c, hipMemsetAsync(m->slot_len.p, 0, ns * 4, c->stream));
  MapHeader h{};
  h.og_min_x = h.og_min_y = UINT32_MAX;
  m->host_hdr = h;
  HIP_TRY(c, hipMemcpyAsync(m->hdr.p, &m->host_hdr, sizeof(h), hipMemcpyHostToDevice, c->stream));
  if (m->og_count) HIP_TRY(c, hipMemsetAsync(m->og_key.p, 0, (size_t)m->og_count * 8, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  m->built = false;
  m->spec = false;
  m->builds = 0;
  m->points_upper = 0;
  m->build_pts = 0;
  m->known_pts = ~0ull;
  return NDTPSO_OK;
}

int map_fetch_header(ndtpso_map* m) {
  ndtpso_ctx* c = m->ctx;
  HIP_TRY(c, hipMemcpyAsync(&m->host_hdr, m->hdr.p, sizeof(MapHeader), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  m->known_pts = m->spec ? ~0ull : m->build_pts;  // (a speculative build's header may yet be taken back)
  if (m->host_hdr.status & kMapPoolExhausted) return fail(c, NDTPSO_E_CAPACITY, "map point pool exhausted");
  return NDTPSO_OK;
}

unsigned created_upper(const ndtpso_map* m) {
  return (unsigned)std::min<unsigned long long>((unsigned long long)m->p.n_cells, m->points_upper);
}

int map_enqueue_cells(ndtpso_map* m, MapUndo* undo) {  // NDTCell::build on every created cell
  ndtpso_ctx* c = m->ctx;
  const unsigned nc = created_upper(m);
  if (nc) {
    // half a wave per workgroup: a cell's points are read by one lane, chunk after chunk (every load instruction touches
    // one line per lane), and the few hundred created cells of a live map spread over more compute units (256 threads
    // per workgroup: 14.9 us per build on the live sequence, 64: 12.8, 32: 11.9, 8: 11.0 -- the rest is the chain of
    // dependent loads)
    constexpr unsigned kBuildLanes = 32;
    hipLaunchKernelGGL(k_map_build, dim3((nc + kBuildLanes - 1) / kBuildLanes), dim3(kBuildLanes), 0, c->stream, m->p, undo);
    HIP_TRY(c, hipGetLastError());
  }
  return NDTPSO_OK;
}

int map_enqueue_occupancy(ndtpso_map* m) {  // the occupancy-grid branch of build(), as build number m->builds + 1
  ndtpso_ctx* c = m->ctx;
  const unsigned nc = created_upper(m);
  const int per_cell = m->og_count ? (int)std::floor(m->grid.cell_side / m->og_cell_size) : 0;  // ndtframe.cpp:70
  if (nc && per_cell > 0) {
    const size_t total = (size_t)nc * per_cell * per_cell;
    hipLaunchKernelGGL(k_map_occupancy, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, m->p, per_cell,
                       m->og_cell_size, m->og_height, m->og_count, m->builds + 1, (unsigned long long*)m->og_key.p);
    HIP_TRY(c, hipGetLastError());
  }
  return NDTPSO_OK;
}

int map_enqueue_pack(ndtpso_map* m, MapHeader* mirror = nullptr, uint32_t seq = 0) {  // the alignment table of the built cells
  ndtpso_ctx* c = m->ctx;
  // (the bitmap of the BUILT cells' bounding box is assembled in LDS: room for the whole grid's where that fits, else for as much
  // as LDS holds -- ~650 000 cells of explored box; a larger box is assembled in the image itself, k_map_pack)
  const int pack_lds = std::min(kCtrlBytes + m->n_words_max * 8, kMaxLds);
  hipLaunchKernelGGL(k_map_pack, dim3(1), dim3(1024), pack_lds, c->stream, m->p, (unsigned char*)m->image.p, mirror, seq,
                     (pack_lds - kCtrlBytes) / 8);
  HIP_TRY(c, hipGetLastError());
  return NDTPSO_OK;
}

// build() of the frame: every created cell, then the occupancy grid, then the alignment table.  Asynchronous.
int map_enqueue_build(ndtpso_map* m) {
  if (int rc = map_enqueue_cells(m, nullptr)) return rc;
  if (int rc = map_enqueue_occupancy(m)) return rc;
  if (int rc = map_enqueue_pack(m)) return rc;
  ++m->builds;
  m->built = true;
  m->build_pts = m->points_upper;
  m->known_pts = ~0ull;
  return NDTPSO_OK;
}

// A speculative build becomes the real one: only the occupancy grid is still owed (the alignment does not read it).
int map_commit_speculation(ndtpso_map* m) {
  if (int rc = map_enqueue_occupancy(m)) return rc;
  ++m->builds;
  m->built = true;
  m->spec = false;
  return NDTPSO_OK;
}

// ... or is taken back: the map is again as the last insert left it.
int map_settle(ndtpso_map* m) {
  if (!m->spec) return NDTPSO_OK;
  ndtpso_ctx* c = m->ctx;
  const unsigned nc = created_upper(m);
  if (nc) {
    hipLaunchKernelGGL(k_map_undo, dim3((nc + 255) / 256), dim3(256), 0, c->stream, m->p, (const MapUndo*)m->undo.p);
    HIP_TRY(c, hipGetLastError());
  }
  m->known_pts = ~0ull;
  m->build_pts = m->spec_prev_pts;
  m->spec = false;
  return NDTPSO_OK;
}

int map_commit_speculation_cb(void* m) { return map_commit_speculation(static_cast<ndtpso_map*>(m)); }

// the window of the table a header describes: what the LDS plan of an alignment or a cost goes by
WinP window_of(const MapHeader& h) {
  WinP wn;
  wn.x0 = h.x0;
  wn.y0 = h.y0;
  wn.w = h.x1 - h.x0 + 1;
  wn.h = h.y1 - h.y0 + 1;
  wn.n_words = (int)h.n_words;
  wn.rec_cap = std::max<int>((int)h.n_built, 1);
  return wn;
}

// Late window binding: a speculative build's header is still on its way when the node asks for the alignment (the
// pack kernel has not even run) -- instead of waiting for it, the layout is planned for an upper bound (the whole grid;
// the built cells of the header this host saw last plus one per point inserted since) and the kernel takes the real
// window from the device.  The host then enqueues the alignment straight behind the build, and the device goes from
// one to the other without the 10-20 us of idle time the header's trip to the host and the launch cost.  Any doubt (no
// earlier header, a plan that is not the dense form -- the caller probes that with `ub` --, the bound exceeded, an
// alignment to be redone) ends in the synchronous path: map_await_header.
bool map_late_bound(const ndtpso_map* m, int mode, WinP* ub) {
  static const bool allow_late = [] {
    const char* e = std::getenv("NDTPSO_LATE_WINDOW");  // tuning / test knob: =0 always waits for the header
    return !(e && e[0] == '0');
  }();
  if (!m->spec || !allow_late || mode == NDTPSO_SCORE_F64 || m->known_pts == ~0ull || m->known_pts != m->spec_prev_pts ||
      m->build_pts < m->known_pts)
    return false;
  const unsigned long long grown = (unsigned long long)m->host_hdr.n_built + (m->build_pts - m->known_pts);
  ub->x0 = 0;
  ub->y0 = 0;
  ub->w = m->p.g.W;
  ub->h = m->p.g.H;
  ub->n_words = (ub->w * ub->h + 31) / 32;
  ub->rec_cap = (int)std::min<unsigned long long>((unsigned long long)m->p.n_cells, std::max<unsigned long long>(grown, 1ull));
  static const bool test_overflow = std::getenv("NDTPSO_LATE_TEST_OVERFLOW") != nullptr;  // test hook: a bound the table exceeds
  if (test_overflow) ub->rec_cap = 1;
  return true;
}

// the header of a speculative build whose pack kernel has run (it wrote it to pinned memory itself) becomes the host's
int map_take_spec_header(ndtpso_map* m) {
  m->host_hdr = *m->spec_hdr;
  m->known_pts = m->build_pts;
  if (m->host_hdr.status & kMapPoolExhausted) return fail(m->ctx, NDTPSO_E_CAPACITY, "map point pool exhausted");
  return NDTPSO_OK;
}

// the header of the map's latest build with the host: a speculative build's is already on its way, any other is fetched
int map_await_header(ndtpso_map* m) {
  if (!m->spec) return map_fetch_header(m);
  if (int rc = wait_pinned_word(m->ctx, reinterpret_cast<const uint32_t*>(m->spec_hdr) + kSpecSeqWord, m->spec_seq)) return rc;
  return map_take_spec_header(m);
}

// NDTFrame::addPoint for every point (ndtframe.cpp:215-225): a point that lands in the frame clears `built`, one that
// does not leaves it alone -- and that matters, because a build repeated on unchanged cells is not a no-op in floating
// point (WINDOW_ADD, ndtcell.h:13-15: (global + partial) - partial).  `accepted`: 1 some point lands in the frame,
// 0 none does, -1 not known to the host.  Only a map that is currently built needs the answer; if the host does not
// have it, the device's count of stored points is read before and after (one synchronisation, off the node's path:
// update() and loadLaser() clear the flag themselves, ndtpso_map_mark_unbuilt).
// The point pool grows instead of running out (the reference's cells just grow their std::vectors): the host keeps an
// upper bound of the chunks in use -- every inserted point can open at most one -- and only when that bound reaches the
// pool does it read the true figure from the device (one synchronisation per ~pool/1081 scans); a pool more than half
// full is then doubled: new buffers, device-to-device copies of the used part, chunk numbers stay what they are.
// A failed allocation leaves the old pool in place (the insert then reports NDTPSO_E_CAPACITY when it does run out).
int map_grow_pool_if_needed(ndtpso_map* m, uint32_t n_upper) {
  ndtpso_ctx* c = m->ctx;
  const unsigned long long cap = (unsigned long long)m->p.pool_chunks;
  if (m->chunks_bound + n_upper <= cap) {
    m->chunks_bound += n_upper;
    return NDTPSO_OK;
  }
  if (int rc = map_fetch_header(m)) return rc;  // synchronises
  const long long used = std::max<long long>(0, (long long)m->host_hdr.pool_bump - std::max(0, m->host_hdr.pool_free));
  m->chunks_bound = (unsigned long long)used + n_upper;
  if ((unsigned long long)used + n_upper <= cap / 2) return NDTPSO_OK;
  const unsigned long long want = std::min<unsigned long long>((unsigned long long)INT_MAX, std::max(2 * cap, (unsigned long long)used + 4ull * n_upper));
  if (want <= cap) return NDTPSO_OK;
  if (std::getenv("NDTPSO_MAP_POOL_FIXED")) return NDTPSO_OK;  // (tests of the exhaustion path; read on this slow path only)
  DevBuf pts, next, freel;
  hipError_t e = pts.reserve((size_t)want * kChunk * 16);
  if (e == hipSuccess) e = next.reserve((size_t)want * 4);
  if (e == hipSuccess) e = freel.reserve((size_t)want * 4);
  if (e != hipSuccess) {
    pts.release();
    next.release();
    freel.release();
    (void)hipGetLastError();
    return NDTPSO_OK;  // keep going with what there is
  }
  const size_t bump = (size_t)std::min<long long>(std::max(0, m->host_hdr.pool_bump), (long long)cap);
  const size_t nfree = (size_t)std::min<long long>(std::max(0, m->host_hdr.pool_free), (long long)cap);
  // (DevBuf has no destructor: every error path below gives the three new buffers back)
  hipError_t ce = hipSuccess;
  if (bump) {
    ce = hipMemcpyAsync(pts.p, m->chunk_pts.p, bump * kChunk * 16, hipMemcpyDeviceToDevice, c->stream);
    if (ce == hipSuccess) ce = hipMemcpyAsync(next.p, m->chunk_next.p, bump * 4, hipMemcpyDeviceToDevice, c->stream);
  }
  if (ce == hipSuccess && nfree) ce = hipMemcpyAsync(freel.p, m->free_list.p, nfree * 4, hipMemcpyDeviceToDevice, c->stream);
  // a pool that had already run over (an earlier grow could not allocate): the bump pointer goes back to the old
  // capacity so that the new chunks are handed out; the sticky kMapPoolExhausted flag stays -- points WERE dropped then,
  // and the next synchronising call reports it
  if (ce == hipSuccess && (long long)m->host_hdr.pool_bump > (long long)cap) {
    const int32_t clamped = (int32_t)cap;
    ce = hipMemcpyAsync(reinterpret_cast<unsigned char*>(m->p.hdr) + offsetof(MapHeader, pool_bump), &clamped, sizeof(clamped),
                        hipMemcpyHostToDevice, c->stream);
  }
  if (ce == hipSuccess) ce = hipStreamSynchronize(c->stream);  // the old buffers are freed next
  if (ce != hipSuccess) {
    pts.release();
    next.release();
    freel.release();
    return fail(c, NDTPSO_E_HIP, std::string("growing the map's point pool: ") + hipGetErrorString(ce));
  }
  m->chunk_pts.release();
  m->chunk_next.release();
  m->free_list.release();
  m->chunk_pts = pts;
  m->chunk_next = next;
  m->free_list = freel;
  m->p.chunk_pts = (double2*)m->chunk_pts.p;
  m->p.chunk_next = (int*)m->chunk_next.p;
  m->p.free_list = (int*)m->free_list.p;
  m->p.pool_chunks = (int)want;
  return NDTPSO_OK;
}

int map_insert_device(ndtpso_map* m, const double2* d_xy, uint32_t n_upper, const uint32_t* d_n, const double* pose,
                      int accepted) {
  ndtpso_ctx* c = m->ctx;
  if (n_upper == 0 || accepted == 0) return NDTPSO_OK;
  if (int rc = map_grow_pool_if_needed(m, n_upper)) return rc;
  const bool ask = m->built && accepted < 0;
  unsigned long long stored_before = 0;
  if (ask) {
    if (int rc = map_fetch_header(m)) return rc;
    stored_before = m->host_hdr.n_points;
  }
  if (int rc = map_settle(m)) return rc;
  const int do_trans = pose ? 1 : 0;
  const double th = pose ? pose[2] : 0.;
  const CosSin cs = host_cos_sin(th);
  hipLaunchKernelGGL(k_map_insert, dim3(1), dim3(kInsertThreads), 0, c->stream, m->p, d_xy, (int)n_upper, d_n, do_trans,
                     cs.c, cs.s, pose ? pose[0] : 0., pose ? pose[1] : 0.);
  HIP_TRY(c, hipGetLastError());
  m->points_upper += n_upper;
  if (ask) {
    if (int rc = map_fetch_header(m)) return rc;
    if (m->host_hdr.n_points != stored_before) m->built = false;
  } else {
    m->built = false;
  }
  return NDTPSO_OK;
}

}  // namespace

extern "C" {

int ndtpso_points_create(ndtpso_ctx* c, uint32_t capacity, ndtpso_points** out) {
  if (!c || !out || capacity == 0) return fail(c, NDTPSO_E_ARG, "null argument");
  *out = nullptr;
  HIP_TRY(c, hipSetDevice(c->device));
  ndtpso_points* p = new ndtpso_points();
  p->ctx = c;
  p->capacity = capacity;
  hipError_t e = p->xy.reserve((size_t)capacity * 16);
  if (e == hipSuccess) e = p->n_dev.reserve(256);
  if (e == hipSuccess) e = hipMemsetAsync(p->n_dev.p, 0, 256, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    p->xy.release();
    p->n_dev.release();
    delete p;
    return fail(c, NDTPSO_E_HIP, hipGetErrorString(e));
  }
  *out = p;
  return NDTPSO_OK;
}

void ndtpso_points_destroy(ndtpso_points* p) {
  if (!p) return;
  (void)hipSetDevice(p->ctx->device);
  (void)hipStreamSynchronize(p->ctx->stream);
  p->xy.release();
  p->n_dev.release();
  p->ranges.release();
  delete p;
}

int ndtpso_points_load_scan(ndtpso_points* p, const float* ranges, const ndtpso_scan_geom* geom, const double trans[3],
                            const ndtpso_grid* clip, int append) {
  if (!p) return NDTPSO_E_ARG;
  ndtpso_ctx* c = p->ctx;
  if (!ranges || !geom || geom->n_beams == 0) return fail(c, NDTPSO_E_ARG, "null argument");
  const uint32_t upper = (append ? p->n_upper : 0u) + geom->n_beams;
  if (upper > p->capacity) return fail(c, NDTPSO_E_CAPACITY, "resident scan capacity exceeded");
  HIP_TRY(c, hipSetDevice(c->device));
  // the ranges go into a pinned slot and the kernel reads them there (4 KB, each read once): no copy operation
  void* staged = nullptr;
  int slot = 0;
  HIP_TRY(c, c->pinned.stage((size_t)geom->n_beams * 4, &staged, &slot, c->align_seen));
  std::memcpy(staged, ranges, (size_t)geom->n_beams * 4);
  const double zero[3] = {0., 0., 0.};
  const double* t = trans ? trans : zero;
  const int do_trans = trans_is_zero(t) ? 0 : 1;
  const CosSin cs = host_cos_sin(t[2]);
  ScanP sp;
  const double2* dirs = nullptr;
  if (int rc = make_scan(c, geom, &sp, &dirs)) return rc;
  hipLaunchKernelGGL(k_scan_to_resident, dim3(1), dim3(1024), kCtrlBytes, c->stream, (const float*)staged,
                     sp, dirs, do_trans, cs.c, cs.s, t[0], t[1],
                     clip ? clip->width / 2. : 0., clip ? clip->height / 2. : 0., (double2*)p->xy.p,
                     (uint32_t*)p->n_dev.p, append ? 1 : 0, (int)p->capacity);
  HIP_TRY(c, hipGetLastError());
  c->pinned.fence_until(slot, c->stream, c->align_issued + 1);  // free once an alignment launched from now on has reported
  p->n_upper = upper;
  return NDTPSO_OK;
}

int ndtpso_points_set(ndtpso_points* p, const double* xy, uint32_t n) {
  if (!p) return NDTPSO_E_ARG;
  ndtpso_ctx* c = p->ctx;
  if ((!xy && n) || n > p->capacity) return fail(c, n > p->capacity ? NDTPSO_E_CAPACITY : NDTPSO_E_ARG, "bad point list");
  HIP_TRY(c, hipSetDevice(c->device));
  if (n) HIP_TRY(c, hipMemcpyAsync(p->xy.p, xy, (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(p->n_dev.p, &n, 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  p->n_upper = n;
  return NDTPSO_OK;
}

int ndtpso_points_get(ndtpso_points* p, double* xy, uint32_t max_points, uint32_t* n_out) {
  if (!p || !n_out) return NDTPSO_E_ARG;
  ndtpso_ctx* c = p->ctx;
  HIP_TRY(c, hipSetDevice(c->device));
  uint32_t n = 0;
  HIP_TRY(c, hipMemcpyAsync(&n, p->n_dev.p, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  *n_out = n;
  p->n_upper = n;
  const uint32_t k = std::min(n, max_points);
  if (k && xy) HIP_TRY(c, hipMemcpy(xy, p->xy.p, (size_t)k * 16, hipMemcpyDeviceToHost));
  return NDTPSO_OK;
}

int ndtpso_map_create(ndtpso_ctx* c, const ndtpso_grid* grid, double og_cell_size, uint64_t pool_bytes, ndtpso_map** out) {
  if (!c || !out) return fail(c, NDTPSO_E_ARG, "null argument");
  *out = nullptr;
  GridP g;
  if (make_grid(grid, &g) != NDTPSO_OK) return fail(c, NDTPSO_E_ARG, "bad grid");
  HIP_TRY(c, hipSetDevice(c->device));
  ndtpso_map* m = new ndtpso_map();
  m->ctx = c;
  m->grid = *grid;
  const size_t nc = (size_t)g.W * g.H, ns = nc * kWinSlots;
  if (pool_bytes == 0) pool_bytes = 1ull << 30;
  const size_t chunks = std::max<size_t>(64, (size_t)(pool_bytes / (kChunk * 16)));
  if (chunks > (size_t)INT_MAX || nc >= (1u << 21)) {  // the insert sort key is (cell << 11 | position) in 32 bits, all ones = no point
    delete m;
    return fail(c, NDTPSO_E_ARG, chunks > (size_t)INT_MAX ? "point pool too large" : "frame has 2^21 cells or more");
  }
  m->n_words_max = (int)((nc + 31) / 32);
  if (og_cell_size > 0.) {  // ndtframe.cpp:36-46
    m->og_cell_size = og_cell_size;
    m->og_width = (uint32_t)std::ceil(grid->width / og_cell_size);
    m->og_height = (uint32_t)std::ceil(grid->height / og_cell_size);
    m->og_count = m->og_width * m->og_height;
  }
  hipError_t e = m->cell.reserve(nc * sizeof(MapCell));
  if (e == hipSuccess) e = m->win_sum.reserve(ns * 16);
  if (e == hipSuccess) e = m->win_cov.reserve(ns * 32);
  if (e == hipSuccess) e = m->win_count.reserve(ns * 4);
  if (e == hipSuccess) e = m->slot_head.reserve(ns * 4);
  if (e == hipSuccess) e = m->slot_tail.reserve(ns * 4);
  if (e == hipSuccess) e = m->slot_len.reserve(ns * 4);
  if (e == hipSuccess) e = m->chunk_pts.reserve(chunks * kChunk * 16);
  if (e == hipSuccess) e = m->chunk_next.reserve(chunks * 4);
  if (e == hipSuccess) e = m->free_list.reserve(chunks * 4);
  if (e == hipSuccess) e = m->created.reserve(nc * 4);
  if (e == hipSuccess) e = m->hdr.reserve(256);
  if (e == hipSuccess) e = m->image.reserve((size_t)image_bytes(m->n_words_max, (int)nc));
  if (e == hipSuccess && m->og_count) e = m->og_key.reserve((size_t)m->og_count * 8);
  if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_map_pack),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
  if (e != hipSuccess) {
    map_release(m);
    delete m;
    return fail(c, NDTPSO_E_HIP, std::string("map allocation: ") + hipGetErrorString(e));
  }
  MapP& p = m->p;
  p.g = g;
  p.n_cells = (int)nc;
  p.pool_chunks = (int)chunks;
  p.cell = (MapCell*)m->cell.p;
  p.win_sum = (double2*)m->win_sum.p;
  p.win_cov = (double4*)m->win_cov.p;
  p.win_count = (int*)m->win_count.p;
  p.slot_head = (int*)m->slot_head.p;
  p.slot_tail = (int*)m->slot_tail.p;
  p.slot_len = (int*)m->slot_len.p;
  p.chunk_pts = (double2*)m->chunk_pts.p;
  p.chunk_next = (int*)m->chunk_next.p;
  p.free_list = (int*)m->free_list.p;
  p.created = (int*)m->created.p;
  p.hdr = (MapHeader*)m->hdr.p;
  const int rc = map_clear(m);
  if (rc != NDTPSO_OK) {
    map_release(m);
    delete m;
    return rc;
  }
  *out = m;
  return NDTPSO_OK;
}

void ndtpso_map_destroy(ndtpso_map* m) {
  if (!m) return;
  (void)hipSetDevice(m->ctx->device);
  (void)hipStreamSynchronize(m->ctx->stream);
  if (std::getenv("NDTPSO_LOG_LATE") && (m->late_aligned || m->late_fallbacks))
    std::fprintf(stderr, "ndtpso: late window binding: %llu alignments, %llu redone the usual way\n", m->late_aligned, m->late_fallbacks);
  map_release(m);
  delete m;
}

int ndtpso_map_clear(ndtpso_map* m) {
  if (!m) return NDTPSO_E_ARG;
  HIP_TRY(m->ctx, hipSetDevice(m->ctx->device));
  return map_clear(m);
}

int ndtpso_map_reset(ndtpso_map* m) {
  if (!m) return NDTPSO_E_ARG;
  ndtpso_ctx* c = m->ctx;
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = map_settle(m)) return rc;
  const unsigned nc = created_upper(m);
  if (nc) {
    hipLaunchKernelGGL(k_map_reset_cells, dim3((nc + 255) / 256), dim3(256), 0, c->stream, m->p);
    HIP_TRY(c, hipGetLastError());
  }
  m->known_pts = ~0ull;
  return NDTPSO_OK;  // NDTFrame::built is not touched by resetCells
}

int ndtpso_map_mark_unbuilt(ndtpso_map* m) {
  if (!m) return NDTPSO_E_ARG;
  m->built = false;  // (a speculative build only exists while the flag is already false)
  return NDTPSO_OK;
}

int ndtpso_map_insert(ndtpso_map* m, const ndtpso_points* pts, const double pose[3]) {
  if (!m || !pts) return NDTPSO_E_ARG;
  HIP_TRY(m->ctx, hipSetDevice(m->ctx->device));
  return map_insert_device(m, (const double2*)pts->xy.p, pts->n_upper, (const uint32_t*)pts->n_dev.p, pose,
                           m->built ? -1 : 1);
}

int ndtpso_map_insert_host(ndtpso_map* m, const double* xy, uint32_t n, const double pose[3]) {
  if (!m) return NDTPSO_E_ARG;
  ndtpso_ctx* c = m->ctx;
  if (!xy && n) return fail(c, NDTPSO_E_ARG, "null argument");
  if (n == 0) return NDTPSO_OK;
  int accepted = 1;  // (irrelevant while the map is not built)
  if (m->built) {
    accepted = -1;
    if (!pose) {  // untransformed points: the frame test of getCellIndex (ndtframe.cpp:242) can be made here
      accepted = 0;
      const double hw = m->p.g.hw, hh = m->p.g.hh;
      for (uint32_t i = 0; i < n && !accepted; ++i)
        accepted = (xy[2 * i] > -hw && xy[2 * i] < hw && xy[2 * i + 1] > -hh && xy[2 * i + 1] < hh) ? 1 : 0;
      if (!accepted) return NDTPSO_OK;
    }
  }
  HIP_TRY(c, hipSetDevice(c->device));
  // the previous insert may still be reading the staging buffer
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, m->stage.reserve((size_t)n * 16));
  HIP_TRY(c, hipMemcpyAsync(m->stage.p, xy, (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
  return map_insert_device(m, (const double2*)m->stage.p, n, nullptr, pose, accepted);
}

int ndtpso_map_build(ndtpso_map* m) {
  if (!m) return NDTPSO_E_ARG;
  HIP_TRY(m->ctx, hipSetDevice(m->ctx->device));
  if (m->spec) return map_commit_speculation(m);
  return map_enqueue_build(m);
}

int ndtpso_map_speculate_build(ndtpso_map* m) {
  if (!m) return NDTPSO_E_ARG;
  ndtpso_ctx* c = m->ctx;
  if (m->spec || m->built) return NDTPSO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const unsigned nc = created_upper(m);
  // (the bound grows by a scan's points per update until it reaches the grid's cells -- thirteen scans of 1081 points in a
  // 60 m frame of 0.5 m cells -- and a buffer sized to it was freed and allocated again at every one of them: a device-wide
  // synchronisation each, 17 - 38 ms for every replica of a process that runs 32.  Sized for the whole grid at once where that
  // is at most 64 MB, else in doublings.)
  {
    const size_t all = sizeof(MapUndo) * (size_t)std::max<unsigned>((unsigned)m->p.n_cells, 1u), need = sizeof(MapUndo) * (size_t)std::max(nc, 1u);
    if (m->undo.cap < need) HIP_TRY(c, m->undo.reserve(all <= (64u << 20) ? all : std::min(all, std::max(need, 2 * m->undo.cap))));
  }
  if (!m->spec_hdr) {
    HIP_TRY(c, hipHostMalloc((void**)&m->spec_hdr, 256, hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(m->spec_hdr, 0, 256);
  }
  if (int rc = map_enqueue_cells(m, (MapUndo*)m->undo.p)) return rc;
  if (int rc = map_enqueue_pack(m, m->spec_hdr, ++m->spec_seq)) return rc;  // (no event: the kernel publishes the header itself)
  m->spec_prev_pts = m->build_pts;
  m->build_pts = m->points_upper;
  m->spec = true;
  return NDTPSO_OK;
}

int ndtpso_map_get_info(ndtpso_map* m, ndtpso_map_info* info) {
  if (!m || !info) return NDTPSO_E_ARG;
  HIP_TRY(m->ctx, hipSetDevice(m->ctx->device));
  if (int rc = map_settle(m)) return rc;
  const int rc = map_fetch_header(m);
  std::memcpy(info, &m->host_hdr, sizeof(*info));
  return rc;
}

int ndtpso_map_align(ndtpso_map* m, const ndtpso_points* pts, const double guess[3], const double deviation[3],
                     const ndtpso_pso_config* cfg, uint32_t seed, const int32_t* rand_table, int mode,
                     double out_pose[3], double* out_cost, ndtpso_align_stats* stats) {
  if (!m || !pts) return NDTPSO_E_ARG;
  ndtpso_ctx* c = m->ctx;
  if (!guess || !deviation || !out_pose) return fail(c, NDTPSO_E_ARG, "null argument");
  if (mode != NDTPSO_SCORE_F32 && mode != NDTPSO_SCORE_F64 && mode != NDTPSO_SCORE_EXACT) return fail(c, NDTPSO_E_ARG, "bad score mode");
  if (int rc = check_pso(c, cfg)) return rc;
  if (int rc = exact_mode_resolve(c, &mode)) return rc;
  c->clk_enter = std::chrono::steady_clock::now();
  HIP_TRY(c, hipSetDevice(c->device));
  if (!m->spec && !m->built) {  // cost_function's lazy build, core.cpp:27-28
    if (int rc = map_enqueue_build(m)) return rc;
  }
  const size_t n_draw = ndtpso_rand_draws(cfg);
  HIP_TRY(c, c->out.reserve(256));
  HIP_TRY(c, c->table.reserve(kGuessBytes + (rand_table ? n_draw * 4 : 0)));
  double gd[6] = {guess[0], guess[1], guess[2], deviation[0], deviation[1], deviation[2]};
  // Guess, deviation and the rand() table go into a pinned slot and the kernel fetches them from there itself (k_align,
  // table_src): the upload was a copy operation plus two engine hand-overs between k_scan_to_resident and the
  // alignment, 38 us of the live sequence's 0.5 ms.  align_finish returns after the last kernel that reads the slot,
  // so it needs no fence.
  {
    void* staged = nullptr;
    int slot = 0;
    HIP_TRY(c, c->pinned.stage(kGuessBytes + (rand_table ? (n_draw * 4 + 15) / 16 * 16 : 0), &staged, &slot, c->align_seen));
    std::memcpy(staged, gd, sizeof(gd));
    if (rand_table) std::memcpy((unsigned char*)staged + kGuessBytes, rand_table, n_draw * 4);
    c->inputs = staged;
    c->inputs_pinned = true;
  }
  // late window binding: planned for an upper bound, launched straight behind the speculative build (map_late_bound)
  bool late_done = false;  // the late path ran: speculation committed, header with the host
  AlignSrc src{(const unsigned char*)m->image.p, m->p.g, WinP{}, (const double2*)pts->xy.p,
               std::max<uint32_t>(pts->n_upper, 1u), (const uint32_t*)pts->n_dev.p, out_cost != nullptr};
  Plan probe;
  if (map_late_bound(m, mode, &src.wn) &&
      make_plan(NDTPSO_SCORE_F32, src.g, src.wn, (int)src.n, cfg->population, &probe, false, true, true, mode == NDTPSO_SCORE_EXACT) &&
      probe.path == 2) {
    src.late_hdr = reinterpret_cast<const uint32_t*>(m->hdr.p);
    double host[kResultDoubles];
    const AfterLaunch og{&map_commit_speculation_cb, m};
    if (int rc = align_once(c, src, cfg, seed, rand_table != nullptr, mode, host, true, og)) return rc;
    if (int rc = map_take_spec_header(m)) return rc;  // written by the pack kernel, which precedes the alignment on the stream
    const AlignStats st = result_of(host);
    if (!must_redo_alone(st)) {
      result_of(host, out_pose, out_cost, stats);
      ++m->late_aligned;
      return NDTPSO_OK;
    }
    late_done = true;
    ++m->late_fallbacks;
    if (st.status & kStatusNeedsF64) mode = NDTPSO_SCORE_F64;  // (what align_finish would do next)
    src.late_hdr = nullptr;
  }
  // the table's window and size decide the LDS plan
  const bool still_speculative = m->spec;  // built and packed ahead of time, its header already on its way to the host
  if (still_speculative || !late_done)
    if (int rc = map_await_header(m)) return rc;
  src.wn = window_of(m->host_hdr);
  // the occupancy grid a committed speculation still owes is not read by the alignment: it follows it
  const AfterLaunch og{still_speculative ? &map_commit_speculation_cb : nullptr, m};
  return align_finish(c, src, cfg, seed, rand_table != nullptr, mode, out_pose, out_cost, stats, og);
}

}  // extern "C"

#include "ndtpso_map_batch.inc"

extern "C" {

// cost_function (core.cpp:26-48) of the points of a loaded scan against the map, for m poses; builds first if points
// were inserted since the last build, like the reference.  Synchronous.
int ndtpso_map_cost(ndtpso_map* m, ndtpso_points* pts, const double* poses, uint32_t n_poses, int mode, double* costs) {
  if (!m || !pts) return NDTPSO_E_ARG;
  ndtpso_ctx* c = m->ctx;
  if (!poses || !costs || n_poses == 0) return fail(c, NDTPSO_E_ARG, "null argument");
  if (mode == NDTPSO_SCORE_EXACT) mode = NDTPSO_SCORE_F64;  // a single cost: the exact mode is the fp64 score
  if (mode != NDTPSO_SCORE_F32 && mode != NDTPSO_SCORE_F64) return fail(c, NDTPSO_E_ARG, "bad score mode");
  HIP_TRY(c, hipSetDevice(c->device));
  if (m->spec) {
    if (int rc = map_commit_speculation(m)) return rc;
  } else if (!m->built) {
    if (int rc = map_enqueue_build(m)) return rc;
  }
  if (int rc = map_fetch_header(m)) return rc;
  uint32_t n = 0;
  HIP_TRY(c, hipMemcpy(&n, pts->n_dev.p, 4, hipMemcpyDeviceToHost));
  pts->n_upper = n;
  return cost_launch(c, (const unsigned char*)m->image.p, m->p.g, window_of(m->host_hdr), (const double2*)pts->xy.p, n, poses, n_poses,
                     mode, costs, nullptr);
}

// ---- exports (shutdown / inspection; synchronous, the host walks the downloaded structures) -----------------------

int ndtpso_map_get_cells(ndtpso_map* m, ndtpso_cell_row* rows, uint32_t max_rows, uint32_t* n_rows) {
  if (!m || !n_rows) return NDTPSO_E_ARG;
  ndtpso_ctx* c = m->ctx;
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = map_settle(m)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  std::vector<MapCell> cells((size_t)m->p.n_cells);
  HIP_TRY(c, hipMemcpy(cells.data(), m->cell.p, cells.size() * sizeof(MapCell), hipMemcpyDeviceToHost));
  uint32_t n = 0;
  for (int i = 0; i < m->p.n_cells; ++i) {
    const MapCell& s = cells[(size_t)i];
    if (!(s.flags & kCellCreated)) continue;
    if (rows && n < max_rows) {
      ndtpso_cell_row& r = rows[n];
      r.index = i;
      r.count = s.global_count;
      r.built = (s.flags & kCellBuilt) ? 1 : 0;
      r.reserved = s.cur_id;
      r.mean[0] = s.mean.x;
      r.mean[1] = s.mean.y;
      r.icov[0] = s.icov.x;
      r.icov[1] = s.icov.y;
      r.icov[2] = s.icov.z;
      r.icov[3] = s.icov.w;
    }
    ++n;
  }
  *n_rows = n;
  return NDTPSO_OK;
}

int ndtpso_map_get_points(ndtpso_map* m, int slot0_only, double* xy, uint64_t max_points, uint64_t* n_points) {
  if (!m || !n_points) return NDTPSO_E_ARG;
  ndtpso_ctx* c = m->ctx;
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = map_settle(m)) return rc;
  if (int rc = map_fetch_header(m)) return rc;
  const size_t nc = (size_t)m->p.n_cells, ns = nc * kWinSlots;
  const size_t used = (size_t)std::min<int>(std::max(m->host_hdr.pool_bump, 0), m->p.pool_chunks);
  std::vector<int> head(ns), len(ns), next(used);
  std::vector<double> pool(used * kChunk * 2);
  HIP_TRY(c, hipMemcpy(head.data(), m->slot_head.p, ns * 4, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(len.data(), m->slot_len.p, ns * 4, hipMemcpyDeviceToHost));
  if (used) {
    HIP_TRY(c, hipMemcpy(next.data(), m->chunk_next.p, used * 4, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(pool.data(), m->chunk_pts.p, used * kChunk * 16, hipMemcpyDeviceToHost));
  }
  uint64_t n = 0;
  // cell order, then window-slot order, then insertion order: the order dumpMap (ndtframe.cpp:314-328) and
  // cost_function (core.cpp:33-36, slot 0 only) visit the points in
  for (size_t ci = 0; ci < nc; ++ci)
    for (int s = 0; s < (slot0_only ? 1 : kWinSlots); ++s) {
      int left = len[ci * kWinSlots + s];
      for (int ch = head[ci * kWinSlots + s]; ch >= 0 && left > 0; ch = next[(size_t)ch]) {
        const int k = std::min(left, kChunk);
        for (int i = 0; i < k; ++i, ++n)
          if (xy && n < max_points) {
            xy[2 * n] = pool[((size_t)ch * kChunk + i) * 2];
            xy[2 * n + 1] = pool[((size_t)ch * kChunk + i) * 2 + 1];
          }
        left -= k;
      }
    }
  *n_points = n;
  return NDTPSO_OK;
}

int ndtpso_map_get_occupancy(ndtpso_map* m, int8_t* og, uint64_t og_bytes, uint32_t* og_width, uint32_t* og_height,
                             uint32_t extent[4]) {
  if (!m) return NDTPSO_E_ARG;
  ndtpso_ctx* c = m->ctx;
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = map_settle(m)) return rc;
  if (int rc = map_fetch_header(m)) return rc;
  if (og_width) *og_width = m->og_width;
  if (og_height) *og_height = m->og_height;
  if (extent) {
    extent[0] = m->host_hdr.og_min_x;
    extent[1] = m->host_hdr.og_max_x;
    extent[2] = m->host_hdr.og_min_y;
    extent[3] = m->host_hdr.og_max_y;
  }
  if (og && m->og_count) {
    if (og_bytes < m->og_count) return fail(c, NDTPSO_E_ARG, "occupancy buffer too small");
    std::vector<unsigned long long> keys(m->og_count);
    HIP_TRY(c, hipMemcpy(keys.data(), m->og_key.p, (size_t)m->og_count * 8, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < m->og_count; ++i) og[i] = (int8_t)(uint8_t)(keys[i] & 0xffu);
  }
  return NDTPSO_OK;
}

}  // extern "C"
