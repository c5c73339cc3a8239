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
//   trace_hits/passes[]    free-space evidence per occupancy entry (ndtpso_map_trace), allocated at the first trace


#include "ndtpso_map_device.inc"

#include "ndtpso_map_jobs.h"
#include "ndtpso_map_search.h"
#include "ndtpso_map_search_jobs.h"
#include "ndtpso_map_snapshot.h"
#include "ndtpso_map_curvature.h"
#include "ndtpso_map_trace.h"

// ---- the kernels of the single calls: one map (or one scan) each, the bodies in ndtpso_map_device.inc ---------------------
__global__ void __launch_bounds__(kInsertThreads)
k_map_insert(MapP m, const double2* __restrict__ pts, int n, const uint32_t* __restrict__ n_ptr, int do_trans,
             double tc, double ts, double ttx, double tty) {
  map_insert_wg(m, pts, n, n_ptr, do_trans, tc, ts, ttx, tty);
}

__global__ void __launch_bounds__(256)
k_map_build(MapP m, MapUndo* __restrict__ undo) {
  map_build_cell(m, undo, blockIdx.x * blockDim.x + threadIdx.x);
}

__global__ void __launch_bounds__(1024)
k_map_pack(MapP m, unsigned char* __restrict__ image, MapHeader* __restrict__ mirror, uint32_t seq, int cap_words) {
  map_pack_wg(m, image, mirror, seq, cap_words);
}

__global__ void __launch_bounds__(1024)
k_scan_to_resident(const float* __restrict__ ranges, ScanP sp, const double2* __restrict__ dirs, int do_trans, double tc, double ts, double ttx,
                   double tty, double clip_hw, double clip_hh, double2* __restrict__ out_xy, uint32_t* __restrict__ n_io,
                   int append, int capacity) {
  scan_to_resident_wg(ranges, sp, dirs, do_trans, tc, ts, ttx, tty, clip_hw, clip_hh, out_xy, n_io, append, capacity);
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
  // ndtpso_map_trace: hits (uint32) and passes (uint64) per occupancy entry and a TraceTotals, allocated at the first trace; nav:
  // the staged bytes of ndtpso_map_get_nav_grid
  DevBuf trace_hits, trace_passes, trace_tot, nav;
  DevBuf snap, snap_idx;       // ndtpso_map_snapshot / ndtpso_map_restore: the staged blob and its index, for the length of a call
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

int trace_zero(ndtpso_map* m);  // (ndtpso_map_trace.inc)

void map_release(ndtpso_map* m) {
  for (DevBuf* b : {&m->cell, &m->win_sum, &m->win_cov, &m->win_count, &m->slot_head, &m->slot_tail, &m->slot_len,
                    &m->chunk_pts, &m->chunk_next, &m->free_list, &m->created, &m->hdr, &m->image, &m->og_key, &m->stage,
                    &m->undo, &m->snap, &m->snap_idx, &m->trace_hits, &m->trace_passes, &m->trace_tot, &m->nav})
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
  if (m->trace_tot.p)
    if (int rc = trace_zero(m)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  m->built = false;
  m->spec = false;
  m->builds = 0;
  m->points_upper = 0;
  m->build_pts = 0;
  m->known_pts = ~0ull;
  return NDTPSO_OK;
}

// the header's trip to the host in two halves, so that a call with several maps (ndtpso_map_search_batch) waits once for all of them
int map_fetch_header_enqueue(ndtpso_map* m) {
  ndtpso_ctx* c = m->ctx;
  HIP_TRY(c, hipMemcpyAsync(&m->host_hdr, m->hdr.p, sizeof(MapHeader), hipMemcpyDeviceToHost, c->stream));
  return NDTPSO_OK;
}
int map_fetch_header_arrived(ndtpso_map* m) {
  m->known_pts = m->spec ? ~0ull : m->build_pts;  // (a speculative build's header may yet be taken back)
  if (m->host_hdr.status & kMapPoolExhausted) return fail(m->ctx, NDTPSO_E_CAPACITY, "map point pool exhausted");
  return NDTPSO_OK;
}

int map_fetch_header(ndtpso_map* m) {
  ndtpso_ctx* c = m->ctx;
  if (int rc = map_fetch_header_enqueue(m)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return map_fetch_header_arrived(m);
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

int map_pack_lds(const ndtpso_map* m);

int map_enqueue_pack(ndtpso_map* m, MapHeader* mirror = nullptr, uint32_t seq = 0) {  // the alignment table of the built cells
  ndtpso_ctx* c = m->ctx;
  // (the bitmap of the BUILT cells' bounding box is assembled in LDS: room for the whole grid's where that fits, else for as much
  // as LDS holds -- ~650 000 cells of explored box; a larger box is assembled in the image itself, k_map_pack)
  const int pack_lds = map_pack_lds(m);
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

// An insert in three steps, so that ndtpso_map_insert's own launch and the shared launch of ndtpso_map_update_batch run the same
// code around k_map_insert's body: prepare (the pool, the question a built map asks the device, a pending speculation taken
// back), the kernel with map_insert_job's arguments, after (the host's bounds and `built`).
struct InsertPrep {
  bool ask = false;
  unsigned long long stored_before = 0;
};

bool map_insert_skips(uint32_t n_upper, int accepted) { return n_upper == 0 || accepted == 0; }

// the preparation would wait for the device: a pool to be measured (and perhaps grown), a built map's count of stored points
bool map_insert_asks_device(const ndtpso_map* m, uint32_t n_upper, int accepted) {
  return m->chunks_bound + n_upper > (unsigned long long)m->p.pool_chunks || (m->built && accepted < 0);
}

int map_insert_prepare(ndtpso_map* m, uint32_t n_upper, int accepted, InsertPrep* prep) {
  if (int rc = map_grow_pool_if_needed(m, n_upper)) return rc;
  prep->ask = m->built && accepted < 0;
  if (prep->ask) {
    if (int rc = map_fetch_header(m)) return rc;
    prep->stored_before = m->host_hdr.n_points;
  }
  return map_settle(m);
}

MapUpdateJob map_insert_job(const ndtpso_map* m, const double2* d_xy, uint32_t n_upper, const uint32_t* d_n, const double* pose) {
  MapUpdateJob j;
  std::memset(&j, 0, sizeof(j));
  const CosSin cs = host_cos_sin(pose ? pose[2] : 0.);
  j.m = m->p;
  j.pts = d_xy;
  j.n_ptr = d_n;
  j.n = (int)n_upper;
  j.do_trans = pose ? 1 : 0;
  j.tc = cs.c;
  j.ts = cs.s;
  j.ttx = pose ? pose[0] : 0.;
  j.tty = pose ? pose[1] : 0.;
  return j;
}

int map_insert_after(ndtpso_map* m, uint32_t n_upper, const InsertPrep& prep) {
  m->points_upper += n_upper;
  if (prep.ask) {
    if (int rc = map_fetch_header(m)) return rc;
    if (m->host_hdr.n_points != prep.stored_before) m->built = false;
  } else {
    m->built = false;
  }
  return NDTPSO_OK;
}

int map_insert_device(ndtpso_map* m, const double2* d_xy, uint32_t n_upper, const uint32_t* d_n, const double* pose,
                      int accepted) {
  ndtpso_ctx* c = m->ctx;
  if (map_insert_skips(n_upper, accepted)) return NDTPSO_OK;
  InsertPrep prep;
  if (int rc = map_insert_prepare(m, n_upper, accepted, &prep)) return rc;
  const MapUpdateJob j = map_insert_job(m, d_xy, n_upper, d_n, pose);
  hipLaunchKernelGGL(k_map_insert, dim3(1), dim3(kInsertThreads), 0, c->stream, j.m, j.pts, j.n, j.n_ptr, j.do_trans, j.tc, j.ts,
                     j.ttx, j.tty);
  HIP_TRY(c, hipGetLastError());
  return map_insert_after(m, n_upper, prep);
}

// A speculative build in the same three steps (ndtpso_map_speculate_build, ndtpso_map_update_batch).
bool map_speculate_wanted(const ndtpso_map* m) { return !(m->spec || m->built); }

size_t map_undo_need(const ndtpso_map* m, unsigned long long points_upper) {
  const unsigned nc = (unsigned)std::min<unsigned long long>((unsigned long long)m->p.n_cells, points_upper);
  return sizeof(MapUndo) * (size_t)std::max(nc, 1u);
}

// the preparation would allocate (a device-wide synchronisation): the undo log for `points_upper` points, the pinned header
bool map_speculate_allocates(const ndtpso_map* m, unsigned long long points_upper) {
  return m->undo.cap < map_undo_need(m, points_upper) || !m->spec_hdr;
}

int map_speculate_prepare(ndtpso_map* m) {
  ndtpso_ctx* c = m->ctx;
  // (the bound grows by a scan's points per update until it reaches the grid's cells -- thirteen scans of 1081 points in a
  // 60 m frame of 0.5 m cells -- and a buffer sized to it was freed and allocated again at every one of them: a device-wide
  // synchronisation each, 17 - 38 ms for every replica of a process that runs 32.  Sized for the whole grid at once where that
  // is at most 64 MB, else in doublings.)
  {
    const size_t all = sizeof(MapUndo) * (size_t)std::max<unsigned>((unsigned)m->p.n_cells, 1u), need = map_undo_need(m, m->points_upper);
    if (m->undo.cap < need) HIP_TRY(c, m->undo.reserve(all <= (64u << 20) ? all : std::min(all, std::max(need, 2 * m->undo.cap))));
  }
  if (!m->spec_hdr) {
    HIP_TRY(c, hipHostMalloc((void**)&m->spec_hdr, 256, hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(m->spec_hdr, 0, 256);
  }
  return NDTPSO_OK;
}

// LDS of the map's pack launch: room for the whole grid's bitmap where that fits, else for as much as LDS holds
int map_pack_lds(const ndtpso_map* m) { return std::min(kCtrlBytes + m->n_words_max * 8, kMaxLds); }

void map_speculate_job(ndtpso_map* m, MapUpdateJob* j) {  // the build's and the pack's arguments; numbers the build
  j->m = m->p;
  j->undo = (MapUndo*)m->undo.p;
  j->image = (unsigned char*)m->image.p;
  j->mirror = m->spec_hdr;
  j->seq = ++m->spec_seq;
  j->cap_words = (map_pack_lds(m) - kCtrlBytes) / 8;
}

void map_speculate_after(ndtpso_map* m) {
  m->spec_prev_pts = m->build_pts;
  m->build_pts = m->points_upper;
  m->spec = true;
}

// One scan load, checked and described: ndtpso_points_load_scan's own launch and the shared one of ndtpso_points_load_scans
// take k_scan_to_resident's arguments from here.  `staged`: the job's ranges in pinned memory.
int scan_load_check(ndtpso_points* p, const float* ranges, const ndtpso_scan_geom* geom, int append, uint32_t* upper) {
  ndtpso_ctx* c = p->ctx;
  if (!ranges || !geom || geom->n_beams == 0) return fail(c, NDTPSO_E_ARG, "null argument");
  *upper = (append ? p->n_upper : 0u) + geom->n_beams;
  if (*upper > p->capacity) return fail(c, NDTPSO_E_CAPACITY, "resident scan capacity exceeded");
  return NDTPSO_OK;
}

int scan_load_job(ndtpso_points* p, const float* staged, const ndtpso_scan_geom* geom, const double trans[3], const ndtpso_grid* clip,
                  int append, ScanLoadJob* j) {
  std::memset(j, 0, sizeof(*j));
  const double zero[3] = {0., 0., 0.};
  const double* t = trans ? trans : zero;
  const CosSin cs = host_cos_sin(t[2]);
  if (int rc = make_scan(p->ctx, geom, &j->sp, &j->dirs)) return rc;
  j->ranges = staged;
  j->do_trans = trans_is_zero(t) ? 0 : 1;
  j->tc = cs.c;
  j->ts = cs.s;
  j->ttx = t[0];
  j->tty = t[1];
  j->clip_hw = clip ? clip->width / 2. : 0.;
  j->clip_hh = clip ? clip->height / 2. : 0.;
  j->out_xy = (double2*)p->xy.p;
  j->n_io = (uint32_t*)p->n_dev.p;
  j->append = append ? 1 : 0;
  j->capacity = (int)p->capacity;
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
  uint32_t upper = 0;
  if (int rc = scan_load_check(p, ranges, geom, append, &upper)) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  // the ranges go into a pinned slot and the kernel reads them there (4 KB, each read once): no copy operation
  void* staged = nullptr;
  int slot = 0;
  HIP_TRY(c, c->pinned.stage((size_t)geom->n_beams * 4, &staged, &slot, c->align_seen));
  std::memcpy(staged, ranges, (size_t)geom->n_beams * 4);
  ScanLoadJob j;
  if (int rc = scan_load_job(p, (const float*)staged, geom, trans, clip, append, &j)) return rc;
  hipLaunchKernelGGL(k_scan_to_resident, dim3(1), dim3(1024), kCtrlBytes, c->stream, j.ranges, j.sp, j.dirs, j.do_trans, j.tc, j.ts,
                     j.ttx, j.tty, j.clip_hw, j.clip_hh, j.out_xy, j.n_io, j.append, j.capacity);
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
  if (!map_speculate_wanted(m)) return NDTPSO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = map_speculate_prepare(m)) return rc;
  MapUpdateJob j;
  map_speculate_job(m, &j);
  if (int rc = map_enqueue_cells(m, j.undo)) return rc;
  if (int rc = map_enqueue_pack(m, j.mirror, j.seq)) return rc;  // (no event: the kernel publishes the header itself)
  map_speculate_after(m);
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
  if (int rc = check_mode(c, mode)) return rc;
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
  // (the probe only asks whether align_once will find the dense form for the upper bound: map_late_bound refuses the fp64 score)
  bool late = map_late_bound(m, mode, &src.wn);
  if (late) {
    const ScorePlan probe = resolve_score_plan(mode, src.g, src.wn, (int)src.n, cfg->population, prebuilt_table_ask());
    late = probe.ok && probe.plan.path == 2;
  }
  if (late) {
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
#include "ndtpso_map_update.inc"

extern "C" {

// cost_function (core.cpp:26-48) of the points of a loaded scan against the map, for m poses; builds first if points
// were inserted since the last build, like the reference.  Synchronous.
int ndtpso_map_cost(ndtpso_map* m, ndtpso_points* pts, const double* poses, uint32_t n_poses, int mode, double* costs) {
  if (!m || !pts) return NDTPSO_E_ARG;
  ndtpso_ctx* c = m->ctx;
  if (!poses || !costs || n_poses == 0) return fail(c, NDTPSO_E_ARG, "null argument");
  if (int rc = check_mode(c, mode)) return rc;
  if (mode == NDTPSO_SCORE_EXACT) mode = NDTPSO_SCORE_F64;  // a single cost: the exact mode is the fp64 score
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

}  // extern "C"

#include "ndtpso_map_search.inc"
#include "ndtpso_map_search_batch.inc"
#include "ndtpso_map_curvature.inc"
#include "ndtpso_map_trace.inc"

extern "C" {

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

#include "ndtpso_map_snapshot.inc"
