// ndtpso_map_snapshot.inc -- a resident map saved to a blob and restored bit for bit (ndtpso_map_snapshot_size, ndtpso_map_snapshot,
// ndtpso_map_restore, ndtpso_snapshot_describe).  The host lays out, checks and copies; what is gathered and scattered is the
// kernels' work (ndtpso_map_snapshot.hip).  Included at the end of ndtpso_map.inc's entries (same translation unit: ndtpso_map).
//
// Primary state -- what the blob holds, for what the map actually contains: the created list in creation order, a MapCell per
// created cell, per cell the used window slots (win_sum, win_cov, win_count, slot_len), every stored point chain by chain in
// insertion order, the MapHeader, the occupancy keys inside the header's og_min .. og_max box (the kernel that writes a key
// widens the box in the same thread, so nothing non-zero lies outside it), and the host's fields that decide later behaviour:
// built, builds (part of every occupancy key), points_upper, chunks_bound, build_pts.
// Derived state -- what it leaves out: the alignment table image, which k_map_pack rebuilds from the cells when `built` is set.
// Chunk ids are not state: the blob numbers chunks consecutively in (created order, slot order, chain order), and a restored pool
// has pool_bump = n_chunks and pool_free = 0.  Later inserts may take other ids than the original's would; no result depends on a
// chunk's number, only on the chain's order.
// The created list IS state and is saved as it stands: the cells one insert creates enter it in the order that insert's atomics
// landed (k_map_insert), so two maps accumulated apart from the same scans may list them differently -- and give blobs that
// differ there and hold the same cells.  No result depends on the order either (build, occupancy and pack are per cell; the
// exports sort by index); a restored map keeps its blob's order, which is what makes snapshot(restore(blob)) == blob.
//
// Format 1 (little-endian, every section 16-byte aligned, 64-bit sizes and offsets):
//   SnapHeader | created int32[n] | cells MapCell[n] | index SnapCellIndex[n] | win_sum 16 B[s] | win_cov 32 B[s] |
//   win_count int32[s] | slot_len int32[s] | chunks 512 B[c] | og keys uint64[box]
// checksum: FNV-1a over the 64-bit words behind the header; header_checksum: the same over the header with both fields zero.

namespace {

constexpr char kSnapMagic[8] = {'N', 'D', 'T', 'P', 'S', 'O', 'M', 'P'};
constexpr uint32_t kSnapVersion = 1;
enum { kSecCreated, kSecCells, kSecIndex, kSecWinSum, kSecWinCov, kSecWinCount, kSecSlotLen, kSecChunks, kSecOg, kSnapSections };
const char* const kSnapSectionName[kSnapSections] = {"off_created", "off_cells", "off_index", "off_win_sum", "off_win_cov",
                                                     "off_win_count", "off_slot_len", "off_chunks", "off_og"};

struct SnapHeader {
  char magic[8];
  uint32_t version, header_bytes;
  uint32_t window_size, max_points_per_cell, chunk_points, sizeof_cell;
  uint64_t bytes, checksum;
  uint16_t grid_width, grid_height;
  uint32_t built;
  double cell_side, og_cell_size;
  uint32_t n_created, reserved0;
  uint64_t n_slots_used, n_chunks, n_points_stored, og_box_entries;
  uint64_t builds, points_upper, chunks_bound, build_pts;
  MapHeader map;  // pool_bump = n_chunks, pool_free = 0
  uint64_t off[kSnapSections];
  uint64_t header_checksum;
  uint64_t reserved[4];
};
static_assert(sizeof(SnapHeader) == 320 && sizeof(SnapHeader) % 16 == 0, "snapshot header layout");
static_assert(offsetof(SnapHeader, bytes) == NDTPSO_SNAPSHOT_BYTES_OFFSET && offsetof(SnapHeader, cell_side) == 56 && offsetof(SnapHeader, map) == 144 &&
                  offsetof(SnapHeader, off) == 208,
              "snapshot header layout");

uint64_t snap_fnv1a(const void* p, size_t bytes, uint64_t h = 0xcbf29ce484222325ull) {  // over 64-bit words; bytes % 8 == 0
  const unsigned char* s = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i + 8 <= bytes; i += 8) {
    uint64_t w;
    std::memcpy(&w, s + i, 8);
    h = (h ^ w) * 0x100000001b3ull;
  }
  return h;
}

uint64_t snap_header_checksum(SnapHeader h) {
  h.checksum = 0;
  h.header_checksum = 0;
  return snap_fnv1a(&h, sizeof(h));
}

uint64_t snap_align16(uint64_t v) { return (v + 15u) & ~15ull; }

// the one layout rule: the section offsets and the blob's size from the header's counts
uint64_t snap_layout(const SnapHeader& h, uint64_t off[kSnapSections]) {
  const uint64_t n = h.n_created, s = h.n_slots_used;
  const uint64_t size[kSnapSections] = {4 * n, sizeof(MapCell) * n, sizeof(SnapCellIndex) * n, 16 * s, 32 * s, 4 * s, 4 * s,
                                        (uint64_t)kChunk * 16 * h.n_chunks, 8 * h.og_box_entries};
  uint64_t at = sizeof(SnapHeader);
  for (int k = 0; k < kSnapSections; ++k) {
    off[k] = at;
    at = snap_align16(at + size[k]);
  }
  return at;
}

// the occupancy box a header describes, in entries (0: no grid, or nothing rasterised yet)
uint64_t snap_og_entries(const MapHeader& h, bool has_grid) {
  if (!has_grid || h.og_min_x > h.og_max_x || h.og_min_y > h.og_max_y) return 0;
  return ((uint64_t)h.og_max_x - h.og_min_x + 1) * ((uint64_t)h.og_max_y - h.og_min_y + 1);
}

ndtpso_grid snap_grid(const SnapHeader& h) {
  ndtpso_grid g{};
  g.width = h.grid_width;
  g.height = h.grid_height;
  g.cell_side = h.cell_side;
  return g;
}

size_t snap_pool_chunks(uint64_t pool_bytes) {  // ndtpso_map_create's rule
  if (pool_bytes == 0) pool_bytes = 1ull << 30;
  return std::max<size_t>(64, (size_t)(pool_bytes / (kChunk * 16)));
}

// Everything a restore relies on, checked on the host before any device memory is touched: the kernels then index with what the
// blob says.  `why` names the field that is wrong.
int snap_validate(const void* blob, uint64_t bytes, SnapHeader* out, std::string* why) {
  auto bad = [&](const char* field) {
    *why = std::string("snapshot: bad ") + field;
    return NDTPSO_E_ARG;
  };
  if (!blob || bytes < sizeof(SnapHeader)) return bad("bytes (shorter than the header)");
  SnapHeader h;
  std::memcpy(&h, blob, sizeof(h));
  if (std::memcmp(h.magic, kSnapMagic, 8) != 0) return bad("magic");
  if (h.version != kSnapVersion) return bad("version");
  if (h.header_bytes != sizeof(SnapHeader)) return bad("header_bytes");
  if (h.window_size != (uint32_t)NDTPSO_WINDOW_SIZE) return bad("window_size (NDTPSO_WINDOW_SIZE)");
  if (h.max_points_per_cell != (uint32_t)NDTPSO_MAX_POINTS_PER_CELL) return bad("max_points_per_cell (NDTPSO_MAX_POINTS_PER_CELL)");
  if (h.chunk_points != (uint32_t)kChunk) return bad("chunk_points");
  if (h.sizeof_cell != sizeof(MapCell)) return bad("sizeof_cell");
  if (h.header_checksum != snap_header_checksum(h)) return bad("header_checksum");
  const ndtpso_grid grid = snap_grid(h);
  GridP g;
  if (make_grid(&grid, &g) != NDTPSO_OK) return bad("grid");
  const uint64_t n_cells = (uint64_t)g.W * g.H;
  if (n_cells >= (1u << 21)) return bad("grid (2^21 cells or more)");
  if (!(h.og_cell_size >= 0.) || !std::isfinite(h.og_cell_size)) return bad("og_cell_size");
  if (h.built > 1) return bad("built");
  if (h.n_created > n_cells || h.map.n_created != h.n_created) return bad("n_created");
  if (h.n_slots_used > (uint64_t)h.n_created * kWinSlots) return bad("n_slots_used");
  if (h.n_chunks > (uint64_t)INT_MAX || h.map.pool_bump != (int32_t)h.n_chunks || h.map.pool_free != 0) return bad("n_chunks");
  if (h.map.status & kMapPoolExhausted) return bad("map.status (the point pool had run out)");
  if (h.og_box_entries != snap_og_entries(h.map, h.og_cell_size > 0.)) return bad("og_box_entries");
  if (h.og_box_entries > (1ull << 34)) return bad("og_box_entries");
  uint64_t off[kSnapSections];
  const uint64_t total = snap_layout(h, off);
  for (int k = 0; k < kSnapSections; ++k)
    if (h.off[k] != off[k]) return bad(kSnapSectionName[k]);
  if (h.bytes != total || bytes != total) return bad("bytes");
  const unsigned char* base = static_cast<const unsigned char*>(blob);
  if (h.checksum != snap_fnv1a(base + sizeof(SnapHeader), (size_t)(total - sizeof(SnapHeader)))) return bad("checksum");
  // count consistency: the index is the running sum of its own masks and of the lengths, n_chunks == sum ceil(slot_len / 32)
  std::vector<bool> seen((size_t)n_cells, false);
  uint64_t slots = 0, chunks = 0, points = 0;
  for (uint64_t t = 0; t < h.n_created; ++t) {
    int32_t ci;
    SnapCellIndex ix;
    std::memcpy(&ci, base + off[kSecCreated] + 4 * t, 4);
    std::memcpy(&ix, base + off[kSecIndex] + sizeof(ix) * t, sizeof(ix));
    if (ci < 0 || (uint64_t)ci >= n_cells || seen[(size_t)ci]) return bad("created[]");
    seen[(size_t)ci] = true;
    if (ix.mask[3] >> (kWinSlots - 96)) return bad("index[].mask");
    if (ix.slot_base != slots || ix.chunk_base != chunks) return bad("index[] (not the running sums)");
    const uint64_t used = (uint64_t)(__builtin_popcount(ix.mask[0]) + __builtin_popcount(ix.mask[1]) + __builtin_popcount(ix.mask[2]) +
                                     __builtin_popcount(ix.mask[3]));
    if (slots + used > h.n_slots_used) return bad("n_slots_used");
    for (uint64_t k = slots; k < slots + used; ++k) {
      int32_t len;
      std::memcpy(&len, base + off[kSecSlotLen] + 4 * k, 4);
      if (len < 0) return bad("slot_len[]");
      chunks += ((uint64_t)len + kChunk - 1) / kChunk;
      points += (uint64_t)len;
    }
    slots += used;
  }
  if (slots != h.n_slots_used) return bad("n_slots_used");
  if (chunks != h.n_chunks) return bad("n_chunks (not the sum of ceil(slot_len / 32))");
  if (points != h.n_points_stored) return bad("n_points_stored");
  *out = h;
  return NDTPSO_OK;
}

SnapBlobP snap_sections(void* staged, const uint64_t off[kSnapSections]) {  // `staged`: a blob's image in device memory
  unsigned char* d = static_cast<unsigned char*>(staged);
  SnapBlobP b;
  b.created = reinterpret_cast<int*>(d + off[kSecCreated]);
  b.cells = reinterpret_cast<MapCell*>(d + off[kSecCells]);
  b.index = reinterpret_cast<SnapCellIndex*>(d + off[kSecIndex]);
  b.win_sum = reinterpret_cast<double2*>(d + off[kSecWinSum]);
  b.win_cov = reinterpret_cast<double4*>(d + off[kSecWinCov]);
  b.win_count = reinterpret_cast<int*>(d + off[kSecWinCount]);
  b.slot_len = reinterpret_cast<int*>(d + off[kSecSlotLen]);
  b.chunks = reinterpret_cast<double2*>(d + off[kSecChunks]);
  b.og = reinterpret_cast<unsigned long long*>(d + off[kSecOg]);
  return b;
}

SnapOgP snap_og_box(const ndtpso_map* m, const SnapHeader& h) {
  SnapOgP og{};
  og.og_key = (unsigned long long*)m->og_key.p;
  og.og_height = m->og_height;
  og.og_count = m->og_count;
  if (h.og_box_entries) {
    og.x0 = h.map.og_min_x;
    og.y0 = h.map.og_min_y;
    og.w = h.map.og_max_x - h.map.og_min_x + 1;
    og.h = h.map.og_max_y - h.map.og_min_y + 1;
  }
  return og;
}

constexpr size_t kSnapIndexAt = 64;  // ndtpso_map::snap_idx: the totals, and at this byte the index

// Settles the map, counts what it holds and scans the counts into offsets (left in m->snap_idx); fills the header but for the
// two checksums.  Synchronous.
int snap_measure(ndtpso_map* m, SnapHeader* h) {
  ndtpso_ctx* c = m->ctx;
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = map_settle(m)) return rc;
  if (int rc = map_fetch_header(m)) return rc;  // (a map whose pool ran out has lost points: refused, NDTPSO_E_CAPACITY)
  const MapHeader& mh = m->host_hdr;
  const unsigned n = std::min<unsigned>(mh.n_created, (unsigned)m->p.n_cells);
  unsigned long long totals[kSnapTotals] = {0, 0, 0};
  if (n) {
    HIP_TRY(c, m->snap_idx.reserve(kSnapIndexAt + sizeof(SnapCellIndex) * (size_t)n));
    unsigned long long* d_totals = (unsigned long long*)m->snap_idx.p;
    SnapCellIndex* d_index = reinterpret_cast<SnapCellIndex*>((unsigned char*)m->snap_idx.p + kSnapIndexAt);
    HIP_TRY(c, hipMemsetAsync(d_totals, 0, kSnapIndexAt, c->stream));
    snapshot_count_launch(c->stream, &m->p, n, d_index, d_totals);
    HIP_TRY(c, hipGetLastError());
    snapshot_scan_launch(c->stream, n, d_index, d_totals);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(totals, d_totals, sizeof(totals), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  std::memset(h, 0, sizeof(*h));
  std::memcpy(h->magic, kSnapMagic, 8);
  h->version = kSnapVersion;
  h->header_bytes = (uint32_t)sizeof(SnapHeader);
  h->window_size = NDTPSO_WINDOW_SIZE;
  h->max_points_per_cell = NDTPSO_MAX_POINTS_PER_CELL;
  h->chunk_points = kChunk;
  h->sizeof_cell = (uint32_t)sizeof(MapCell);
  h->grid_width = m->grid.width;
  h->grid_height = m->grid.height;
  h->cell_side = m->grid.cell_side;
  h->og_cell_size = m->og_cell_size;
  h->built = m->built ? 1u : 0u;
  h->n_created = n;
  h->n_slots_used = totals[0];
  h->n_chunks = totals[1];
  h->n_points_stored = totals[2];
  h->builds = m->builds;
  h->points_upper = m->points_upper;
  h->chunks_bound = m->chunks_bound;
  h->build_pts = m->build_pts;
  h->map = mh;
  h->map.n_created = n;
  h->map.pool_bump = (int32_t)h->n_chunks;
  h->map.pool_free = 0;
  if (!m->built) {
    // the header's table fields describe the last pack, and a pack is derived state: with points inserted since, nothing reads
    // them before the next build's pack rewrites them -- and a speculative build that was taken back has left ITS values there
    // (k_map_undo restores cells and window terms, not these).  An unbuilt map is saved without them, so that the settled map
    // and the map that never speculated give the same bytes.
    h->map.n_built = h->map.n_words = 0;
    h->map.x0 = h->map.x1 = h->map.y0 = h->map.y1 = 0;
  }
  h->og_box_entries = snap_og_entries(h->map, m->og_count != 0);
  h->bytes = snap_layout(*h, h->off);
  return NDTPSO_OK;
}

void snap_release(ndtpso_map* m) {  // the staged blob is as large as the map's content: not kept between calls
  m->snap.release();
  m->snap_idx.release();
}

void snap_info(const SnapHeader& h, ndtpso_snapshot_info* info) {
  std::memset(info, 0, sizeof(*info));
  info->version = h.version;
  info->n_created = h.n_created;
  info->n_built = h.map.n_built;
  info->built = h.built;
  info->n_slots_used = h.n_slots_used;
  info->n_chunks = h.n_chunks;
  info->n_points_stored = h.n_points_stored;
  info->og_box_entries = h.og_box_entries;
  info->bytes = h.bytes;
  info->grid = snap_grid(h);
  info->og_cell_size = h.og_cell_size;
}

}  // namespace

extern "C" {

int ndtpso_map_snapshot_size(ndtpso_map* m, uint64_t* bytes) {
  if (!m) return NDTPSO_E_ARG;
  if (!bytes) return fail(m->ctx, NDTPSO_E_ARG, "null argument");
  SnapHeader h;
  const int rc = snap_measure(m, &h);
  snap_release(m);
  if (rc == NDTPSO_OK) *bytes = h.bytes;
  return rc;
}

int ndtpso_map_snapshot(ndtpso_map* m, void* blob, uint64_t capacity, uint64_t* bytes) {
  if (!m) return NDTPSO_E_ARG;
  ndtpso_ctx* c = m->ctx;
  if (!bytes || (!blob && capacity)) return fail(c, NDTPSO_E_ARG, "null argument");
  SnapHeader h;
  int rc = snap_measure(m, &h);
  if (rc == NDTPSO_OK) {
    *bytes = h.bytes;
    if (capacity < h.bytes) rc = fail(c, NDTPSO_E_CAPACITY, "snapshot: capacity is smaller than the blob (bytes says how large)");
  }
  if (rc == NDTPSO_OK) rc = [&]() -> int {
    unsigned char* out = static_cast<unsigned char*>(blob);
    const size_t body = (size_t)(h.bytes - sizeof(SnapHeader));
    if (h.n_created) {
      // staged in one device buffer (the header's place stays empty, so that a section's offset is the same in both), the padding
      // between sections zero; one copy brings it to the host
      HIP_TRY(c, m->snap.reserve((size_t)h.bytes));
      HIP_TRY(c, hipMemsetAsync(m->snap.p, 0, (size_t)h.bytes, c->stream));
      const SnapCellIndex* d_index = reinterpret_cast<const SnapCellIndex*>((const unsigned char*)m->snap_idx.p + kSnapIndexAt);
      snapshot_gather_launch(c->stream, &m->p, h.n_created, d_index, snap_sections(m->snap.p, h.off), snap_og_box(m, h));
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, hipMemcpyAsync(out + sizeof(SnapHeader), (const unsigned char*)m->snap.p + sizeof(SnapHeader), body,
                                hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    } else if (body) {
      std::memset(out + sizeof(SnapHeader), 0, body);
    }
    h.checksum = snap_fnv1a(out + sizeof(SnapHeader), body);
    h.header_checksum = snap_header_checksum(h);
    std::memcpy(out, &h, sizeof(h));
    return NDTPSO_OK;
  }();
  snap_release(m);
  return rc;
}

int ndtpso_map_restore(ndtpso_ctx* c, const void* blob, uint64_t bytes, uint64_t pool_bytes, ndtpso_map** out) {
  if (!c || !out) return fail(c, NDTPSO_E_ARG, "null argument");
  *out = nullptr;
  SnapHeader h;
  std::string why;
  if (int rc = snap_validate(blob, bytes, &h, &why)) return fail(c, rc, why);
  if (h.n_chunks > snap_pool_chunks(pool_bytes))
    return fail(c, NDTPSO_E_CAPACITY, "snapshot: pool_bytes is too small for the blob's n_chunks");
  const ndtpso_grid grid = snap_grid(h);
  ndtpso_map* m = nullptr;
  if (int rc = ndtpso_map_create(c, &grid, h.og_cell_size, pool_bytes, &m)) return rc;  // (leaves a cleared map)
  const int rc = [&]() -> int {
    m->host_hdr = h.map;
    if (h.n_created) {
      const size_t body = (size_t)(h.bytes - sizeof(SnapHeader));
      HIP_TRY(c, m->snap.reserve((size_t)h.bytes));
      HIP_TRY(c, hipMemcpyAsync((unsigned char*)m->snap.p + sizeof(SnapHeader), static_cast<const unsigned char*>(blob) + sizeof(SnapHeader),
                                body, hipMemcpyHostToDevice, c->stream));
      restore_scatter_launch(c->stream, &m->p, h.n_created, snap_sections(m->snap.p, h.off), snap_og_box(m, h));
      HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipMemcpyAsync(m->hdr.p, &m->host_hdr, sizeof(MapHeader), hipMemcpyHostToDevice, c->stream));
    m->built = h.built != 0;
    m->builds = h.builds;
    m->points_upper = h.points_upper;
    m->chunks_bound = h.chunks_bound;
    m->build_pts = h.build_pts;
    // the alignment table is derived: packed again from the cells, as the build that set `built` packed it
    if (m->built)
      if (int prc = map_enqueue_pack(m)) return prc;
    if (int frc = map_fetch_header(m)) return frc;  // synchronises: the caller's blob and the staged copy are done with
    if (!m->built) m->known_pts = ~0ull;  // (an unbuilt map's table fields were not saved: no bound for late window binding yet)
    return NDTPSO_OK;
  }();
  snap_release(m);
  if (rc != NDTPSO_OK) {
    const std::string err = c->err;
    ndtpso_map_destroy(m);
    c->err = err;
    return rc;
  }
  *out = m;
  return NDTPSO_OK;
}

int ndtpso_snapshot_describe(const void* blob, uint64_t bytes, ndtpso_snapshot_info* info) {
  if (!info) return NDTPSO_E_ARG;
  SnapHeader h;
  std::string why;
  if (int rc = snap_validate(blob, bytes, &h, &why)) return rc;
  snap_info(h, info);
  return NDTPSO_OK;
}

}  // extern "C"
