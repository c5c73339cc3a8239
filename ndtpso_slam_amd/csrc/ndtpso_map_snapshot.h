// ndtpso_map_snapshot.h -- the kernels' side of ndtpso_map_snapshot / ndtpso_map_restore (ndtpso_map_snapshot.inc): the sections
// of a staged blob as the kernels address them, and the host functions through which the rest of the library reaches the kernels,
// which are a translation unit of their own (ndtpso_map_snapshot.hip), as the job and search kernels are and for the same reason:
// nothing the kernels of the existing entries are compiled from changes.  Included behind ndtpso_map_device.inc (MapP, MapCell)
// by both units.
#ifndef NDTPSO_MAP_SNAPSHOT_H
#define NDTPSO_MAP_SNAPSHOT_H

// One created cell's entry of the blob's index section: which of its 100 window slots the blob holds (bit s of mask[s / 32]),
// and where the cell's slots and chunks begin in the slot and chunk sections -- exclusive prefix sums over the created list, in
// creation order.  k_snapshot_count leaves the cell's two COUNTS in slot_base / chunk_base; k_snapshot_scan turns them into offsets.
struct alignas(16) SnapCellIndex {
  uint32_t mask[4];
  unsigned long long slot_base, chunk_base;
};
static_assert(sizeof(SnapCellIndex) == 32, "blob index entry");

// The sections of a blob staged in device memory.  Slots: the used slots of cell 0 of the created list in slot order, then cell
// 1's, ...; chunks: chain by chain in the same order, 32 points each, the unused tail of a chain's last chunk zero.
struct SnapBlobP {
  int* created;
  MapCell* cells;
  SnapCellIndex* index;
  double2* win_sum;
  double4* win_cov;
  int* win_count;
  int* slot_len;
  double2* chunks;
  unsigned long long* og;  // the occupancy keys of the box, row by row: entry r * w + c is og_key[(x0 + c) + og_height * (y0 + r)]
};

// the occupancy box (MapHeader's og_min .. og_max; w == 0: no box) inside the map's key array
struct SnapOgP {
  unsigned long long* og_key;
  uint32_t og_height, og_count, x0, y0, w, h;
};

constexpr int kSnapTotals = 3;  // k_snapshot_count / k_snapshot_scan: {used slots, chunks, stored points} of the whole map

// n_created > 0 everywhere.  `map_p`: the map's MapP (a type without linkage: each unit has its own, from the same text).  `index`: n_created entries; `totals`: kSnapTotals words, zero before the count.
__attribute__((visibility("hidden"))) void snapshot_count_launch(hipStream_t stream, const void* map_p, unsigned n_created, SnapCellIndex* index,
                                                                 unsigned long long* totals);
__attribute__((visibility("hidden"))) void snapshot_scan_launch(hipStream_t stream, unsigned n_created, SnapCellIndex* index,
                                                                unsigned long long* totals);
__attribute__((visibility("hidden"))) void snapshot_gather_launch(hipStream_t stream, const void* map_p, unsigned n_created,
                                                                  const SnapCellIndex* index, const SnapBlobP& blob, const SnapOgP& og);
// into a map that map_clear has just left; the blob's index and lengths have been checked by the host (snap_validate)
__attribute__((visibility("hidden"))) void restore_scatter_launch(hipStream_t stream, const void* map_p, unsigned n_created, const SnapBlobP& blob,
                                                                  const SnapOgP& og);

#endif
