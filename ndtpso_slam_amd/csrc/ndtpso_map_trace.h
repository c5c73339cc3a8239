// ndtpso_map_trace.h -- the kernels' side of ndtpso_map_trace / ndtpso_map_trace_batch / ndtpso_map_get_nav_grid
// (ndtpso_map_trace.inc): the descriptor of one job of a launch, the totals a map keeps on the device, and the host functions
// through which the rest of the library reaches the kernels, which are a translation unit of their own (ndtpso_map_trace.hip)
// for the reason ndtpso_map_search.hip is one: nothing the kernels of the existing entries are compiled from changes.  Needs
// only the HIP runtime's types.
#ifndef NDTPSO_MAP_TRACE_H
#define NDTPSO_MAP_TRACE_H

// What a traced map keeps on the device besides the two counter arrays: ndtpso_trace_info's extent and totals.
struct alignas(16) TraceTotals {
  unsigned long long n_rays, n_skipped, n_steps;
  uint32_t min_x, max_x, min_y, max_y;
  unsigned long long pad;
};
static_assert(sizeof(TraceTotals) == 48, "TraceTotals is uploaded and downloaded as it stands");

// One job of a launch: a scan, the pose it was taken at and the map's counters.  The host writes a table of these into a pinned
// staging block; the kernel reads its entry in place, with wave-uniform loads.  Column x of the launch's grid is job x; the column is
// as long as the launch's largest scan needs, and a job's spare workgroups leave at once.
struct alignas(16) TraceJob {
  const double2* xy;
  const uint32_t* n_ptr;  // the scan's count on the device; n: the host's upper bound of it
  uint32_t* hits;
  unsigned long long* passes;
  TraceTotals* tot;
  double theta, tx, ty;  // the pose
  double hw, hh, cs;     // width / 2., height / 2., og_cell_size
  uint32_t og_height, og_count, n, reserved;
};
static_assert(sizeof(TraceJob) % 16 == 0, "job descriptors are read with wide uniform loads");

constexpr unsigned kTraceThreads = 256;

// `jobs`: TraceJob[n_jobs], readable by the device; blocks_y: the largest job's ceil(n / kTraceThreads), 1 .. 65535.
// aggregate: a workgroup adds its rays' passes of the origin's cell with one atomic (0: every lane its own; same counters).
__attribute__((visibility("hidden"))) hipError_t trace_jobs_launch(hipStream_t stream, const void* jobs, unsigned n_jobs, unsigned blocks_y,
                                                                   int aggregate);
// grid[at] for at < og_count from the occupancy keys and the counters (hits == nullptr: a map never traced), ndtpso_map_get_nav_grid's rule
__attribute__((visibility("hidden"))) hipError_t nav_grid_launch(hipStream_t stream, const unsigned long long* og_key, const uint32_t* hits,
                                                                 const unsigned long long* passes, uint32_t og_count, int8_t* grid);

#endif
