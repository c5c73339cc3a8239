// ndtpso_map_search_jobs.h -- the kernels' side of ndtpso_map_search_batch (ndtpso_map_search_batch.inc): the descriptors of the
// jobs of a shared launch and the host functions through which the rest of the library reaches the job kernels, which are a
// translation unit of their own (ndtpso_map_search_jobs.hip) for the reason ndtpso_align_jobs.hip is one: nothing the kernels of
// the existing entries are compiled from changes.  Included behind ndtpso_device_common.inc (Layout) and ndtpso_map_search.h
// (LatticeP, SearchKey) by both units.
#ifndef NDTPSO_MAP_SEARCH_JOBS_H
#define NDTPSO_MAP_SEARCH_JOBS_H

// One lattice of a launch of several: the fields of SweepArgs, and how the launch's workgroups are dealt to it.  The host writes
// a table of these into a pinned staging block; the kernel reads its entry in place, with wave-uniform loads.
//   - A launch has `n_shares` SHARES (the sweep's second argument).  A job owns `share` consecutive ones from `share0` on; share
//     s of a job takes the job's items s, s + share, ...  Workgroup b takes the shares b, b + grid, ...: with fewer jobs than
//     workgroups every workgroup has one share, and a job has shares in proportion to its items; with more, a share is a whole
//     job.  A workgroup stages a job's table once per share.
//   - k_lattice_cost_jobs (the exact mode's rescoring) reads the same descriptor: not the lattice but the nodes listed at
//     cand[0 .. cand_hdr[0]) -- k_lattice_collect_jobs' output of the same call -- are scored, candidate e into out[e] =
//     {cost, node}; share s of a job takes the candidates s, s + share, ... one wave each.  A list that the host will not use
//     (cand_hdr[1] != 0: a NaN cost; cand_hdr[0] > cand_cap) is skipped.
struct alignas(16) SweepJob {
  const unsigned char* image;
  const double2* xy;
  double* costs;         // the job's place in the shared cost buffer: one per node
  const uint32_t* cand;  // k_lattice_cost_jobs: the nodes to score, [count, NaNs] at cand_hdr
  const uint32_t* cand_hdr;
  SearchKey* out;        // ... and their fp64 costs, in pinned host memory
  ndtpso::GridP g;
  ndtpso::WinP wn;
  Layout L;
  ndtpso::DenseP dn;
  LatticeP lat;
  int n;
  uint32_t share0, share, cand_cap;
};
static_assert(sizeof(SweepJob) % 16 == 0, "job descriptors are read with wide uniform loads");

// One workgroup of a selection launch: the best k of its part, in order, into keys[out ...] (k_lattice_select's rule).
// First stage: nodes [lo, hi) of the job whose costs begin at costs[src]; the keys carry the node's number within the job.
// Second stage: the valid ones of keys[src + lo .. src + hi), the first stage's lists of one job.
struct SelectPart {
  uint32_t src, lo, hi, k, out, job, pad[2];
};
static_assert(sizeof(SelectPart) == 32, "part descriptors are read with wide uniform loads");

// What the collect kernel knows of a job: where its K-th key lies, how many points its scan has, where its candidates go
// (cand[hdr] = count, cand[hdr + 1] = NaNs, both zero before the launch; cand[list ...] = nodes, `cap` at most).
struct CollectJob {
  uint32_t kth, n_points, hdr, list, cap, pad[3];
};

// mode: kScoreF32 / kScoreF64; path: Plan::path (0, 1, 4, 5; fp32 also 2).  `jobs`: SweepJob[] of that kind, `share_job`: the job of
// every share; both readable by the device.  lds_bytes: the largest job's.
__attribute__((visibility("hidden"))) hipError_t search_jobs_sweep_launch(int mode, int path, unsigned grid, int lds_bytes, hipStream_t stream,
                                                                          const void* jobs, const uint32_t* share_job, uint32_t n_shares);
// the fp64 score of the jobs' collected candidates; path: the fp64 plan's (0, 1, 4, 5)
__attribute__((visibility("hidden"))) hipError_t search_jobs_cost_launch(int path, unsigned grid, int lds_bytes, hipStream_t stream,
                                                                         const void* jobs, const uint32_t* share_job, uint32_t n_shares);
// both stages of the selection, one launch each: n_first first-stage parts, then n_second (one per job)
__attribute__((visibility("hidden"))) hipError_t search_jobs_select_launch(hipStream_t stream, const double* costs, void* keys, const void* first,
                                                                           uint32_t n_first, const void* second, uint32_t n_second);
// the exact mode's candidates of every job whose K-th fp32 cost is a number below -kTinyCost: the nodes with
// c32 <= c32_K + kArbAbsPerPoint * n_points (the host's two operations), over the first stage's parts
__attribute__((visibility("hidden"))) hipError_t search_jobs_collect_launch(hipStream_t stream, const double* costs, const void* keys,
                                                                            const void* parts, uint32_t n_parts, const void* jobs,
                                                                            uint32_t* cand);

#endif
