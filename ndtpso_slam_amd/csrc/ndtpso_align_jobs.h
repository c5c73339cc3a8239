// ndtpso_align_jobs.h -- the job kernels' side of ndtpso_map_align_batch (ndtpso_map_batch.inc): the descriptor of one job and
// the two host functions through which the rest of the library reaches k_align_jobs, which is compiled as a translation unit of
// its own (ndtpso_align_jobs.hip).  Included behind ndtpso_device_common.inc (Layout) by both translation units.
#ifndef NDTPSO_ALIGN_JOBS_H
#define NDTPSO_ALIGN_JOBS_H

// One alignment of a launch of several (ndtpso_map_align_batch): everything k_align takes as kernel arguments and that differs
// from one alignment to the next.  The host writes a table of these into a pinned staging slot; the kernel reads its entry in
// place.  (`guess` points at [guess | deviation], as the single path's staged inputs do.)
struct AlignJob {
  const unsigned char* image;
  const double2* xy;
  const uint32_t* n_ptr;
  const double* guess;
  const int4* table_src;   // the job's rand() table in the staging slot, nullptr: the device replays srand(seed)
  int4* table_dst;         // its copies in HBM, one per workgroup of the job's cluster
  double* out;             // [pose | cost | AlignStats] in HBM
  double* mirror;          // the job's pinned result slot
  const uint32_t* late_hdr;
  GridP g;
  WinP wn;
  Layout L;
  DenseP dn;
  int n, late_table_cap, late_rec_cap, spec_off;
  uint32_t seed, seq;
  int want_cost, pad[3];
};
static_assert(sizeof(AlignJob) % 16 == 0, "job descriptors are read with wide uniform loads");

// kind: 0 fp32 score on the dense table, 1 the same arbitrating (exact mode), 2 the fp64 score on the bitmap of power-of-two
// cells; cluster: a cluster of cl.K workgroups per job, else one workgroup.  `jobs`: AlignJob[], readable by the device.
__attribute__((visibility("hidden"))) hipError_t align_jobs_allow_big_lds();
__attribute__((visibility("hidden"))) void align_jobs_launch(int kind, bool cluster, unsigned grid, unsigned threads, int lds_bytes,
                                                             hipStream_t stream, const void* jobs, const ndtpso::PsoP& ps,
                                                             const ndtpso::ClusterP& cl, int table_vec);

#endif
