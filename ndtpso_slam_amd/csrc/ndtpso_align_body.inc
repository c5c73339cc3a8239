// ndtpso_align_body.inc -- one alignment against a prebuilt table image by the calling workgroup (or by the workgroup's cluster):
// the body of k_align, where the alignment's inputs are the kernel's arguments, and of k_align_jobs, where they are locals of the
// same names filled in from the job's descriptor.  Included TEXTUALLY by both (ndtpso_hip.hip), like ndtpso_pairs_body.inc: the
// same text as an inlined function cost a kernel 6 % (DESIGN 3.3), and k_align keeps the machine code it had when the text stood
// in the kernel itself (scripts/kernel_isa_diff.py).
// In scope: image, xy, n, n_ptr, g, wn, L, dn, ps, guess, dev, seed, table, ws, out_pose, out_cost, stats, cl (placed: cl.rank,
// cl.spec and, in a launch of several clusters, cl.xc are this workgroup's), mirror, table_src, table_dst, table_vec, late_hdr,
// late_table_cap, late_rec_cap, seq.
  if (CLUSTER && cl.rank == cl.absent) return;
  // The rand() table in a pinned HOST slot (table_src; ndtpso_map_align): fetched in one sweep into this workgroup's
  // own copy in HBM, the loads in flight together -- one trip over the host link instead of a copy operation ahead of
  // the kernel.  (Read in place, an iteration's draws one iteration ahead, the trips were not hidden: the memory counter
  // retires in order, so every later load waited for them; 66 us per alignment.)  The first reader comes after the
  // barrier below.
  const int32_t* draws_table = table;
  if (table_src) {
    int4* dst = table_dst + (size_t)cl.rank * (size_t)table_vec;
    for (int q = (int)threadIdx.x; q < table_vec; q += (int)blockDim.x) dst[q] = table_src[q];
    draws_table = reinterpret_cast<const int32_t*>(dst);
  }
  if (threadIdx.x == 0 && cl.rank == 0 && stats) *stats = AlignStats{0, 0, 0, 0, 0, 0, 0, 0};  // only this workgroup writes it
  if constexpr (PATH == 2) {
    if (late_hdr) {  // late window binding (AlignSrc::late_hdr): uniform, and the same in every workgroup of a cluster
      const int nb = (int)late_hdr[1], x0 = (int)late_hdr[4], x1 = (int)late_hdr[5], y0 = (int)late_hdr[6], y1 = (int)late_hdr[7];
      wn.x0 = x0;
      wn.y0 = y0;
      wn.w = x1 - x0 + 1;
      wn.h = y1 - y0 + 1;
      wn.n_words = (int)late_hdr[3];
      wn.rec_cap = max(nb, 1);
      dn.dw = wn.w + 1;
      dn.dh = wn.h + 1;
      dn.ox = x0 - 1;
      dn.oy = y0 - 1;
      dense_set_limits(dn, g.hw, g.hh, g.inv_cs);
      if (dense_entries(dn.dw, dn.dh) > late_table_cap || wn.rec_cap > late_rec_cap) {
        if (threadIdx.x == 0 && cl.rank == 0 && stats) {
          stats->status = kStatusLateOverflow;
          if (mirror) {
            reinterpret_cast<AlignStats*>(mirror + 4)->status = kStatusLateOverflow;
            publish_pinned_word(reinterpret_cast<uint32_t*>(mirror + 8), seq);
          }
        }
        return;
      }
    }
  }
  if (n_ptr) n = min((int)*n_ptr, n);  // the point count lives on the device (resident scan); n is its capacity
  double2* pts = reinterpret_cast<double2*>(g_lds + L.pts_off);
  stage_image<MODE, PATH>(image, g, wn, L, dn);
  copy16(pts, xy, n * 16);
  pad_points_wg(pts, n);
  __syncthreads();
  EvalCtx E = PATH >= 4 ? make_eval_ctx_global(g, wn, dn, image) : make_eval_ctx(g, wn, L, dn);
  E.light = CLUSTER ? 0 : ps.light;
  if constexpr (ARB) enable_arbitration<PATH == 3>(lds_ctrl(L.ctrl_off), g, wn, dn, image, L);  // exact mode: the staged image holds the fp64 records
  // a swarm too large for LDS lives in an HBM workspace, one per workgroup of a cluster (each keeps the whole swarm)
  // Two copies of the PSO, one per home of the swarm, so that in each the compiler knows the address space of the
  // swarm arrays: selecting the base pointer at run time made every swarm access a FLAT instruction (74 of them), and
  // the proposal / commit phases -- one or two waves working, the rest waiting -- are chains of exactly those accesses.
  if (L.swarm_global) {
    const Swarm sw = swarm_carve(ws + (size_t)cl.rank * swarm_bytes(ps.P, true, true), ps.P, ARB, true);
    pso_run_wg<MODE, PATH, CLUSTER, ARB, false, true>(E, pts, n, ps, guess, dev, seed, draws_table, sw, lds_ctrl(L.ctrl_off), out_pose,
                                         out_cost, stats, cl);
  } else {
    const Swarm sw = swarm_carve(g_lds + L.region_off, ps.P, ARB, swarm_has_raw2(ps.P, false));
    pso_run_wg<MODE, PATH, CLUSTER, ARB>(E, pts, n, ps, guess, dev, seed, draws_table, sw, lds_ctrl(L.ctrl_off), out_pose,
                                         out_cost, stats, cl);
  }
  if (threadIdx.x == 0 && stats && cl.rank == 0) {
    const ImageHeader* h = reinterpret_cast<const ImageHeader*>(g_lds + L.hdr_off);
    stats->n_built = h->n_built;
    stats->status = (stats->status & (kStatusNeedsF64 | kStatusClusterTimeout | 0xffff0000u)) | h->status;
    // the host's copy of {pose, cost, statistics}: written into its pinned slot from here (this thread wrote all of it),
    // so that no copy operation stands between the end of the kernel and the host's wake-up
    if (mirror) {
      static_assert(sizeof(AlignStats) == 32, "result slot layout");
#pragma unroll
      for (int k = 0; k < 4; ++k) mirror[k] = out_pose[k];  // [3] is the cost's place (out_cost, when wanted)
      const double* sd = reinterpret_cast<const double*>(stats);
#pragma unroll
      for (int k = 0; k < 4; ++k) mirror[4 + k] = sd[k];
      publish_pinned_word(reinterpret_cast<uint32_t*>(mirror + 8), seq);  // the host polls this word (wait_pinned_word)
    }
  }
