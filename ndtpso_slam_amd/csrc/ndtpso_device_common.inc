// ndtpso_device_common.inc -- what every translation unit of the library's device code starts from: the LDS layout shared by
// every kernel (and the host code that plans it), the helpers that stage a table image into it, and the last store of a result
// into pinned host memory.  Included by ndtpso_hip.hip and by ndtpso_align_jobs.hip (the job kernels are a translation unit of
// their own, so that their instantiations cannot move the code of the kernels that share pso_run_wg's with them).
using namespace ndtpso;

static_assert(sizeof(CellRow) == sizeof(ndtpso_cell_row), "cell row ABI");
static_assert(sizeof(AlignStats) == sizeof(ndtpso_align_stats), "stats ABI");

namespace {

constexpr int kMaxLds = 160 * 1024;  // gfx950: 160 KiB per workgroup
constexpr int kCtrlBytes = 1440;     // control block (PsoShared + compaction counters)

// LDS layout shared by every kernel.
//   bitmap form: [ctrl | header | bitmap | mean | (ab | cd) | (chol) | points | region]
//                header..chol are contiguous exactly as in the HBM image
//   dense form : [u16 cell table @0 | ctrl | dense records (cap+1, blocks of 16 means + 16 factors) | header | points | region]
//   dense form of the fp64 score: [ctrl | records (cap+1) x 48 B | u16 cell table | header | points | region]
//                (records first: their LDS byte addresses are the table's u16 entries)
//   region = max(table-build scratch {key, cellkey, cnt, bm2, plist, (bm)}, swarm)
struct Layout {
  int ctrl_off, hdr_off, bm_off, mean_off, ab_off, cd_off, chol_off, drec_off, pts_off, region_off, total;
  int key_off, cellkey_off, cnt_off, bm2_off, plist_off;  // build scratch inside region
  int swarm_global;  // 1: the swarm does not fit in LDS and lives in an HBM workspace (large-swarm configs)
  int xs_off, xs_slots;  // exact mode: partial-sum scratch of the arbitration, xs_slots x 512 bytes (exact_tasks_wg); -1: none
  int dtab_off;          // fp64 score on the dense table (PATH 8 / 9): the u16 cell table; -1: none
};

// fmt: kScoreF32 -> mean+chol, kScoreF64 -> mean+ab+cd, 2 -> everything (table build kernel);
// ddw > 0: dense form with a ddw x ddh cell table (fp32 score only)
Layout make_layout(int n_words, int rec_cap, int n_max, int P, int fmt, int ddw = 0, int ddh = 0,
                   bool swarm_global = false, bool exact = false, bool exact_units = false) {
  Layout L;
  L.swarm_global = swarm_global ? 1 : 0;
  const bool dense = ddw > 0, d64 = dense && fmt == kScoreF64;
  int off = (dense && !d64) ? dense_tab_bytes(ddw, ddh) : 0;
  L.ctrl_off = off;
  off += kCtrlBytes;
  L.drec_off = -1;
  L.dtab_off = -1;
  if (d64) {
    L.drec_off = off;
    off += align16(d64_rec_bytes(rec_cap + 1));
    L.dtab_off = off;
    off += dense_tab_bytes(ddw, ddh);
  } else if (dense) {
    L.drec_off = off;
    off += dense_rec_bytes(rec_cap + 1);
  }
  L.hdr_off = off;
  off += kImageHeaderBytes;
  L.bm_off = L.mean_off = L.ab_off = L.cd_off = L.chol_off = -1;
  if (!dense) {
    L.bm_off = off;
    off += align16(n_words * 8);
    L.mean_off = off;
    off += 16 * rec_cap;
    if (fmt == kScoreF64 || fmt == 2) {
      L.ab_off = off;
      L.cd_off = off + 16 * rec_cap;
      off += 32 * rec_cap;
    }
    if (fmt == kScoreF32 || fmt == 2) {
      L.chol_off = off;
      off += 16 * rec_cap;
    }
  }
  L.pts_off = off;
  off += round_up(n_max, kPointPad) * 16;
  L.region_off = off;
  const int ints = align16(n_max * 4);
  L.key_off = L.region_off;
  L.cellkey_off = L.key_off + ints;
  L.cnt_off = L.cellkey_off + ints;
  L.bm2_off = L.cnt_off + ints;
  L.plist_off = L.bm2_off + align16(n_words * 8);
  int scratch = 3 * ints + align16(n_words * 8) + align16(n_max * 2);
  if (dense) {  // the built-cell bitmap is only needed while the table is being built
    L.bm_off = L.region_off + scratch;
    scratch += align16(n_words * 8);
  }
  const int swarm = (P > 0 && !swarm_global) ? swarm_bytes(P, exact, swarm_has_raw2(P, false)) : 0;
  L.total = L.region_off + std::max(scratch, swarm);
  L.xs_off = -1;
  L.xs_slots = 0;
  // The fused pairs kernels with the swarm in LDS split the arbitration's fp64 scores into units; a single alignment's
  // kernels and the kernels of swarms kept in HBM score whole tasks per wave (the arbitration is 1 % of their time).
  // The unit form on the HBM-swarm kernels is what rounds 3 and 4 saw return wrong poses in some builds: not a matter of
  // the workgroup size (round 3's reading) but of the callers' code around the two out-of-line scoring functions under
  // interprocedural register allocation -- six builds made with it fail identically, the same sources without it pass
  // (NOTEBOOK, "The unit form on swarms kept in HBM") -- and the library is built without IPRA since (build.py).
  // tests/test_gpu_fullsize.py::test_unit_form_on_swarms_kept_in_hbm keeps running those kernels WITH units
  // (NDTPSO_UNITS_HBM=<slots>, tests only) against the fp64 mode in every build.
  static const int units_hbm = [] {  // tests only: scratch slots of the unit form for swarms kept in HBM (0: whole tasks)
    const char* e = std::getenv("NDTPSO_UNITS_HBM");
    // (a task's four units take four consecutive slots: a multiple of four, at most 64)
    return e ? std::min(std::max(std::atoi(e), 0) & ~3, 64) : 0;
  }();
  if (exact && exact_units && (!swarm_global || units_hbm > 0)) {
    L.xs_slots = swarm_global ? units_hbm : 8;  // one unit per wave of the workgroup
    L.xs_off = L.total;
    L.total += L.xs_slots * kWave * 8;
  }
  return L;
}

DenseP make_dense(const GridP& g, const WinP& wn, const Layout& L) {
  DenseP d;
  d.clip = ((double)g.W * g.cs - 2. * g.hw > 1e-9 * g.hw || (double)g.H * g.cs - 2. * g.hh > 1e-9 * g.hh) ? 1 : 0;
  d.dw = wn.w + 1;
  d.dh = wn.h + 1;
  d.ox = wn.x0 - 1;
  d.oy = wn.y0 - 1;
  d.rec_off = L.drec_off;
  dense_set_limits(d, g.hw, g.hh, g.inv_cs);
  return d;
}

}  // namespace

static_assert(sizeof(PsoShared) + 32 * sizeof(int) <= kCtrlBytes, "control block too small");

// cluster kernels run at most 8 waves per workgroup (cluster_shape), which leaves each wave 256 VGPRs
constexpr int kClusterMaxThreads = 512;

extern __shared__ __attribute__((aligned(16))) unsigned char g_lds[];

__device__ __forceinline__ PsoShared* lds_ctrl(int ctrl_off) { return reinterpret_cast<PsoShared*>(g_lds + ctrl_off); }
__device__ __forceinline__ int* lds_cnt(int ctrl_off) {
  return reinterpret_cast<int*>(g_lds + ctrl_off + sizeof(PsoShared));
}

__device__ __forceinline__ void copy16(void* dst, const void* src, int bytes) {
  // bytes is a multiple of 16; 16 B per lane, consecutive lanes consecutive addresses (coalesced)
  const uint4* s = reinterpret_cast<const uint4*>(src);
  uint4* d = reinterpret_cast<uint4*>(dst);
  for (int i = threadIdx.x; i < (bytes >> 4); i += blockDim.x) d[i] = s[i];
}

__device__ __forceinline__ TableView lds_table_view(const Layout& L) {
  TableView T;
  T.bm = L.bm_off >= 0 ? reinterpret_cast<const uint2*>(g_lds + L.bm_off) : nullptr;
  T.mean = L.mean_off >= 0 ? reinterpret_cast<const double2*>(g_lds + L.mean_off) : nullptr;
  T.ab = L.ab_off >= 0 ? reinterpret_cast<const double2*>(g_lds + L.ab_off) : nullptr;
  T.cd = L.cd_off >= 0 ? reinterpret_cast<const double2*>(g_lds + L.cd_off) : nullptr;
  T.chol = L.chol_off >= 0 ? reinterpret_cast<const float4*>(g_lds + L.chol_off) : nullptr;
  return T;
}
__device__ __forceinline__ TableOut lds_table_out(const Layout& L) {
  TableOut T;
  T.bm = reinterpret_cast<uint2*>(g_lds + L.bm_off);
  T.mean = L.mean_off >= 0 ? reinterpret_cast<double2*>(g_lds + L.mean_off) : nullptr;
  T.ab = L.ab_off >= 0 ? reinterpret_cast<double2*>(g_lds + L.ab_off) : nullptr;
  T.cd = L.cd_off >= 0 ? reinterpret_cast<double2*>(g_lds + L.cd_off) : nullptr;
  T.chol = L.chol_off >= 0 ? reinterpret_cast<float4*>(g_lds + L.chol_off) : nullptr;
  return T;
}
__device__ __forceinline__ EvalCtx make_eval_ctx(const GridP& g, const WinP& wn, const Layout& L, const DenseP& dn) {
  EvalCtx E;
  E.g = g;
  E.wn = wn;
  E.T = lds_table_view(L);
  E.dn = dn;
  E.lds0 = g_lds;
  E.light = 0;
  E.guard_lds = 0;
  E.d64_tab = 0;
  return E;
}

// bitmap-form table views into an image in HBM: [header | bitmap | mean | ab | cd | chol]
__device__ __forceinline__ TableView image_table_view(const WinP& wn, const unsigned char* __restrict__ image) {
  TableView T;
  T.bm = reinterpret_cast<const uint2*>(image + kImageHeaderBytes);
  T.mean = reinterpret_cast<const double2*>(image + image_mean_offset(wn.n_words));
  T.ab = reinterpret_cast<const double2*>(image + image_ab_offset(wn.n_words, wn.rec_cap));
  T.cd = reinterpret_cast<const double2*>(image + image_cd_offset(wn.n_words, wn.rec_cap));
  T.chol = reinterpret_cast<const float4*>(image + image_chol_offset(wn.n_words, wn.rec_cap));
  return T;
}
// exact mode (fp32-score dense kernels): the fp64 table the arbitration reads, where its image lies in HBM, goes into
// the LDS parameter block of exact_tasks (thread 0 writes; the barriers of the swarm initialisation publish it)
template <bool BYTE>
__device__ __forceinline__ void enable_arbitration(PsoShared* sh, const GridP& g, const WinP& wn, const DenseP& dn,
                                                   const unsigned char* __restrict__ image, const Layout& L) {
  if (threadIdx.x == 0) {
    ExactArgs& a = sh->xa;
    a.xs_lds = L.xs_slots ? (unsigned)(uintptr_t)(const unsigned char __attribute__((address_space(3)))*)(g_lds + L.xs_off) : 0u;
    a.xs_slots = L.xs_slots;
    a.g = g;
    a.dw = dn.dw;
    a.dh = dn.dh;
    a.ox = dn.ox;
    a.oy = dn.oy;
    a.null_entry = BYTE ? (unsigned)dn.rec_off : (unsigned)dn.rec_off >> 4;
    const TableView T = image_table_view(wn, image);
    a.xmean = T.mean;
    a.xab = T.ab;
    a.xcd = T.cd;
  }
}

// the table image where it lies in HBM, for maps whose table does not fit in LDS (PATH 4 / 5)
__device__ __forceinline__ EvalCtx make_eval_ctx_global(const GridP& g, const WinP& wn, const DenseP& dn,
                                                        const unsigned char* __restrict__ image) {
  EvalCtx E;
  E.g = g;
  E.wn = wn;
  E.T = image_table_view(wn, image);
  E.dn = dn;
  E.lds0 = g_lds;
  E.light = 0;
  E.guard_lds = 0;
  E.d64_tab = 0;
  return E;
}

// stage a table image (HBM) into LDS in the form the kernel's PATH wants
template <int MODE, int PATH>
__device__ __forceinline__ void stage_image(const unsigned char* __restrict__ image, const GridP& g, const WinP& wn,
                                            const Layout& L, const DenseP& dn) {
  if constexpr (PATH >= 4) {  // table stays in HBM (served by L2); only the header is staged
    copy16(g_lds + L.hdr_off, image, kImageHeaderBytes);
  } else if constexpr (PATH == 2) {
    copy16(g_lds + L.hdr_off, image, kImageHeaderBytes);
    dense_from_image_wg(g, wn, image, dn, g_lds);
  } else if constexpr (MODE == kScoreF64) {
    copy16(g_lds + L.hdr_off, image, image_chol_offset(wn.n_words, wn.rec_cap));  // header .. cd, contiguous
  } else {
    copy16(g_lds + L.hdr_off, image, image_ab_offset(wn.n_words, wn.rec_cap));  // header .. mean
    copy16(g_lds + L.chol_off, image + image_chol_offset(wn.n_words, wn.rec_cap), 16 * wn.rec_cap);
  }
}

// the last store of a result a kernel leaves in pinned host memory: everything this thread wrote before it is visible to
// the host that reads the word
__device__ __forceinline__ void publish_pinned_word(uint32_t* word, uint32_t value) {
  __threadfence_system();
  __hip_atomic_store(word, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
