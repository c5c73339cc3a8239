// ndtpso_hip.hip -- __global__ entry points and the C-ABI (include/ndtpso_hip.h) of the gfx950
// NDT-PSO alignment path.  Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -shared -fPIC.
#include "ndtpso_kernels.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <sched.h>
#include <sys/prctl.h>
#include <time.h>

#include "../../include/ndtpso_hip.h"

#include "ndtpso_device_common.inc"
#include "ndtpso_align_jobs.h"

// ---- K3a -------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024)
k_scan_to_points(const float* __restrict__ ranges, ScanP sp, const double2* __restrict__ dirs, int do_trans, double tc, double ts, double ttx,
                 double tty, double2* __restrict__ out_xy, uint32_t* __restrict__ out_n) {
  const size_t b = blockIdx.x;
  const int n = scan_to_points_wg(ranges + b * sp.n_beams, sp, dirs, do_trans != 0, tc, ts, ttx, tty,
                                  out_xy + b * sp.n_beams, lds_cnt(0));
  if (threadIdx.x == 0) out_n[b] = (uint32_t)n;
}

// ---- K3b -------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024)
k_build_table(const double2* __restrict__ xy, int n, GridP g, WinP wn, Layout L, unsigned char* __restrict__ image_out,
              CellRow* __restrict__ rows, uint32_t* __restrict__ n_rows) {
  double2* pts = reinterpret_cast<double2*>(g_lds + L.pts_off);
  copy16(pts, xy, n * 16);
  __syncthreads();
  build_table_wg(g, wn, pts, n, reinterpret_cast<ImageHeader*>(g_lds + L.hdr_off), lds_table_out(L),
                 reinterpret_cast<int*>(g_lds + L.key_off), reinterpret_cast<int*>(g_lds + L.cellkey_off),
                 reinterpret_cast<int*>(g_lds + L.cnt_off), reinterpret_cast<uint2*>(g_lds + L.bm2_off),
                 reinterpret_cast<unsigned short*>(g_lds + L.plist_off), rows, n_rows, nullptr, nullptr);
  // LDS -> HBM image (fmt 2 layout == image layout)
  copy16(image_out, g_lds + L.hdr_off, image_bytes(wn.n_words, wn.rec_cap));
}

// ---- K3c: transform + bin a point list (NDTFrame::update / addPoint, ndtframe.cpp:187-198,215-235) ---------
__global__ void __launch_bounds__(256)
k_points_to_cells(const double2* __restrict__ xy, int n, GridP g, int do_trans, double tc, double ts, double ttx,
                  double tty, double2* __restrict__ xy_out, int32_t* __restrict__ idx_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double2 p = xy[i];
  if (do_trans) {  // transform_point, core.h:28-31 (separate roundings)
    const double x = p.x * tc - p.y * ts + ttx;
    const double y = p.x * ts + p.y * tc + tty;
    p.x = x;
    p.y = y;
  }
  int idx = -1;
  if (fabs(p.x) < g.hw && fabs(p.y) < g.hh) {  // NDTFrame::getCellIndex, ndtframe.cpp:240-249
    int ix, iy;
    cell_coords_rt(g, p.x, p.y, ix, iy);
    idx = ix + g.W * iy;
    if (idx >= g.W * g.H) idx = -1;  // fl(y + h/2) == h: out-of-range access in the reference, dropped here
  }
  xy_out[i] = p;
  idx_out[i] = idx;
}

// ---- K3a+K3c fused: NDTFrame::loadLaser (ndtframe.cpp:144-185) -> points and their cells, one workgroup ----
__global__ void __launch_bounds__(1024)
k_scan_to_cells(const float* __restrict__ ranges, ScanP sp, const double2* __restrict__ dirs, int do_trans, double tc, double ts, double ttx, double tty,
                GridP g, double2* __restrict__ out_xy, int32_t* __restrict__ out_idx, uint32_t* __restrict__ out_n) {
  const int n = scan_to_points_wg(ranges, sp, dirs, do_trans != 0, tc, ts, ttx, tty, out_xy, lds_cnt(0));
  __syncthreads();  // out_xy was written by this workgroup (global memory, workgroup scope)
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    int ix, iy, idx = -1;
    if (point_cell(g, out_xy[i], ix, iy)) {
      // point_cell folds the reference's row wrap (fl(x + w/2) == w -> next row, column 0): same linear index
      idx = ix + g.W * iy;
    }
    out_idx[i] = idx;
  }
  if (threadIdx.x == 0) out_n[0] = (uint32_t)n;
}

// int8_t(p * 100.) as the reference's x86-64 build evaluates it (ndtframe.cpp:105): cvttsd2si to 32 bits -- which
// yields INT_MIN for NaN and for values outside int32, where the GPU's conversion saturates -- then the low byte.
// Only matters for the garbage Gaussians a resetCells can leave behind (p = inf), but those are reproduced too.
__device__ __forceinline__ int8_t x86_int8_of(double v) {
  const int32_t i = (v > -2147483649. && v < 2147483648.) ? (int32_t)v : INT32_MIN;
  return (int8_t)(uint8_t)((uint32_t)i & 0xffu);
}

// ---- occupancy-grid values of built cells (NDTFrame::build, ndtframe.cpp:79-112) ----------------------------
__global__ void __launch_bounds__(256)
k_occupancy_values(int n_cells, int per_cell, double og_cs, double hw, double hh, int W, int H,
                   const int32_t* __restrict__ index, const double2* __restrict__ mean, const double4* __restrict__ icov,
                   int8_t* __restrict__ values) {
  const int kk2 = per_cell * per_cell;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)n_cells * kk2) return;
  const int c = (int)(t / kk2), r = (int)(t % kk2), j = r / per_cell, k = r % per_cell;
  const unsigned i = (unsigned)index[c];
  const unsigned cx = i % (unsigned)W, cy = i / (unsigned)H;  // sic (ndtframe.cpp:81)
  const double x_c = ((double)(cx * (unsigned)per_cell + (unsigned)j) * og_cs + og_cs / 2.) - hw;
  const double y_c = ((double)(cy * (unsigned)per_cell + (unsigned)k) * og_cs + og_cs / 2.) - hh;
  const double2 m = mean[c];
  const double4 ic = icov[c];
  const double d0 = x_c - m.x, d1 = y_c - m.y;  // NDTCell::normalDistribution, ndtcell.cpp:70-78
  const double r0 = d0 * ic.x + d1 * ic.z;
  const double r1 = d0 * ic.y + d1 * ic.w;
  const double p = exp(-(r0 * d0 + r1 * d1) / 2.);
  values[t] = (p > 0.) ? x86_int8_of(p * 100.) : (int8_t)-1;
}

// ---- K3d: NDTCell::build with sliding-window state, one thread per created cell (ndtcell.cpp:36-68,93-111) ----
struct CellWindow {  // == ndtpso_cell_window
  double global_sum[2], global_covar_sum[4], slot_sum[2], slot_covar[4], mean[2], icov[4];
  int32_t global_count, slot_count, current_count, built;
};
static_assert(sizeof(CellWindow) == sizeof(ndtpso_cell_window), "cell window ABI");

__global__ void __launch_bounds__(256)
k_cells_build_windowed(CellWindow* __restrict__ cells, int n_cells, const uint32_t* __restrict__ off,
                       const double2* __restrict__ pts) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cells) return;
  CellWindow w = cells[c];
  const uint32_t p0 = off[c], p1 = off[c + 1];
  // s_current_partial_sum: running sum, in insertion order, of the points added since the last rotation
  // (ndtcell.cpp:30,61-65).  Those are the slot's whole point vector -- except right after a rotation onto a slot
  // that still holds the points of the previous lap of the window (the vector is only cleared by the next addPoint,
  // ndtcell.cpp:22-27): then the sum is zero while the covariance below still runs over the stale points.
  double cx = 0., cy = 0.;
  if (w.current_count > 0)
    for (uint32_t i = p0; i < p1; ++i) {
      cx += pts[i].x;
      cy += pts[i].y;
    }
  // WINDOW_ADD (ndtcell.h:13-15): global = (global + partial) - partials[idx]; partials[idx] = partial
  w.global_sum[0] = (w.global_sum[0] + cx) - w.slot_sum[0];
  w.global_sum[1] = (w.global_sum[1] + cy) - w.slot_sum[1];
  w.slot_sum[0] = cx;
  w.slot_sum[1] = cy;
  w.global_count = (w.global_count + w.current_count) - w.slot_count;
  w.slot_count = w.current_count;
  if (w.global_count > 2) {
    const double mx = w.global_sum[0] / (double)w.global_count;  // ndtcell.cpp:44
    const double my = w.global_sum[1] / (double)w.global_count;
    double c00 = 0., c01 = 0., c10 = 0., c11 = 0.;
    for (uint32_t i = p0; i < p1; ++i) {  // ndtcell.cpp:49-52
      const double d0 = pts[i].x - mx, d1 = pts[i].y - my;
      c00 += d0 * d0;
      c01 += d0 * d1;
      c10 += d1 * d0;
      c11 += d1 * d1;
    }
    const double cov[4] = {c00, c01, c10, c11};
    for (int k = 0; k < 4; ++k) {  // ndtcell.cpp:54-55
      w.global_covar_sum[k] = (w.global_covar_sum[k] + cov[k]) - w.slot_covar[k];
      w.slot_covar[k] = cov[k];
    }
    // s_calc_covar_inverse, ndtcell.cpp:93-111 (eigenvalues as Eigen's EigenSolver computes them)
    const double nn = (double)w.global_count;
    const double v00 = w.global_covar_sum[0] / nn, v01 = w.global_covar_sum[1] / nn;
    const double v10 = w.global_covar_sum[2] / nn, v11 = w.global_covar_sum[3] / nn;
    w.mean[0] = mx;
    w.mean[1] = my;
    covar_inverse_eigen(v00, v01, v10, v11, w.icov);
    w.built = 1;
  }
  cells[c] = w;
}

// fp32 Cholesky records of a table image whose mean/ab/cd arrays were uploaded by the host
__global__ void __launch_bounds__(256)
k_fill_chol(unsigned char* __restrict__ image, int n_words, int rec_cap, int n_cells) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_cells) return;
  const double2 ab = reinterpret_cast<const double2*>(image + image_ab_offset(n_words, rec_cap))[s];
  const double2 cd = reinterpret_cast<const double2*>(image + image_cd_offset(n_words, rec_cap))[s];
  float l[4];
  make_chol(ab.x, ab.y, cd.x, cd.y, l);
  reinterpret_cast<float4*>(image + image_chol_offset(n_words, rec_cap))[s] = make_float4(l[0], l[1], l[2], l[3]);
}

// ---- K1 --------------------------------------------------------------------------------------
template <int MODE, int PATH, bool DUMP>
__global__ void __launch_bounds__(1024)
k_cost_batch(const unsigned char* __restrict__ image, const double2* __restrict__ xy, int n, GridP g, WinP wn,
             Layout L, DenseP dn, const double* __restrict__ poses, int m, double* __restrict__ costs,
             int32_t* __restrict__ dump) {
  double2* pts = reinterpret_cast<double2*>(g_lds + L.pts_off);
  stage_image<MODE, PATH>(image, g, wn, L, dn);
  copy16(pts, xy, n * 16);
  pad_points_wg(pts, n);
  __syncthreads();
  const EvalCtx E = PATH >= 4 ? make_eval_ctx_global(g, wn, dn, image) : make_eval_ctx(g, wn, L, dn);
  const int n_waves = blockDim.x >> 6;
  for (int k = blockIdx.x * n_waves + wave_id(); k < m; k += gridDim.x * n_waves) {
    const double th = poses[3 * k + 2];
    double sn, cn;
    sincos(th, &sn, &cn);
    const double tx = poses[3 * k], ty = poses[3 * k + 1];
    int32_t* dp = DUMP ? dump + (size_t)k * n : nullptr;
    double cost;
    if constexpr (PATH == 2)
      cost = eval_pose_wave_dense<DUMP>(E.g, E.dn, E.lds0, pts, n, cn, sn, tx, ty, dp);
    else
      cost = eval_pose_wave_t<MODE, (PATH & 3) == 1, DUMP>(E.g, E.wn, E.T, pts, n, cn, sn, tx, ty, dp);
    if constexpr (MODE == kScoreF32) {
      if (cost > -kTinyCost) cost = eval_pose_wave_tiny<PATH>(E, pts, n, cn, sn, tx, ty);  // underflow regime
    }
    if (lane_id() == 0) costs[k] = cost;
  }
}

// ---- K2 --------------------------------------------------------------------------------------
// CLUSTER: gridDim.x workgroups share this one alignment (see ClusterP in ndtpso_kernels.hpp)
template <int MODE, int PATH, bool CLUSTER, bool ARB = false>
__global__ void __launch_bounds__(CLUSTER ? kClusterMaxThreads : 1024)
k_align(const unsigned char* __restrict__ image, const double2* __restrict__ xy, int n,
        const uint32_t* __restrict__ n_ptr, GridP g, WinP wn, Layout L, DenseP dn, PsoP ps,
        const double* __restrict__ guess, const double* __restrict__ dev, uint32_t seed,
        const int32_t* __restrict__ table, unsigned char* __restrict__ ws, double* __restrict__ out_pose,
        double* __restrict__ out_cost, AlignStats* __restrict__ stats, ClusterP cl, double* __restrict__ mirror,
        const int4* __restrict__ table_src, int4* __restrict__ table_dst, int table_vec,
        const uint32_t* __restrict__ late_hdr, int late_table_cap, int late_rec_cap, uint32_t seq) {
  if constexpr (CLUSTER) {
    size_t c0;
    if (!cluster_place(cl, &c0, &cl.rank)) return;  // (one cluster; the seven in eight workgroups that only place it leave here)
    cl.spec = cl.spec_off >= 0 ? reinterpret_cast<double*>(g_lds + cl.spec_off) : nullptr;
  } else {
    cl.rank = 0;
  }
#include "ndtpso_align_body.inc"
}

// The guard of the one-workgroup dense kernels when the box of scan B's DISC does not fit the table beside scan A's (cells of
// 0.25 - 0.3 m at two workgroups per CU: nine evaluations in ten took the clamped trips).  Scan B's own extent under the guess's
// heading instead, grown by what a heading within `dth` of it moves a point (at most rho * dth): the box of the same room as scan
// A's, a few cells wider.  The guard then holds for those headings only (DenseGuard::t_lo / t_hi, a third flag beside TX's and
// TY's).  Every thread of the workgroup calls it; the result is left in LDS (`out`, valid after the call's last barrier).
struct BoxGuardOut {
  DenseGuard guard;
  double t_lo, t_hi;
  int x0, y0, w, h;
  int ok;
};
static_assert(sizeof(BoxGuardOut) <= 24 * sizeof(int), "BoxGuardOut lives in the counters' first slots");
__device__ __attribute__((noinline)) void box_guard_wg(const float* __restrict__ ranges, const ScanP* sp,
                                                       const double2* __restrict__ dirs, const GridP* g, const double* guess,
                                                       const double* dev, double rc, double cx, double cy, const WinP* wn,
                                                       int dense_cap, int clip, int* slots, BoxGuardOut* out,
                                                       int metres = 0 /* fp64 score: the guard is on the translation in metres */) {
  constexpr double kMarginCells = 4.;
  const double th0 = guess[2];
  const double dth = fmin(0.1, fmax(0.02, 16. * fabs(dev[2])));
  double s0, c0;
  sincos(th0, &s0, &c0);
  int e[4];
  const bool have = scan_extent_wg(ranges, *sp, dirs, c0, s0, g->inv_cs, slots, e);
  if (threadIdx.x == 0) {
    out->ok = 0;
    if (have && fabs(th0) < 1e6 && dth == dth) {
      const double grow = rc * dth + 1e-6;  // cells (rc: rho in cells with the transform's rounding)
      const double ex0 = (double)e[0] * (1. / 256.) - grow, ex1 = (double)e[1] * (1. / 256.) + grow;
      const double ey0 = (double)e[2] * (1. / 256.) - grow, ey1 = (double)e[3] * (1. / 256.) + grow;
      const int cx0 = max((int)floor(cx + ex0 - kMarginCells), 0), cx1 = min((int)floor(cx + ex1 + kMarginCells), g->W - 1);
      const int cy0 = max((int)floor(cy + ey0 - kMarginCells), 0), cy1 = min((int)floor(cy + ey1 + kMarginCells), g->H - 1);
      if (cx1 >= cx0 && cy1 >= cy0) {
        const int vx0 = min(wn->x0, cx0), vy0 = min(wn->y0, cy0);
        const int vw = max(wn->x0 + wn->w - 1, cx1) - vx0 + 1, vh = max(wn->y0 + wn->h - 1, cy1) - vy0 + 1;
        if (dense_entries(vw + 1, vh + 1) <= dense_cap) {
          // a point's table coordinate is TX + e, e in [ex0, ex1]: 0 <= TX + ex0 and TX + ex1 < w + 2 (and below the frame's
          // upper bound where the last cells overhang it)
          double hx = (double)(vw + 2) - ex1, hy = (double)(vh + 2) - ey1;
          if (clip) {
            hx = fmin(hx, (2. * g->hw) * g->inv_cs - (double)(vx0 - 1) - ex1);
            hy = fmin(hy, (2. * g->hh) * g->inv_cs - (double)(vy0 - 1) - ey1);
          }
          out->guard = DenseGuard{-ex0, hx, -ey0, hy};
          if (metres) {
            // fp64 score (score_trip_d64 under the guard: no frame, wrap or window test, and an index that is the reference's
            // only for a point inside the frame): every point strictly inside the frame AND inside the window.  A point is at
            // t + e, e in [ex0, ex1] cells; the bounds as the disc's guard has them (k_align_pairs), the disc's radius replaced
            const double cs = g->cs, sl = 1e-6 * cs;
            const double xl = fmax(-g->hw, (double)vx0 * cs - g->hw) - ex0 * cs + sl, xh = fmin(g->hw, (double)(vx0 + vw) * cs - g->hw) - ex1 * cs - sl;
            const double yl = fmax(-g->hh, (double)vy0 * cs - g->hh) - ey0 * cs + sl, yh = fmin(g->hh, (double)(vy0 + vh) * cs - g->hh) - ey1 * cs - sl;
            out->guard = DenseGuard{xl, xh, yl, yh};
          }
          out->t_lo = th0 - dth;
          out->t_hi = th0 + dth;
          out->x0 = vx0;
          out->y0 = vy0;
          out->w = vw;
          out->h = vh;
          out->ok = 1;
        }
      }
    }
  }
  __syncthreads();
}

// ---- fused scan pairs: K3a(ref) + K3b + K3a(new) + K2, everything in LDS -------------------------
//
// gate == 0: every workgroup runs.  gate != 0: a redo launch -- only alignments an earlier launch flagged with
// one of those status bits run (the others exit on their first instruction), and the bits are cleared.
// PATH 2 sizes its staging window per alignment (bounding box of the occupied cells, `dense_cap` table
// entries provisioned); a box that does not fit flags kStatusNeedsBitmap and leaves the alignment to the
// bitmap-form kernel, whose window is the static range box.
// CLUSTER (small batches: fewer alignments than compute units): cl.K consecutive workgroups share alignment
// blockIdx.x / K -- each of them ingests both scans and builds the table for itself (identical arithmetic, so the
// copies agree), then the PSO runs as a cluster (ClusterP).  Never combined with a gate.
// SWARM: 2 = the kernel carries both copies of the PSO (swarm in LDS / in its HBM workspace, chosen by L.swarm_global);
// 0 / 1 = only the LDS / only the HBM copy.  The NOCLIP kernels -- the ones the batches of the benchmark run -- exist as
// 0 and 1: at 128 registers what is inlined beside the hot loop decides its allocation (fp32-score kernel of config 3:
// 21 spills with both copies, none with its own).
template <int MODE, int PATH, bool CLUSTER, bool ARB = false, bool NOCLIP = false, int SWARM = 2, bool BOX = false, bool PAIR = false>
__global__ void __launch_bounds__(CLUSTER ? kClusterMaxThreads : 1024)
k_align_pairs(const float* __restrict__ ref_ranges, const float* __restrict__ new_ranges, ScanP sp, GridP g, WinP wn,
              Layout L, DenseP dn, int dense_cap, PsoP ps, const double* __restrict__ guess,
              const double* __restrict__ dev, const uint32_t* __restrict__ seeds, const int32_t* __restrict__ tables,
              size_t table_stride, unsigned char* __restrict__ ws, size_t ws_stride, double* __restrict__ out_pose,
              double* __restrict__ out_cost, AlignStats* __restrict__ stats, uint32_t gate, ClusterP cl,
              const double2* __restrict__ beam_dirs, unsigned char* __restrict__ ximg, size_t ximg_stride,
              uint32_t* __restrict__ feedback /* counts the alignments whose box outgrew the cell table (pinned host word) */) {
  static_assert(!PAIR || (SWARM == 0 && NOCLIP && !CLUSTER && !BOX), "two items per wave: the batches' kernels with the swarm in LDS");
  size_t b = blockIdx.x;
#include "ndtpso_pairs_body.inc"
}

// the same alignment as a function of the pair, for the kernels that stride when gated (k_align_pairs_s below)
template <int MODE, int PATH, bool CLUSTER, bool ARB = false, bool NOCLIP = false, int SWARM = 2, bool BOX = false>
__device__ __forceinline__ void
align_pair_wg(size_t b, const float* __restrict__ ref_ranges, const float* __restrict__ new_ranges, ScanP sp, GridP g, WinP wn,
              Layout L, DenseP dn, int dense_cap, PsoP ps, const double* __restrict__ guess,
              const double* __restrict__ dev, const uint32_t* __restrict__ seeds, const int32_t* __restrict__ tables,
              size_t table_stride, unsigned char* __restrict__ ws, size_t ws_stride, double* __restrict__ out_pose,
              double* __restrict__ out_cost, AlignStats* __restrict__ stats, uint32_t gate, ClusterP cl,
              const double2* __restrict__ beam_dirs, unsigned char* __restrict__ ximg, size_t ximg_stride,
              uint32_t* __restrict__ feedback) {
  constexpr bool PAIR = false;  // (two items per wave: main launches only)
#include "ndtpso_pairs_body.inc"
}

// Gated launches -- "redo the alignments whose status carries this flag" -- used to be a workgroup per pair, 511 in 512 of which
// left on their first instruction.  Cheap on an idle device; but with two batches in flight every compute unit's LDS and
// registers are held by the other lane's main kernel, a workgroup that only wants to look at a flag waits for one of ITS
// workgroups to end like any other, and 512 of them trickled through the few free slots for 0.6 ms on average (a fifth of the
// traced kernel time, profiles/r05_kernel_stats_two_in_flight.csv) while their lane's next main launch waited behind them.
// The kernels that serve as redo kernels -- every one but the fp32 score's dense form, whose gated launch (largest table) is
// issued only where tables have been overflowing -- therefore have a second kernel for their gated launches, k_align_pairs_s,
// which STRIDES: a few workgroups (launch_pairs: 8, or twice what the previous call of the configuration found flagged) walk
// over the pairs and run the flagged ones one after the other, and workgroup 0 leaves the number of flagged pairs in a pinned
// word for the host's next choice of the grid.  (k_align_pairs itself -- every main launch -- is untouched.)
template <int MODE, int PATH, bool CLUSTER>
__host__ __device__ constexpr bool gate_strides() {
  return !CLUSTER && !(MODE == kScoreF32 && path_is_dense(PATH));
}

template <int MODE, int PATH, bool ARB = false, bool NOCLIP = false, int SWARM = 2, bool BOX = false>
__global__ void __launch_bounds__(1024)
k_align_pairs_s(const float* __restrict__ ref_ranges, const float* __restrict__ new_ranges, ScanP sp, GridP g, WinP wn,
                Layout L, DenseP dn, int dense_cap, PsoP ps, const double* __restrict__ guess,
                const double* __restrict__ dev, const uint32_t* __restrict__ seeds, const int32_t* __restrict__ tables,
                size_t table_stride, unsigned char* __restrict__ ws, size_t ws_stride, double* __restrict__ out_pose,
                double* __restrict__ out_cost, AlignStats* __restrict__ stats, uint32_t gate, ClusterP cl,
                const double2* __restrict__ beam_dirs, unsigned char* __restrict__ ximg, size_t ximg_stride,
                uint32_t* __restrict__ feedback, uint32_t n_pairs, uint32_t* __restrict__ gate_count) {
  if (gate_count && blockIdx.x == 0) {
    unsigned* cnt = reinterpret_cast<unsigned*>(g_lds);
    if (threadIdx.x == 0) *cnt = 0u;
    __syncthreads();
    unsigned mine = 0;
    for (uint32_t i = threadIdx.x; i < n_pairs; i += blockDim.x) mine += (stats[i].status & gate) ? 1u : 0u;
    if (mine) atomicAdd(cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(gate_count, *cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __syncthreads();
  }
  // this workgroup's pairs are blockIdx.x, blockIdx.x + gridDim.x, ...: 64 of their flags per sweep, one per lane, in every wave
  // alike (one after the other a workgroup's 64 loads took as long as 45 us of an otherwise empty launch)
  for (size_t base = blockIdx.x; base < (size_t)n_pairs; base += (size_t)gridDim.x * kWave) {
    const size_t mine = base + (size_t)lane_id() * gridDim.x;
    unsigned long long todo = __ballot(mine < (size_t)n_pairs && (stats[mine].status & gate) != 0u);
    while (todo) {  // (uniform: every wave has read the same flags, and a pair's flag changes only while that pair is run)
      const int k = __ffsll((long long)todo) - 1;
      todo &= todo - 1ull;
      align_pair_wg<MODE, PATH, false, ARB, NOCLIP, SWARM, BOX>(base + (size_t)k * gridDim.x, ref_ranges, new_ranges, sp, g, wn, L, dn, dense_cap, ps,
                                                               guess, dev, seeds, tables, table_stride, ws, ws_stride, out_pose, out_cost, stats,
                                                               gate, cl, beam_dirs, ximg, ximg_stride, feedback);
      __syncthreads();  // (the next alignment of this workgroup sets the same LDS up again)
    }
  }
}

// The pairs a redo launch on CLUSTERS serves (launch_pairs: redo_list): list[0] = how many (at most `cap`), list[1 ..] = the
// pairs whose status carries one of `mask`'s flags, in order; *seen (pinned) = how many there were in all, for the host's next
// choice.  One wave: 64 flags per sweep.
__global__ void __launch_bounds__(64)
k_redo_list(const AlignStats* __restrict__ stats, uint32_t n_pairs, uint32_t mask, uint32_t* __restrict__ list, uint32_t cap,
            uint32_t* __restrict__ seen) {
  uint32_t n = 0;
  for (uint32_t base = 0; base < n_pairs; base += kWave) {
    const uint32_t i = base + (uint32_t)lane_id();
    const bool f = i < n_pairs && (stats[i].status & mask) != 0u;
    const unsigned long long m = __ballot(f);
    const uint32_t at = n + (uint32_t)__popcll(m & ((1ull << lane_id()) - 1ull));
    if (f && at < cap) list[1 + at] = i;
    n += (uint32_t)__popcll(m);
  }
  if (lane_id() == 0) {
    list[0] = min(n, cap);
    if (seen) __hip_atomic_store(seen, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// =================================================================================================
// host side
// =================================================================================================

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) cap = bytes;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// Pinned host staging for the per-scan uploads of the resident path (ranges, std::rand() table): the caller's buffer
// is copied into a pinned slot and the DMA runs from there, so the call returns without waiting for the device and the
// caller may reuse its buffer at once.  Four slots, reused round robin; a slot is waited for only if its previous
// transfer is still in flight.
struct PinnedRing {
  static constexpr int kSlots = 4;
  void* host[kSlots] = {nullptr, nullptr, nullptr, nullptr};
  size_t cap[kSlots] = {0, 0, 0, 0};
  hipEvent_t ev[kSlots] = {nullptr, nullptr, nullptr, nullptr};
  bool busy[kSlots] = {false, false, false, false};
  // fence_until(): the slot's reader is a kernel of `rs`, and it precedes single alignment number `need` of the context on
  // that stream -- once the host has seen that alignment's result the slot is free, with no event of its own (an event
  // recorded between two kernels of the live sequence cost the device 6 us each time)
  unsigned long long need[kSlots] = {0, 0, 0, 0};
  hipStream_t rs[kSlots] = {nullptr, nullptr, nullptr, nullptr};
  int next = 0;
  hipError_t upload(void* dst, const void* src, size_t bytes, hipStream_t stream) {
    return upload2(dst, src, bytes, 0, nullptr, 0, stream);
  }
  // A pinned slot of `bytes` for the caller to fill: the device reads it where it lies (kernels take the slot's address
  // -- hipHostMalloc memory is mapped into the device's address space -- so a small per-scan input costs no copy
  // operation between two kernels of the stream, each of which was 4-6 us plus the wait for the copy engine's signal).
  // fence() after the last operation that reads the slot has been enqueued.
  hipError_t stage(size_t bytes, void** out, int* slot, unsigned long long done_seq = 0) {
    const int k = next;
    next = (next + 1) % kSlots;
    hipError_t e = hipSuccess;
    if (need[k]) {
      if (done_seq < need[k]) {  // no alignment has followed the reader (or none has reported yet): wait for the stream
        e = hipStreamSynchronize(rs[k]);
        if (e != hipSuccess) return e;
      }
      need[k] = 0;
    }
    if (busy[k]) {
      e = hipEventSynchronize(ev[k]);
      if (e != hipSuccess) return e;
      busy[k] = false;
    }
    if (!ev[k]) {
      e = hipEventCreateWithFlags(&ev[k], hipEventDisableTiming);
      if (e != hipSuccess) return e;
    }
    if (cap[k] < bytes) {
      if (host[k]) (void)hipHostFree(host[k]);
      host[k] = nullptr;
      cap[k] = 0;
      e = hipHostMalloc(&host[k], bytes, hipHostMallocMapped | hipHostMallocCoherent);
      if (e != hipSuccess) return e;
      cap[k] = bytes;
    }
    *out = host[k];
    *slot = k;
    return hipSuccess;
  }
  hipError_t fence(int k, hipStream_t stream) {
    busy[k] = true;
    return hipEventRecord(ev[k], stream);
  }
  void fence_until(int k, hipStream_t stream, unsigned long long seq) {
    need[k] = seq;
    rs[k] = stream;
  }
  hipError_t settle() {  // the context is about to change streams: the tickets would no longer mean anything
    for (int k = 0; k < kSlots; ++k) {
      if (!need[k]) continue;
      const hipError_t e = hipStreamSynchronize(rs[k]);
      if (e != hipSuccess) return e;
      need[k] = 0;
    }
    return hipSuccess;
  }
  // two host buffers, one transfer: [a | padding up to b_offset | b]
  hipError_t upload2(void* dst, const void* a, size_t a_bytes, size_t b_offset, const void* b, size_t b_bytes,
                     hipStream_t stream) {
    const size_t bytes = b_bytes ? b_offset + b_bytes : a_bytes;
    void* h = nullptr;
    int k = 0;
    hipError_t e = stage(bytes, &h, &k);
    if (e != hipSuccess) return e;
    std::memcpy(h, a, a_bytes);
    if (b_bytes) std::memcpy((unsigned char*)h + b_offset, b, b_bytes);
    e = hipMemcpyAsync(dst, h, bytes, hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return e;
    return fence(k, stream);
  }
  void release() {
    for (int k = 0; k < kSlots; ++k) {
      if (ev[k]) (void)hipEventDestroy(ev[k]);
      if (host[k]) (void)hipHostFree(host[k]);
      ev[k] = nullptr;
      host[k] = nullptr;
      cap[k] = 0;
      busy[k] = false;
      need[k] = 0;
    }
  }
};

struct BeamDirs {
  uint32_t n = 0;
  float amin = 0.f, ainc = 0.f;
  DevBuf buf;
};

struct ndtpso_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  std::string err;
  // reference table currently staged in HBM (image layout == LDS layout)
  bool have_ref = false;
  ndtpso_grid grid{};
  GridP g{};
  WinP wn{};
  uint32_t n_rows = 0;
  int n_cus = 256;  // compute units of the device (multiProcessorCount)
  // A cluster whose workgroups were not scheduled together gave up (bounded wait) and its alignment was redone on one
  // workgroup: the device is shared with other work.  The next `cluster_penalty` single alignments do not try again.
  int cluster_penalty = 0;
  DevBuf image, rows, xy, xy2, ranges, ranges2, poses, costs, dump, small, table, out, seeds, ws, gate, cluster_xc, ximg;
  PinnedRing pinned;
  BeamDirs beam_dirs[4];  // cached beam directions of the scan geometries in use (beam_directions)
  unsigned beam_dirs_next = 0;
  // Batches in flight (ndtpso_set_pipeline_depth): consecutive ndtpso_align_pairs_dev calls alternate between lanes --
  // a stream of the context's own and the workspaces a launch writes (HBM swarms, fp64 table images, internal stats) --
  // so that call k + 1's workgroups take the compute units call k's tail leaves idle (a launch lasts as long as its
  // slowest workgroup, 8 % after the median one).
  struct PipeLane {
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    bool pending = false;
    unsigned long long ticket = 0;  // number of the call it last ran
    DevBuf ws, gate, ximg;
  };
  static constexpr int kMaxPipe = 2;
  PipeLane lanes[kMaxPipe];
  int pipe_depth = 1;
  unsigned long long pipe_calls = 0;  // pipelined calls issued so far
  hipEvent_t pipe_in = nullptr;       // "inputs of the call are ready on the context's stream"
  // NDTPSO_HOST_CLOCK=1 (diagnostics): where the host's time goes around single alignments -- mean time between an
  // alignment's wake-up and the next one's launch (the host's serial path), and from launch to wake-up; printed by
  // ndtpso_ctx_destroy
  double clk_host = 0., clk_wait = 0., clk_pre = 0.;
  unsigned long long clk_n = 0;
  std::chrono::steady_clock::time_point clk_wake{}, clk_enter{};
  // single alignments (align_once) are numbered; the kernel writes its number behind its result in the pinned slot
  unsigned long long align_issued = 0, align_seen = 0;
  uint32_t cluster_nonce = 0;
  int xcd_pref = 0;                   // the XCD this context's lone clusters sit on: contexts take the eight in turn
  bool inputs_pinned = false;         // `inputs` is a pinned host slot (the kernel fetches the table from there itself)
  const void* inputs = nullptr;       // [guess | deviation | pad to kGuessBytes | rand() table] of the alignment about to be launched:
                                      // `table` (uploaded) or a pinned slot the kernel reads in place (ndtpso_map_align)
  // Batches whose cell tables keep overflowing (ndtpso_align_pairs*): the fused kernel counts the alignments whose occupied
  // box outgrew the table sized for two workgroups per compute unit into a pinned word; when more than a quarter of a
  // call's pairs did, the next calls of the same configuration start with the largest table instead (one workgroup per
  // compute unit) -- a scheduling decision only: the results do not depend on it
  uint32_t* pairs_fb = nullptr;
  DevBuf redo_list;                   // [count, pair ...] of a redo launch on clusters (k_redo_list)
  uint32_t fb_seen = 0, fb_last_pairs = 0;
  uint64_t fb_key = 0;
  bool fb_big_first = false, fb_overflowed = true;
  int fb_overflowed_calls = 0;
  int fb_big_calls = 0;  // calls since the largest table was put first (it is tried without every 64 calls)
  void* result_pinned = nullptr;      // pinned landing slot of one alignment's pose / cost / statistics (align_once)
  hipEvent_t result_event = nullptr;
  // ndtpso_map_align_batch: one pinned result slot per job of a launch (kJobSlotBytes each), the device's copies of the results
  // and of the staged rand() tables, and the jobs' numbers -- a counter of its own: the slots are not the single path's
  void* jobs_pinned = nullptr;
  size_t jobs_pinned_cap = 0;
  DevBuf jobs_out, jobs_table;
  DevBuf search_costs, search_keys, search_cand;  // ndtpso_map_search: a cost per node, the best-K lists, the exact mode's candidates
  void* search_pinned = nullptr;      // ndtpso_map_search_batch: the candidates' fp64 costs, written by the rescoring launch itself
  size_t search_pinned_cap = 0;
  uint32_t jobs_issued = 0;
  bool map_jobs_big_lds = false;      // ndtpso_map_update_batch: k_map_pack_jobs may take the whole LDS (set once per context)
};

namespace {

int fail(ndtpso_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

#define HIP_TRY(ctx, expr)                                                                         \
  do {                                                                                             \
    hipError_t e__ = (expr);                                                                       \
    if (e__ != hipSuccess)                                                                         \
      return fail((ctx), NDTPSO_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));        \
  } while (0)

bool is_pow2_double(double v) {
  int e;
  return v > 0. && std::frexp(v, &e) == 0.5;
}

int make_grid(const ndtpso_grid* grid, GridP* g) {
  if (!grid || !(grid->cell_side > 0.) || grid->width == 0 || grid->height == 0) return NDTPSO_E_ARG;
  g->hw = grid->width / 2.;
  g->hh = grid->height / 2.;
  g->cs = grid->cell_side;
  g->cs_pow2 = is_pow2_double(grid->cell_side) ? 1 : 0;
  g->inv_cs = 1. / grid->cell_side;
  // the reference keeps both counts in uint16_t (include/ndtpso_slam/ndtframe.h:32); a frame that would wrap them is refused
  const double w = std::ceil(grid->width / grid->cell_side), h = std::ceil(grid->height / grid->cell_side);
  if (!(w >= 1. && w <= 65535. && h >= 1. && h <= 65535.)) return NDTPSO_E_ARG;
  g->W = (uint16_t)w;  // ndtframe.cpp:27
  g->H = (uint16_t)h;  // ndtframe.cpp:28
  return NDTPSO_OK;
}

// conservative staging window covering [xmin,xmax] x [ymin,ymax] (metres), clipped to the grid
WinP make_window(const GridP& g, double xmin, double xmax, double ymin, double ymax, int rec_cap) {
  auto cell = [&](double v, double h) { return (int)std::floor((v + h) / g.cs); };
  int x0 = std::max(0, cell(xmin, g.hw) - 1), x1 = std::min(g.W - 1, cell(xmax, g.hw) + 1);
  int y0 = std::max(0, cell(ymin, g.hh) - 1), y1 = std::min(g.H - 1, cell(ymax, g.hh) + 1);
  if (x1 < x0) x1 = x0;
  if (y1 < y0) y1 = y0;
  WinP w;
  w.x0 = x0;
  w.y0 = y0;
  w.w = x1 - x0 + 1;
  w.h = y1 - y0 + 1;
  w.n_words = (w.w * w.h + 31) / 32;
  w.rec_cap = std::max(rec_cap, 1);
  return w;
}

// The beam directions of a scan geometry, on the device: (cos, sin) of index_to_angle(i) (core.h:40-42: fp32 multiply,
// fp32 add) from one glibc sincos() of the widened angle each -- what laser_to_point (core.h:45-47) compiles to with
// GCC.  They depend on the geometry only, so they are computed once per geometry on the host (the same libm the
// reference would run on) and kept in HBM; a few geometries are cached (a robot with a front and a back lidar
// alternates between two, launch/lidar_front.launch / lidar_back.launch).
int beam_directions(ndtpso_ctx* c, const ndtpso_scan_geom* s, const double2** out) {
  BeamDirs* hit = nullptr;
  for (BeamDirs& b : c->beam_dirs)
    if (b.n == s->n_beams && b.amin == s->min_angle && b.ainc == s->angle_increment && b.buf.p) hit = &b;
  if (!hit) {
    BeamDirs& b = c->beam_dirs[c->beam_dirs_next];
    c->beam_dirs_next = (c->beam_dirs_next + 1) % (unsigned)(sizeof(c->beam_dirs) / sizeof(c->beam_dirs[0]));
    std::vector<double> host(2 * (size_t)s->n_beams);
    for (uint32_t i = 0; i < s->n_beams; ++i) {
      const float theta = (float)i * s->angle_increment + s->min_angle;  // (this file is built with -ffp-contract=off)
      ::sincos((double)theta, &host[2 * i + 1], &host[2 * i]);
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // a launch still reading the slot's previous table
    for (ndtpso_ctx::PipeLane& l : c->lanes)
      if (l.stream) HIP_TRY(c, hipStreamSynchronize(l.stream));
    HIP_TRY(c, b.buf.reserve(host.size() * 8));
    HIP_TRY(c, hipMemcpy(b.buf.p, host.data(), host.size() * 8, hipMemcpyHostToDevice));
    b.n = s->n_beams;
    b.amin = s->min_angle;
    b.ainc = s->angle_increment;
    hit = &b;
  }
  *out = (const double2*)hit->buf.p;
  return NDTPSO_OK;
}

int make_scan(ndtpso_ctx* c, const ndtpso_scan_geom* s, ScanP* p, const double2** dirs) {
  p->n_beams = (int)s->n_beams;
  p->amin = s->min_angle;
  p->ainc = s->angle_increment;
  p->rmax = s->max_range;
  p->eps = s->laser_ignore_epsilon;
  return beam_directions(c, s, dirs);
}

PsoP make_pso(const ndtpso_pso_config* c, int waves, int mode, bool swarm_global = false) {
  PsoP p;
  p.P = c->population;
  p.I = c->iterations;
  // items per wave and evaluation round.  Two, except for large swarms: a gbest update costs the tail of ONE round in
  // re-evaluations, which at 2048 particles is nothing (0.1 % with rounds of 61), while every round costs its barrier
  // and the ramp-down of its last waves -- config 5: 167.7 ms per 256 pairs with two items per wave, 162.6 with four
  // (158.1 -> 152.2 in the fp32 mode); at 70 particles four items lose 1.5 % (config 3) to 8 % (30 x 50).
  int k = (swarm_global && c->population >= 512) ? 4 : 2;  // (only the HBM-swarm copies of the PSO deal more than two: KGEN)
  if (const char* e = std::getenv("NDTPSO_GROUP")) k = std::max(1, std::atoi(e));  // tuning knob
  if (!swarm_global && k > 2) k = 2;
  p.G = std::min(std::max(waves * k, 1), std::max(c->population, 1));
  // light wave (PsoP::light): rounds of k x (waves - 1) + 1, wave 0 takes one item and does the commits and the generator
  static const bool light = [] {
    const char* e = std::getenv("NDTPSO_LIGHT_WAVE");  // tuning knob: =0 deals every wave two items
    return !(e && e[0] == '0');
  }();
  // (not for the fp64 score: its evaluations are three times as long, the light wave's idle half-round costs more
  // than the commits and the generator it hides -- 7.11 against 6.84 ms per 512 pairs)
  p.light = (light && k >= 2 && waves >= 2 && mode != NDTPSO_SCORE_F64) ? k : 0;  // items per wave other than wave 0
  if (p.light) p.G = std::min(k * (waves - 1) + 1, std::max(c->population, 1));
  p.w = c->w;
  p.c1 = c->c1;
  p.c2 = c->c2;
  p.wdamp = c->w_damping;
  return p;
}

// Waves per workgroup for the PSO kernels.  The kernels are compiled for <= 128 VGPRs, i.e. 16 waves per CU.
// With many alignments in flight two 8-wave workgroups per CU (when their LDS fits twice) overlap each other's
// serial phases; a lone alignment, or one whose LDS needs more than half a CU, gets all 16 waves.
int pick_waves(int P, int lds_bytes, unsigned n_jobs, unsigned n_cus = 0) {
  if (const char* e = std::getenv("NDTPSO_WAVES")) {  // tuning knob
    const int w = std::atoi(e);
    if (w >= 1 && w <= 16) return w;
  }
  // two 8-wave workgroups per CU only when there are more alignments than compute units to pair up
  int w = (n_jobs > std::max(1u, n_cus) && lds_bytes <= kMaxLds / 2) ? 8 : 16;
  while (w > 1 && w / 2 >= P) w /= 2;  // never more than ~2 waves per particle
  return w;
}

// Which score-loop variant a launch uses, and its LDS layout.
//   path 2 (dense fast path): fp32 score, power-of-two cell side, and the dense table fits in LDS.
struct Plan {
  int path;  // 0 division + bitmap, 1 pow2 + bitmap, 2 dense
  Layout L;
  DenseP dn;
  int dense_cap;  // cell-table entries provisioned (fused kernel: the window is chosen per alignment)
  bool shrunk;    // ... fewer than the static window's: an alignment's box may not fit (kStatusNeedsBitmap)
  bool boxy;      // ... fewer than half of them: the box of scan B's disc will rarely fit beside scan A's -> the kernels that carry the
                  // box guard (box_guard_wg).  (The benchmark's table is 86 % of its static window and every disc fits; at 52 - 57 %
                  // -- 361 / 541 beams, 0.3 m cells -- most discs still fit and the copies' flags cost 3 - 7 %.)
};
// Plan overrides, per host thread: what the start-up check of the exact mode (ndtpso_selftest.inc) uses to send ONE small
// problem through every kernel instantiation the dispatchers below can reach -- the swarm's home, the table entries' form, the
// box-guard copies and the cluster form are otherwise picked by the problem's size.  -1 / 0: as planned.  Results never depend on
// them (every form returns the same poses: that is what the check compares).
struct PlanForce {
  int swarm_hbm = -1;     // 1: the swarm in its HBM workspace although it would fit LDS
  int byte_entries = -1;  // 0: table entries in 16-byte units (PATH 2) although the records lie below 64 KB (PATH 3)
  int table_side = 0;     // > 0: the fused kernels' dense table provisioned as side x side entries (a shrunk table)
  int boxy = -1;          // 1 / 0: the box-guard copies / the plain ones, whatever the table's share of the static window
  int cluster = -1;       // 1 / 0: a batch as clusters of workgroups / one workgroup per alignment, whatever its size
  int pair = -1;          // 1 / 0: the kernels that score two items per wave / one, whatever the scan's length (k_align_pairs<..., PAIR>)
};
thread_local PlanForce t_plan_force;
thread_local bool t_in_exact_check = false;  // this thread is running the start-up check of the exact mode (ndtpso_selftest.inc)
// NDTPSO_NO_REDO (diagnostics: what the main launch alone leaves flagged) -- not for the start-up check's own batches
static bool no_redo_requested() { return !t_in_exact_check && std::getenv("NDTPSO_NO_REDO") != nullptr; }
// what the last main (ungated) launch of this thread was: k_align_pairs / k_align instantiation as
// PATH | CL << 4 | ARB << 5 | NOCLIP << 6 | SWARM << 7 | BOX << 9 | (fused pairs kernel) << 10 | (fp64 score) << 11 | (two items per wave) << 12
thread_local uint32_t t_last_launch = 0;
constexpr uint32_t launch_code(bool f64, int path, bool cl, bool arb, bool noclip, int swarm, bool box, bool pairs, bool two_items = false) {
  return (uint32_t)path | (uint32_t)cl << 4 | (uint32_t)arb << 5 | (uint32_t)noclip << 6 | (uint32_t)swarm << 7 | (uint32_t)box << 9 |
         (uint32_t)pairs << 10 | (uint32_t)f64 << 11 | (uint32_t)two_items << 12;
}

// `wn` is the staging window: final for a prebuilt table; for the fused pairs kernel (dynamic_window) it is the
// static range box -- the worst case the bitmap form must hold -- while the dense form sizes its window per
// alignment and its table is provisioned as large as still leaves two workgroups per CU (else as large as
// fits).  Preference: dense over bitmap (measured, profiles/r01_occupancy_study.md: dense at one workgroup per
// CU still beats bitmap at two), swarm in LDS over swarm in HBM.
// allow_global: when neither form fits, read the table from its HBM image (path 4 / 5; kernels that stage a prebuilt
// table only -- a long-lived map can hold more built cells than LDS has room for).
// big_table (fused pairs kernel, a redo launch): the largest table a workgroup can hold, whatever that does to the number of
// workgroups per compute unit -- for the alignments whose box did not fit the table of the first launch
struct PlanAsk {
  bool dynamic_window = false;  // the fused pairs kernel: `wn` is the static range box, the dense table sized per alignment
  bool allow_dense = true;
  bool allow_global = false;
  bool exact = false;           // the swarm keeps the arbitration's four arrays
  bool big_table = false;
};
bool make_plan(int mode, const GridP& g, const WinP& wn, int n_max, int P, const PlanAsk& ask, Plan* plan) {
  const bool dynamic_window = ask.dynamic_window, allow_dense = ask.allow_dense, allow_global = ask.allow_global, exact = ask.exact,
             big_table = ask.big_table;
  const int bitmap_path = g.cs_pow2 ? 1 : 0;
  plan->shrunk = false;
  plan->boxy = false;
  int force = -1;
  if (const char* e = std::getenv("NDTPSO_PATH")) force = std::atoi(e);  // tuning knob
  // (fp64 score: the dense form exists in the fused pairs kernel only -- dynamic_window -- and needs every record below 64 KB)
  const bool d64_ok = allow_dense && mode == kScoreF64 && dynamic_window && force != 0 && force != 1 &&
                      kCtrlBytes + d64_rec_bytes(wn.rec_cap + 1) <= 65536;
  const bool dense_ok = (allow_dense && mode == kScoreF32 && force != 0 && force != 1) || d64_ok;
  const bool force_global = allow_global && (force == 4 || force == 5);
  for (int swarm_global = (t_plan_force.swarm_hbm == 1 && P > 0) ? 1 : 0; swarm_global < 2 && !force_global; ++swarm_global) {
    if (swarm_global && P <= 0) break;
    if (dense_ok) {
      const int full_w = wn.w + 1, full_h = wn.h + 1;
      Layout Ld = make_layout(wn.n_words, wn.rec_cap, n_max, P, mode, full_w, full_h, swarm_global != 0, exact, dynamic_window);
      int cap = dense_entries(full_w, full_h);
      if (dynamic_window && !big_table && t_plan_force.table_side > 0 && t_plan_force.table_side * t_plan_force.table_side < full_w * full_h) {
        const int side = t_plan_force.table_side;  // (the start-up check: a table of this size, see PlanForce)
        Ld = make_layout((side * side + 31) / 32, wn.rec_cap, n_max, P, mode, side, side, swarm_global != 0, exact, dynamic_window);
        cap = dense_entries(side, side);
      } else if (dynamic_window && Ld.total > (big_table ? kMaxLds : kMaxLds / 2)) {
        // shrink the provisioned (square) table until two workgroups fit per CU, else until one does;
        // never below 64 x 64 cells
        for (int limit : {kMaxLds / 2, kMaxLds}) {
          if (big_table && limit != kMaxLds) continue;
          bool found = false;
          auto fits = [&](int side, Layout* out) {
            *out = make_layout((side * side + 31) / 32, wn.rec_cap, n_max, P, mode, side, side, swarm_global != 0, exact, dynamic_window);
            return out->total <= limit;
          };
          for (int side = (int)std::sqrt((double)(full_w * full_h)); side >= 64; side -= 4) {
            Layout Lt;
            if (fits(side, &Lt)) {
              // (to the cell: a room at 0.25 m is ~18 000 cells, the table of the four-cell step below ended 4 % short of it)
              for (int up = 3; up >= 1; --up) {
                Layout Lu;
                if (fits(side + up, &Lu)) {
                  Lt = Lu;
                  side += up;
                  break;
                }
              }
              Ld = Lt;
              cap = dense_entries(side, side);
              found = true;
              break;
            }
          }
          if (found) break;
        }
      }
      if (Ld.total <= kMaxLds) {
        plan->path = d64_ok ? (8 | bitmap_path) : 2;
        plan->L = Ld;
        plan->dn = make_dense(g, wn, Ld);
        plan->dense_cap = cap;
        plan->shrunk = cap < dense_entries(full_w, full_h);
        plan->boxy = plan->shrunk && (long)cap * 2 < (long)dense_entries(full_w, full_h);
        // (fp64 score: its table, next to 48-byte records, is smaller still; below a quarter of the static window not even the
        // room's own box fits it often enough to pay for the copies' flags -- measured: 0.3 m cells + 10-13 %, 0.25 m - 3 %)
        if (d64_ok && (long)cap * 4 < (long)dense_entries(full_w, full_h)) plan->boxy = false;
        if (t_plan_force.boxy >= 0) plan->boxy = t_plan_force.boxy != 0;
        return true;
      }
    }
    const Layout Lb = make_layout(wn.n_words, wn.rec_cap, n_max, P, mode, 0, 0, swarm_global != 0, exact, dynamic_window);
    if (Lb.total <= kMaxLds) {
      plan->path = bitmap_path;
      plan->L = Lb;
      plan->dn = DenseP{0, 0, 0, 0, 0, 0, 0., 0.};
      plan->dense_cap = 0;
      return true;
    }
    plan->L = Lb;
  }
  plan->path = bitmap_path;
  plan->dn = DenseP{0, 0, 0, 0, 0, 0, 0., 0.};
  plan->dense_cap = 0;
  if (allow_global) {
    for (int swarm_global = 0; swarm_global < 2; ++swarm_global) {
      if (swarm_global && P <= 0) break;
      const Layout Lg = make_layout(0, 0, n_max, P, mode, 0, 0, swarm_global != 0, exact);
      if (Lg.total <= kMaxLds) {
        plan->path = bitmap_path | 4;
        plan->L = Lg;
        return true;
      }
    }
  }
  return false;
}

// cos and sin of a pose's heading as the reference obtains them.  transform_point (core.h:28-31) takes both of the
// same argument, which GCC -- the compiler the reference is built with -- turns into ONE sincos() call; glibc's sincos
// differs from its cos / sin in the last bit for about 0.15 % of arguments (measured), enough to move a transformed
// point by an ulp.  So: sincos, explicitly, whatever this translation unit's compiler would have made of two calls.
struct CosSin {
  double c, s;
};
CosSin host_cos_sin(double th) {
  CosSin r;
  ::sincos(th, &r.s, &r.c);
  return r;
}

bool trans_is_zero(const double t[3]) {  // Vector3d::isZero(1e-6), ndtframe.cpp:152
  return std::fabs(t[0]) <= 1e-6 && std::fabs(t[1]) <= 1e-6 && std::fabs(t[2]) <= 1e-6;
}

template <typename K>
hipError_t allow_big_lds(K kernel) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
}

// the kernels that exist with two items per wave (k_align_pairs<..., PAIR = true>: short scans): the fp32 score's dense form
// with byte entries, no clipping trips, the swarm in LDS, no box-guard copy -- with and without arbitration
template <int MODE, int PATH, bool CL, bool NOCLIP, int SWARM, bool BOX>
constexpr bool pair_items_kernel() {
  return MODE == kScoreF32 && PATH == 3 && !CL && NOCLIP && SWARM == 0 && !BOX;
}
template <int MODE, int PATH, bool CL, bool ARB, bool NOCLIP, int SWARM, bool BOX, typename... Args>
void launch_pairs_pair_items(dim3 grid, dim3 block, int lds, hipStream_t stream, Args... args) {
  if constexpr (pair_items_kernel<MODE, PATH, CL, NOCLIP, SWARM, BOX>()) {
    static const hipError_t big = allow_big_lds(k_align_pairs<MODE, PATH, CL, ARB, NOCLIP, SWARM, BOX, true>);  // once per instantiation
    (void)big;
    hipLaunchKernelGGL((k_align_pairs<MODE, PATH, CL, ARB, NOCLIP, SWARM, BOX, true>), grid, block, lds, stream, args...);
  }
}
// a gated launch of a kernel that strides (gate_strides): a function template, so that k_align_pairs_s exists only for those
template <int MODE, int PATH, bool CL, bool ARB, bool NOCLIP, int SWARM, bool BOX, typename... Args>
void launch_pairs_gated(dim3 grid, dim3 block, int lds, hipStream_t stream, Args... args) {
  if constexpr (gate_strides<MODE, PATH, CL>()) {
    static const hipError_t big = allow_big_lds(k_align_pairs_s<MODE, PATH, ARB, NOCLIP, SWARM, BOX>);  // once per instantiation
    (void)big;
    hipLaunchKernelGGL((k_align_pairs_s<MODE, PATH, ARB, NOCLIP, SWARM, BOX>), grid, block, lds, stream, args...);
  }
}

int check_pso(ndtpso_ctx* ctx, const ndtpso_pso_config* cfg) {
  if (!cfg || cfg->population < 1 || cfg->iterations < 0) return fail(ctx, NDTPSO_E_ARG, "bad PSO config");
  return NDTPSO_OK;
}
int check_mode(ndtpso_ctx* ctx, int mode) {
  if (mode != NDTPSO_SCORE_F32 && mode != NDTPSO_SCORE_F64 && mode != NDTPSO_SCORE_EXACT) return fail(ctx, NDTPSO_E_ARG, "bad score mode");
  return NDTPSO_OK;
}

// The score mode a table is aligned with, and its plan.  The exact mode is the fp32 score with arbitration where the table
// takes the dense form (plan.path == 2), else the fp64 score itself; the other two modes run as asked.  `ok`: the plan fits
// (make_plan); the plan of a failure is still the last form tried.  What a caller refuses beyond that -- a swarm in HBM, a form
// its kernels do not have -- it says itself, at the call.
struct ScorePlan {
  bool ok;
  int mode;         // NDTPSO_SCORE_F32 or NDTPSO_SCORE_F64
  bool arbitrates;  // the fp32 score, arbitrating in fp64
  Plan plan;
};
ScorePlan resolve_score_plan(int asked, const GridP& g, const WinP& wn, int n_max, int P, PlanAsk ask) {
  ScorePlan r;
  r.mode = asked;
  r.arbitrates = false;
  if (asked == NDTPSO_SCORE_EXACT) {
    ask.exact = true;
    if (make_plan(NDTPSO_SCORE_F32, g, wn, n_max, P, ask, &r.plan) && r.plan.path == 2) {
      r.ok = r.arbitrates = true;
      r.mode = NDTPSO_SCORE_F32;
      return r;
    }
    r.mode = NDTPSO_SCORE_F64;
    ask.exact = false;
  }
  r.ok = make_plan(r.mode, g, wn, n_max, P, ask, &r.plan);
  return r;
}
// a table built ahead of the alignment (k_align, k_cost_batch, the job kernels): either form in LDS, else read from its HBM image
PlanAsk prebuilt_table_ask() {
  PlanAsk ask;
  ask.allow_global = true;
  return ask;
}

int exact_mode_resolve(ndtpso_ctx* c, int* mode);  // ndtpso_selftest.inc: the start-up check of NDTPSO_SCORE_EXACT
int exact_jobs_resolve(ndtpso_ctx* c, int asked, int* mode);  // ... and its second part, the arbitrating job kernels (ndtpso_map_align_batch)

}  // namespace

extern "C" {

int ndtpso_ctx_create(int device, ndtpso_ctx** out) {
  if (!out) return NDTPSO_E_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return NDTPSO_E_HIP;
  ndtpso_ctx* c = new ndtpso_ctx();
  c->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&c->own_stream) != hipSuccess) {
    delete c;
    return NDTPSO_E_HIP;
  }
  c->stream = c->own_stream;
  {
    static std::atomic<unsigned> n_contexts{0};
    c->xcd_pref = (int)(n_contexts.fetch_add(1) & 7u);
  }
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c->n_cus = cus;
  }
  hipError_t e = hipSuccess;
  if (e == hipSuccess) e = allow_big_lds(k_build_table);
#define BIG_PATHS(K, ...)                                                      \
  if (e == hipSuccess) e = allow_big_lds(K<kScoreF32, 0 __VA_ARGS__>);         \
  if (e == hipSuccess) e = allow_big_lds(K<kScoreF32, 1 __VA_ARGS__>);         \
  if (e == hipSuccess) e = allow_big_lds(K<kScoreF32, 2 __VA_ARGS__>);         \
  if (e == hipSuccess) e = allow_big_lds(K<kScoreF64, 0 __VA_ARGS__>);         \
  if (e == hipSuccess) e = allow_big_lds(K<kScoreF64, 1 __VA_ARGS__>);
#define COMMA ,
  BIG_PATHS(k_cost_batch, COMMA false)
  BIG_PATHS(k_cost_batch, COMMA true)
  BIG_PATHS(k_align, COMMA false)
  BIG_PATHS(k_align, COMMA true)
  BIG_PATHS(k_align_pairs, COMMA false)
  BIG_PATHS(k_align_pairs, COMMA true)
  if (e == hipSuccess) e = allow_big_lds(k_align_pairs<kScoreF32, 3, false>);
  if (e == hipSuccess) e = allow_big_lds(k_align_pairs<kScoreF32, 3, true>);
  if (e == hipSuccess) e = allow_big_lds(k_align_pairs<kScoreF64, 8, false>);
  if (e == hipSuccess) e = allow_big_lds(k_align_pairs<kScoreF64, 9, false>);
  // exact mode (arbitrating variants of the fp32-score dense kernels)
  if (e == hipSuccess) e = allow_big_lds(k_align_pairs<kScoreF32, 2, false, true>);
  if (e == hipSuccess) e = allow_big_lds(k_align_pairs<kScoreF32, 2, true, true>);
  if (e == hipSuccess) e = allow_big_lds(k_align_pairs<kScoreF32, 3, false, true>);
  if (e == hipSuccess) e = allow_big_lds(k_align_pairs<kScoreF32, 3, true, true>);
  if (e == hipSuccess) e = allow_big_lds(k_align_pairs<kScoreF32, 3, false, false, true, 0>);
  if (e == hipSuccess) e = allow_big_lds(k_align_pairs<kScoreF32, 2, false, false, true, 0>);
  if (e == hipSuccess) e = allow_big_lds(k_align_pairs<kScoreF32, 2, false, true, true, 0>);
  if (e == hipSuccess) e = allow_big_lds(k_align_pairs<kScoreF32, 3, false, true, true, 0>);
  if (e == hipSuccess) e = allow_big_lds(k_align_pairs<kScoreF32, 3, false, false, true, 1>);
  if (e == hipSuccess) e = allow_big_lds(k_align_pairs<kScoreF32, 2, false, false, true, 1>);
  if (e == hipSuccess) e = allow_big_lds(k_align_pairs<kScoreF32, 2, false, true, true, 1>);
  if (e == hipSuccess) e = allow_big_lds(k_align_pairs<kScoreF32, 3, false, true, true, 1>);
  // (the copies that carry the box guard: tables smaller than the static window)
  if (e == hipSuccess) e = allow_big_lds(k_align_pairs<kScoreF32, 2, false, false, true, 0, true>);
  if (e == hipSuccess) e = allow_big_lds(k_align_pairs<kScoreF32, 3, false, false, true, 0, true>);
  if (e == hipSuccess) e = allow_big_lds(k_align_pairs<kScoreF32, 2, false, true, true, 0, true>);
  if (e == hipSuccess) e = allow_big_lds(k_align_pairs<kScoreF32, 3, false, true, true, 0, true>);
  if (e == hipSuccess) e = allow_big_lds(k_align_pairs<kScoreF32, 2, false, false, false, 2, true>);
  if (e == hipSuccess) e = allow_big_lds(k_align_pairs<kScoreF32, 3, false, false, false, 2, true>);
  if (e == hipSuccess) e = allow_big_lds(k_align_pairs<kScoreF32, 2, false, true, false, 2, true>);
  if (e == hipSuccess) e = allow_big_lds(k_align_pairs<kScoreF32, 3, false, true, false, 2, true>);
  if (e == hipSuccess) e = allow_big_lds(k_align_pairs<kScoreF64, 8, false, false, false, 2, true>);
  if (e == hipSuccess) e = allow_big_lds(k_align_pairs<kScoreF64, 9, false, false, false, 2, true>);
  if (e == hipSuccess) e = allow_big_lds(k_align<kScoreF32, 2, false, true>);
  if (e == hipSuccess) e = allow_big_lds(k_align<kScoreF32, 2, true, true>);
  if (e == hipSuccess) e = align_jobs_allow_big_lds();  // the job kernels (ndtpso_map_align_batch; ndtpso_align_jobs.hip)
#define GLOBAL_PATHS(K, ...)                                                   \
  if (e == hipSuccess) e = allow_big_lds(K<kScoreF32, 4 __VA_ARGS__>);         \
  if (e == hipSuccess) e = allow_big_lds(K<kScoreF32, 5 __VA_ARGS__>);         \
  if (e == hipSuccess) e = allow_big_lds(K<kScoreF64, 4 __VA_ARGS__>);         \
  if (e == hipSuccess) e = allow_big_lds(K<kScoreF64, 5 __VA_ARGS__>);
  GLOBAL_PATHS(k_cost_batch, COMMA false)
  GLOBAL_PATHS(k_cost_batch, COMMA true)
  GLOBAL_PATHS(k_align, COMMA false)
  GLOBAL_PATHS(k_align, COMMA true)
#undef GLOBAL_PATHS
#undef COMMA
#undef BIG_PATHS
  if (e != hipSuccess) {
    (void)hipStreamDestroy(c->own_stream);
    delete c;
    return NDTPSO_E_HIP;
  }
  *out = c;
  return NDTPSO_OK;
}

void ndtpso_ctx_destroy(ndtpso_ctx* c) {
  if (c && c->clk_n)
    std::fprintf(stderr, "ndtpso: host clock over %llu alignments (us): wake-up to next launch %.1f (of which inside the align call %.1f), launch to wake-up %.1f\n",
                 c->clk_n, 1e6 * c->clk_host / c->clk_n, 1e6 * c->clk_pre / c->clk_n, 1e6 * c->clk_wait / c->clk_n);
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  for (DevBuf* b : {&c->image, &c->rows, &c->xy, &c->xy2, &c->ranges, &c->ranges2, &c->poses, &c->costs, &c->dump,
                    &c->small, &c->table, &c->out, &c->seeds, &c->ws, &c->gate, &c->cluster_xc, &c->ximg, &c->jobs_out, &c->jobs_table,
                    &c->search_costs, &c->search_keys, &c->search_cand})
    b->release();
  for (BeamDirs& b : c->beam_dirs) b.buf.release();
  c->pinned.release();
  for (ndtpso_ctx::PipeLane& l : c->lanes) {
    if (l.stream) (void)hipStreamSynchronize(l.stream);
    l.ws.release();
    l.gate.release();
    l.ximg.release();
    if (l.done) (void)hipEventDestroy(l.done);
    if (l.stream) (void)hipStreamDestroy(l.stream);
  }
  if (c->pipe_in) (void)hipEventDestroy(c->pipe_in);
  if (c->result_event) (void)hipEventDestroy(c->result_event);
  if (c->result_pinned) (void)hipHostFree(c->result_pinned);
  if (c->jobs_pinned) (void)hipHostFree(c->jobs_pinned);
  if (c->search_pinned) (void)hipHostFree(c->search_pinned);
  if (c->pairs_fb) (void)hipHostFree(c->pairs_fb);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;
}

const char* ndtpso_last_error(const ndtpso_ctx* c) { return c ? c->err.c_str() : "null context"; }

int ndtpso_set_stream(ndtpso_ctx* c, void* s) {
  if (!c) return NDTPSO_E_ARG;
  hipStream_t ns = s ? reinterpret_cast<hipStream_t>(s) : c->own_stream;
  if (ns != c->stream) HIP_TRY(c, c->pinned.settle());
  c->stream = ns;
  return NDTPSO_OK;
}

int ndtpso_pipeline_flush(ndtpso_ctx* c, int keep_newest) {
  if (!c || keep_newest < 0) return NDTPSO_E_ARG;
  for (ndtpso_ctx::PipeLane& l : c->lanes) {
    if (!l.pending) continue;
    if ((unsigned long long)keep_newest >= c->pipe_calls - l.ticket) continue;  // one of the newest calls: left in flight
    HIP_TRY(c, hipStreamWaitEvent(c->stream, l.done, 0));
    l.pending = false;
  }
  return NDTPSO_OK;
}

int ndtpso_set_pipeline_depth(ndtpso_ctx* c, int depth) {
  if (!c || depth < 1 || depth > ndtpso_ctx::kMaxPipe) return fail(c, NDTPSO_E_ARG, "pipeline depth must be 1 or 2");
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = ndtpso_pipeline_flush(c, 0)) return rc;
  if (depth > 1) {
    if (!c->pipe_in) HIP_TRY(c, hipEventCreateWithFlags(&c->pipe_in, hipEventDisableTiming));
    for (int i = 0; i < depth; ++i) {
      ndtpso_ctx::PipeLane& l = c->lanes[i];
      if (!l.stream) HIP_TRY(c, hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking));
      if (!l.done) HIP_TRY(c, hipEventCreateWithFlags(&l.done, hipEventDisableTiming));
    }
  }
  c->pipe_depth = depth;
  return NDTPSO_OK;
}

int ndtpso_synchronize(ndtpso_ctx* c) {
  if (!c) return NDTPSO_E_ARG;
  if (int rc = ndtpso_pipeline_flush(c, 0)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return NDTPSO_OK;
}

size_t ndtpso_rand_draws(const ndtpso_pso_config* cfg) {
  if (!cfg) return 0;
  return 3u + 3u * (size_t)cfg->population + 6u * (size_t)cfg->population * (size_t)cfg->iterations;
}

// ---- K3 ------------------------------------------------------------------------------------------

int ndtpso_scan_to_points(ndtpso_ctx* c, const float* ranges, const ndtpso_scan_geom* geom, const double trans[3],
                          double* xy_out, uint32_t* n_out) {
  if (!c || !ranges || !geom || !xy_out || !n_out || geom->n_beams == 0) return fail(c, NDTPSO_E_ARG, "null argument");
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t nb = geom->n_beams;
  HIP_TRY(c, c->ranges.reserve(nb * 4));
  HIP_TRY(c, c->xy.reserve(nb * 16));
  HIP_TRY(c, c->small.reserve(256));
  HIP_TRY(c, hipMemcpyAsync(c->ranges.p, ranges, nb * 4, hipMemcpyHostToDevice, c->stream));
  const double zero[3] = {0., 0., 0.};
  const double* t = trans ? trans : zero;
  const int do_trans = trans_is_zero(t) ? 0 : 1;
  const CosSin cs = host_cos_sin(t[2]);
  ScanP sp;
  const double2* dirs = nullptr;
  if (int rc = make_scan(c, geom, &sp, &dirs)) return rc;
  hipLaunchKernelGGL(k_scan_to_points, dim3(1), dim3(1024), kCtrlBytes, c->stream, (const float*)c->ranges.p,
                     sp, dirs, do_trans, cs.c, cs.s, t[0], t[1], (double2*)c->xy.p,
                     (uint32_t*)c->small.p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(n_out, c->small.p, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (*n_out) HIP_TRY(c, hipMemcpy(xy_out, c->xy.p, (size_t)*n_out * 16, hipMemcpyDeviceToHost));
  return NDTPSO_OK;
}

static int build_from_device_points(ndtpso_ctx* c, const ndtpso_grid* grid, const GridP& g, const WinP& wn, int n) {
  c->have_ref = false;  // the staged image is about to be overwritten: no table until this one is complete
  const Layout L = make_layout(wn.n_words, wn.rec_cap, std::max(n, 1), 0, 2);
  if (L.total > kMaxLds) return fail(c, NDTPSO_E_CAPACITY, "reference table does not fit in LDS");
  HIP_TRY(c, c->image.reserve(image_bytes(wn.n_words, wn.rec_cap)));
  HIP_TRY(c, c->rows.reserve(sizeof(CellRow) * (size_t)std::max(n, 1)));
  HIP_TRY(c, c->small.reserve(256));
  hipLaunchKernelGGL(k_build_table, dim3(1), dim3(1024), L.total, c->stream, (const double2*)c->xy.p, n, g, wn, L,
                     (unsigned char*)c->image.p, (CellRow*)c->rows.p, (uint32_t*)c->small.p);
  HIP_TRY(c, hipGetLastError());
  uint32_t n_rows = 0;
  ImageHeader hdr;
  HIP_TRY(c, hipMemcpyAsync(&n_rows, c->small.p, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(&hdr, c->image.p, sizeof(hdr), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (hdr.status & 1u) return fail(c, NDTPSO_E_CAPACITY, "a reference point fell outside the staging window");
  if (hdr.status & 2u) return fail(c, NDTPSO_E_CAPACITY, "more built cells than record capacity");
  c->grid = *grid;
  c->g = g;
  c->wn = wn;
  c->n_rows = n_rows;
  c->have_ref = true;
  return NDTPSO_OK;
}

int ndtpso_ref_from_points(ndtpso_ctx* c, const ndtpso_grid* grid, const double* xy, uint32_t n) {
  if (!c || (!xy && n)) return fail(c, NDTPSO_E_ARG, "null argument");
  GridP g;
  if (make_grid(grid, &g) != NDTPSO_OK) return fail(c, NDTPSO_E_ARG, "bad grid");
  HIP_TRY(c, hipSetDevice(c->device));
  double xmin = 0., xmax = 0., ymin = 0., ymax = 0.;
  bool any = false;
  for (uint32_t i = 0; i < n; ++i) {
    const double x = xy[2 * i], y = xy[2 * i + 1];
    if (!(std::fabs(x) < g.hw && std::fabs(y) < g.hh)) continue;  // dropped by addPoint anyway
    if (!any) {
      xmin = xmax = x;
      ymin = ymax = y;
      any = true;
    } else {
      xmin = std::min(xmin, x);
      xmax = std::max(xmax, x);
      ymin = std::min(ymin, y);
      ymax = std::max(ymax, y);
    }
  }
  const WinP wn = make_window(g, xmin, xmax, ymin, ymax, (int)(n / 3) + 1);
  HIP_TRY(c, c->xy.reserve((size_t)std::max<uint32_t>(n, 1) * 16));
  if (n) HIP_TRY(c, hipMemcpyAsync(c->xy.p, xy, (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
  return build_from_device_points(c, grid, g, wn, (int)n);
}

int ndtpso_ref_from_scan(ndtpso_ctx* c, const ndtpso_grid* grid, const float* ranges, const ndtpso_scan_geom* geom,
                         const double trans[3]) {
  if (!c || !ranges || !geom || geom->n_beams == 0) return fail(c, NDTPSO_E_ARG, "null argument");
  GridP g;
  if (make_grid(grid, &g) != NDTPSO_OK) return fail(c, NDTPSO_E_ARG, "bad grid");
  HIP_TRY(c, hipSetDevice(c->device));
  const double zero[3] = {0., 0., 0.};
  const double* t = trans ? trans : zero;
  const size_t nb = geom->n_beams;
  HIP_TRY(c, c->ranges.reserve(nb * 4));
  HIP_TRY(c, c->xy.reserve(nb * 16));
  HIP_TRY(c, c->small.reserve(256));
  HIP_TRY(c, hipMemcpyAsync(c->ranges.p, ranges, nb * 4, hipMemcpyHostToDevice, c->stream));
  const int do_trans = trans_is_zero(t) ? 0 : 1;
  const CosSin cs = host_cos_sin(t[2]);
  ScanP sp;
  const double2* dirs = nullptr;
  if (int rc = make_scan(c, geom, &sp, &dirs)) return rc;
  hipLaunchKernelGGL(k_scan_to_points, dim3(1), dim3(1024), kCtrlBytes, c->stream, (const float*)c->ranges.p,
                     sp, dirs, do_trans, cs.c, cs.s, t[0], t[1], (double2*)c->xy.p,
                     (uint32_t*)c->small.p);
  HIP_TRY(c, hipGetLastError());
  uint32_t n = 0;
  HIP_TRY(c, hipMemcpyAsync(&n, c->small.p, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const double r = (double)geom->max_range;
  const double cx = do_trans ? t[0] : 0., cy = do_trans ? t[1] : 0.;
  const WinP wn = make_window(g, cx - r, cx + r, cy - r, cy + r, (int)(n / 3) + 1);
  return build_from_device_points(c, grid, g, wn, (int)n);
}

int ndtpso_ref_set_cells(ndtpso_ctx* c, const ndtpso_grid* grid, uint32_t n_cells, const int32_t* index,
                         const double* mean, const double* icov) {
  if (!c || (n_cells && (!index || !mean || !icov))) return fail(c, NDTPSO_E_ARG, "null argument");
  GridP g;
  if (make_grid(grid, &g) != NDTPSO_OK) return fail(c, NDTPSO_E_ARG, "bad grid");
  HIP_TRY(c, hipSetDevice(c->device));
  int x0 = 0, x1 = 0, y0 = 0, y1 = 0;
  for (uint32_t i = 0; i < n_cells; ++i) {
    if (index[i] < 0 || index[i] >= g.W * g.H) return fail(c, NDTPSO_E_ARG, "cell index outside the grid");
    const int ix = index[i] % g.W, iy = index[i] / g.W;
    if (i == 0) {
      x0 = x1 = ix;
      y0 = y1 = iy;
    } else {
      x0 = std::min(x0, ix);
      x1 = std::max(x1, ix);
      y0 = std::min(y0, iy);
      y1 = std::max(y1, iy);
    }
  }
  WinP wn;
  wn.x0 = x0;
  wn.y0 = y0;
  wn.w = x1 - x0 + 1;
  wn.h = y1 - y0 + 1;
  wn.n_words = (wn.w * wn.h + 31) / 32;
  wn.rec_cap = std::max<int>((int)n_cells, 1);
  // (a table too large for LDS is read from this image where it lies in HBM: paths 4 / 5 of the kernels)
  // pack the LDS image on the host: bitmap words {bits, exclusive prefix}, records in ascending cell order
  const size_t bytes = image_bytes(wn.n_words, wn.rec_cap);
  std::vector<unsigned char> img(bytes, 0);
  ImageHeader* hdr = reinterpret_cast<ImageHeader*>(img.data());
  uint2* bm = reinterpret_cast<uint2*>(img.data() + kImageHeaderBytes);
  double2* t_mean = reinterpret_cast<double2*>(img.data() + image_mean_offset(wn.n_words));
  double2* t_ab = reinterpret_cast<double2*>(img.data() + image_ab_offset(wn.n_words, wn.rec_cap));
  double2* t_cd = reinterpret_cast<double2*>(img.data() + image_cd_offset(wn.n_words, wn.rec_cap));
  std::vector<std::pair<int, uint32_t>> order(n_cells);
  for (uint32_t i = 0; i < n_cells; ++i) {
    const int ix = index[i] % g.W, iy = index[i] / g.W;
    const int k = (iy - wn.y0) * wn.w + (ix - wn.x0);
    if ((bm[k >> 5].x >> (k & 31)) & 1u) return fail(c, NDTPSO_E_ARG, "duplicate cell index");
    bm[k >> 5].x |= 1u << (k & 31);
    order[i] = {k, i};
  }
  std::sort(order.begin(), order.end());
  uint32_t run = 0;
  for (int w = 0; w < wn.n_words; ++w) {
    bm[w].y = run;
    run += (uint32_t)__builtin_popcount(bm[w].x);
  }
  for (uint32_t s = 0; s < n_cells; ++s) {
    const uint32_t i = order[s].second;
    t_mean[s] = make_double2(mean[2 * i], mean[2 * i + 1]);
    t_ab[s] = make_double2(icov[4 * i], icov[4 * i + 1]);
    t_cd[s] = make_double2(icov[4 * i + 2], icov[4 * i + 3]);
  }
  hdr->n_built = n_cells;
  hdr->n_created = n_cells;
  c->have_ref = false;
  HIP_TRY(c, c->image.reserve(bytes));
  HIP_TRY(c, hipMemcpyAsync(c->image.p, img.data(), bytes, hipMemcpyHostToDevice, c->stream));
  if (n_cells) {
    hipLaunchKernelGGL(k_fill_chol, dim3((n_cells + 255) / 256), dim3(256), 0, c->stream, (unsigned char*)c->image.p,
                       wn.n_words, wn.rec_cap, (int)n_cells);
    HIP_TRY(c, hipGetLastError());
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->grid = *grid;
  c->g = g;
  c->wn = wn;
  c->n_rows = 0;
  c->have_ref = true;
  return NDTPSO_OK;
}

int ndtpso_ref_get_cells(ndtpso_ctx* c, ndtpso_cell_row* rows, uint32_t max_rows, uint32_t* n_rows) {
  if (!c || !n_rows) return fail(c, NDTPSO_E_ARG, "null argument");
  if (!c->have_ref) return fail(c, NDTPSO_E_STATE, "no reference table");
  *n_rows = c->n_rows;
  const uint32_t n = std::min(max_rows, c->n_rows);
  if (n && rows) {
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpy(rows, c->rows.p, sizeof(CellRow) * (size_t)n, hipMemcpyDeviceToHost));
  }
  return NDTPSO_OK;
}

int ndtpso_points_to_cells(ndtpso_ctx* c, const ndtpso_grid* grid, const double* xy, uint32_t n, const double trans[3],
                           double* xy_out, int32_t* cell_idx) {
  if (!c || (n && (!xy || !xy_out || !cell_idx))) return fail(c, NDTPSO_E_ARG, "null argument");
  GridP g;
  if (make_grid(grid, &g) != NDTPSO_OK) return fail(c, NDTPSO_E_ARG, "bad grid");
  if (n == 0) return NDTPSO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, c->xy.reserve((size_t)n * 16));
  HIP_TRY(c, c->xy2.reserve((size_t)n * 16));
  HIP_TRY(c, c->dump.reserve((size_t)n * 4));
  HIP_TRY(c, hipMemcpyAsync(c->xy.p, xy, (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
  const int do_trans = trans ? 1 : 0;
  const CosSin cs = host_cos_sin(trans ? trans[2] : 0.);
  const double tc = trans ? cs.c : 1., ts = trans ? cs.s : 0.;
  hipLaunchKernelGGL(k_points_to_cells, dim3((n + 255) / 256), dim3(256), 0, c->stream, (const double2*)c->xy.p, (int)n,
                     g, do_trans, tc, ts, trans ? trans[0] : 0., trans ? trans[1] : 0., (double2*)c->xy2.p,
                     (int32_t*)c->dump.p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(xy_out, c->xy2.p, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(cell_idx, c->dump.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return NDTPSO_OK;
}

int ndtpso_scan_to_cells(ndtpso_ctx* c, const float* ranges, const ndtpso_scan_geom* geom, const double trans[3],
                         const ndtpso_grid* grid, double* xy_out, int32_t* cell_idx, uint32_t* n_out) {
  if (!c || !ranges || !geom || !xy_out || !cell_idx || !n_out || geom->n_beams == 0)
    return fail(c, NDTPSO_E_ARG, "null argument");
  GridP g;
  if (make_grid(grid, &g) != NDTPSO_OK) return fail(c, NDTPSO_E_ARG, "bad grid");
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t nb = geom->n_beams;
  HIP_TRY(c, c->ranges.reserve(nb * 4));
  HIP_TRY(c, c->xy.reserve(nb * 16));
  HIP_TRY(c, c->dump.reserve(nb * 4));
  HIP_TRY(c, c->small.reserve(256));
  HIP_TRY(c, hipMemcpyAsync(c->ranges.p, ranges, nb * 4, hipMemcpyHostToDevice, c->stream));
  const double zero[3] = {0., 0., 0.};
  const double* t = trans ? trans : zero;
  const int do_trans = trans_is_zero(t) ? 0 : 1;
  const CosSin cs = host_cos_sin(t[2]);
  ScanP sp;
  const double2* dirs = nullptr;
  if (int rc = make_scan(c, geom, &sp, &dirs)) return rc;
  hipLaunchKernelGGL(k_scan_to_cells, dim3(1), dim3(1024), kCtrlBytes, c->stream, (const float*)c->ranges.p, sp, dirs,
                     do_trans, cs.c, cs.s, t[0], t[1], g, (double2*)c->xy.p, (int32_t*)c->dump.p,
                     (uint32_t*)c->small.p);
  HIP_TRY(c, hipGetLastError());
  // one synchronisation: the count travels with the (full-size) payload
  HIP_TRY(c, hipMemcpyAsync(n_out, c->small.p, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(xy_out, c->xy.p, nb * 16, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(cell_idx, c->dump.p, nb * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return NDTPSO_OK;
}

int ndtpso_occupancy_values(ndtpso_ctx* c, const ndtpso_grid* grid, double og_cell_size, uint32_t n_cells,
                            const int32_t* index, const double* mean, const double* icov, int8_t* values) {
  if (!c || !(og_cell_size > 0.) || (n_cells && (!index || !mean || !icov || !values)))
    return fail(c, NDTPSO_E_ARG, "null argument");
  GridP g;
  if (make_grid(grid, &g) != NDTPSO_OK) return fail(c, NDTPSO_E_ARG, "bad grid");
  const int per_cell = (int)std::floor(grid->cell_side / og_cell_size);  // ndtframe.cpp:70
  if (n_cells == 0 || per_cell <= 0) return NDTPSO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t total = (size_t)n_cells * per_cell * per_cell;
  HIP_TRY(c, c->seeds.reserve((size_t)n_cells * 4));
  HIP_TRY(c, c->xy.reserve((size_t)n_cells * 16));
  HIP_TRY(c, c->xy2.reserve((size_t)n_cells * 32));
  HIP_TRY(c, c->dump.reserve(total));
  HIP_TRY(c, hipMemcpyAsync(c->seeds.p, index, (size_t)n_cells * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->xy.p, mean, (size_t)n_cells * 16, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->xy2.p, icov, (size_t)n_cells * 32, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_occupancy_values, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, (int)n_cells,
                     per_cell, og_cell_size, g.hw, g.hh, g.W, g.H, (const int32_t*)c->seeds.p, (const double2*)c->xy.p,
                     (const double4*)c->xy2.p, (int8_t*)c->dump.p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(values, c->dump.p, total, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return NDTPSO_OK;
}

int ndtpso_cells_build_windowed(ndtpso_ctx* c, uint32_t n_cells, ndtpso_cell_window* cells, const uint32_t* pts_offset,
                                const double* pts_xy) {
  if (!c || (n_cells && (!cells || !pts_offset))) return fail(c, NDTPSO_E_ARG, "null argument");
  if (n_cells == 0) return NDTPSO_OK;
  const size_t n_pts = pts_offset[n_cells];
  if (n_pts && !pts_xy) return fail(c, NDTPSO_E_ARG, "null points");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, c->rows.reserve(sizeof(CellWindow) * (size_t)n_cells));
  HIP_TRY(c, c->seeds.reserve(4 * ((size_t)n_cells + 1)));
  HIP_TRY(c, c->xy.reserve(std::max<size_t>(n_pts, 1) * 16));
  HIP_TRY(c, hipMemcpyAsync(c->rows.p, cells, sizeof(CellWindow) * (size_t)n_cells, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->seeds.p, pts_offset, 4 * ((size_t)n_cells + 1), hipMemcpyHostToDevice, c->stream));
  if (n_pts) HIP_TRY(c, hipMemcpyAsync(c->xy.p, pts_xy, n_pts * 16, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_cells_build_windowed, dim3((n_cells + 255) / 256), dim3(256), 0, c->stream, (CellWindow*)c->rows.p,
                     (int)n_cells, (const uint32_t*)c->seeds.p, (const double2*)c->xy.p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(cells, c->rows.p, sizeof(CellWindow) * (size_t)n_cells, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->n_rows = 0;  // rows buffer reused
  return NDTPSO_OK;
}

// ---- K1 ------------------------------------------------------------------------------------------

// cost_function for m poses against a table image and a point list that are both on the device
static int cost_launch(ndtpso_ctx* c, const unsigned char* image, const GridP& g, const WinP& wn, const double2* d_xy,
                       uint32_t n, const double* poses, uint32_t m, int mode, double* costs, int32_t* cell_idx) {
  Plan plan;
  if (!make_plan(mode, g, wn, std::max<int>((int)n, 1), 0, prebuilt_table_ask(), &plan))
    return fail(c, NDTPSO_E_CAPACITY, "points do not fit in LDS");
  const Layout& L = plan.L;
  HIP_TRY(c, c->poses.reserve((size_t)m * 24));
  HIP_TRY(c, c->costs.reserve((size_t)m * 8));
  if (cell_idx) HIP_TRY(c, c->dump.reserve((size_t)m * std::max<uint32_t>(n, 1) * 4));
  HIP_TRY(c, hipMemcpyAsync(c->poses.p, poses, (size_t)m * 24, hipMemcpyHostToDevice, c->stream));
  const int waves = 16;
  const int grid = (int)std::min<uint32_t>((m + waves - 1) / waves, 512u);
#define LAUNCH_COST(MODE, PATH, DUMP)                                                                             \
  hipLaunchKernelGGL((k_cost_batch<MODE, PATH, DUMP>), dim3(grid), dim3(waves * 64), L.total, c->stream,          \
                     image, d_xy, (int)n, g, wn, L, plan.dn,                                                      \
                     (const double*)c->poses.p, (int)m, (double*)c->costs.p, (int32_t*)c->dump.p)
#define LAUNCH_COST2(MODE, PATH) \
  do { if (cell_idx) LAUNCH_COST(MODE, PATH, true); else LAUNCH_COST(MODE, PATH, false); } while (0)
  if (mode == NDTPSO_SCORE_F32) {
    switch (plan.path) {
      case 2: LAUNCH_COST2(kScoreF32, 2); break;
      case 1: LAUNCH_COST2(kScoreF32, 1); break;
      case 4: LAUNCH_COST2(kScoreF32, 4); break;
      case 5: LAUNCH_COST2(kScoreF32, 5); break;
      default: LAUNCH_COST2(kScoreF32, 0);
    }
  } else {
    switch (plan.path) {
      case 1: LAUNCH_COST2(kScoreF64, 1); break;
      case 4: LAUNCH_COST2(kScoreF64, 4); break;
      case 5: LAUNCH_COST2(kScoreF64, 5); break;
      default: LAUNCH_COST2(kScoreF64, 0);
    }
  }
#undef LAUNCH_COST2
#undef LAUNCH_COST
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(costs, c->costs.p, (size_t)m * 8, hipMemcpyDeviceToHost, c->stream));
  if (cell_idx && n) HIP_TRY(c, hipMemcpyAsync(cell_idx, c->dump.p, (size_t)m * n * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (mode == NDTPSO_SCORE_F32) {
    // a NaN score in the fp32 form: a pose touched a cell whose inverse covariance has no Cholesky factor (make_chol).
    // The fp64 form evaluates the reference's expression as it stands; the batch is redone with it.
    for (uint32_t i = 0; i < m; ++i)
      if (costs[i] != costs[i]) return cost_launch(c, image, g, wn, d_xy, n, poses, m, NDTPSO_SCORE_F64, costs, nullptr);
  }
  return NDTPSO_OK;
}

int ndtpso_cost_batch(ndtpso_ctx* c, const double* xy, uint32_t n, const double* poses, uint32_t m, int mode,
                      double* costs, int32_t* cell_idx) {
  if (!c || (!xy && n) || !poses || !costs || m == 0) return fail(c, NDTPSO_E_ARG, "null argument");
  if (int rc = check_mode(c, mode)) return rc;
  if (!c->have_ref) return fail(c, NDTPSO_E_STATE, "no reference table");
  if (mode == NDTPSO_SCORE_EXACT) mode = NDTPSO_SCORE_F64;  // a cost has nothing to arbitrate: the fp64 score (as ndtpso_map_cost)
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, c->xy2.reserve((size_t)std::max<uint32_t>(n, 1) * 16));
  if (n) HIP_TRY(c, hipMemcpyAsync(c->xy2.p, xy, (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
  return cost_launch(c, (const unsigned char*)c->image.p, c->g, c->wn, (const double2*)c->xy2.p, n, poses, m, mode, costs,
                     cell_idx);
}

// ---- K2 ------------------------------------------------------------------------------------------

// c->table of a single alignment: [guess, deviation (6 doubles, padded to 64 bytes) | std::rand() table]
constexpr size_t kGuessBytes = 64;

// work to enqueue right after the alignment kernel, before the host waits for it (runs behind it on the stream)
struct AfterLaunch {
  int (*fn)(void*);
  void* arg;
};

// where one alignment's inputs live on the device: table image + its grid/window, new-frame points (count known
// to the host, or only an upper bound with the count itself on the device)
struct AlignSrc {
  const unsigned char* image;
  GridP g;
  WinP wn;
  const double2* xy;
  uint32_t n;
  const uint32_t* n_ptr;
  bool want_cost = true;  // false: the caller asked for the pose only (NDTFrame::align does) -- the exact mode then skips
                          // the fp64 score of the returned pose, which nothing else needs
  // Late window binding (resident map, dense form): `wn` is an UPPER BOUND the host planned the LDS layout with, and the
  // kernel takes the table's real window and record count from the map's header on the device -- {n_created, n_built,
  // status, n_words, x0, x1, y0, y1} -- which the pack kernel ahead of it on the stream has written.  The host then need
  // not wait for that header before it launches the alignment.
  const uint32_t* late_hdr = nullptr;
};

// How many workgroups share one alignment (cluster mode, see ClusterP).  One item per wave and round: enough waves
// for the whole swarm (P + 1 items in the first round), 4 per workgroup (one per SIMD) for small swarms, 8 for larger
// ones, at most 32 workgroups -- the shapes tests/campaigns/cluster_sweep.py found fastest (30 x 50: 8 x 4 waves, 0.43 ms vs
// 0.63 ms on one workgroup; 70 x 70: 0.64 ms vs 1.49 ms).  NDTPSO_CLUSTER=0 keeps a lone alignment on one
// workgroup, =K forces K workgroups; NDTPSO_CLUSTER_WAVES sets the waves per workgroup.
static void cluster_shape(int P, bool swarm_in_lds, bool allow, int* K, int* cw) {
  *K = 1;
  *cw = (P + 1 <= 32) ? 4 : 8;
  if (const char* e = std::getenv("NDTPSO_CLUSTER_WAVES")) *cw = std::min(kClusterMaxThreads / 64, std::max(1, std::atoi(e)));
  int k = std::min(32, (P + 1 + *cw - 1) / *cw);
  if (P + 1 <= 16) k = 0;  // one workgroup already has a wave per item
  if (const char* e = std::getenv("NDTPSO_CLUSTER")) k = std::min(128, std::max(0, std::atoi(e)));
  if (allow && swarm_in_lds && k >= 2) *K = k;
}
// Exchange slots of the clusters of one launch (ClusterP::xc).  They need no zeroing: a slot counts only when it carries
// the launch's nonce and the round's number.
static int cluster_slots(ndtpso_ctx* c, size_t xc_bytes, uint4** xc) {
  HIP_TRY(c, c->cluster_xc.reserve(xc_bytes));
  *xc = (uint4*)c->cluster_xc.p;
  return NDTPSO_OK;
}

// tags of a launch's exchange slots carry this number (ClusterP::nonce, all 32 bits of it: xslot_tag_a / _b)
static uint32_t next_cluster_nonce(ndtpso_ctx* c) {
  if (++c->cluster_nonce == 0u) c->cluster_nonce = 1u;
  return c->cluster_nonce;
}

// Room behind a cluster workgroup's LDS layout for the two ready-made next proposals of every coordinate (SpecP:
// 16 (P + 1) doubles), where it fits and the swarm is small enough for wave 0 to hold its comparisons (one per lane);
// NDTPSO_CLUSTER_SPEC=0 leaves it out (the usual commit and proposal steps: same results)
static void cluster_spec_room(int P, int* lds_total, ClusterP* cl) {
  const char* e = std::getenv("NDTPSO_CLUSTER_SPEC");
  if (e && e[0] == '0') return;
  const int at = round_up(*lds_total, 16), bytes = 16 * (P + 1) * 8;
  if (P > kWave || at + bytes > kMaxLds) return;
  cl->spec_off = at;
  *lds_total = at + bytes;
}
// NDTPSO_CLUSTER_SPREAD=1: a cluster's workgroups where the dispatcher puts consecutive ones (all eight XCDs) instead of on
// one XCD (ClusterP::one_xcd) -- for comparison; the results do not depend on it
static int cluster_one_xcd() {
  const char* e = std::getenv("NDTPSO_CLUSTER_SPREAD");
  return (e && e[0] == '1') ? 0 : 1;
}
// NDTPSO_CLUSTER_TEST_ABSENT=r (tests only): rank r of every cluster leaves immediately, so the others run into the
// bounded wait and the one-workgroup rerun is exercised
static int cluster_flags() {  // ClusterP::flags from the environment
  static const int f = [] {
    const char* e = std::getenv("NDTPSO_CLUSTER_HEARTBEAT");  // =0: no flow control between the exchange's rounds (as before round 5)
    return (e && e[0] == '0') ? kClusterNoHeartbeat : 0;
  }();
  return f;
}
static int cluster_test_absent() {
  // NDTPSO_CLUSTER_TEST_LAG=r (tests only): rank r dawdles 60 us in every round in which it has no item (ClusterP::absent = -(2 + r))
  if (const char* l = std::getenv("NDTPSO_CLUSTER_TEST_LAG")) return -(2 + std::max(0, std::atoi(l)));
  const char* e = std::getenv("NDTPSO_CLUSTER_TEST_ABSENT");
  return e ? std::atoi(e) : -1;
}
// a cluster must bring at least one and a half times the waves of one 16-wave workgroup to pay for its exchanges
// (measured, scripts/small_batch_check.py: 80 pairs of 70 x 70 on 3 x 8 waves 1.33 ms against 1.66 ms, 100 pairs on 2 x 8
// 1.82 against 1.68; twice the waves it was before the exchange went through tagged slots); forced shapes
// (NDTPSO_CLUSTER) are taken as given
static bool cluster_worthwhile(int K, int cw) { return std::getenv("NDTPSO_CLUSTER") != nullptr || K * cw >= 24; }

// The host's side of publish_pinned_word: spin on a word of pinned memory until the kernel has written `want` there.
// No event stands behind the kernel for this (the device would spend microseconds on it between two
// kernels, and the host would hear of the result later).  A kernel that died, or ended without reporting, must still end
// the wait: every 10 ms the stream is asked whether it is still busy -- not more often, because the query itself puts a
// marker into the queue, and a marker between two kernels of the live sequence costs the device 6 us.
static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#elif defined(__aarch64__)
  __asm__ __volatile__("yield");
#else
  std::this_thread::yield();
#endif
}

// How many CPUs this process may really keep busy: the affinity mask cut by the control group's quota (a container shows all of
// the box's logical CPUs and gives the process a fraction of them: the GPU boxes of this project 256 and 16).
static int host_cpu_budget() {
  static const int budget = [] {
    int n = (int)std::max(1u, std::thread::hardware_concurrency());
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0 && CPU_COUNT(&set) > 0) n = std::min(n, (int)CPU_COUNT(&set));
    double quota = 0.;
    if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {  // cgroup v2: "<quota us | max> <period us>"
      char q[64];
      double per = 0.;
      if (std::fscanf(f, "%63s %lf", q, &per) == 2 && q[0] != 'm' && per > 0.) quota = std::atof(q) / per;
      std::fclose(f);
    } else {
      double q = -1., per = 0.;
      if (FILE* fq = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
        if (std::fscanf(fq, "%lf", &q) != 1) q = -1.;
        std::fclose(fq);
      }
      if (FILE* fp = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
        if (std::fscanf(fp, "%lf", &per) != 1) per = 0.;
        std::fclose(fp);
      }
      if (q > 0. && per > 0.) quota = q / per;
    }
    if (quota >= 1.) n = std::min(n, (int)quota);
    if (const char* e = std::getenv("NDTPSO_CPU_BUDGET")) n = std::atoi(e);  // (tests)
    return std::max(1, n);
  }();
  return budget;
}
// The control group may be shared with OTHER processes (two processes of sixteen replicas each are the best way to serve 32:
// DESIGN 6) whose spinning threads this one cannot count -- but it can see their effect: cpu.stat's nr_throttled goes up whenever
// the group ran out of quota in a period.  Looked at no more than every 50 ms, by whichever waiting thread gets there first; a
// throttled period makes every wait of this process a polite one for the next two seconds.
static std::atomic<long long> g_throttle_look_ns{0}, g_polite_until_ns{0}, g_throttled_seen{-1};
static bool quota_is_biting() {
  const long long now = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
  long long last = g_throttle_look_ns.load(std::memory_order_relaxed);
  if (now - last > 50000000LL && g_throttle_look_ns.compare_exchange_strong(last, now, std::memory_order_relaxed)) {
    long long n = -1;
    for (const char* path : {"/sys/fs/cgroup/cpu.stat", "/sys/fs/cgroup/cpu/cpu.stat"}) {
      if (FILE* f = std::fopen(path, "r")) {
        char key[64];
        long long v;
        while (std::fscanf(f, "%63s %lld", key, &v) == 2)
          if (std::strcmp(key, "nr_throttled") == 0) n = v;
        std::fclose(f);
        break;
      }
    }
    const long long before = g_throttled_seen.exchange(n, std::memory_order_relaxed);
    if (n >= 0 && before >= 0 && n > before) g_polite_until_ns.store(now + 2000000000LL, std::memory_order_relaxed);
  }
  return now < g_polite_until_ns.load(std::memory_order_relaxed);
}
static std::atomic<int> g_word_waiters{0};              // host threads inside wait_pinned_word right now
static std::atomic<unsigned long long> g_polite_waits{0};    // waits that slept instead of spinning
static std::atomic<unsigned long long> g_cluster_timeouts{0};  // alignments whose cluster ran into the bounded wait
static std::atomic<int> g_aligns_in_flight{0};                 // single alignments between launch and result, process-wide
static std::atomic<unsigned long long> g_crowded_aligns{0};    // alignments kept on one workgroup because too many were in flight
static std::atomic<unsigned long long> g_redo_cluster_launches{0};  // batches whose flagged pairs were given to clusters (align_pairs_dev_on_stream)

// One waiter spins: the word arrives a microsecond after the kernel wrote it, and a robot's one matcher thread has a CPU to
// itself.  MANY waiters must not: R replicas of the live sequence are R threads in this loop at once, and past the CPUs the
// process may use (host_cpu_budget) spinning threads take the time slices of the threads that have launches to make -- under a
// control group's quota worse than that: 32 threads spinning on a quota of 16 CPUs spend it in half of every 100 ms period and
// the WHOLE process is frozen for the other half (the 50 - 110 ms stalls and the fall of the aggregate rate beyond 16 replicas
// that round 5 put down to the hardware queues).  So: with more waiters than half the budget, a waiter sleeps between looks
// (20 us, the thread's timer slack set to 1 us: ~25 us per look) -- a scan of 350 us hears of its pose a dozen microseconds later
// and the process's CPU time goes to the threads that launch.  NDTPSO_WAIT=spin / sleep overrides the choice.
static int wait_pinned_word(ndtpso_ctx* c, const uint32_t* word, uint32_t want) {
  static const int policy = [] {
    const char* e = std::getenv("NDTPSO_WAIT");
    return !e ? 0 : (e[0] == 's' && e[1] == 'p' ? 1 : (e[0] == 's' && e[1] == 'l' ? 2 : 0));
  }();
  struct Count {
    Count() { g_word_waiters.fetch_add(1, std::memory_order_relaxed); }
    ~Count() { g_word_waiters.fetch_sub(1, std::memory_order_relaxed); }
  } counted;
  std::chrono::steady_clock::time_point last{};
  bool slept = false, throttled = false;
  for (unsigned spins = 1;; ++spins) {
    if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == want) return NDTPSO_OK;
    const bool crowded = policy == 2 || (policy == 0 && (2 * g_word_waiters.load(std::memory_order_relaxed) > host_cpu_budget() ||
                                                       ((spins & 1023u) == 65u && quota_is_biting()) || throttled));
    if (crowded) throttled = true;  // (once polite, polite to the end of this wait)
    if (crowded && spins > 64u) {  // (the first looks spin: a result that is all but there)
      static thread_local bool slack_set = false;
      if (!slack_set) {
        slack_set = true;
        (void)prctl(PR_SET_TIMERSLACK, 1000UL, 0UL, 0UL, 0UL);
      }
      if (!slept) {
        slept = true;
        g_polite_waits.fetch_add(1, std::memory_order_relaxed);
      }
      const timespec ts{0, 20000};
      (void)nanosleep(&ts, nullptr);
    } else {
      cpu_relax();
    }
    if ((spins & 4095u) == 0 || (crowded && (spins & 255u) == 0)) {
      const auto now = std::chrono::steady_clock::now();
      if (last.time_since_epoch().count() == 0) last = now;
      if (now - last < std::chrono::milliseconds(10)) continue;
      last = now;
      const hipError_t e = hipStreamQuery(c->stream);
      if (e == hipErrorNotReady) continue;
      if (e != hipSuccess) return fail(c, NDTPSO_E_HIP, std::string("while waiting for a kernel's word: ") + hipGetErrorString(e));
      if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == want) return NDTPSO_OK;
      return fail(c, NDTPSO_E_HIP, "kernel ended without reporting");
    }
  }
}

int ndtpso_process_counters(uint64_t* out, int n) {
  if (!out || n < 1) return NDTPSO_E_ARG;
  const uint64_t v[6] = {g_cluster_timeouts.load(), g_polite_waits.load(), (uint64_t)host_cpu_budget(), (uint64_t)g_word_waiters.load(),
                         g_crowded_aligns.load(), g_redo_cluster_launches.load()};
  for (int i = 0; i < n && i < 6; ++i) out[i] = v[i];
  return NDTPSO_OK;
}

// Whether `n` alignments about to be launched from this context may run on clusters, and their count among the process's
// alignments in flight until release() or the end of the scope.
// A cluster's workgroups wait for each other, which is safe only while every cluster in flight is resident: alignments launched
// from more host threads than the device has hardware queues to run side by side (16; a process's streams share them, and
// streams on one queue take turns) are the case in which some cluster's workgroups sit behind another stream's kernel while
// their siblings spin towards the exchange's bounded wait.  Past that many alignments in flight in the process, the next ones
// run on ONE workgroup each: half as fast, and they wait for nobody.  (NDTPSO_CLUSTER_MAX_INFLIGHT, default 16.)
struct ClusterAdmission {
  bool allow;
  ClusterAdmission(ndtpso_ctx* c, int n_aligns, bool allow_in = true) : allow(allow_in), n(n_aligns) {
    static const int max_in_flight = [] {
      const char* e = std::getenv("NDTPSO_CLUSTER_MAX_INFLIGHT");
      return e ? std::max(0, std::atoi(e)) : 16;
    }();
    if (allow && c->cluster_penalty > 0) {  // (after a timeout: note_cluster_timeout)
      --c->cluster_penalty;
      allow = false;
    }
    const int before = g_aligns_in_flight.fetch_add(n, std::memory_order_relaxed);
    if (allow && before + n > max_in_flight) {
      allow = false;
      g_crowded_aligns.fetch_add((unsigned long long)n, std::memory_order_relaxed);
    }
  }
  void release() {
    if (n) g_aligns_in_flight.fetch_sub(n, std::memory_order_relaxed);
    n = 0;
  }
  ~ClusterAdmission() { release(); }
  ClusterAdmission(const ClusterAdmission&) = delete;
  ClusterAdmission& operator=(const ClusterAdmission&) = delete;

 private:
  int n;
};

// An alignment's cluster ran into the bounded wait (it was not co-resident: device shared with other work): counted, and no
// new attempt from this context for the next 200 alignments (a robot's 5-20 s; one under the test hook).
static void note_cluster_timeout(ndtpso_ctx* c) {
  g_cluster_timeouts.fetch_add(1, std::memory_order_relaxed);
  c->cluster_penalty = cluster_test_absent() >= 0 ? 1 : 200;
}

// How many workgroups share each of the `n_units` alignments of a launch, and their waves.  `share_device`: a cluster per
// alignment only while the device has the compute units for all of them, and only one that pays for its exchanges.
static void cluster_launch_k(const ndtpso_ctx* c, int P, uint32_t n_units, bool allow, bool share_device, int* K, int* cw) {
  cluster_shape(P, true, allow, K, cw);
  if (!share_device) return;
  if (*K > 1) *K = std::min<int>(*K, c->n_cus / (int)std::min<uint32_t>(n_units, (uint32_t)c->n_cus));
  if (*K < 2 || !cluster_worthwhile(*K, *cw)) *K = 1;
}

// The rest of a launch's shape once K and the LDS plan are known (launch_pairs' plan depends on K): the ClusterP, and for
// K > 1 the items per round in `ps`, the speculation scratch behind `lds_total` (null: the caller's jobs have a layout each
// and make that room themselves) and `unit_slots`, the uint4 exchange slots one alignment needs -- the caller provides
// n_units * unit_slots of them as cl->xc.  `xcd`: the XCD of cluster 0.
static void cluster_launch_shape(ndtpso_ctx* c, int P, int K, int waves, uint32_t n_units, int xcd, const uint32_t* redo_list,
                                 uint32_t redo_mask, int* lds_total, PsoP* ps, ClusterP* cl, size_t* unit_slots) {
  *cl = ClusterP{K, 0, 0, cluster_test_absent(), nullptr, 0u, cluster_one_xcd() ? 1 + xcd : 0, (int)n_units, -1,
                 reinterpret_cast<double*>(const_cast<uint32_t*>(redo_list)) /* ClusterP::spec, on the host's side */,
                 cluster_flags() | (int)(redo_mask << kClusterRedoShift)};
  // (one XCD holds an eighth of the compute units: one XCD per cluster only while an XCD's share of the clusters finds a compute
  // unit per workgroup there; a forced K, a partitioned part, a batch that fills the device are spread as the dispatcher
  // spreads them instead of spinning to the exchange's timeout)
  if (((int)n_units + 7) / 8 * K > std::max(1, c->n_cus / 8)) cl->one_xcd = 0;
  *unit_slots = 0;
  if (K < 2) return;
  if (lds_total) cluster_spec_room(P, lds_total, cl);
  ps->G = std::min(std::max(P, 1), K * waves);  // one item per wave and round
  cl->stride = round_up(P + 1, 8);
  // two exchange buffers of `stride` slots and one slot per rank, padded to eight: the kernels address them by the same rule
  // (k_align_jobs in ndtpso_align_jobs.hip, k_align_pairs in ndtpso_pairs_body.inc)
  *unit_slots = 2 * (size_t)cl->stride + (size_t)round_up(K, 8);
  cl->nonce = next_cluster_nonce(c);
}

// A result slot -- [pose, cost | AlignStats] in doubles -- taken apart; a null destination is left out.
constexpr size_t kResultDoubles = 4 + sizeof(AlignStats) / 8;
static AlignStats result_of(const double* slot, double pose[3] = nullptr, double* cost = nullptr, ndtpso_align_stats* stats = nullptr) {
  AlignStats st;
  std::memcpy(&st, slot + 4, sizeof(st));
  if (pose) std::memcpy(pose, slot, 3 * sizeof(double));
  if (cost) *cost = slot[3];
  if (stats) std::memcpy(stats, slot + 4, sizeof(AlignStats));
  return st;
}
// the alignment of a shared or late-bound launch must be redone alone: with the fp64 score, behind the header, on one workgroup
static bool must_redo_alone(const AlignStats& st) { return (st.status & (kStatusNeedsF64 | kStatusLateOverflow | kStatusClusterTimeout)) != 0; }

static int align_once(ndtpso_ctx* c, const AlignSrc& src, const ndtpso_pso_config* cfg, uint32_t seed, bool have_table,
                      int mode, double host[kResultDoubles], bool allow_cluster = true,
                      AfterLaunch after = AfterLaunch{nullptr, nullptr}) {
  const uint32_t n = src.n;
  const ScorePlan resolved = resolve_score_plan(mode, src.g, src.wn, std::max<int>((int)n, 1), cfg->population, prebuilt_table_ask());
  if (!resolved.ok) return fail(c, NDTPSO_E_CAPACITY, "points + swarm do not fit in LDS");
  const Plan& plan = resolved.plan;
  const bool exact = resolved.arbitrates;
  mode = resolved.mode;
  if (src.late_hdr && plan.path != 2) return fail(c, NDTPSO_E_STATE, "late window binding needs the dense form");  // (the caller probes)
  const Layout& L = plan.L;
  double* d_out = (double*)c->out.p;  // [0..2] pose, [3] cost, then stats
  AlignStats* d_stats = reinterpret_cast<AlignStats*>(d_out + 4);
  if (!c->result_pinned) {
    HIP_TRY(c, hipHostMalloc(&c->result_pinned, 256, hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(c->result_pinned, 0, 256);
    HIP_TRY(c, hipEventCreateWithFlags(&c->result_event, hipEventDisableTiming));
  }
  int K, cw;
  const ClusterAdmission admitted(c, 1, allow_cluster);
  // (a lone alignment has the device to itself: no cap by compute units, and a cluster of any size is taken)
  cluster_launch_k(c, cfg->population, 1, admitted.allow, false, &K, &cw);
  const unsigned long long seq = ++c->align_issued;
  const bool staged_table = have_table && c->inputs_pinned;
  const int table_vec = (int)((ndtpso_rand_draws(cfg) * 4 + 15) / 16);
  if (staged_table) HIP_TRY(c, c->table.reserve(kGuessBytes + (size_t)K * (size_t)table_vec * 16));  // one copy per workgroup of the cluster
  if (L.swarm_global) HIP_TRY(c, c->ws.reserve((size_t)swarm_bytes(cfg->population, true, true) * (size_t)K));
  const int waves = K > 1 ? cw : pick_waves(cfg->population, L.total, 1);
  PsoP ps = make_pso(cfg, waves, mode, L.swarm_global != 0);
  ClusterP cl;
  int lds_total = L.total;
  size_t unit_slots = 0;
  // (the context's own XCD for its lone cluster: contexts of one process spread over the eight)
  cluster_launch_shape(c, cfg->population, K, waves, 1, c->xcd_pref, nullptr, 0, &lds_total, &ps, &cl, &unit_slots);
  if (K > 1)
    if (int rc = cluster_slots(c, unit_slots * sizeof(uint4), &cl.xc)) return rc;
#define LAUNCH_ALIGN_CA(MODE, PATH, CL, ARB)                                                                       \
  do {                                                                                                             \
  t_last_launch = launch_code(MODE == kScoreF64, PATH, CL, ARB, false, 0, false, false);                           \
  hipLaunchKernelGGL((k_align<MODE, PATH, CL, ARB>), dim3(CL ? cluster_grid(cl) : 1u), dim3(waves * 64), lds_total, c->stream, \
                     src.image, src.xy, (int)n, src.n_ptr, src.g, src.wn, L, plan.dn,                              \
                     ps, (const double*)c->inputs, (const double*)c->inputs + 3, seed,                             \
                     have_table && !staged_table ? (const int32_t*)((const unsigned char*)c->inputs + kGuessBytes) : nullptr, \
                     (unsigned char*)c->ws.p, d_out, src.want_cost ? d_out + 3 : nullptr, d_stats, cl,             \
                     (double*)c->result_pinned,                                                                    \
                     staged_table ? (const int4*)((const unsigned char*)c->inputs + kGuessBytes) : nullptr,        \
                     (int4*)((unsigned char*)c->table.p + kGuessBytes), table_vec,                                 \
                     (plan.path == 2 ? src.late_hdr : nullptr), dense_entries(plan.dn.dw, plan.dn.dh), src.wn.rec_cap,  \
                     (uint32_t)seq);                                                                               \
  } while (0)
#define LAUNCH_ALIGN_C(MODE, PATH, CL) LAUNCH_ALIGN_CA(MODE, PATH, CL, false)
#define LAUNCH_ALIGN(MODE, PATH) \
  do { if (K > 1) LAUNCH_ALIGN_C(MODE, PATH, true); else LAUNCH_ALIGN_C(MODE, PATH, false); } while (0)
  if (mode == NDTPSO_SCORE_F32 && exact) {  // (plan.path == 2, see above)
    if (K > 1) LAUNCH_ALIGN_CA(kScoreF32, 2, true, true); else LAUNCH_ALIGN_CA(kScoreF32, 2, false, true);
  } else if (mode == NDTPSO_SCORE_F32) {
    switch (plan.path) {
      case 2: LAUNCH_ALIGN(kScoreF32, 2); break;
      case 1: LAUNCH_ALIGN(kScoreF32, 1); break;
      case 4: LAUNCH_ALIGN(kScoreF32, 4); break;
      case 5: LAUNCH_ALIGN(kScoreF32, 5); break;
      default: LAUNCH_ALIGN(kScoreF32, 0);
    }
  } else {
    switch (plan.path) {
      case 1: LAUNCH_ALIGN(kScoreF64, 1); break;
      case 4: LAUNCH_ALIGN(kScoreF64, 4); break;
      case 5: LAUNCH_ALIGN(kScoreF64, 5); break;
      default: LAUNCH_ALIGN(kScoreF64, 0);
    }
  }
#undef LAUNCH_ALIGN
#undef LAUNCH_ALIGN_C
#undef LAUNCH_ALIGN_CA
  HIP_TRY(c, hipGetLastError());
  // The result comes back through a pinned slot and an event of its own: the host waits for the pose only, while what
  // `after` enqueues (the occupancy grid a committed speculative build still owes) runs in the shadow of the host's
  // wake-up.  (With a pageable destination the copy call itself blocked until the kernel was done, `after` was
  // enqueued late and then waited for: 30 us per scan on the live path.)
  if (after.fn)
    if (int rc = after.fn(after.arg)) return rc;
  static const bool host_clock = std::getenv("NDTPSO_HOST_CLOCK") != nullptr;
  std::chrono::steady_clock::time_point t_launch;
  if (host_clock) t_launch = std::chrono::steady_clock::now();
  if (int rc = wait_pinned_word(c, reinterpret_cast<const uint32_t*>(static_cast<const double*>(c->result_pinned) + 8), (uint32_t)seq)) return rc;
  c->align_seen = seq;
  if (host_clock) {
    const auto now = std::chrono::steady_clock::now();
    if (c->clk_wake.time_since_epoch().count()) {
      c->clk_host += std::chrono::duration<double>(t_launch - c->clk_wake).count();
      c->clk_pre += std::chrono::duration<double>(t_launch - c->clk_enter).count();
      c->clk_wait += std::chrono::duration<double>(now - t_launch).count();
      ++c->clk_n;
    }
    c->clk_wake = now;
  }
  std::memcpy(host, c->result_pinned, kResultDoubles * sizeof(double));
  if (K > 1 && (result_of(host).status & kStatusClusterTimeout)) {  // the cluster was not co-resident: one workgroup
    note_cluster_timeout(c);
    static bool logged = false;
    if (!logged) {
      logged = true;
      std::fprintf(stderr, "ndtpso: a cluster of %d workgroups did not meet within 20 ms (device shared?); alignments run on one workgroup for a while\n", K);
    }
    return align_once(c, src, cfg, seed, have_table, exact ? NDTPSO_SCORE_EXACT : mode, host, false);
  }
  return NDTPSO_OK;
}

static int align_finish(ndtpso_ctx* c, const AlignSrc& src, const ndtpso_pso_config* cfg, uint32_t seed, bool have_table,
                        int mode, double out_pose[3], double* out_cost, ndtpso_align_stats* stats,
                        AfterLaunch after = AfterLaunch{nullptr, nullptr}, bool allow_cluster = true);

// ndtpso_align; allow_cluster = false keeps the alignment on one workgroup (the start-up check runs both forms)
static int align_points(ndtpso_ctx* c, const double* xy, uint32_t n, const double guess[3], const double deviation[3],
                        const ndtpso_pso_config* cfg, uint32_t seed, const int32_t* rand_table, int mode, double out_pose[3],
                        double* out_cost, ndtpso_align_stats* stats, bool allow_cluster);

int ndtpso_align(ndtpso_ctx* c, const double* xy, uint32_t n, const double guess[3], const double deviation[3],
                 const ndtpso_pso_config* cfg, uint32_t seed, const int32_t* rand_table, int mode, double out_pose[3],
                 double* out_cost, ndtpso_align_stats* stats) {
  return align_points(c, xy, n, guess, deviation, cfg, seed, rand_table, mode, out_pose, out_cost, stats, true);
}

static int align_points(ndtpso_ctx* c, const double* xy, uint32_t n, const double guess[3], const double deviation[3],
                        const ndtpso_pso_config* cfg, uint32_t seed, const int32_t* rand_table, int mode, double out_pose[3],
                        double* out_cost, ndtpso_align_stats* stats, bool allow_cluster) {
  if (!c || (!xy && n) || !guess || !deviation || !out_pose) return fail(c, NDTPSO_E_ARG, "null argument");
  if (int rc = check_mode(c, mode)) return rc;
  if (int rc = check_pso(c, cfg)) return rc;
  if (!c->have_ref) return fail(c, NDTPSO_E_STATE, "no reference table");
  if (int rc = exact_mode_resolve(c, &mode)) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t n_draw = ndtpso_rand_draws(cfg);
  HIP_TRY(c, c->xy2.reserve((size_t)std::max<uint32_t>(n, 1) * 16));
  HIP_TRY(c, c->out.reserve(256));
  HIP_TRY(c, c->table.reserve(kGuessBytes + (rand_table ? n_draw * 4 : 0)));
  if (n) HIP_TRY(c, hipMemcpyAsync(c->xy2.p, xy, (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
  double gd[6] = {guess[0], guess[1], guess[2], deviation[0], deviation[1], deviation[2]};
  HIP_TRY(c, c->pinned.upload2(c->table.p, gd, sizeof(gd), kGuessBytes, rand_table, rand_table ? n_draw * 4 : 0, c->stream));
  c->inputs = c->table.p;
  c->inputs_pinned = false;
  const AlignSrc src{(const unsigned char*)c->image.p, c->g, c->wn, (const double2*)c->xy2.p, n, nullptr, out_cost != nullptr};
  return align_finish(c, src, cfg, seed, rand_table != nullptr, mode, out_pose, out_cost, stats, AfterLaunch{nullptr, nullptr}, allow_cluster);
}

// launch, fetch pose/cost/stats; an alignment the fp32 score flags (underflow regime, see ndtpso_kernels.hpp) is
// redone with the fp64 score
static int align_finish(ndtpso_ctx* c, const AlignSrc& src, const ndtpso_pso_config* cfg, uint32_t seed, bool have_table,
                        int mode, double out_pose[3], double* out_cost, ndtpso_align_stats* stats, AfterLaunch after,
                        bool allow_cluster) {
  double host[kResultDoubles];
  int rc = align_once(c, src, cfg, seed, have_table, mode, host, allow_cluster, after);
  if (rc != NDTPSO_OK) return rc;
  if (mode != NDTPSO_SCORE_F64 && (result_of(host).status & kStatusNeedsF64)) {
    static const bool log_redo = std::getenv("NDTPSO_LOG_REDO") != nullptr;  // diagnostics: how often this happens
    if (log_redo) std::fprintf(stderr, "ndtpso: alignment handed to the fp64-score kernel\n");
    rc = align_once(c, src, cfg, seed, have_table, NDTPSO_SCORE_F64, host);
    if (rc != NDTPSO_OK) return rc;
  }
  result_of(host, out_pose, out_cost, stats);
  return NDTPSO_OK;
}

// ---- fused pairs -----------------------------------------------------------------------------------

#include "ndtpso_pairs.inc"

#ifdef NDTPSO_VERIFY_MARGIN
// diagnostic builds only (tests/test_gpu_margin.py): per alignment of the fused-pairs launches since the last reset, kVerifyRow (24) doubles
int ndtpso_profile_verify_margin(double* out, uint32_t n_blocks, int reset) {
  if (n_blocks > kVerifyMaxBlocks) return NDTPSO_E_ARG;
  if (hipDeviceSynchronize() != hipSuccess) return NDTPSO_E_HIP;
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_verify), (size_t)n_blocks * kVerifyRow * sizeof(double)) != hipSuccess) return NDTPSO_E_HIP;
  if (reset) {
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_verify)) != hipSuccess || hipMemset(p, 0, sizeof(double) * kVerifyRow * kVerifyMaxBlocks) != hipSuccess)
      return NDTPSO_E_HIP;
  }
  return NDTPSO_OK;
}
#endif

#ifdef NDTPSO_TRACE_ARB
// diagnostic builds only (scripts/units_hbm_diag.py): the arbitration trace of the first n_blocks workgroups; reset: clear it
int ndtpso_profile_arb_trace(double* out, uint32_t n_blocks, int reset) {
  if (n_blocks > kTraceBlocks) return NDTPSO_E_ARG;
  if (hipDeviceSynchronize() != hipSuccess) return NDTPSO_E_HIP;
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_arbtrace), (size_t)n_blocks * kTraceDoubles * sizeof(double)) != hipSuccess) return NDTPSO_E_HIP;
  if (reset) {
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_arbtrace)) != hipSuccess || hipMemset(p, 0, sizeof(double) * kTraceDoubles * kTraceBlocks) != hipSuccess)
      return NDTPSO_E_HIP;
  }
  return NDTPSO_OK;
}
#endif

#ifdef NDTPSO_PHASE_BUDGET
// diagnostic builds only (scripts/phase_budget.py): the per-workgroup phase times of the last fused-pairs launches
int ndtpso_profile_phase_budget(uint32_t* out, uint32_t n_blocks) {
  if (!out || n_blocks > kBudgetMaxBlocks) return NDTPSO_E_ARG;
  if (hipDeviceSynchronize() != hipSuccess) return NDTPSO_E_HIP;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_budget), (size_t)n_blocks * 16 * sizeof(uint32_t)) != hipSuccess) return NDTPSO_E_HIP;
  return NDTPSO_OK;
}
#endif

}  // extern "C"

#include "ndtpso_map.inc"
#include "ndtpso_shard.inc"
#include "ndtpso_selftest.inc"
