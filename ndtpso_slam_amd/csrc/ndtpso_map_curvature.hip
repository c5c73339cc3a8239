// ndtpso_map_curvature.hip -- the kernel of ndtpso_map_curvature and ndtpso_map_curvature_batch: cost_function (core.cpp:26-48)
// with NDTCell::normalDistribution (ndtcell.cpp:70-78), differentiated twice by the pose.  The reference has no counterpart.  A
// translation unit of its own, as the search kernels are: nothing the kernels of the existing entries are compiled from changes.
//
// Per point in a built cell, with A = s_inv_covar (row-major a00 a01 a10 a11, not assumed symmetric), (rx, ry) the point turned by
// the heading, q = (rx, ry) + t, d = q - mean, Q = (d^T A) d and e = exp(-Q / 2) exactly as the fp64 score forms them:
//   B = A + A^T (b00 = 2 a00, b01 = a01 + a10, b11 = 2 a11),  v = B d,
//   g = (v0, v1, -ry v0 + rx v1)                                   dQ / d(tx, ty, theta)
//   h00, h01, h11 = b00, b01, b11;  h02 = -b00 ry + b01 rx;  h12 = -b01 ry + b11 rx
//   h22 = ry^2 b00 - 2 rx ry b01 + rx^2 b11 - (v0 rx + v1 ry)      d2Q
//   cost = -sum e,  gradient_k = sum e g_k / 2,  hessian_kl = sum e (h_kl / 2 - g_k g_l / 4)
// Cell membership is held fixed (the score is piecewise smooth).
//
// The cost is k_cost_batch's fp64 score bit for bit: the trips below restate score_trip<kScoreF64> (ndtpso_kernels.hpp: the same
// lookup, the same masked exp) and the terms go into the four lane accumulators in eval_pose_wave_t's order -- groups of four
// chunks, the chunks behind the last group into the first, then (a0 + a1) + (a2 + a3) through wave_sum.  The nine derivative sums
// have one lane accumulator each, fed point by point in the list's order, and a wave_sum each.  One wave owns one pose from the
// first point to the last: no atomics, no reduction across waves, so the ten sums are a pure function of (map, scan, pose).
#include "ndtpso_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "../../include/ndtpso_hip.h"

#include "ndtpso_device_common.inc"
#include "ndtpso_map_curvature.h"

namespace {

struct CurvatureAcc {
  double e[4];   // the cost's lane accumulators (eval_pose_wave_t)
  double g[3];   // sum e g_k / 2
  double h[6];   // sum e (h_kl / 2 - g_k g_l / 4): xx, xy, xth, yy, yth, thth
  uint32_t hit;  // points of this lane that landed in a built cell
};

// U chunks of 64 points from `base`: score_trip<kScoreF64, POW2, U, false>'s lookup and term, then the derivatives' share of each
// point while its rx, ry, d and A are still at hand.
template <bool POW2, int U>
__device__ __forceinline__ void curvature_trip(const GridP& g, const WinP& wn, const TableView& T, const double2* __restrict__ pts,
                                               int base, double c, double s, double tx, double ty, CurvatureAcc& acc) {
  const int lane = lane_id();
  double2 p[U];
#pragma unroll
  for (int u = 0; u < U; ++u) p[u] = pts[base + u * kWave + lane];

  double rx[U], ry[U], qx[U], qy[U];
  unsigned lin[U];
  bool ok[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    rx[u] = p[u].x * c - p[u].y * s;  // reference rounding, no fma (transform_point, core.h:28-31)
    ry[u] = p[u].x * s + p[u].y * c;
    qx[u] = rx[u] + tx;
    qy[u] = ry[u] + ty;
    const bool inframe = (int)(fabs(qx[u]) < g.hw) & (int)(fabs(qy[u]) < g.hh);  // strict bounds, ndtframe.cpp:242
    int ix, iy;
    cell_coords<POW2>(g, qx[u], qy[u], ix, iy);
    const bool wrap = (ix == g.W);  // fl(x + w/2) == w: the reference's linear index lands in the next row
    ix = wrap ? 0 : ix;
    iy = wrap ? iy + 1 : iy;
    const unsigned cx = (unsigned)(ix - wn.x0), cy = (unsigned)(iy - wn.y0);
    ok[u] = (int)inframe & (int)(cx < (unsigned)wn.w) & (int)(cy < (unsigned)wn.h);
    lin[u] = ok[u] ? __umul24(cy, (unsigned)wn.w) + cx : 0u;
  }

  unsigned long long w[U];
#pragma unroll
  for (int u = 0; u < U; ++u) w[u] = reinterpret_cast<const unsigned long long*>(T.bm)[lin[u] >> 5];

  unsigned slot[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const unsigned bits = (unsigned)w[u], pre = (unsigned)(w[u] >> 32), bit = lin[u] & 31u;
    ok[u] = (int)ok[u] & (int)((bits >> bit) & 1u);
    const unsigned sl = pre + __popc(bits & ((1u << bit) - 1u));
    slot[u] = ok[u] ? sl : 0u;
  }

  double2 m[U], ab[U], cd[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    m[u] = T.mean[slot[u]];
    ab[u] = T.ab[slot[u]];
    cd[u] = T.cd[slot[u]];
  }
  double d0[U], d1[U], e[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    d0[u] = qx[u] - m[u].x;
    d1[u] = qy[u] - m[u].y;
    const double r0 = d0[u] * ab[u].x + d1[u] * cd[u].x;  // (diff^T * inv_covar), ndtcell.cpp:73-75
    const double r1 = d0[u] * ab[u].y + d1[u] * cd[u].y;
    const double x = -(r0 * d0[u] + r1 * d1[u]) / 2.;
    e[u] = exp(ok[u] ? x : -(double)__builtin_inff());  // exp(-inf) = 0; a NaN exponent stays NaN (select, not fmin)
    acc.e[u] += e[u];
    acc.hit += ok[u] ? 1u : 0u;
  }
  // The derivatives, one point after the other (thirteen fp64 accumulators are live: the arithmetic is not unrolled against them).
  // A term of exactly +0. -- a miss, or an exponent below the subnormal range -- adds exactly zero to every sum: selected, not
  // multiplied, so that 0 * inf makes no NaN.  A NaN term makes every sum NaN.
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const double b00 = 2. * ab[u].x, b01 = ab[u].y + cd[u].x, b11 = 2. * cd[u].y;  // B = A + A^T
    const double v0 = b00 * d0[u] + b01 * d1[u], v1 = b01 * d0[u] + b11 * d1[u];
    const double g0 = v0, g1 = v1, g2 = -ry[u] * v0 + rx[u] * v1;
    const double h02 = -b00 * ry[u] + b01 * rx[u];
    const double h12 = -b01 * ry[u] + b11 * rx[u];
    const double h22 = ry[u] * ry[u] * b00 - 2. * rx[u] * ry[u] * b01 + rx[u] * rx[u] * b11 - (v0 * rx[u] + v1 * ry[u]);
    const bool live = !(e[u] == 0.);  // (a NaN is live)
    const double ee = e[u];
    acc.g[0] += live ? ee * g0 / 2. : 0.;
    acc.g[1] += live ? ee * g1 / 2. : 0.;
    acc.g[2] += live ? ee * g2 / 2. : 0.;
    acc.h[0] += live ? ee * (b00 / 2. - g0 * g0 / 4.) : 0.;
    acc.h[1] += live ? ee * (b01 / 2. - g0 * g1 / 4.) : 0.;
    acc.h[2] += live ? ee * (h02 / 2. - g0 * g2 / 4.) : 0.;
    acc.h[3] += live ? ee * (b11 / 2. - g1 * g1 / 4.) : 0.;
    acc.h[4] += live ? ee * (h12 / 2. - g1 * g2 / 4.) : 0.;
    acc.h[5] += live ? ee * (h22 / 2. - g2 * g2 / 4.) : 0.;
  }
}

}  // namespace

// One wave per pose, eight waves per workgroup (two a SIMD, 256 VGPRs each): the thirteen fp64 accumulators beside a four-chunk
// trip take about 198, which sixteen waves' budget of 128 would spill; k_lattice_cost_jobs runs eight for the same reason.  The scan is staged as it
// is and padded (pad_points_wg), the table as the plan says (stage_image); the job's descriptor is wave-uniform.
template <int PATH>
__global__ void __launch_bounds__(kCurvatureThreads)
k_curvature_jobs(const CurvatureJob* __restrict__ jobs, const uint32_t* __restrict__ share_job, uint32_t n_shares) {
  const uint32_t n_waves = blockDim.x >> 6;
  bool staged = false;
  for (uint32_t sh = blockIdx.x; sh < n_shares; sh += gridDim.x) {
    const CurvatureJob* __restrict__ job = jobs + share_job[sh];
    const uint32_t n_poses = job->n_poses;
    const uint32_t first = (sh - job->share0) * n_waves, step = job->share * n_waves;
    if (first >= n_poses) continue;  // (uniform)
    const unsigned char* __restrict__ image = job->image;
    const double2* __restrict__ xy = job->xy;
    const double* __restrict__ poses = job->poses;
    CurvatureOut* __restrict__ out = job->out;
    const GridP g = job->g;
    const WinP wn = job->wn;
    const Layout L = job->L;
    const DenseP dn = job->dn;
    const int n = job->n;
    double2* pts = reinterpret_cast<double2*>(g_lds + L.pts_off);
    if (staged) __syncthreads();  // the previous share's last reads of its table and points
    staged = true;
    stage_image<kScoreF64, PATH>(image, g, wn, L, dn);
    copy16(pts, xy, n * 16);
    pad_points_wg(pts, n);
    __syncthreads();
    const EvalCtx E = PATH >= 4 ? make_eval_ctx_global(g, wn, dn, image) : make_eval_ctx(g, wn, L, dn);
    const int n_pad = round_up(n, kWave);
    for (uint32_t k = first + (uint32_t)wave_id(); k < n_poses; k += step) {
      const double th = poses[3 * (size_t)k + 2];
      double sn, cn;
      sincos(th, &sn, &cn);
      const double tx = poses[3 * (size_t)k], ty = poses[3 * (size_t)k + 1];
      CurvatureAcc acc;
#pragma unroll
      for (int i = 0; i < 4; ++i) acc.e[i] = 0.;
#pragma unroll
      for (int i = 0; i < 3; ++i) acc.g[i] = 0.;
#pragma unroll
      for (int i = 0; i < 6; ++i) acc.h[i] = 0.;
      acc.hit = 0u;
      int base = 0;
      for (; base + 4 * kWave <= n_pad; base += 4 * kWave)  // (eval_pose_wave_t's trips: NDTPSO_UNROLL = 4 chunks, then single ones)
        curvature_trip<(PATH & 3) == 1, 4>(E.g, E.wn, E.T, pts, base, cn, sn, tx, ty, acc);
      for (; base < n_pad; base += kWave)
        curvature_trip<(PATH & 3) == 1, 1>(E.g, E.wn, E.T, pts, base, cn, sn, tx, ty, acc);
      CurvatureOut r;
      r.cost = -wave_sum((acc.e[0] + acc.e[1]) + (acc.e[2] + acc.e[3]));
#pragma unroll
      for (int i = 0; i < 3; ++i) r.gradient[i] = wave_sum(acc.g[i]);
#pragma unroll
      for (int i = 0; i < 6; ++i) r.hessian[i] = wave_sum(acc.h[i]);
      uint32_t hit = acc.hit;
#pragma unroll
      for (int off = 32; off; off >>= 1) hit += (uint32_t)__shfl_xor((int)hit, off);
      r.n_points = (uint32_t)n;
      r.n_hit = hit;
      r.path = (uint32_t)PATH;
      r.reserved = 0u;
      if (lane_id() == 0) out[k] = r;
    }
  }
}

static_assert(NDTPSO_UNROLL == 4, "the curvature trips restate eval_pose_wave_t's groups of four chunks");

hipError_t curvature_jobs_launch(int path, unsigned grid, int lds_bytes, hipStream_t stream, const void* jobs, const uint32_t* share_job,
                                 uint32_t n_shares) {
  const CurvatureJob* d_jobs = static_cast<const CurvatureJob*>(jobs);
  hipError_t e = hipSuccess;
#define NDTPSO_CURVATURE_KERNEL(PATH)                                                                                                  \
  do {                                                                                                                                 \
    /* (per launch, as the search: the attribute is the current device's) */                                                           \
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_curvature_jobs<PATH>), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds); \
    if (e == hipSuccess)                                                                                                               \
      hipLaunchKernelGGL((k_curvature_jobs<PATH>), dim3(grid), dim3(kCurvatureThreads), lds_bytes, stream, d_jobs, share_job, n_shares); \
  } while (0)
  switch (path) {
    case 1: NDTPSO_CURVATURE_KERNEL(1); break;
    case 4: NDTPSO_CURVATURE_KERNEL(4); break;
    case 5: NDTPSO_CURVATURE_KERNEL(5); break;
    default: NDTPSO_CURVATURE_KERNEL(0);
  }
#undef NDTPSO_CURVATURE_KERNEL
  return e != hipSuccess ? e : hipGetLastError();
}
