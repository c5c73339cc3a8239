// ndtpso_selftest.inc -- probes of the device arithmetic the parity claims rest on (included by ndtpso_hip.hip).
//
//   ndtpso_selftest_exp   exp_neg_half (the fp64 score's spelt-out exponential, ndtpso_kernels.hpp) against the math
//                         library's exp on the device, bit for bit, over whole binades of arguments
//   ndtpso_device_math    the device's exp / exp_neg_half / sincos on the caller's arguments (compared with glibc's by
//                         tests/test_gpu_exp.py: the particle headings' sincos and the fp64 exp come from the device's library)
//   exact_mode_resolve    the start-up known-answer check of NDTPSO_SCORE_EXACT (below)

namespace {

__device__ __forceinline__ uint64_t selftest_mix(uint64_t z) {  // splitmix64's finaliser
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// out[0] checked, out[1] mismatched, out[2] / out[3]: the bits of the first mismatching argument seen (atomicMin of the
// index decides), out[4] its index + 1
__global__ void __launch_bounds__(256)
k_selftest_exp(int exp2_lo, int n_binades, uint32_t per_binade, uint32_t seed, int positive, unsigned long long* out) {
  const uint64_t total = (uint64_t)n_binades * per_binade;
  uint64_t bad = 0, first = ~0ull;
  double first_x = 0.;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
    const int b = exp2_lo + (int)(i / per_binade);
    const uint64_t h = selftest_mix(((uint64_t)seed << 32) ^ i);
    // (1 + u) 2^b with 52 random mantissa bits; b below -1022 gives subnormals by the shift
    uint64_t bits;
    if (b >= -1022)
      bits = ((uint64_t)(b + 1023) << 52) | (h >> 12);
    else
      bits = ((1ull << 52) | (h >> 12)) >> (uint64_t)min(-1022 - b, 63);
    const double x = __longlong_as_double((long long)(bits | (positive ? 0ull : 0x8000000000000000ull)));
    const double want = exp(x), got = exp_neg_half(-2. * x);
    const bool same = __double_as_longlong(want) == __double_as_longlong(got) || (want != want && got != got);
    if (!same) {
      ++bad;
      if (i < first) {
        first = i;
        first_x = x;
      }
    }
  }
  if (bad) {
    atomicAdd(&out[1], (unsigned long long)bad);
    const unsigned long long prev = atomicMin(&out[4], (unsigned long long)first + 1ull);
    if (first + 1ull < prev) out[2] = (unsigned long long)__double_as_longlong(first_x);  // (last writer among the minima: good enough)
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) out[0] = total;
}

__global__ void __launch_bounds__(256)
k_device_math(int kind, const double* __restrict__ x, uint32_t n, double* __restrict__ o0, double* __restrict__ o1) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double v = x[i];
  if (kind == 0) {
    o0[i] = exp(v);
  } else if (kind == 1) {
    o0[i] = exp_neg_half(-2. * v);
  } else {
    double sn, cn;
    sincos(v, &sn, &cn);
    o0[i] = sn;
    o1[i] = cn;
  }
}

}  // namespace

extern "C" {

int ndtpso_selftest_exp(ndtpso_ctx* c, int exp2_lo, int exp2_hi, uint32_t per_binade, uint32_t seed, int positive,
                        uint64_t* checked, uint64_t* mismatched, double* first_bad) {
  if (!c) return NDTPSO_E_ARG;
  if (exp2_hi < exp2_lo || exp2_lo < -1074 || exp2_hi > 1023 || per_binade == 0) return fail(c, NDTPSO_E_ARG, "bad binade range");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, c->small.reserve(64));
  unsigned long long h[5] = {0, 0, 0, 0, ~0ull};
  HIP_TRY(c, hipMemcpyAsync(c->small.p, h, sizeof(h), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_selftest_exp, dim3(4096), dim3(256), 0, c->stream, exp2_lo, exp2_hi - exp2_lo + 1, per_binade, seed,
                     positive, (unsigned long long*)c->small.p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(h, c->small.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (checked) *checked = h[0];
  if (mismatched) *mismatched = h[1];
  if (first_bad) {
    const long long b = (long long)h[2];
    std::memcpy(first_bad, &b, 8);
    if (!h[1]) *first_bad = std::nan("");
  }
  return NDTPSO_OK;
}

int ndtpso_device_math(ndtpso_ctx* c, int kind, const double* x, uint32_t n, double* out0, double* out1) {
  if (!c) return NDTPSO_E_ARG;
  if (!x || !out0 || kind < 0 || kind > 2 || (kind == 2 && !out1)) return fail(c, NDTPSO_E_ARG, "bad argument");
  if (n == 0) return NDTPSO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, c->xy.reserve((size_t)n * 8));
  HIP_TRY(c, c->xy2.reserve((size_t)n * 16));
  double* d0 = (double*)c->xy2.p;
  double* d1 = d0 + n;
  HIP_TRY(c, hipMemcpyAsync(c->xy.p, x, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_device_math, dim3((n + 255) / 256), dim3(256), 0, c->stream, kind, (const double*)c->xy.p, n, d0, d1);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(out0, d0, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
  if (kind == 2) HIP_TRY(c, hipMemcpyAsync(out1, d1, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return NDTPSO_OK;
}

}  // extern "C"

// ---- start-up known-answer check of the exact mode ---------------------------------------------------------------------
//
// NDTPSO_SCORE_EXACT promises the fp64 mode's pose and cost bit for bit.  That rests on the arbitration's fp64 scores being
// the fp64 kernels' -- computed in the fp32-score kernels through two out-of-line functions (exact_unit_call,
// exact_task_call) whose callers a code-generation defect has broken before (interprocedural register allocation: wrong
// poses in 7 of 130 pairs, silently -- PER CALLER, i.e. per kernel instantiation; the library is built with
// -mllvm -enable-ipra=0 since, ndtpso_slam_amd/build.py).  So nothing is taken on trust: the first time a process asks a
// device for the exact mode, a temporary context sends a fixed small problem through EVERY arbitrating instantiation the
// dispatchers can reach (kExactFamilies below: k_align_pairs<F32, PATH 2 / 3, ...> x one workgroup per alignment without and
// with clipping trips / clusters of workgroups x swarm in LDS / in HBM x plain / box-guard copies, and k_align<F32, 2, one
// workgroup / cluster> -- the lone alignment of ndtpso_align and of the resident map), each forced by a plan override
// (PlanForce) and CONFIRMED by the instantiation the launch recorded, in the exact mode, and compares poses and costs bit for
// bit with the fp64 mode's; the problem is built so that comparisons ARE arbitrated (a swarm started inside 30 um of the
// guess), which the check verifies per family.  On any difference the exact mode is refused for that device: every request
// for it runs the fp64 score instead (slower, same results by definition) and ndtpso_last_error says why.  A failure that is
// not a verdict (no memory for the temporary context, a HIP error) refuses nothing for good: that request runs the fp64 score
// and the check is run again by the next one (three attempts).  NDTPSO_EXACT_CHECK=0 skips the check; ndtpso_exact_check and
// ndtpso_exact_check_report report it.
namespace {

struct ExactFamily {
  const char* name;
  int grid;          // 0: 0.5 m cells (no cell overhangs the frame), 1: 0.3 m cells in a 40 m frame (clipping trips)
  int single;        // 0: fused pairs kernel; 1: k_align on one workgroup; 2: k_align on a cluster
  PlanForce force;   // {swarm_hbm, byte_entries, table_side, boxy, cluster, pair}
  uint32_t code;     // launch_code() of the instantiation the family must reach
};
// table sides: the room's occupied box (26 x 18 cells at 0.5 m, 44 x 30 at 0.3 m) fits, the box of scan B's disc does not
const ExactFamily kExactFamilies[] = {
    {"pairs: byte entries, swarm in LDS", 0, 0, {-1, -1, 0, 0, 0, 0}, launch_code(false, 3, false, true, true, 0, false, true)},
    {"pairs: two items per wave (short scans), byte entries, swarm in LDS", 0, 0, {-1, -1, 0, 0, 0, 1}, launch_code(false, 3, false, true, true, 0, false, true, true)},
    {"pairs: 16-byte-unit entries, swarm in LDS", 0, 0, {-1, 0, 0, 0, 0, 0}, launch_code(false, 2, false, true, true, 0, false, true)},
    {"pairs: byte entries, swarm in HBM", 0, 0, {1, -1, 0, 0, 0, 0}, launch_code(false, 3, false, true, true, 1, false, true)},
    {"pairs: 16-byte-unit entries, swarm in HBM", 0, 0, {1, 0, 0, 0, 0, 0}, launch_code(false, 2, false, true, true, 1, false, true)},
    {"pairs: byte entries, box guard", 0, 0, {-1, -1, 40, 1, 0, 0}, launch_code(false, 3, false, true, true, 0, true, true)},
    {"pairs: 16-byte-unit entries, box guard", 0, 0, {-1, 0, 40, 1, 0, 0}, launch_code(false, 2, false, true, true, 0, true, true)},
    {"pairs: clipping trips, byte entries", 1, 0, {-1, -1, 0, 0, 0, 0}, launch_code(false, 3, false, true, false, 2, false, true)},
    {"pairs: clipping trips, 16-byte-unit entries", 1, 0, {-1, 0, 0, 0, 0, 0}, launch_code(false, 2, false, true, false, 2, false, true)},
    {"pairs: clipping trips, swarm in HBM", 1, 0, {1, -1, 0, 0, 0, 0}, launch_code(false, 3, false, true, false, 2, false, true)},
    {"pairs: clipping trips, byte entries, box guard", 1, 0, {-1, -1, 56, 1, 0, 0}, launch_code(false, 3, false, true, false, 2, true, true)},
    {"pairs: clipping trips, 16-byte-unit entries, box guard", 1, 0, {-1, 0, 56, 1, 0, 0}, launch_code(false, 2, false, true, false, 2, true, true)},
    {"pairs: clusters of workgroups, byte entries", 0, 0, {-1, -1, 0, 0, 1, 0}, launch_code(false, 3, true, true, false, 2, false, true)},
    {"pairs: clusters of workgroups, 16-byte-unit entries", 0, 0, {-1, 0, 0, 0, 1, 0}, launch_code(false, 2, true, true, false, 2, false, true)},
    {"single alignment on one workgroup (ndtpso_align, resident map)", 0, 1, {-1, -1, 0, -1, -1, -1}, launch_code(false, 2, false, true, false, 0, false, false)},
    {"single alignment on a cluster of workgroups (ndtpso_align, resident map)", 0, 2, {-1, -1, 0, -1, -1, -1}, launch_code(false, 2, true, true, false, 0, false, false)},
};
constexpr int kExactFamilyCount = (int)(sizeof(kExactFamilies) / sizeof(kExactFamilies[0]));

struct ExactFamilyResult {
  int state = 0;  // 0 not run, 1 passed, 2 refused (bits differ / nothing arbitrated), 3 not reachable on this device
  uint32_t launched = 0, arbitrated = 0, mismatched = 0, units = 0;
};

struct ExactCheck {
  std::mutex mu;
  std::atomic<int> state{0};  // 0 not run, 1 passed, 2 refused
  int attempts = 0;           // runs that ended without a verdict (infrastructure failures)
  std::string why;
  uint32_t arbitrated_batch = 0, arbitrated_single = 0;
  double ms = 0.;
  ExactFamilyResult fam[kExactFamilyCount];
};
ExactCheck g_exact_check[64];
// (t_in_exact_check: ndtpso_hip.hip, next to the plan overrides)

// a 181-beam scan of a 13 m x 9 m room with a pillar, seen from (px, py, pth); a deterministic +-4 mm jitter per beam
void kat_scan(double px, double py, double pth, uint32_t salt, int n_beams, float amin, float ainc, float* out) {
  const double box[2][4] = {{-6., 7., -4., 5.}, {2., 3., 1., 2.}};  // xmin, xmax, ymin, ymax: the room (from inside), a pillar (from outside)
  uint32_t lcg = 12345u + 2654435761u * salt;
  for (int i = 0; i < n_beams; ++i) {
    const double a = pth + (double)((float)i * ainc + amin);
    const double dx = std::cos(a), dy = std::sin(a);
    double best = 1e9;
    for (int b = 0; b < 2; ++b) {
      const double* q = box[b];
      const double cand[4] = {dx != 0. ? (q[0] - px) / dx : -1., dx != 0. ? (q[1] - px) / dx : -1.,
                              dy != 0. ? (q[2] - py) / dy : -1., dy != 0. ? (q[3] - py) / dy : -1.};
      for (int k = 0; k < 4; ++k) {
        const double t = cand[k];
        if (!(t > 0.) || t >= best) continue;
        const double hx = px + t * dx, hy = py + t * dy;
        const bool on = k < 2 ? (hy >= q[2] - 1e-9 && hy <= q[3] + 1e-9) : (hx >= q[0] - 1e-9 && hx <= q[1] + 1e-9);
        if (on) best = t;
      }
    }
    lcg = lcg * 1664525u + 1013904223u;
    out[i] = (float)(best + 0.004 * ((double)(lcg >> 8) / 8388608. - 1.));
  }
}

bool same_bits(const double* a, const double* b, size_t n) { return std::memcmp(a, b, n * sizeof(double)) == 0; }

struct ForceScope {  // a family's plan override, for the calling thread, for as long as the scope lives
  explicit ForceScope(const PlanForce& f) { t_plan_force = f; }
  ~ForceScope() { t_plan_force = PlanForce{}; }
};

// -> true: a verdict was reached (ec.state 1 or 2); false: the check could not run (nothing refused for good)
bool run_exact_check(int device, ExactCheck& ec) {
  const auto t0 = std::chrono::steady_clock::now();
  auto refuse = [&](const std::string& why) {
    ec.why = "NDTPSO_SCORE_EXACT refused on device " + std::to_string(device) + " (requests run the fp64 score instead): " + why;
    ec.state.store(2);
    return true;
  };
  auto no_verdict = [&](const std::string& why) {
    ec.why = "the start-up check of NDTPSO_SCORE_EXACT could not run on device " + std::to_string(device) + " (this request runs the fp64 score, the next one tries again): " + why;
    return false;
  };
  for (ExactFamilyResult& r : ec.fam) r = ExactFamilyResult{};
  ec.arbitrated_batch = ec.arbitrated_single = 0;
  ndtpso_ctx* t = nullptr;
  if (ndtpso_ctx_create(device, &t) != NDTPSO_OK) return no_verdict("no context for the start-up check");
  struct Guard {
    ndtpso_ctx* t;
    ~Guard() { ndtpso_ctx_destroy(t); }
  } guard{t};
  constexpr int kBeams = 181, kBase = 8;
  const ndtpso_scan_geom geom{(uint32_t)kBeams, -2.356194f, 4.712389f / 180.f, 20.f, 0.1f};
  const ndtpso_grid grids[2] = {{40, 40, 0.5}, {40, 40, 0.3}};
  ndtpso_pso_config cfg{20, 24, -1, 0.8, 2., 2., 1.};
  // a swarm that starts within 30 um / 1 urad of the guess: its costs lie within the arbitration margin of each other again
  // and again without ever being equal -- a handful of arbitrated comparisons per alignment, none handed to the fp64 kernel
  const double dev3[3] = {3e-5, 3e-5, 1e-6};
  std::vector<float> base_a((size_t)kBase * kBeams), base_b((size_t)kBase * kBeams);
  for (int i = 0; i < kBase; ++i) {
    const double ax = 0.3 * std::cos(0.9 * i), ay = 0.2 * std::sin(1.3 * i), ath = 0.11 * i;
    kat_scan(ax, ay, ath, 2u * i, kBeams, geom.min_angle, geom.angle_increment, &base_a[(size_t)i * kBeams]);
    kat_scan(ax + 0.04 * std::cos(2.1 * i), ay + 0.03 * std::sin(1.7 * i), ath + 0.008 * std::cos(3. * i), 2u * i + 1u, kBeams,
             geom.min_angle, geom.angle_increment, &base_b[(size_t)i * kBeams]);
  }
  // a batch small enough to run as clusters where a family asks for them (two pairs' clusters per compute-unit budget), and as
  // one workgroup per alignment where it does not: the instantiation, not the launch's shape, is what is under test
  const uint32_t B = (uint32_t)std::max(8, std::min(40, t->n_cus / 6));
  std::vector<float> ra((size_t)B * kBeams), rb((size_t)B * kBeams);
  std::vector<double> guess((size_t)B * 3, 0.), dev((size_t)B * 3);
  std::vector<uint32_t> seeds(B);
  for (uint32_t b = 0; b < B; ++b) {
    std::memcpy(&ra[(size_t)b * kBeams], &base_a[(size_t)(b % kBase) * kBeams], kBeams * sizeof(float));
    std::memcpy(&rb[(size_t)b * kBeams], &base_b[(size_t)(b % kBase) * kBeams], kBeams * sizeof(float));
    for (int k = 0; k < 3; ++k) dev[(size_t)b * 3 + k] = dev3[k];
    seeds[b] = 1000u + b;
  }
  // the fp64 mode's results, once per grid (default plan)
  std::vector<double> p64[2], c64[2];
  std::vector<ndtpso_align_stats> st(B);
  for (int gi = 0; gi < 2; ++gi) {
    p64[gi].resize((size_t)B * 3);
    c64[gi].resize(B);
    if (ndtpso_align_pairs(t, B, ra.data(), rb.data(), &geom, &grids[gi], guess.data(), dev.data(), &cfg, seeds.data(), nullptr,
                           NDTPSO_SCORE_F64, p64[gi].data(), c64[gi].data(), st.data()) != NDTPSO_OK)
      return no_verdict(std::string("the check's fp64 batch failed: ") + ndtpso_last_error(t));
  }
  // the lone alignment's table and points (grid 0)
  std::vector<double> xy((size_t)kBeams * 2);
  uint32_t n_pts = 0;
  const double zero3[3] = {0., 0., 0.};
  int rc = ndtpso_ref_from_scan(t, &grids[0], base_a.data(), &geom, zero3);
  if (rc == NDTPSO_OK) rc = ndtpso_scan_to_points(t, base_b.data(), &geom, zero3, xy.data(), &n_pts);
  if (rc != NDTPSO_OK) return no_verdict(std::string("the check's reference table failed: ") + ndtpso_last_error(t));
  std::vector<double> px((size_t)B * 3), cx(B);
  std::string first_bad;
  for (int f = 0; f < kExactFamilyCount; ++f) {
    const ExactFamily& fam = kExactFamilies[f];
    ExactFamilyResult& r = ec.fam[f];
    if (fam.single == 0) {
      r.units = B;
      {
        ForceScope scope(fam.force);
        t_last_launch = 0;
        rc = ndtpso_align_pairs(t, B, ra.data(), rb.data(), &geom, &grids[fam.grid], guess.data(), dev.data(), &cfg, seeds.data(), nullptr,
                                NDTPSO_SCORE_EXACT, px.data(), cx.data(), st.data());
        r.launched = t_last_launch;
      }
      if (rc != NDTPSO_OK) return no_verdict(std::string("the check's batch (") + fam.name + ") failed: " + ndtpso_last_error(t));
      if (r.launched != fam.code) {  // the dispatcher did not take this family's road on this device (too few compute units for
        r.state = 3;                 // clusters, ...): what it cannot reach here it cannot run here either
        continue;
      }
      for (uint32_t b = 0; b < B; ++b) {
        r.arbitrated += NDTPSO_STATUS_ARBITRATED(st[b].status);
        r.mismatched += !same_bits(&px[(size_t)b * 3], &p64[fam.grid][(size_t)b * 3], 3) || !same_bits(&cx[b], &c64[fam.grid][b], 1);
      }
      ec.arbitrated_batch += r.arbitrated;
    } else {
      r.units = 2;
      for (uint32_t seed = 1; seed <= 2; ++seed) {
        double pe[3], ce = 0., pf[3], cf = 0.;
        ndtpso_align_stats se, sf;
        t_last_launch = 0;
        rc = align_points(t, xy.data(), n_pts, zero3, dev3, &cfg, seed, nullptr, NDTPSO_SCORE_EXACT, pe, &ce, &se, fam.single == 2);
        r.launched = t_last_launch;
        if (rc == NDTPSO_OK) rc = align_points(t, xy.data(), n_pts, zero3, dev3, &cfg, seed, nullptr, NDTPSO_SCORE_F64, pf, &cf, &sf, fam.single == 2);
        if (rc != NDTPSO_OK) return no_verdict(std::string("the check's single alignment failed: ") + ndtpso_last_error(t));
        if (r.launched != fam.code) break;
        r.arbitrated += NDTPSO_STATUS_ARBITRATED(se.status);
        r.mismatched += !same_bits(pe, pf, 3) || !same_bits(&ce, &cf, 1);
      }
      if (r.launched != fam.code) {
        r.state = 3;
        continue;
      }
      ec.arbitrated_single += r.arbitrated;
    }
    r.state = (r.mismatched == 0 && r.arbitrated > 0) ? 1 : 2;
    if (r.state == 2 && first_bad.empty()) {
      first_bad = r.mismatched ? std::string("poses or costs of ") + std::to_string(r.mismatched) + " of " + std::to_string(r.units) +
                                     " alignments of the family \"" + fam.name + "\" differ from the fp64 mode's in the start-up check "
                                     "(miscompiled arbitration? see ndtpso_slam_amd/build.py)"
                               : std::string("the start-up check's family \"") + fam.name + "\" arbitrated no comparison: it no longer exercises what it is there for";
    }
  }
  ec.ms = 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (!first_bad.empty()) {
    int n_bad = 0;
    for (const ExactFamilyResult& r : ec.fam) n_bad += r.state == 2;
    return refuse(first_bad + (n_bad > 1 ? " (and " + std::to_string(n_bad - 1) + " more families: ndtpso_exact_check_report)" : std::string()));
  }
  ec.why.clear();
  ec.state.store(1);
  return true;
}

// NDTPSO_SCORE_EXACT -> itself where the device has passed the check, NDTPSO_SCORE_F64 where it has not
int exact_mode_resolve(ndtpso_ctx* c, int* mode) {
  if (!c || *mode != NDTPSO_SCORE_EXACT || t_in_exact_check) return NDTPSO_OK;
  static const bool skip = [] {
    const char* e = std::getenv("NDTPSO_EXACT_CHECK");
    return e && e[0] == '0';
  }();
  if (skip) return NDTPSO_OK;
  ExactCheck& ec = g_exact_check[c->device & 63];
  if (ec.state.load(std::memory_order_acquire) == 1) return NDTPSO_OK;  // the usual case: no lock
  std::lock_guard<std::mutex> lock(ec.mu);
  bool verdict = true;
  if (ec.state.load() == 0) {
    t_in_exact_check = true;
    const PlanForce keep = t_plan_force;
    verdict = run_exact_check(c->device, ec);
    t_plan_force = keep;
    t_in_exact_check = false;
    if (!verdict && ++ec.attempts >= 3) {  // not a verdict, three times over: stop trying
      ec.why += " -- third failure: the mode stays refused";
      ec.state.store(2);
    }
    if (ec.state.load() == 2 || !verdict) std::fprintf(stderr, "ndtpso: %s\n", ec.why.c_str());
    (void)hipSetDevice(c->device);
  }
  if (ec.state.load() != 1) {
    c->err = ec.why;
    *mode = NDTPSO_SCORE_F64;
  }
  return NDTPSO_OK;
}


// ---- ... and of the arbitrating job kernels (ndtpso_map_align_batch) ---------------------------------------------------------
// k_align_jobs<F32, 2, one workgroup / cluster, ARB> are two more callers of the arbitration's out-of-line scores, so the rule
// holds for them too: checked before trusted.  A second table beside kExactFamilies (which, with its budget, stays as it is), run
// the first time a process asks ndtpso_map_align_batch for the exact mode on a device: the same fixed problem as a resident map
// and four jobs of one launch, each family forced (PlanForce::cluster) and confirmed by the instantiation the launch recorded
// (kLaunchJobForm), compared bit for bit with the fp64 mode's single alignments.  A family that fails refuses the exact mode to
// the batch entry only: its exact-mode jobs run the fp64 score, and ndtpso_last_error says why.
struct ExactJobFamily {
  const char* name;
  int cluster;    // PlanForce::cluster of the family
  uint32_t code;  // launch_code() | kLaunchJobForm of the instantiation it must reach
};
const ExactJobFamily kExactJobFamilies[] = {
    {"jobs of one launch, one workgroup each (ndtpso_map_align_batch)", 0, launch_code(false, 2, false, true, false, 0, false, false) | kLaunchJobForm},
    {"jobs of one launch, a cluster of workgroups each (ndtpso_map_align_batch)", 1, launch_code(false, 2, true, true, false, 0, false, false) | kLaunchJobForm},
};
constexpr int kExactJobFamilyCount = (int)(sizeof(kExactJobFamilies) / sizeof(kExactJobFamilies[0]));

struct ExactJobsCheck {
  std::mutex mu;
  std::atomic<int> state{0};  // 0 not run, 1 passed, 2 refused
  int attempts = 0;
  bool ran = false;           // fam[] holds a run's results
  std::string why;
  double ms = 0.;
  ExactFamilyResult fam[kExactJobFamilyCount];
};
ExactJobsCheck g_exact_jobs_check[64];

bool run_exact_jobs_check(int device, ExactJobsCheck& ec) {
  const auto t0 = std::chrono::steady_clock::now();
  auto no_verdict = [&](const std::string& why) {
    ec.why = "the check of NDTPSO_SCORE_EXACT's job kernels could not run on device " + std::to_string(device) +
             " (this call's jobs run the fp64 score, the next one tries again): " + why;
    return false;
  };
  for (ExactFamilyResult& r : ec.fam) r = ExactFamilyResult{};
  ndtpso_ctx* t = nullptr;
  if (ndtpso_ctx_create(device, &t) != NDTPSO_OK) return no_verdict("no context for the check");
  struct Guard {
    ndtpso_ctx* t;
    ndtpso_map* map = nullptr;
    ndtpso_points *a = nullptr, *b = nullptr;
    ~Guard() {
      if (map) ndtpso_map_destroy(map);
      if (a) ndtpso_points_destroy(a);
      if (b) ndtpso_points_destroy(b);
      ndtpso_ctx_destroy(t);
    }
  } gd{t};
  constexpr int kBeams = 181, kJobs = 4;
  const ndtpso_scan_geom geom{(uint32_t)kBeams, -2.356194f, 4.712389f / 180.f, 20.f, 0.1f};
  const ndtpso_grid grid{40, 40, 0.5};
  ndtpso_pso_config cfg{20, 24, -1, 0.8, 2., 2., 1.};
  const double dev3[3] = {3e-5, 3e-5, 1e-6}, zero3[3] = {0., 0., 0.};  // (run_exact_check: comparisons ARE arbitrated)
  std::vector<float> ra(kBeams), rb(kBeams);
  kat_scan(0.3, 0., 0., 0u, kBeams, geom.min_angle, geom.angle_increment, ra.data());  // (pair 0 of run_exact_check's batch)
  kat_scan(0.3 + 0.04, 0., 0.008, 1u, kBeams, geom.min_angle, geom.angle_increment, rb.data());
  int rc = ndtpso_points_create(t, kBeams, &gd.a);
  if (rc == NDTPSO_OK) rc = ndtpso_points_create(t, kBeams, &gd.b);
  if (rc == NDTPSO_OK) rc = ndtpso_map_create(t, &grid, 0., 4u << 20, &gd.map);
  if (rc == NDTPSO_OK) rc = ndtpso_points_load_scan(gd.a, ra.data(), &geom, zero3, nullptr, 0);
  if (rc == NDTPSO_OK) rc = ndtpso_points_load_scan(gd.b, rb.data(), &geom, zero3, nullptr, 0);
  if (rc == NDTPSO_OK) rc = ndtpso_map_insert(gd.map, gd.a, zero3);
  if (rc == NDTPSO_OK) rc = ndtpso_map_build(gd.map);
  if (rc != NDTPSO_OK) return no_verdict(std::string("the check's map failed: ") + ndtpso_last_error(t));
  double p64[kJobs][3], c64[kJobs];
  for (int j = 0; j < kJobs; ++j) {
    ndtpso_align_stats st;
    rc = ndtpso_map_align(gd.map, gd.b, zero3, dev3, &cfg, 1u + (uint32_t)j, nullptr, NDTPSO_SCORE_F64, p64[j], &c64[j], &st);
    if (rc != NDTPSO_OK) return no_verdict(std::string("the check's fp64 alignment failed: ") + ndtpso_last_error(t));
  }
  std::string first_bad;
  for (int f = 0; f < kExactJobFamilyCount; ++f) {
    const ExactJobFamily& fam = kExactJobFamilies[f];
    ExactFamilyResult& r = ec.fam[f];
    r.units = kJobs;
    ndtpso_map_align_job jobs[kJobs];
    std::memset(jobs, 0, sizeof(jobs));
    for (int j = 0; j < kJobs; ++j) {
      jobs[j].map = gd.map;
      jobs[j].new_points = gd.b;
      for (int k = 0; k < 3; ++k) jobs[j].deviation[k] = dev3[k];
      jobs[j].seed = 1u + (uint32_t)j;
      jobs[j].flags = 1u;
    }
    {
      PlanForce force;
      force.cluster = fam.cluster;
      ForceScope scope(force);
      t_last_launch = 0;
      rc = ndtpso_map_align_batch(t, jobs, kJobs, &cfg, NDTPSO_SCORE_EXACT);
      r.launched = t_last_launch;
    }
    if (rc != NDTPSO_OK) return no_verdict(std::string("the check's launch (") + fam.name + ") failed: " + ndtpso_last_error(t));
    if (r.launched != fam.code) {  // (too few compute units for a cluster per job, ...: what the entry cannot reach here it cannot run here)
      r.state = 3;
      continue;
    }
    for (int j = 0; j < kJobs; ++j) {
      r.arbitrated += NDTPSO_STATUS_ARBITRATED(jobs[j].stats.status);
      r.mismatched += jobs[j].route < 1 || !same_bits(jobs[j].pose, p64[j], 3) || !same_bits(&jobs[j].cost, &c64[j], 1);
    }
    r.state = (r.mismatched == 0 && r.arbitrated > 0) ? 1 : 2;
    if (r.state == 2 && first_bad.empty())
      first_bad = r.mismatched ? std::string("poses or costs of ") + std::to_string(r.mismatched) + " of " + std::to_string(r.units) +
                                     " jobs of the family \"" + fam.name + "\" differ from the fp64 mode's (miscompiled arbitration? see ndtpso_slam_amd/build.py)"
                               : std::string("the family \"") + fam.name + "\" arbitrated no comparison: it no longer exercises what it is there for";
  }
  ec.ms = 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  ec.ran = true;
  if (!first_bad.empty()) {
    ec.why = "NDTPSO_SCORE_EXACT refused to ndtpso_map_align_batch on device " + std::to_string(device) +
             " (its exact-mode jobs run the fp64 score instead): " + first_bad;
    ec.state.store(2);
    return true;
  }
  ec.why.clear();
  ec.state.store(1);
  return true;
}

// The batch entry was asked for NDTPSO_SCORE_EXACT (`asked`; *mode is what exact_mode_resolve made of it): the exact mode only
// where the job kernels have passed too.  The check runs whatever the start-up check said, so that the report is complete.
int exact_jobs_resolve(ndtpso_ctx* c, int asked, int* mode) {
  if (!c || asked != NDTPSO_SCORE_EXACT || t_in_exact_check) return NDTPSO_OK;
  static const bool skip = [] {
    const char* e = std::getenv("NDTPSO_EXACT_CHECK");
    return e && e[0] == '0';
  }();
  if (skip) return NDTPSO_OK;
  ExactJobsCheck& ec = g_exact_jobs_check[c->device & 63];
  if (ec.state.load(std::memory_order_acquire) == 1) return NDTPSO_OK;
  std::lock_guard<std::mutex> lock(ec.mu);
  if (ec.state.load() == 0) {
    t_in_exact_check = true;
    const PlanForce keep = t_plan_force;
    const uint32_t keep_launch = t_last_launch;
    const bool verdict = run_exact_jobs_check(c->device, ec);
    t_plan_force = keep;
    t_last_launch = keep_launch;
    t_in_exact_check = false;
    if (!verdict && ++ec.attempts >= 3) {
      ec.why += " -- third failure: the mode stays refused";
      ec.state.store(2);
    }
    if (ec.state.load() == 2 || !verdict) std::fprintf(stderr, "ndtpso: %s\n", ec.why.c_str());
    (void)hipSetDevice(c->device);
  }
  if (ec.state.load() != 1) {
    c->err = ec.why;
    *mode = NDTPSO_SCORE_F64;
  }
  return NDTPSO_OK;
}

}  // namespace

extern "C" int ndtpso_exact_check(ndtpso_ctx* c, int* state, uint32_t* arbitrated_batch, uint32_t* arbitrated_single, double* ms) {
  if (!c) return NDTPSO_E_ARG;
  int mode = NDTPSO_SCORE_EXACT;
  if (int rc = exact_mode_resolve(c, &mode)) return rc;
  ExactCheck& ec = g_exact_check[c->device & 63];
  std::lock_guard<std::mutex> lock(ec.mu);
  if (state) *state = ec.state.load();
  if (arbitrated_batch) *arbitrated_batch = ec.arbitrated_batch;
  if (arbitrated_single) *arbitrated_single = ec.arbitrated_single;
  if (ms) *ms = ec.ms;
  return NDTPSO_OK;
}

// One line per kernel family of the start-up check, as JSON: {"state": .., "ms": .., "families": [{"name", "state": "passed" |
// "refused" | "not reachable on this device" | "not run", "instantiation": code, "alignments", "arbitrated", "mismatched"}, ...]}.
// Returns the length the text needs (without the terminating 0); writes at most cap - 1 characters.
extern "C" int ndtpso_exact_check_report(ndtpso_ctx* c, char* buf, uint32_t cap) {
  if (!c) return NDTPSO_E_ARG;
  int mode = NDTPSO_SCORE_EXACT;
  if (int rc = exact_mode_resolve(c, &mode)) return rc;
  ExactCheck& ec = g_exact_check[c->device & 63];
  std::lock_guard<std::mutex> lock(ec.mu);
  static const char* names[4] = {"not run", "passed", "refused", "not reachable on this device"};
  std::string s = "{\"state\": " + std::to_string(ec.state.load()) + ", \"ms\": " + std::to_string(ec.ms) + ", \"families\": [";
  for (int f = 0; f < kExactFamilyCount; ++f) {
    const ExactFamilyResult& r = ec.fam[f];
    s += std::string(f ? ", " : "") + "{\"name\": \"" + kExactFamilies[f].name + "\", \"state\": \"" + names[r.state & 3] +
         "\", \"instantiation\": " + std::to_string(kExactFamilies[f].code) + ", \"launched\": " + std::to_string(r.launched) +
         ", \"alignments\": " + std::to_string(r.units) + ", \"arbitrated\": " + std::to_string(r.arbitrated) +
         ", \"mismatched\": " + std::to_string(r.mismatched) + "}";
  }
  s += "], \"job_families\": [";  // the job kernels' families (exact_jobs_resolve): empty until that check has run
  {
    ExactJobsCheck& jc = g_exact_jobs_check[c->device & 63];
    std::lock_guard<std::mutex> jlock(jc.mu);
    for (int f = 0; jc.ran && f < kExactJobFamilyCount; ++f) {
      const ExactFamilyResult& r = jc.fam[f];
      s += std::string(f ? ", " : "") + "{\"name\": \"" + kExactJobFamilies[f].name + "\", \"state\": \"" + names[r.state & 3] +
           "\", \"instantiation\": " + std::to_string(kExactJobFamilies[f].code) + ", \"launched\": " + std::to_string(r.launched) +
           ", \"alignments\": " + std::to_string(r.units) + ", \"arbitrated\": " + std::to_string(r.arbitrated) +
           ", \"mismatched\": " + std::to_string(r.mismatched) + "}";
    }
  }
  s += "]}";
  if (buf && cap) {
    const size_t n = std::min<size_t>(s.size(), cap - 1);
    std::memcpy(buf, s.data(), n);
    buf[n] = 0;
  }
  return (int)s.size();
}

// Runs the check of the arbitrating job kernels if it has not run (after the start-up check itself): state 1 passed, 2 refused,
// 0 no verdict (the exact mode is refused to the device altogether, the check is switched off, or it could not run).
extern "C" int ndtpso_exact_check_jobs(ndtpso_ctx* c, int* state) {
  if (!c) return NDTPSO_E_ARG;
  int mode = NDTPSO_SCORE_EXACT;
  if (int rc = exact_mode_resolve(c, &mode)) return rc;
  if (int rc = exact_jobs_resolve(c, NDTPSO_SCORE_EXACT, &mode)) return rc;
  ExactJobsCheck& ec = g_exact_jobs_check[c->device & 63];
  std::lock_guard<std::mutex> lock(ec.mu);
  if (state) *state = ec.state.load();
  return NDTPSO_OK;
}
