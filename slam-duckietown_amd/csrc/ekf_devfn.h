// Device-side helpers shared by the kernel translation units: LDS hand-off macros, the motion model of
// src/replay_no_ros.py:368-417 and the measurement model of :443-469, a cadence step's landmark range, buffer-instruction
// accessors.  gfx950 only.
#pragma once
#include <type_traits>

#include "ekf_device.h"

// (launchers) a run-time choice as a template argument: f(std::integral_constant<...>{}), the argument's ::value being the flag /
// the slot count (1, 2, 4, 8, 16: ekf_host_plan.h cap_for) -- one launch statement instead of a ladder per instantiation
template <typename F>
inline void with_flag(bool flag, F&& f) {
  if (flag) f(std::true_type{});
  else f(std::false_type{});
}
template <typename F>
inline void with_mcap(int mcap, F&& f) {
  switch (mcap) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    default: f(std::integral_constant<int, 16>{}); break;
  }
}

// LDS hand-off between lanes of ONE wave (the other waves of the workgroup have exited): LDS
// operations of a wave execute in issue order, so only the compiler must be kept from reordering.
#define WAVE_SYNC()                                              \
  do {                                                           \
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");       \
    __builtin_amdgcn_wave_barrier();                             \
  } while (0)

// LDS hand-off between two waves of a workgroup: the writer's LDS stores have landed (lgkmcnt(0)) before it
// flips the slot word, the reader issues its LDS loads after it saw the word; the "memory" clobber keeps the
// compiler from moving LDS accesses across.  Unlike a workgroup fence this leaves the wave's global loads
// and stores in flight (a fence drains vmcnt too).
#define LDS_SYNC() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

// Workgroup barrier for data handed over through LDS only: the wave's LDS operations have completed, its global
// loads and stores stay in flight (`__syncthreads()` and workgroup fences drain vmcnt as well: a store
// acknowledgement is ~500 cycles away).  WAVE_LDS_SYNC: the same between lanes of one wave, where LDS operations
// execute in issue order and only the compiler must be kept from reordering them.
#define WG_LDS_BARRIER()                                         \
  do {                                                           \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");           \
    __builtin_amdgcn_s_barrier();                                \
    asm volatile("" ::: "memory");                               \
  } while (0)
#define WAVE_LDS_SYNC()                                          \
  do {                                                           \
    asm volatile("" ::: "memory");                               \
    __builtin_amdgcn_wave_barrier();                             \
    asm volatile("" ::: "memory");                               \
  } while (0)

namespace ekf {

typedef double double4_t __attribute__((ext_vector_type(4)));

// W is stored in MFMA A-operand tiles: k-tile (4 ranks) major, then 16-row groups, then [k&3][row&15],
// so that one 8-byte-per-lane load of 64 consecutive doubles is exactly one 16x4 A fragment.
__host__ __device__ __forceinline__ long wm_index(int ld16, int k, int i) {
  return ((long)(k >> 2) * ld16 + (i >> 4)) * 64 + (k & 3) * 16 + (i & 15);
}

__device__ __forceinline__ double wrap_pi(double a) {
  // (a + pi) % (2 pi) - pi with NumPy remainder semantics, result in [-pi, pi)
  // (src/replay_no_ros.py:397, :458).  fma(-k, 2pi, x) is the exact remainder when k is the right
  // quotient (the remainder is representable); the two fix-ups cover a quotient that is off by one.
  const double two_pi = 2.0 * M_PI;
  const double x = a + M_PI;
  const double k = floor(x * (1.0 / two_pi));
  double r = fma(-k, two_pi, x);
  if (r < 0.0) r += two_pi;
  else if (r >= two_pi) r -= two_pi;
  return r - M_PI;
}

// The motion model of src/replay_no_ros.py:368-417 at the pose (x, y, th): the new pose and G[0,2], G[1,2] of its Jacobian.
// The ONE statement of it on the device: every kernel that predicts -- solve_body (ekf_kernels.hip), the cadence chain
// (ekf_solve_cad_body.inc), small_step (ekf_small.hip), loc_solve_body (ekf_loc_chain.h) -- calls it; each keeps its own test
// of the step's FLAG_PREDICT, its own way of fetching the pose and of publishing the result.  (disable_motion_model leaves the
// pose and a zero Jacobian; the callers that test it in front of the call keep the branch their kernels had.)
struct Motion {
  double x, y, th, g0, g1;
};
__device__ __forceinline__ Motion motion_model(double x, double y, double th, double lin, double ang, const DeviceConfig& cfg) {
  Motion r{x, y, th, 0.0, 0.0};
  if (cfg.disable_motion_model) return r;
  double s0, c0;
  sincos(th, &s0, &c0);
  if (cfg.enable_circular_interpolation && fabs(ang) > cfg.arc_threshold) {   // :390 arc
    double s1, c1;
    sincos(th + ang, &s1, &c1);
    const double rr = lin / ang;
    r.x += -rr * s0 + rr * s1;
    r.y += rr * c0 - rr * c1;
    r.th = wrap_pi(th + ang);                            // :397
    r.g0 = -rr * c0 + rr * c1;                           // :401
    r.g1 = -rr * s0 + rr * s1;                           // :402
  } else {                                               // :376 straight / :405-417 linear mode
    r.x += lin * c0;
    r.y += lin * s0;
    if (!cfg.enable_circular_interpolation) r.th = th + ang;   // no wrap (:409); :381 keeps theta
    r.g0 = -lin * s0;
    r.g1 = lin * c0;
  }
  return r;
}

// 1 / x from the hardware estimate (v_rcp_f64: ~1e-8 relative... in fact 2^-26) and two Newton steps -- each squares the error:
// <= 1 ulp for finite NORMAL x whose reciprocal is normal too; inf / NaN / 0 behave like the IEEE division (1/0 = inf,
// 1/inf = 0, NaN through).  Where the estimate itself is not finite or zero -- x subnormal (v_rcp_f64 gives inf there), 0 or
// inf -- or x is so large that 1/x is subnormal, the Newton terms would turn the estimate into NaN / lose its bits: those take
// the IEEE division (a branch that is never taken on the solve's chain: S = H P H^T + Q with Q = meas_sigma^2 > 0).  The IEEE
// division behind `1.0 / x` is a v_div_scale / v_div_fmas / v_div_fixup sequence of ~250 dependent cycles on the solve's chain.
__device__ __forceinline__ double fast_recip(double x) {
  double r = __builtin_amdgcn_rcp(x);
  const double e0 = fma(-x, r, 1.0);
  const double r1 = fma(r, e0, r);
  const double e1 = fma(-x, r1, 1.0);
  const double r2 = fma(r1, e1, r1);
  const double ax = fabs(x);
  // (2.2250738585072014e-308 = DBL_MIN; 1 / x is normal for |x| <= 2^1022)
  if (!(ax >= 2.2250738585072014e-308 && ax <= 4.49423283715578976932e307)) return 1.0 / x;
  return r2;
}

// Innovation and 2x5 Jacobian of one range/bearing observation (src/replay_no_ros.py:443-469), in two parts: the
// Jacobian (needed first, by the covariance chain) and the innovation (atan2: twice as long, needed only by the mean).
// h[r][k] = row r, column k on {x, y, theta, lx, ly}.  q == 0 gives NaN rows like NumPy's 0/0.
struct LinGeom {
  double dx, dy, th, sq;
};
__device__ __forceinline__ LinGeom linearize_h(double mx, double my, double mth, double lx, double ly, double (&h)[2][5]) {
  LinGeom g;
  g.dx = lx - mx;                                                 // :443
  g.dy = ly - my;
  g.th = mth;
  const double dx = g.dx, dy = g.dy;
  const double q = dx * dx + dy * dy;                             // :446
  // 1/sqrt(q) once (hardware estimate + two Newton steps, <= 1 ulp); sqrt(q) = q * rs, 1/q = rs * rs.
  // q == 0 -> rs = inf -> NaN rows below, like NumPy's 0/0 at :466-469.
  double rs = __builtin_amdgcn_rsq(q);
  rs = rs * fma(-0.5 * q * rs, rs, 1.5);
  rs = rs * fma(-0.5 * q * rs, rs, 1.5);
  g.sq = q * rs;
  const double rq = rs * rs;
  const double nanv = __builtin_nan("");
  h[0][0] = -rs * dx;                                             // (-sqrt(q) dx) / q
  h[0][1] = -rs * dy;
  h[0][2] = (q > 0.0) ? 0.0 : nanv;                               // .0 / q
  h[0][3] = rs * dx;
  h[0][4] = rs * dy;
  h[1][0] = dy * rq;
  h[1][1] = -dx * rq;
  h[1][2] = (q > 0.0 && q < __builtin_inf()) ? -1.0 : nanv;       // -q / q
  h[1][3] = -dy * rq;
  h[1][4] = dx * rq;
  return g;
}
typedef unsigned int uint2v_t __attribute__((ext_vector_type(2)));
typedef unsigned int uint4v_t __attribute__((ext_vector_type(4)));
// buffer access with a 32-bit byte offset per lane (one instruction, no 64-bit address arithmetic)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rs_rsrc(const void* base) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, -1, 0x00020000);
}
__device__ __forceinline__ double ldb8(__amdgpu_buffer_rsrc_t rs, unsigned lane_bytes, unsigned row_bytes) {
  return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, (int)lane_bytes, (int)row_bytes, 0));
}

// lane `src` (wave-uniform) of a double, through the scalar registers
__device__ __forceinline__ double read_lane(double v, int src) {
  const uint2v_t u = __builtin_bit_cast(uint2v_t, v);
  const unsigned lo = __builtin_amdgcn_readlane(u.x, src), hi = __builtin_amdgcn_readlane(u.y, src);
  return __builtin_bit_cast(double, uint2v_t{lo, hi});
}
__device__ __forceinline__ void innovation(const LinGeom& g, double z_range, double z_bearing, double& y0, double& y1) {
  y0 = z_range - g.sq;                                            // :455
  y1 = wrap_pi(z_bearing - (atan2(g.dy, g.dx) - g.th));           // :453-458
}

// Touched step p of a cadence (CadPlan): its landmark count m (none while the measurement model is off) and the part of them
// this cadence applies, [lo, lo + cnt) -- the first step starts at the plan's j0, the last one ends at its jend.  The ONE
// statement of it: cad_positions (ekf_cadence.hip), the column gather of ekf_solve_cad_body.inc and k_innov_cad
// (ekf_innovations.hip) each run their own prefix sum over cnt.
struct CadRange {
  int m, lo, cnt;
};
__device__ __forceinline__ CadRange cad_step_range(const CadPlan& pl, const StepIn* st, int p, int meas) {
  const int m = ((st->flags & FLAG_UPDATE) && meas) ? min(st->m, MMAX) : 0;
  const int lo = p == 0 ? pl.j0 : 0;
  const int hi = p == pl.ns - 1 ? min(pl.jend, m) : m;
  return CadRange{m, lo, max(hi - lo, 0)};
}

constexpr int RS_QSTRIDE = 32;          // k_flush_rs: words between the per-XCD queue heads (one cache line each)

}  // namespace ekf
