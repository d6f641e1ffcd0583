// k_copy_traj: copy whole filter states between trajectories on the device (ekf_copy_trajectories) -- the stored upper
// triangle of P_base, the mean, the size word and the sticky flags, from trajectories of one handle to trajectories of the same
// or of another handle on the same GPU, on the layout of ekf_device.h on BOTH sides (row-major up to ld = 4096, column panels
// beyond: the two handles may differ).
//
// A bandwidth kernel.  The launch takes a table of GROUPS (ekf_host_plan.h: plan_copy): one source and up to COPY_FANOUT of its
// destinations.  blockIdx.x is the group; blockIdx.y < tiles enumerates the 64 x 64 tiles (row block rb, 64-column strip s,
// rb <= s) that reach the upper triangle -- tiles wholly below the diagonal do not exist in the grid --, strip by strip.  A
// workgroup of 256 threads loads its tile ONCE, 16 bytes per lane along the rows (32 lanes: one 512-byte row segment; a
// thread holds 8 rows' worth: 32 KB per workgroup in registers), and then stores it to every destination of the group: a
// 1 -> 31 fork reads one triangle and writes 31.  Nothing relies on a cache for that: 31 x 64 MB of stores pass between two
// uses of a source line.  A 64-column strip never straddles a panel, so each side needs p_col(ld, j0) and p_lds(ld) only.
// In a tile on the diagonal a row is copied from its diagonal column on, rounded down to the 16-byte boundary; the one entry
// below the diagonal this may carry is never read (every reader mirrors the upper triangle first).  Columns at and beyond n
// are not touched.  blockIdx.y == tiles copies the mean (n entries, each side's own stride), writes the destination's size
// word and hands the source's sticky flags over (a source never carries EKF_FLAG_INTERNAL: the call refuses it; the
// destination's is thereby cleared, as by an upload).
// NT: nontemporal stores (the destinations are written once and read much later).  Plain C++, vector stores only.
#include "ekf_device.h"
#include "ekf_host_plan.h"
#include "ekf_launch.h"

namespace ekf {

constexpr int CP_THREADS = 256;
constexpr int CP_TILE = 64;             // rows of a tile = columns of a strip
constexpr int CP_Q = CP_TILE * CP_TILE / 2 / CP_THREADS;   // 16-byte pieces per thread (8)
typedef double cp_d2 __attribute__((ext_vector_type(2)));

template <bool NT>
__global__ __launch_bounds__(CP_THREADS) void k_copy_traj(const double* __restrict__ Ps, double* __restrict__ Pd,
                                                          const double* __restrict__ mus, double* __restrict__ mud,
                                                          int* __restrict__ nd, const unsigned* __restrict__ fs,
                                                          unsigned* __restrict__ fd, const int* __restrict__ tab, int groups,
                                                          int tiles, int lds, long pss, int ldd, long psd) {
  const int* g = tab + COPY_GROUP_WORDS * blockIdx.x;
  const int sb = g[0], cnt = g[2], n = g[3];
  const int* dl = tab + COPY_GROUP_WORDS * groups + g[1];
  const int tid = threadIdx.x;
  if ((int)blockIdx.y == tiles) {                      // the mean, the size word, the sticky flags
    const double* ms = mus + (long)sb * lds;
    for (int c = tid; c < n; c += CP_THREADS) {
      const double v = ms[c];
      for (int q = 0; q < cnt; ++q) mud[(long)dl[q] * ldd + c] = v;
    }
    if (tid < cnt) {
      nd[dl[tid]] = n;
      fd[dl[tid]] = fs[sb];
    }
    return;
  }
  // tile t of the strip-by-strip enumeration: strip s holds the row blocks 0 .. s, t = s (s + 1) / 2 + rb
  const int t = blockIdx.y;
  int s = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
  while ((s + 1) * (s + 2) / 2 <= t) ++s;
  while (s * (s + 1) / 2 > t) --s;
  const int rb = t - s * (s + 1) / 2;
  const int i0 = rb * CP_TILE, j0 = s * CP_TILE;
  if (j0 >= n) return;                                 // (the grid is sized by the launch's largest source)
  const int c0 = j0 + 2 * (tid & 31);                  // this lane's two columns
  const int r0 = i0 + (tid >> 5);                      // ... of the rows r0 + 8 q
  const double* src = Ps + (long)sb * pss + p_col(lds, j0) + 2 * (tid & 31);
  const long rs = p_lds(lds), rd = p_lds(ldd);
  cp_d2 v[CP_Q];
  bool on[CP_Q];
#pragma unroll
  for (int q = 0; q < CP_Q; ++q) {
    const int i = r0 + 8 * q;
    on[q] = i < n && c0 < n && c0 >= (i & ~1);
    v[q] = on[q] ? *reinterpret_cast<const cp_d2*>(src + (long)i * rs) : cp_d2{0.0, 0.0};
  }
  const long dcol = p_col(ldd, j0) + 2 * (tid & 31);
  for (int k = 0; k < cnt; ++k) {
    double* dst = Pd + (long)dl[k] * psd + dcol;
#pragma unroll
    for (int q = 0; q < CP_Q; ++q) {
      if (!on[q]) continue;
      cp_d2* p = reinterpret_cast<cp_d2*>(dst + (long)(r0 + 8 * q) * rd);
      if (NT) __builtin_nontemporal_store(v[q], p);
      else *p = v[q];
    }
  }
}

void launch_copy_traj(hipStream_t st, bool nt, const BankView& src, const BankView& dst, const double* mus, double* mud,
                      const int* tab, int groups, int n_hi) {
  const int tiles = copy_tiles(n_hi);
  const dim3 grid(groups, tiles + 1);            // (tiles + 1 <= 58 312 at EKF_N_MAX_LIMIT: inside the 65 535 of grid.y)
  if (nt)
    hipLaunchKernelGGL(k_copy_traj<true>, grid, dim3(CP_THREADS), 0, st, src.P, dst.P, mus, mud, dst.nact, src.flags, dst.flags, tab,
                       groups, tiles, src.ld, src.pstride, dst.ld, dst.pstride);
  else
    hipLaunchKernelGGL(k_copy_traj<false>, grid, dim3(CP_THREADS), 0, st, src.P, dst.P, mus, mud, dst.nact, src.flags, dst.flags, tab,
                       groups, tiles, src.ld, src.pstride, dst.ld, dst.pstride);
}

}  // namespace ekf
