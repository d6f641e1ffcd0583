// k_remove: marginalise landmarks out of a running filter (ekf_remove_landmarks) -- the in-place compaction of the stored
// upper triangle of P_base and of the mean, on the layout of ekf_device.h (row-major up to ld = 4096, column panels beyond).
//
// Removing landmarks from a Gaussian deletes their rows and columns: nothing is recomputed, stored values only move.  With
// src[t] the old state index of new index t (the same table for every trajectory of the launch: one removal list) and r0 the
// first removed state index, every stored entry (src[t], src[c]), t <= c < n_new, goes to (t, c).  Entries with both indices
// below r0 stay where they are.  A destination is never above its source in either layout (src[t] >= t), so:
//   - a row t < r0 only compacts its columns [r0, n_new) within itself: the workgroup reads them all, then writes them;
//   - a row t >= r0 is written from old row src[t] > t, and its own memory holds old row t, the source of new row dst[t] < t
//     (dst: old index -> new index, -1 removed).  The workgroup of new row t reads its whole source row into registers and
//     announces that (its word of `rflag` <- the launch's sequence number, written through: device scope); before it writes
//     row t it waits until the workgroup of new row dst[t] has announced the same.  Every wait is for a row with a LOWER
//     index of the same trajectory -- a workgroup dispatched earlier, whose reads wait for nothing -- so the order of dispatch
//     alone rules out a dead lock (the cadence counters of ekf_cadence.hip rely on the same).
// No workgroup ever reads a value written in this launch, so the XCDs' L2s need no write-back in between: the reads are of
// the previous launches' data, the announcements go past the L2 (device-scope store after s_waitcnt vmcnt(0): the row is in
// registers), the waits poll past it.  A wait that runs into its bound sets EKF_FLAG_INTERNAL (the state is undefined; the
// call reports EKF_ERR_STATE).
// The vacated strip beyond n_new is left as it is: nothing reads the triangle beyond a trajectory's size (the small-state load,
// k_pack_small / k_pack_dense, k_mirror and the dense product stop at n; ekf_add_landmarks and the device association write
// every entry of the columns they add, as after an upload of a smaller state).
// One workgroup of 256 threads per (trajectory, new row), NQ columns per thread (ekf_host_plan.h: plan_remove); blockIdx.x = 0
// compacts the mean, blockIdx.x = 1 + t takes row t.  Vector stores only.
#include "ekf_host_plan.h"
#include "ekf_launch.h"

namespace ekf {

constexpr int RM_SPIN_LIMIT = 1 << 20;  // bounded waits (s_sleep + one load past the L2 each): about a second

__device__ __forceinline__ bool rm_wait(const unsigned* word, unsigned seq) {
  for (int spin = 0; spin < RM_SPIN_LIMIT; ++spin) {
    if (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == seq) return true;
    __builtin_amdgcn_s_sleep(2);
  }
  return false;
}

template <int NQ>
__global__ __launch_bounds__(RM_THREADS) void k_remove(double* __restrict__ P, double* __restrict__ mu, const int* __restrict__ nact,
                                                  const int* __restrict__ src, const int* __restrict__ dst,
                                                  unsigned* __restrict__ rflag, unsigned* __restrict__ flags, int b0, int k2,
                                                  int r0, unsigned seq, int ld, long pstride) {
  const int b = b0 + blockIdx.y, tid = threadIdx.x;
  const int n_new = nact[b] - k2;
  if (blockIdx.x == 0) {                               // the mean: mu[t] <- mu[src[t]], t in [r0, n_new)
    double* m = mu + (long)b * ld;
    double v[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int c = r0 + tid + RM_THREADS * q;
      v[q] = c < n_new ? m[src[c]] : 0.0;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int c = r0 + tid + RM_THREADS * q;
      if (c < n_new) m[c] = v[q];
    }
    return;
  }
  const int t = blockIdx.x - 1;
  if (t >= n_new) return;
  const bool moves = t >= r0;                          // (uniform)
  const int s = moves ? src[t] : t;
  const int c0 = moves ? t : r0;                       // first column written: the row's diagonal, or r0 for a row that stays
  if (c0 >= n_new) return;
  double* Pb = P + (long)b * pstride;
  const long srow = (long)s * p_lds(ld);
  double v[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int c = c0 + tid + RM_THREADS * q;
    v[q] = c < n_new ? Pb[p_col(ld, src[c]) + srow] : 0.0;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the row is in registers ...
  __syncthreads();
  if (moves) {
    if (tid == 0) {
      __hip_atomic_store(rflag + (long)b * ld + t, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ... announced
      const int reader = dst[t];                       // who reads old row t (-1: removed, nobody)
      if (reader >= 0 && reader != t && !rm_wait(rflag + (long)b * ld + reader, seq)) atomicOr(flags + b, EKF_FLAG_INTERNAL);
    }
    __syncthreads();
  }
  const long drow = (long)t * p_lds(ld);
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int c = c0 + tid + RM_THREADS * q;
    if (c < n_new) Pb[p_col(ld, c) + drow] = v[q];
  }
}

void launch_remove(hipStream_t st, const BankView& k, double* mu, const RemovePlan& rp, const int* src, const int* dst,
                   unsigned* rflag, int b0, int nb, unsigned seq) {
  const dim3 grid(1 + rp.rows, nb);
#define EKF_RM_CASE(Q) \
  case Q: hipLaunchKernelGGL(k_remove<Q>, grid, dim3(RM_THREADS), 0, st, k.P, mu, k.nact, src, dst, rflag, k.flags, b0, rp.k2, rp.r0, seq, k.ld, k.pstride); break;
  switch (rp.nq) {
    EKF_RM_CASE(1)
    EKF_RM_CASE(2)
    EKF_RM_CASE(4)
    EKF_RM_CASE(8)
    EKF_RM_CASE(16)
    EKF_RM_CASE(32)
    EKF_RM_CASE(64)
    default: hipLaunchKernelGGL(k_remove<96>, grid, dim3(RM_THREADS), 0, st, k.P, mu, k.nact, src, dst, rflag, k.flags, b0, rp.k2, rp.r0, seq, k.ld, k.pstride);
  }
#undef EKF_RM_CASE
}

}  // namespace ekf
