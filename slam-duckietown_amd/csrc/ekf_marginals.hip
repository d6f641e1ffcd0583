// k_marginals: the pose block and every landmark's 2 x 2 block of the CURRENT covariance, without applying the pending
// update (gfx950, wave64).  The covariance is (ekf_kernels.hip)
//     P(a, b) = P_base[a][b] + sum_k W[a][k] V[k][b] + [a == b < 3] dacc[a]      (a <= b)
// and a diagonal block needs P_base at its entries plus the W rows and V columns of its indices over the pending ranks:
// O(n k) per trajectory instead of the O(n^2) covariance pass.  Read-only: nothing the filter owns is written.
//
// What the pass would leave there, read with the pass's bounds (flush_pending / k_flush*):
//   . kb = the pending rank count rounded up to a whole k-tile (plan_pass: 4 * nkt); the pad ranks are zero-filled by the
//     step that appended last, and nothing beyond kb is read;
//   . per trajectory the pass covers the state indices below min(nact[b], so[b].neff); beyond that bound P is P_base alone
//     (an entry (a, b), a <= b, takes the ranks only where b lies below the bound);
//   . with no rank pending (kb == 0) nothing is added at all -- neither ranks nor dacc: the result is P_base bit for bit.
// Layouts: P_base through p_index (column panels beyond ld = 4096), V rank-major with row stride ld, W in MFMA A tiles
// (wm_index).
//
// Shape: a streaming kernel.  Workgroup (x, bi) = 4 waves over the 64 landmarks 64 x .. 64 x + 63 of trajectory b0 + bi,
// lane = landmark (its state indices i = 3 + 2 l, i + 1): per rank a lane reads V[k][i], V[k][i + 1] (16 consecutive bytes,
// consecutive across lanes) and W[i][k], W[i + 1][k] (inside the 128-byte rows of a 16-row group of W's tiles).  The four
// waves split the k-tiles (wave w takes the tiles w, w + 4, ...; the next tile's loads are in flight while one is summed),
// then wave 0 adds their partial sums in a fixed order.  Wave 1 of workgroup x == 0 forms the pose block: lane = rank,
// a butterfly over the lanes per entry.  Blocks of landmarks l in [n_landmarks, cap) are NaN.
#include <cmath>

#include "ekf_device.h"

#include "ekf_devfn.h"
#include "ekf_launch.h"

namespace ekf {

constexpr int MG_WAVES = 4;

struct MargTile {
  double v0[4], v1[4], w0[4], w1[4];   // V[k][i], V[k][i + 1], W[i][k], W[i + 1][k] for the 4 ranks of a k-tile
};

__global__ __launch_bounds__(64 * MG_WAVES) void k_marginals(const double* __restrict__ P, const double* __restrict__ V,
                                                             const double* __restrict__ W, const double* __restrict__ dacc,
                                                             const int* __restrict__ nact, const SolveOut* __restrict__ so,
                                                             int ld, long pstride, int b0, int kb, int cap,
                                                             double* __restrict__ pose_out, double* __restrict__ lm_out) {
  __shared__ double part[MG_WAVES][3][64];
  const int bi = blockIdx.y, b = b0 + bi;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = nact[b];
  const int nl = (n - 3) >> 1;
  const int bound = kb > 0 ? min(n, so[b].neff) : 0;   // state indices below it take the pending ranks
  const double* Pb = P + (long)b * pstride;
  const double* Vb = V + (long)b * KTOT * ld;
  const double* Wb = W + (long)b * KTOT * ld;
  const __amdgpu_buffer_rsrc_t rsV = rs_rsrc(Vb), rsW = rs_rsrc(Wb);
  const int ld16 = ld >> 4;

  // ---- landmarks ----
  const int l0 = blockIdx.x * 64;                      // first landmark of the workgroup
  if (lm_out && l0 < cap) {
    const int l = l0 + lane;
    const bool live = l < nl;
    const int i = live ? 3 + 2 * l : 3;                // (lanes beyond the landmarks read landmark 0's entries, discarded)
    double base00 = 0.0, base01 = 0.0, base11 = 0.0;
    if (wave == 0 && l0 < nl) {                        // the base entries first: their latency hides under the ranks
      base00 = Pb[p_index(ld, i, i)];
      base01 = Pb[p_index(ld, i, i + 1)];
      base11 = Pb[p_index(ld, i + 1, i + 1)];
    }
    double s00 = 0.0, s01 = 0.0, s11 = 0.0;
    const int nkt = kb >> 2;
    // (wave-uniform) some landmark of the workgroup lies below the bound, and this wave has a k-tile
    if (l0 < nl && 3 + 2 * l0 < bound && wave < nkt) {
      const unsigned vi = (unsigned)i * 8u, vrow = (unsigned)ld * 8u;
      const unsigned wi0 = (unsigned)((i >> 4) * 64 + (i & 15)) * 8u;
      const unsigned wi1 = (unsigned)(((i + 1) >> 4) * 64 + ((i + 1) & 15)) * 8u;
      auto load = [&](MargTile& T, int t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = 4 * t + r;
          T.v0[r] = ldb8(rsV, vi, (unsigned)k * vrow);
          T.v1[r] = ldb8(rsV, vi + 8u, (unsigned)k * vrow);
          const unsigned kw = (unsigned)((t * ld16) * 64 + r * 16) * 8u;   // wm_index: rank part (k-tile t, k & 3 = r)
          T.w0[r] = ldb8(rsW, wi0, kw);
          T.w1[r] = ldb8(rsW, wi1, kw);
        }
      };
      MargTile A, B;
      int t = wave;
      load(A, t);
      for (;;) {
        const int tn = t + MG_WAVES;
        if (tn < nkt) load(B, tn);                     // (wave-uniform) the next tile in flight while this one is summed
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s00 = fma(A.w0[r], A.v0[r], s00);
          s01 = fma(A.w0[r], A.v1[r], s01);
          s11 = fma(A.w1[r], A.v1[r], s11);
        }
        if (tn >= nkt) break;
        t = tn;
        const int tn2 = t + MG_WAVES;
        if (tn2 < nkt) load(A, tn2);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s00 = fma(B.w0[r], B.v0[r], s00);
          s01 = fma(B.w0[r], B.v1[r], s01);
          s11 = fma(B.w1[r], B.v1[r], s11);
        }
        if (tn2 >= nkt) break;
        t = tn2;
      }
    }
    part[wave][0][lane] = s00;
    part[wave][1][lane] = s01;
    part[wave][2][lane] = s11;
    __syncthreads();
    if (wave == 0 && l < cap) {
      double o00, o01, o11;
      if (live) {
        double r00 = part[0][0][lane], r01 = part[0][1][lane], r11 = part[0][2][lane];
#pragma unroll
        for (int w = 1; w < MG_WAVES; ++w) {
          r00 += part[w][0][lane];
          r01 += part[w][1][lane];
          r11 += part[w][2][lane];
        }
        o00 = i < bound ? base00 + r00 : base00;
        o01 = i + 1 < bound ? base01 + r01 : base01;
        o11 = i + 1 < bound ? base11 + r11 : base11;
      } else {
        o00 = o01 = o11 = __builtin_nan("");
      }
      double* dst = lm_out + ((long)bi * cap + l) * 4;
      dst[0] = o00;
      dst[1] = o01;
      dst[2] = o01;
      dst[3] = o11;
    }
  }

  // ---- pose block (one wave per trajectory) ----
  if (blockIdx.x == 0 && wave == 1) {
    double s[6];                                       // (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
#pragma unroll
    for (int e = 0; e < 6; ++e) s[e] = 0.0;
    for (int k0 = 0; k0 < kb; k0 += 64) {              // (kb <= 80: two rounds at most)
      const int k = k0 + lane;
      if (k < kb) {
        const unsigned kv = (unsigned)(k * ld) * 8u;
        const unsigned kw = (unsigned)(((k >> 2) * ld16) * 64 + (k & 3) * 16) * 8u;
        const double v0 = ldb8(rsV, kv, 0u), v1 = ldb8(rsV, kv, 8u), v2 = ldb8(rsV, kv, 16u);
        const double w0 = ldb8(rsW, kw, 0u), w1 = ldb8(rsW, kw, 8u), w2 = ldb8(rsW, kw, 16u);
        s[0] = fma(w0, v0, s[0]);
        s[1] = fma(w0, v1, s[1]);
        s[2] = fma(w0, v2, s[2]);
        s[3] = fma(w1, v1, s[3]);
        s[4] = fma(w1, v2, s[4]);
        s[5] = fma(w2, v2, s[5]);
      }
    }
#pragma unroll
    for (int e = 0; e < 6; ++e)
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) s[e] += __shfl_xor(s[e], off, 64);
    if (lane < 9) {                                    // lane = row-major entry of the 3 x 3 block, from its upper triangle
      const int r = lane / 3, c = lane - 3 * r;
      const int a = min(r, c), bb = max(r, c);
      double sum = 0.0;
      if (a == 0) sum = bb == 0 ? s[0] : (bb == 1 ? s[1] : s[2]);
      else if (a == 1) sum = bb == 1 ? s[3] : s[4];
      else sum = s[5];
      double v = Pb[p_index(ld, a, bb)];
      if (kb > 0) {                                    // (the pose indices always lie below the bound)
        v += sum;
        if (a == bb) v += dacc[4 * b + a];
      }
      pose_out[(long)bi * 9 + lane] = v;
    }
  }
}

void launch_marginals(hipStream_t st, const PendingView& f, int cap, double* pose_out, double* lm_out) {
  const int gx = lm_out && cap > 0 ? (cap + 63) / 64 : 1;
  hipLaunchKernelGGL(k_marginals, dim3(gx, f.count), dim3(64 * MG_WAVES), 0, st, f.P, f.V, f.W, f.dacc, f.nact, f.so, f.ld,
                     f.pstride, f.b0, f.kb, cap, pose_out, lm_out);
}

}  // namespace ekf
