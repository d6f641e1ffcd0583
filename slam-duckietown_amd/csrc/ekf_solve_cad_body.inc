// The body of k_solve_cad and k_solve_cad_plog (ekf_cadence.hip), included once for each with EKF_SOLVE_PLOG 0 / 1: the plain
// kernel's code is exactly what it was before the pose log existed (a shared inlined function template changed its register
// allocation), the logging kernel's is the same text plus the lines under #if EKF_SOLVE_PLOG.
  using G = CadGeom;
  constexpr int GM = G::GM, CU = G::CU;
  __shared__ __attribute__((aligned(16))) double Pc[CAD_ROWS][CAD_CS];
  __shared__ double2 hpS[128], kcS[128];
  __shared__ int Cs[128];
  __shared__ double2 zS[CAD_SLOTS];                    // (range, bearing) of slot s
  __shared__ double2 laS[CAD_SLOTS];                   // (lin, ang) of touched step p
  __shared__ int mS[CAD_SLOTS + 1], firstS[CAD_SLOTS + 1], loS[CAD_SLOTS + 1], fS[CAD_SLOTS];
  __shared__ double mot[4];                            // G[0,2], G[1,2] of the step being predicted
  __shared__ double2 hS[2][6];                         // linearisation of slot s in hS[s & 1]: {h[0][k], h[1][k]}, k < 5
  __shared__ double2 siS[2];                           // S^-1 of the slot in flight
  __shared__ double2 yS[2];                            // innovation of slot s in yS[s & 1] (for its record)
#if EKF_SOLVE_PLOG
  __shared__ double poseS[2][POSE_ROW];                // (PLOG) step p's pose mean and block on their way to the ring
#endif
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if ((int)blockIdx.x >= batch) {
    // ---- the COLUMN GATHER beside the chain (round 5) ----
    // The chain keeps one CU per trajectory busy for 55 - 70 us and the rest of the chip idle.  What the panel launch behind it
    // gathers of the covariance has two halves: P(C_u[a], i) for i >= C_u[a] lies in row C_u[a] (64 state indices: 512
    // contiguous bytes), for i < C_u[a] it is stored mirrored, as P_base(i, C_u[a]): one 16-byte pair per ROW i, a 64-byte
    // sector of its own each, and random sectors stream at a third of the rate rows do (PMC: 107 MB more fetched for 62 us
    // more at N = 2000 x 32 when the landmarks of a cadence are scattered over the map instead of consecutive,
    // profiles/r05_scattered_indices.txt).  Nothing of that depends on the chain: workgroups batch.. of THIS launch fetch
    // the mirrored pairs meanwhile -- 512 state indices each, every wave the pairs that lie entirely beyond its 64 indices --
    // and lay them down coalesced, colbuf[b][a][i]; the panel launch reads them as rows.  (The positions C_u are formed
    // from the plan exactly as the chain forms them.)
    // `col_wgs` workgroups (one per CU the chain leaves free, so that all of them are resident at once) share the items
    // (trajectory, 64 state indices), a wave at a time, all of a wave's loads in flight together.  An item costs what lies
    // beyond its state indices -- everything for the first strip, nothing for the last -- and there are a few more items than
    // waves (N = 2000 x 32: 2016 for 1792): dealt strip-major, dearest first, so that the second round is the cheap tail.
    // (Tickets from a global counter instead: 80 us against 60 -- 3800 atomics on one word; profiles/r05_scattered_indices.txt.)
    __shared__ int CsG[CAD_NW][128];                   // (per wave: the positions of the trajectory its item belongs to)
    __shared__ int cntG[CAD_NW][CAD_SLOTS + 1];
    const int strips = (n_hi + 63) >> 6, items = batch * strips;
    const int gwave = ((int)blockIdx.x - batch) * CAD_NW + wave;
    for (int item = gwave; item < items; item += col_wgs * CAD_NW) {
      const int strip = item / batch, b = item - strip * batch, i0 = 64 * strip, i = i0 + lane;
      const CadPlan pl = plan[b];
      const int n = nact[b];
      if (i0 >= n || i0 >= min(n, pl.neff) || pl.nslots == 0) continue;   // (uniform) nothing of this wave is replayed
      // the positions C_u of trajectory b, by this wave alone (cad_positions' shape for one wave: lane p = touched step p)
      int* Cw = CsG[wave];
      int* cw = cntG[wave];
      Cw[lane] = lane < 3 ? lane : 0;
      Cw[64 + lane] = 0;
      int cnt = 0, lo = 0;
      const StepIn* st = nullptr;
      if (lane < pl.ns) {
        st = in + ((long)(pl.t0 + lane) * batch + b);
        const CadRange r = cad_step_range(pl, st, lane, cfg.enable_measurement_model);
        lo = r.lo;
        cnt = r.cnt;
      }
      if (lane <= CAD_SLOTS) cw[lane] = lane < CAD_SLOTS ? cnt : 0;
      WAVE_LDS_SYNC();
      int first = 0;
      for (int u = 0; u < lane && u < CAD_SLOTS; ++u) first += cw[u];
      const int nslots = min(pl.nslots, CAD_SLOTS), s0 = GM - nslots;
      if (lane < pl.ns) {
        for (int j = 0; j < cnt; ++j) {
          const int sl = s0 + first + j;
          if (sl < GM) {
            const int idx = st->idx[lo + j], pq = G::pa(sl);
            Cw[pq] = 3 + 2 * idx;
            Cw[pq + 1] = 4 + 2 * idx;
          }
        }
      }
      WAVE_LDS_SYNC();
      const int ii = i < n ? i : n - 1;
      const double* Pb = P + (long)b * pstride;
      double* cb = colbuf + ((long)b * CAD_CU) * ld;
      v2d_u v[CAD_SLOTS];
      unsigned long long taken = 0ull;                 // (uniform) bit q: pair q is mirrored for this whole wave
      // Pairs whose neighbours in the cadence lie in the same 128-byte line of the row (consecutive landmarks: the 16 columns
      // of a step share one) want the caches -- eight pairs per line fetched once; a pair alone in its line should stream past
      // them (nontemporal: scattered landmarks 106 -> 95 us for the launch; clustered ones lose 8 us when they stream).
      // Decided per ITEM -- one branch around two copies of the loop: a choice per load merges 40 times and the loads wait
      // for one another (profiles/r05_scattered_indices.txt).
      int clustered = 0;
      if (lane < nslots) {
        const int a = 3 + 2 * lane, c0 = Cw[a];
        const int cprev = lane > 0 ? Cw[a - 2] : -64, cnext = lane + 1 < nslots ? Cw[a + 2] : -64;
        clustered = (abs(c0 - cprev) < 16 || abs(c0 - cnext) < 16) ? 1 : 0;
      }
      const bool stream_past = 2 * __popcll(__ballot(clustered != 0)) < nslots;   // (uniform) most pairs are alone in their lines
#define EKF_COLG_LOADS(LOAD)                                                                                              \
  _Pragma("unroll") for (int q = 0; q < CAD_SLOTS; ++q) {                                                                 \
    const int a = 3 + 2 * q;                                                                                              \
    const int c0 = Cw[a], c1 = Cw[a + 1];                                                                                 \
    const bool take = q < nslots && c1 == c0 + 1 && i0 + 63 <= c0 && (c1 & (PPW - 1)) != 0; /* (uniform: k_panels_cad's condition) */ \
    v[q].x = 0.0;                                                                                                         \
    v[q].y = 0.0;                                                                                                         \
    if (take) {                                                                                                           \
      v[q] = LOAD(reinterpret_cast<const v2d_u*>(Pb + p_index(ld, ii, c0)));                                              \
      taken |= 1ull << q;                                                                                                 \
    }                                                                                                                     \
  }
#define EKF_LOAD_CACHED(p) (*(p))
#define EKF_LOAD_STREAM(p) __builtin_nontemporal_load(p)
      if (stream_past) {
        EKF_COLG_LOADS(EKF_LOAD_STREAM)
      } else {
        EKF_COLG_LOADS(EKF_LOAD_CACHED)
      }
#undef EKF_LOAD_STREAM
#undef EKF_LOAD_CACHED
#undef EKF_COLG_LOADS
#pragma unroll
      for (int q = 0; q < CAD_SLOTS; ++q) {
        if (((taken >> q) & 1ull) && i < n) {
          const int a = 3 + 2 * q;
          cb[(long)a * ld + i] = v[q].x;
          cb[(long)(a + 1) * ld + i] = v[q].y;
        }
      }
      WAVE_LDS_SYNC();                                 // (the next item rewrites this wave's positions)
    }
    return;
  }
  const int b = blockIdx.x;
  const double* Pb = P + (long)b * pstride;
  const double* mu_in_b = mu_in + (long)b * ld;
  CadOut& o = out[b];
  const CadPlan pl = plan[b];
  const int nsteps = pl.ns;                            // touched steps
#if EKF_SOLVE_PLOG
  // is the last touched step finished here?  Its landmark count, fetched now and needed behind the last barrier.
  bool last_done = true;
  int pskip = 0, prow0 = 0;                            // steps p < pskip are overwritten in the ring by step p + cap
  if (nsteps > 0) {
    const StepIn& st = in[(long)(pl.t0 + nsteps - 1) * batch + b];
    const int mfull = ((st.flags & FLAG_UPDATE) && cfg.enable_measurement_model) ? min(st.m, MMAX) : 0;
    last_done = pl.jend >= mfull;
  }
  pskip = nsteps - plg.cap;
  prow0 = (int)((plg.slot0 + pl.t0) % plg.cap);
#endif
  // (chained) this workgroup is placed: the previous cadence's covariance pass may fill the rest of the chip now (the panel launch
  // in front of it waits for this word -- a pass that got there first keeps every CU busy for its whole duration, and the solve,
  // which needs a CU to itself, 20 us from being placed: profiles/r06_chained_solves.txt)
  if constexpr (CHAIN) {
    if (sync && threadIdx.x == 0) __hip_atomic_store(sync + SYNC_START * SYNC_STRIDE, start_sigma, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // (chained) block and mean come from k_chain_cad, whole (84 x 88, zeros beyond the positions in use): fetched before the
  // positions are formed -- nothing of it depends on them -- so that the two round trips overlap (2 us of the launch)
  constexpr int RQP = (CAD_CU + CAD_NW - 1) / CAD_NW;  // rows per wave
  double pre0[CHAIN ? RQP : 1], pre1[CHAIN ? RQP : 1], pmu0 = 0.0, pmu1 = 0.0;
  if constexpr (CHAIN) {
    if (gmu) {                                         // (uniform)
#pragma unroll
      for (int q = 0; q < RQP; ++q) {
        const double* gb = gbuf + ((long)b * CAD_ROWS + min(wave + CAD_NW * q, CAD_ROWS - 1)) * CAD_CS;
        pre0[q] = gb[lane];
        pre1[q] = gb[min(64 + lane, CAD_CS - 1)];
      }
      if (wave == 1) {
        pmu0 = gmu[(long)b * 128 + lane];
        pmu1 = gmu[(long)b * 128 + 64 + lane];
      }
    }
  }

  // ---- inputs: the plan's steps (thread p: touched step p), their landmarks' slots and positions ----
  int nslots;
  if (CHAIN && pre) {
    // (uniform) chained: formed one cadence ahead by the chain launch's positions workgroup (CadPre) -- one coalesced round trip
    const CadPre& pp = pre[b];
    if (tid < 128) Cs[tid] = pp.C[tid];
    if (tid <= CAD_SLOTS) {
      mS[tid] = pp.cnt[tid];
      firstS[tid] = pp.first[tid];
      loS[tid] = pp.lo[tid];
    }
    if (tid < CAD_SLOTS) {
      fS[tid] = pp.fl[tid];
      laS[tid] = make_double2(pp.la[tid][0], pp.la[tid][1]);
      zS[tid] = make_double2(pp.z[tid][0], pp.z[tid][1]);
    }
    nslots = pp.nslots;
  } else {
    if (tid < CAD_SLOTS) {
      int fl = 0;
      double2 la = make_double2(0.0, 0.0);
      if (tid < nsteps) {
        const StepIn& st = in[(long)(pl.t0 + tid) * batch + b];
        fl = st.flags;
        if (tid == 0 && pl.j0 > 0) fl &= ~FLAG_PREDICT;   // a step cut by the previous cadence: its prediction has happened
        la = make_double2(st.lin, st.ang);
      }
      fS[tid] = fl;
      laS[tid] = la;
    }
    nslots = cad_positions<true>(pl, in, batch, b, cfg, tid, Cs, mS, firstS, loS,
                                 [&](int s, double zr, double zb) { zS[s] = make_double2(zr, zb); });
  }
  const int s0 = GM - nslots;
  const int cu = 3 + 2 * nslots;                       // positions in use
  const int neff_eff = min(nact[b], pl.neff);
  __syncthreads();
  const int Cl0 = Cs[lane], Cl1 = Cs[64 + lane];       // positions lane and 64 + lane
  if (tid <= CU) o.C[tid] = tid < CU ? Cs[tid] : 0;
  if (tid < CAD_SLOTS) {
    // slot of touched step p's first landmark -- or of the next step's that has one: the panel launch applies a step's
    // prediction when it reaches that slot
    o.sfirst[tid] = tid < nsteps ? s0 + firstS[tid] : GM;
  }
  if (tid == 0) {
    o.nslots = nslots;
    o.neff = neff_eff;
    o.npred = nsteps;
    o.pad0 = 0;
  }

  // (NZ) this trajectory's row of the noise table (ekf_set_noise), loaded once; the other instantiations read cfg.rd / cfg.qd
  const NoiseRow nz = NZ ? noise_row(cfg, b) : NoiseRow{};

  // ---- the mean wave (wave 1): lane l holds the mean at positions l and 64 + l ----
  double mu0 = 0.0, mu1 = 0.0, y0 = 0.0, y1 = 0.0;
  double rdsum0 = 0.0, rdsum1 = 0.0, rdsum2 = 0.0;     // (wave 1) pose-block noise of the whole cadence
  LinGeom lg{};
  auto mean_at = [&](int p) -> double {                // p wave-uniform
    return p < 64 ? read_lane(mu0, p) : read_lane(mu1, p - 64);
  };
  // motion model of step t (src/replay_no_ros.py:368-417) at the current pose mean; publishes G[0,2], G[1,2]
  auto motion = [&](int t) {
    const double2 la = laS[t];
    const bool do_pred = (fS[t] & FLAG_PREDICT) != 0;
    const double th = read_lane(mu0, 2);
    Motion mo{read_lane(mu0, 0), read_lane(mu0, 1), th, 0.0, 0.0};
    if (do_pred && !cfg.disable_motion_model) mo = motion_model(mo.x, mo.y, mo.th, la.x, la.y, cfg);
    if (lane < 3) mu0 = lane == 0 ? mo.x : (lane == 1 ? mo.y : mo.th);
    if (do_pred) {
      rdsum0 += NZ ? nz.rd[0] : cfg.rd[0];
      rdsum1 += NZ ? nz.rd[1] : cfg.rd[1];
      rdsum2 += NZ ? nz.rd[2] : cfg.rd[2];
    }
    if (lane == 0) {
      mot[0] = mo.g0;
      mot[1] = mo.g1;
      *reinterpret_cast<double2*>(o.g[t]) = make_double2(mo.g0, mo.g1);
    }
  };
  auto jacobian_at_mean = [&](int p, int par) {        // landmark at positions p, p + 1: publishes hS[par], keeps the geometry
    double hn[2][5];
    lg = linearize_h(read_lane(mu0, 0), read_lane(mu0, 1), read_lane(mu0, 2), mean_at(p), mean_at(p + 1), hn);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 5; ++k) hS[par][k] = make_double2(hn[0][k], hn[1][k]);
    }
  };

  // ---- gather the block P[C_u, C_u] (nothing is pending: P = P_base -- or the look-ahead gather's copy); wave 1 starts on
  // its means meanwhile ----
  {
    constexpr int RQ = (CU + CAD_NW - 1) / CAD_NW;     // rows per wave
    const int lane_b = min(64 + lane, CAD_CS - 1);
    double gv0[RQ], gv1[RQ];
#pragma unroll
    for (int q = 0; q < RQ; ++q) {
      gv0[q] = 0.0;
      gv1[q] = 0.0;
    }
    if (CHAIN && gmu) {                                // (uniform) chained: fetched at the top of the launch
      if constexpr (CHAIN) {
#pragma unroll
        for (int q = 0; q < RQ; ++q) {
          gv0[q] = pre0[q];
          gv1[q] = pre1[q];
        }
      }
    } else if (gbuf) {
      // (uniform) look-ahead: the block was gathered (base + the ranks still pending then) by k_gather_cad, in `gparts`
      // parts, added here in a fixed order; all loads of a part are in flight together
      // (... four parts' loads in flight together: ten dependent round trips were 8 us of a single trajectory's cadence)
      constexpr int GPB = 4;
#pragma unroll
      for (int g0 = 0; g0 < KTOT / 8; g0 += GPB) {
        if (g0 < gparts) {                             // (uniform)
          double t0[GPB][RQ], t1[GPB][RQ];
#pragma unroll
          for (int u = 0; u < GPB; ++u) {
            const bool on = g0 + u < gparts && g0 + u < KTOT / 8;   // (uniform)
#pragma unroll
            for (int q = 0; q < RQ; ++q) {
              const int r = min(wave + CAD_NW * q, max(cu - 1, 0));
              const double* gb = gbuf + (((long)(on ? g0 + u : 0) * batch + b) * CAD_ROWS + r) * CAD_CS;
              t0[u][q] = on ? gb[lane] : 0.0;
              t1[u][q] = on ? gb[lane_b] : 0.0;
            }
          }
#pragma unroll
          for (int u = 0; u < GPB; ++u) {
#pragma unroll
            for (int q = 0; q < RQ; ++q) {
              gv0[q] += t0[u][q];
              gv1[q] += t1[u][q];
            }
          }
        }
      }
    } else {
#pragma unroll
      for (int q = 0; q < RQ; ++q) {
        const int r = wave + CAD_NW * q;
        if (r < cu) {                                  // (wave-uniform)
          const int Cr = Cs[r];
          gv0[q] = Pb[p_index(ld, min(Cr, Cl0), max(Cr, Cl0))];     // the upper triangle is authoritative
          if (cu > 64) gv1[q] = Pb[p_index(ld, min(Cr, Cl1), max(Cr, Cl1))];
        }
      }
    }
    if (wave == 1) {
      if (CHAIN && gmu) {                              // (uniform) chained: the mean at the positions, from k_chain_cad
        mu0 = pmu0;
        mu1 = pmu1;
      } else {
        mu0 = mu_in_b[Cl0];
        mu1 = mu_in_b[Cl1];
      }
    }
#pragma unroll
    for (int q = 0; q < RQ; ++q) {
      const int r = wave + CAD_NW * q;
      if (r < cu) {
        Pc[r][lane] = gv0[q];
        if (64 + lane < CAD_CS) Pc[r][64 + lane] = gv1[q];
      }
    }
  }
  // wave roles: 0 = the covariance chain (+ a down-date share), 1 = the mean, CAD_NW - 1 = the records (everything the
  // panel kernel gets goes to memory from there, off the chain), the others: down-date
  const bool rec_wave = wave == CAD_NW - 1;
  const int ds = wave == 0 ? 0 : wave - 1;             // down-date slot of this wave (waves 0, 2 .. CAD_NW - 2)
  // The NIS gate (GATE: the instantiations launched while ekf_set_nis_gate has it on; the others are the kernel without it): at
  // b1 y and S^-1 of the slot are in LDS and every wave forms the decision itself from them.  A rejected slot moves nothing: the mean wave skips its mean update, the down-date
  // waves skip the down-date, and the record wave writes the slot's record with H, the K rows and the pose's rank entries
  // zero (y and S^-1 kept), so that the panel launches, w_from_v and k_chain_cad all see two exact zero ranks.
  unsigned long long rmask = 0ull;                     // (record wave) slots rejected
  if (wave == 1) motion(0);
  WG_LDS_BARRIER();
  if (wave == 0) {                                     // (diagnostic record) rows 0, 1 of the block before the cadence
    if (lane < CU) {
      o.prow[0][lane] = Pc[0][lane];
      o.prow[1][lane] = Pc[1][lane];
    }
    if (64 + lane <= CU) {
      o.prow[0][64 + lane] = 64 + lane < CU ? Pc[0][64 + lane] : 0.0;
      o.prow[1][64 + lane] = 64 + lane < CU ? Pc[1][64 + lane] : 0.0;
    }
  }

  double dd0 = 0.0, dd1 = 0.0;                         // (wave 0, lanes 0..2) in-place change of P_base(0, l), P_base(1, l)
  for (int t = 0; t < nsteps; ++t) {
    const int m = __builtin_amdgcn_readfirstlane(mS[t]);
    const int s_first = s0 + __builtin_amdgcn_readfirstlane(firstS[t]);   // (a step without landmarks: the next step's first slot)
    const int ca = G::pa(s_first) + 2;                 // positions in use from this step on: [0, ca)  (s_first == GM: the pose)
    const bool two = ca > 64;                          // (uniform) the second half of the columns is live
    // ---- prediction of step t on the block: P' = G P G^T + R restricted to C_u (:428-430).  Only rows / columns 0, 1
    // change, and the block is exactly symmetric: lane r holds P[0..2][r] = P[r][0..2] and produces P'[r][0], P'[r][1],
    // which for r >= 2 are also P'[0][r], P'[1][r].  Wave 1 linearises the step's first landmark meanwhile.
    if (wave == 0) {
      const bool do_pred = (fS[t] & FLAG_PREDICT) != 0;
      const double g0 = mot[0], g1 = mot[1];
      const double rd0 = do_pred ? (NZ ? nz.rd[0] : cfg.rd[0]) : 0.0, rd1 = do_pred ? (NZ ? nz.rd[1] : cfg.rd[1]) : 0.0,
                   rd2 = do_pred ? (NZ ? nz.rd[2] : cfg.rd[2]) : 0.0;
      const double s20 = Pc[2][0], s21 = Pc[2][1], p22 = Pc[2][2];
      const int r0 = min(lane, ca - 1), r1 = min(64 + lane, CAD_CS - 1);
      const double p0 = Pc[0][r0], p1 = Pc[1][r0], p2 = Pc[2][r0];
      const double q0 = Pc[0][r1], q1 = Pc[1][r1], q2 = Pc[2][r1];
      const double gr = lane == 0 ? g0 : (lane == 1 ? g1 : 0.0);
#if EKF_SOLVE_PLOG  // the pose block behind step t - 1: column `lane` of rows 0..2
      if (t > 0 && lane < 3) {
        poseS[(t - 1) & 1][3 + lane] = p0;
        poseS[(t - 1) & 1][6 + lane] = p1;
        poseS[(t - 1) & 1][9 + lane] = p2;
      }
#endif
      double x0 = p0, x1 = p1, x2 = p2;                // row r of G P, columns 0..2 (rows 0, 1 take g_r x row 2)
      if (lane < 2) {
        x0 = fma(gr, s20, p0);
        x1 = fma(gr, s21, p1);
        x2 = fma(gr, p22, p2);
      }
      double c0n = fma(g0, x2, x0), c1n = fma(g1, x2, x1);
      dd0 += fma(g0, x2, lane < 2 ? gr * s20 : 0.0);   // P'(0, l) - P(0, l) and P'(1, l) - P(1, l) without the noise
      dd1 += fma(g1, x2, lane < 2 ? gr * s21 : 0.0);
      if (lane == 0) c0n += rd0;
      if (lane == 1) c1n += rd1;
      const double e0n = fma(g0, q2, q0), e1n = fma(g1, q2, q1);
      if (lane < ca) {
        Pc[lane][0] = c0n;
        Pc[lane][1] = c1n;
        if (lane >= 2) {
          Pc[0][lane] = c0n;
          Pc[1][lane] = c1n;
        }
        if (lane == 2) Pc[2][2] = p2 + rd2;
      }
      if (two && 64 + lane < ca) {
        Pc[64 + lane][0] = e0n;
        Pc[64 + lane][1] = e1n;
        Pc[0][64 + lane] = e0n;
        Pc[1][64 + lane] = e1n;
      }
    } else if (wave == 1) {
      if (m > 0) jacobian_at_mean(G::pa(s_first), s_first & 1);
    }
    WG_LDS_BARRIER();                                  // S0(t): predicted block and the first Jacobian published
#if EKF_SOLVE_PLOG  // step t - 1's row: parked by waves 1 and 0 before this barrier
    if (rec_wave && t > 0 && t - 1 >= pskip && lane < POSE_ROW) pose_row(plg, prow0, t - 1, batch, b)[lane] = poseS[(t - 1) & 1][lane];
#endif
    if (wave == 1 && m > 0) {
      const double2 z = zS[s_first];
      innovation(lg, z.x, z.y, y0, y1);
      if (lane == 0) yS[s_first & 1] = make_double2(y0, y1);
    }
    // ---- the step's landmarks, sequentially (:436-480) ----
    for (int j = 0; j < m; ++j) {
      const int s = s_first + j, pa = G::pa(s);        // this landmark sits at positions pa, pa + 1; [0, pa) lives on
      const bool two_j = pa + 2 > 64;                  // columns 64.. still in use
      const bool last = j + 1 == m && t + 1 == nsteps; // nothing reads the block after this landmark
      double2 hpa = make_double2(0.0, 0.0), hpb = make_double2(0.0, 0.0);   // (H P)[:, l] of this wave's columns
      if (wave == 0) {
        // phase A: rows sel = {0, 1, 2, pa, pa + 1} of P at column l give (H P)[:, l]; P is symmetric, so P H^T is the
        // transpose and the gain needs no second product
        // (the landmark's linearisation -- published by the mean wave before the barrier -- is read with the rows: one LDS
        //  round trip for both)
        const int la = min(lane, pa + 1), lb = min(64 + lane, CAD_CS - 1);
        double h[2][5];
        double pra[5], prb[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          const double2 tt = hS[s & 1][k];
          h[0][k] = tt.x;
          h[1][k] = tt.y;
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          const int r = k < 3 ? k : pa + (k - 3);
          pra[k] = Pc[r][la];
          prb[k] = 0.0;
        }
        if (two_j) {                                   // (uniform)
#pragma unroll
          for (int k = 0; k < 5; ++k) prb[k] = Pc[k < 3 ? k : pa + (k - 3)][lb];
        }
        hpa = make_double2(h[0][0] * pra[0], h[1][0] * pra[0]);
#pragma unroll
        for (int k = 1; k < 5; ++k) {
          hpa.x = fma(h[0][k], pra[k], hpa.x);
          hpa.y = fma(h[1][k], pra[k], hpa.y);
        }
        hpS[lane] = hpa;
        if (two_j) {
          hpb = make_double2(h[0][0] * prb[0], h[1][0] * prb[0]);
#pragma unroll
          for (int k = 1; k < 5; ++k) {
            hpb.x = fma(h[0][k], prb[k], hpb.x);
            hpb.y = fma(h[1][k], prb[k], hpb.y);
          }
          hpS[64 + lane] = hpb;
        }
        WAVE_LDS_SYNC();
        // phase B: S = H P H^T + Q (:473) from the five pairs at sel, every lane redundantly
        double2 hv[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) hv[k] = hpS[k < 3 ? k : pa + (k - 3)];
        double S00 = NZ ? nz.qd[0] : cfg.qd[0], S01 = 0.0, S10 = 0.0, S11 = NZ ? nz.qd[1] : cfg.qd[1];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          S00 = fma(hv[k].x, h[0][k], S00);
          S01 = fma(hv[k].x, h[1][k], S01);
          S10 = fma(hv[k].y, h[0][k], S10);
          S11 = fma(hv[k].y, h[1][k], S11);
        }
        const double rdet = fast_recip(S00 * S11 - S01 * S10);   // (<= 1 ulp; the IEEE division is ~250 dependent cycles of this chain)
        const double i00 = S11 * rdet, i01 = -S01 * rdet, i10 = -S10 * rdet, i11 = S00 * rdet;
        const double2 ka = make_double2(hpa.x * i00 + hpa.y * i10, hpa.x * i01 + hpa.y * i11);   // K[C_u[l], :]
        kcS[lane] = ka;
        if (two_j) kcS[64 + lane] = make_double2(hpb.x * i00 + hpb.y * i10, hpb.x * i01 + hpb.y * i11);
        if (lane == 0) {
          siS[0] = make_double2(i00, i01);
          siS[1] = make_double2(i10, i11);
        }
      }
      WG_LDS_BARRIER();                                // b1: K, (H P) and S^-1 of this landmark are in LDS
      bool rej = false;
      if constexpr (GATE) {
        const double2 gy = yS[s & 1], ga = siS[0], gc = siS[1];
        rej = innov_reject(gy.x, gy.y, ga.x, ga.y, gc.x, gc.y, cfg.nis_gate);
      }
      if (wave == 1) {
        // the mean (:476); then the next landmark's Jacobian at the new mean, or the next step's motion model
        // (the sums are spelled out as the compiler had contracted them before the gate existed -- the gate's branch would
        //  let it contract them differently: other bits -- with the first products behind empty asm statements)
        const double2 k0 = kcS[lane], k1 = kcS[64 + lane];
        double p0 = k0.x * y0, p1 = k1.y * y1;
        asm volatile("" : "+v"(p0), "+v"(p1));
        if (!rej) {
          if (lane < pa + 2) mu0 += fma(k0.y, y1, p0);
          if (64 + lane < pa + 2) mu1 += fma(k1.x, y0, p1);
        }
        if (j + 1 < m) jacobian_at_mean(pa - 2, (s + 1) & 1);
        else if (t + 1 < nsteps) {
#if EKF_SOLVE_PLOG
          if (lane < 3) poseS[t & 1][lane] = mu0;    // the pose mean behind step t
#endif
          motion(t + 1);
        }
      } else if (rec_wave) {
        // the record of this landmark for the panel kernel, and the pose's own entries of the new ranks
        double2* rec2 = reinterpret_cast<double2*>(o.rec + G::rec_off(s));
        const double2 ka = kcS[lane], kb = kcS[64 + lane];
        if (lane < pa) rec2[8 + lane] = ka;
        if (two_j && 64 + lane < pa) rec2[8 + 64 + lane] = kb;
        if (lane < 5) rec2[lane] = hS[s & 1][lane];
        if (lane == 5 || lane == 6) rec2[lane] = siS[lane - 5];
        if (lane == 7) rec2[7] = yS[s & 1];
        if (lane < 3) {
          const double2 hp = hpS[lane];
          double2* vw = reinterpret_cast<double2*>(o.posevw[s][lane]);
          vw[0] = hp;
          vw[1] = make_double2(-ka.x, -ka.y);
        }
        if (rej) {                                     // (NIS gate) the same places again, zero: H, the K rows, the pose's ranks
          const double2 z = make_double2(0.0, 0.0);
          if (lane < pa) rec2[8 + lane] = z;
          if (two_j && 64 + lane < pa) rec2[8 + 64 + lane] = z;
          if (lane < 5) rec2[lane] = z;
          if (lane < 3) {
            double2* vw = reinterpret_cast<double2*>(o.posevw[s][lane]);
            vw[0] = z;
            vw[1] = z;
          }
          rmask |= 1ull << s;
        }
#if EKF_SOLVE_PLOG
#define EKF_SOLVE_KEEP_LAST (CHAIN || last_done)       /* the pose block behind the cadence's last landmark is a row */
#else
#define EKF_SOLVE_KEEP_LAST CHAIN
#endif
      } else if ((EKF_SOLVE_KEEP_LAST || !last) && !rej) {                     // (CHAIN: the last landmark too -- the pose block behind it is a result)
        // down-date (:480) of what lives on: P[r][l] -= K[r, :] . (H P)[:, l] for r, l < pa; rows ds, ds + CAD_DW, ... are
        // this wave's.  Every access is unconditional and every address one base plus a compile-time offset: a row or a
        // column >= pa is dead (nothing reads it again), so what lands there does not matter, and rows up to
        // ds + CAD_DW (CAD_DQ - 1) <= 83 exist; all reads of a chunk are in flight before its first FMA.
        static_assert(CAD_DW - 1 + CAD_DW * (CAD_DQ - 1) < CAD_ROWS, "down-date rows stay inside the block");
        if (wave != 0) {
          hpa = hpS[lane];
          if (two_j) hpb = hpS[64 + lane];
        }
        const bool lane_b = 64 + lane < CAD_CS;        // second column half: columns 64 .. CAD_CS - 1 exist
        const int lb = lane_b ? 64 + lane : 64;
#pragma unroll
        for (int q0 = 0; q0 < CAD_DQ; q0 += CAD_DCH) {
          if (ds + CAD_DW * q0 < pa) {                 // (uniform)
            double2 kr[CAD_DCH];
            double pv[CAD_DCH], pw[CAD_DCH];
#pragma unroll
            for (int u = 0; u < CAD_DCH; ++u) {
              kr[u] = kcS[ds + CAD_DW * (q0 + u)];
              pv[u] = Pc[ds + CAD_DW * (q0 + u)][lane];
              pw[u] = 0.0;
            }
            if (two_j) {                               // (uniform)
#pragma unroll
              for (int u = 0; u < CAD_DCH; ++u) pw[u] = Pc[ds + CAD_DW * (q0 + u)][lb];
            }
#pragma unroll
            for (int u = 0; u < CAD_DCH; ++u) pv[u] = fma(-kr[u].x, hpa.x, pv[u]);
#pragma unroll
            for (int u = 0; u < CAD_DCH; ++u) pv[u] = fma(-kr[u].y, hpa.y, pv[u]);
#pragma unroll
            for (int u = 0; u < CAD_DCH; ++u) Pc[ds + CAD_DW * (q0 + u)][lane] = pv[u];
            if (two_j) {
#pragma unroll
              for (int u = 0; u < CAD_DCH; ++u) pw[u] = fma(-kr[u].x, hpb.x, pw[u]);
#pragma unroll
              for (int u = 0; u < CAD_DCH; ++u) pw[u] = fma(-kr[u].y, hpb.y, pw[u]);
              if (lane_b) {
#pragma unroll
                for (int u = 0; u < CAD_DCH; ++u) Pc[ds + CAD_DW * (q0 + u)][64 + lane] = pw[u];
              }
            }
          }
        }
      }
      WG_LDS_BARRIER();                                // b2: block down-dated; next Jacobian (or the next step's G) published
      if (wave == 1 && j + 1 < m) {
        const double2 z = zS[s + 1];
        innovation(lg, z.x, z.y, y0, y1);
        if (lane == 0) yS[(s + 1) & 1] = make_double2(y0, y1);
      }
    }
    if (m == 0) {                                      // (uniform) no landmark whose tail could carry the next motion model
      if (wave == 1 && t + 1 < nsteps) {
#if EKF_SOLVE_PLOG
        if (lane < 3) poseS[t & 1][lane] = mu0;
#endif
        motion(t + 1);
      }
      WG_LDS_BARRIER();
    }
  }

  // ---- results the solve owns: the pose mean, the pose block of P_base's rows 0, 1, the pending pose noise ----
  if (wave == 1) {
    double* mu_out_b = mu_out + (long)b * ld;
    bool bad = false;
    if (lane < 3) mu_out_b[lane] = mu0;
    bad = !(fabs(mu0) <= 1.79769313486231570815e308) || (64 + lane < CU && !(fabs(mu1) <= 1.79769313486231570815e308));
    if (__any(bad) && lane == 0) atomicOr(flags + b, EKF_FLAG_NONFINITE);
    if (lane == 0) {
      dacc_out[4 * b + 0] = rdsum0;
      dacc_out[4 * b + 1] = rdsum1;
      dacc_out[4 * b + 2] = rdsum2;
      o.rdsum[0] = rdsum0;                             // (for a cadence that appends no rank anywhere in the bank: see pose_epilogue)
      o.rdsum[1] = rdsum1;
      o.rdsum[2] = rdsum2;
      o.rdsum[3] = 0.0;
    }
  }
  if (wave == 0 && lane < 3) {
    o.ddpose[0][lane] = dd0;                           // entry (0, l)
    o.ddpose[1][lane] = dd1;                           // entry (1, l)
  }
  if constexpr (CHAIN) {
    if (rec_wave && lane < 16) o.posefin[lane >> 2][lane & 3] = ((lane >> 2) < 3 && (lane & 3) < 3) ? Pc[lane >> 2][lane & 3] : 0.0;
  }
  if (GATE && rec_wave && lane == 0) {
    o.rej = rmask;
    if (rmask) cfg.gate_rej[b] += (unsigned long long)__popcll(rmask);
  }
#if EKF_SOLVE_PLOG  // the cadence's last step, if it ends here: nothing writes the block any more
  if (nsteps > 0 && last_done) {
    if (wave == 1 && lane < 3) pose_row(plg, prow0, nsteps - 1, batch, b)[lane] = mu0;
    if (rec_wave && lane < 9) pose_row(plg, prow0, nsteps - 1, batch, b)[3 + lane] = Pc[lane / 3][lane % 3];
  }
#endif
#undef EKF_SOLVE_KEEP_LAST
