// libmhe: the fused single-launch solve of small general problems (mixed scalar rows, extra
// variables z, equality rows) -- k_gn_general.  Included by mhe_core.h inside namespace mhe,
// after the register-resident kernels it is built from.
//
// One workgroup per trajectory runs the whole Gauss-Newton loop of the large-system path's
// general problems (mhe_big.h: k_big_resid -> k_big_assemble -> k_big_chol -> k_big_border ->
// k_big_update, a dozen launches per iteration over an HBM workspace) with the system where
// k_gn keeps it: node-major, H in the MFMA accumulator tiles, everything else in LDS.
//   node phase, gradient     node_phase / grad_phase, as k_gn (per-solve Pw)
//   measurement phase        rows grouped by epoch (bitwise-identical Phi rows, detected when
//                            the constants are built): G_e = sum_{i in e} g_i R_i g_i^T (n x n),
//                            GE_e = sum g_i R_i e_i, and with extra variables the border sums
//                            H_x^T R H_z, H_z^T R H_z, H_z^T R e -- MeasMixed::eval_slots per
//                            row, rows of an epoch in ascending order by the same 8 lanes
//   tiles                    build_tiles / h_element over the E epochs in the place of M rows
//   factorization            factor_forward: H = U^T U, y = U^-T b
//   bordered step            Bd = [H_xz C^T] (dp x K) through U^-T in 16-column panels
//                            (fwd_sweep_panel), Sigma = S - V^T V, LDL^T (big_ldl_factor /
//                            big_ldl_solve) of Sigma w = r - V^T y, y -= V w, then backward():
//                            dx = U^-1 (y - V w), dz = w[0:nz], lambda = w[nz:K] -- the step of
//                            k_big_border (Z = H^-1 Bd there; V^T V = Bd^T Z, V^T y = Bd^T du)
//   update                   (X, z) += (dx, dz), max|(dx, dz)| <= tol (1 + max|(X, z)|)
// No pseudo-Huber rows, no Huber dynamics cost, no bounds, no covariance: those keep the
// large-system path (fg_eligible, mhe_solve).

// ------------------------------------------------------------ layouts
constexpr int FG_LDS_DOUBLES = 160 * 1024 / 8;  // REG_LDS_LIMIT (mhe_launch.h asserts it)

// Constants: the register path's layout for (P, M, n, p = 1, NT) -- k_build_cc fills its Cc
// (no measurement term: the rows are nonlinear), DA, DB; Phi holds the E <= M epoch rows
// Phi_E (E x P), PhiT their transpose (P x M, stride M) -- then the epoch tables and the
// equality rows.
struct FgConst {
  ConstLayout C;
  size_t erow, ne, flag, rowe, eq, eqr, total;
};
__host__ __device__ inline FgConst fg_const_layout(int P, int M, int n, int NT, int nc) {
  FgConst L;
  L.C = const_layout(P, M, n, 1, NT, false);
  size_t o = L.C.total;
  const int Mr = M > 0 ? M : 1, ncr = nc > 0 ? nc : 1;
  L.erow = o; o = align256(o + sizeof(int) * (Mr + 1));  // first row of each epoch, erow[E] = M
  L.ne = o;   o = align256(o + sizeof(int));             // E
  L.flag = o; o = align256(o + sizeof(int) * Mr);        // scratch: row starts a new epoch
  L.rowe = o; o = align256(o + sizeof(int) * Mr);        // row -> epoch
  L.eq = o;   o = align256(o + sizeof(int) * 2 * ncr);   // equality-row index pairs
  L.eqr = o;  o = align256(o + sizeof(double) * ncr);    // their constants
  L.total = o;
  L.C.total = o;  // the buffer resource of the shared phases covers the whole buffer
  return L;
}

// LDS: the register path's layout with EC epochs in the place of the M rows (GE: EC x n,
// G: EC x n x n), then the epoch states, z, the border sums per epoch, the border panels
// (KP x dp, one row-major 16 x 16 block per block row and panel), the Schur system and the
// epoch rows Phi_E (EC x P; build_tiles reads them E times per element).
struct FgSmem {
  SmemLayout S;
  int XE, ZS, GZ, HZZ, GZV, VP, MS, RW, LC, FLG, PHE, total;
};
__host__ __device__ inline FgSmem fg_smem_layout(int P, int EC, int n, int NT, int nz, int nc) {
  constexpr int NZX = MHE_MAX_EXTRA;
  FgSmem F;
  F.S = smem_layout(P, EC, n, NT, true);
  int o = F.S.total;
  const int K = nz + nc, KP = (K + 15) / 16 * 16, dp = 16 * NT;
  F.XE = o;  o += rnd2(EC * n);
  F.ZS = o;  o += NZX;
  F.GZ = o;  o += nz > 0 ? rnd2(EC * n * NZX) : 0;
  F.HZZ = o; o += nz > 0 ? EC * NZX * NZX : 0;
  F.GZV = o; o += nz > 0 ? EC * NZX : 0;
  F.VP = o;  o += KP * dp;
  F.MS = o;  o += rnd2(K * K);
  F.RW = o;  o += rnd2(K);
  F.LC = o;  o += rnd2(K);
  F.FLG = o; o += 2;
  F.PHE = o; o += rnd2(EC * P);
  F.total = o;
  return F;
}

// Epochs the LDS layout holds: min(M, what REG_LDS_LIMIT leaves beside the fixed part).  A
// function of dims alone (fg_eligible needs >= 1); mhe_build_constants refuses a Phi with more
// distinct rows than this.
__host__ __device__ inline int fg_epoch_cap(int P, int M, int n, int NT, int nz, int nc) {
  constexpr int NZX = MHE_MAX_EXTRA;
  const int fixed = fg_smem_layout(P, 0, n, NT, nz, nc).total + 8;  // 8: the rnd2 paddings
  const int per = n + n * n + n + P + (nz > 0 ? n * NZX + NZX * NZX + NZX : 0);
  const int cap = fixed < FG_LDS_DOUBLES ? (FG_LDS_DOUBLES - fixed) / per : 0;
  return M < cap ? M : cap;
}

// ------------------------------------------------------------ residual pass
// Cost, gradient (BV = -g) and the per-node / per-epoch blocks of H at (Xs, z).  `ae` is the
// launch's GnArgs with M replaced by the epoch count E (grad_phase and build_tiles run over
// the epochs); Mf is the row count M.
template <class DYN, class MEAS>
__device__ __forceinline__ double fg_resid(const GnArgs& ae, const FgConst& FC, const FgSmem& FS, double* sm, int b,
                                           int E, int Mf) {
  constexpr int n = DYN::n, NZX = MHE_MAX_EXTRA, q = MEAS::q;
  const ConstLayout& CL = FC.C;
  const SmemLayout& SL = FS.S;
  const int nz = ae.nz;
  double cost = node_phase<DYN>(ae, CL, SL, sm, b);
  const int tid = opaque_tid();
  // interpolated states at the epochs, x_e = sum_j Phi_E[e][j] X_j, and the epoch sums zeroed
  {
    const double* PhiET = (const double*)(ae.cbuf + CL.PhiT);
    const double* Xs = sm + SL.Xs;
    for (int e = tid; e < E; e += NTHREADS) {
      double xe[n];
#pragma unroll
      for (int c = 0; c < n; ++c) xe[c] = 0.0;
      for (int j = 0; j < ae.P; ++j) {
        const double ph = PhiET[(size_t)j * Mf + e];
#pragma unroll
        for (int c = 0; c < n; ++c) xe[c] += ph * Xs[j * n + c];
      }
#pragma unroll
      for (int c = 0; c < n; ++c) sm[FS.XE + e * n + c] = xe[c];
    }
    for (int t = tid; t < E * n * n; t += NTHREADS) sm[SL.G + t] = 0.0;
    for (int t = tid; t < E * n; t += NTHREADS) sm[SL.GE + t] = 0.0;
    if (nz > 0) {
      for (int t = tid; t < E * n * NZX; t += NTHREADS) sm[FS.GZ + t] = 0.0;
      for (int t = tid; t < E * NZX * NZX; t += NTHREADS) sm[FS.HZZ + t] = 0.0;
      for (int t = tid; t < E * NZX; t += NTHREADS) sm[FS.GZV + t] = 0.0;
    }
  }
  __syncthreads();
  // measurement rows, epoch-grouped: 8 consecutive lanes per epoch walk its rows in ascending
  // order; each evaluates the row (eval_slots: at most 7 gradient slots), lane u < 7 adds
  // slot u's row of the outer product -- after merging equal indices the slots of a row touch
  // distinct rows of G_e, so no two lanes add to one element in a step, and the LDS
  // operations of a wave execute in order: every element's sum runs over the rows in ascending
  // order, whatever the batch or the occupancy.  R_i = 0 masks a row before h is evaluated.
  {
    const int* erow = (const int*)(ae.cbuf + FC.erow);
    const double* Rw = ae.Rw ? ae.Rw + (long long)b * ae.rwstride : (const double*)(ae.cbuf + CL.Rw);
    const double* Zs = sm + FS.ZS;
    const int u = tid & 7;
    for (int e = tid >> 3; e < E; e += NTHREADS / 8) {
      const double* xe = sm + FS.XE + e * n;
      double* G = sm + SL.G + e * n * n;
      double* ge = sm + SL.GE + e * n;
      double* Gz = sm + FS.GZ + e * n * NZX;
      double* Hzz = sm + FS.HZZ + e * NZX * NZX;
      double* gz = sm + FS.GZV + e * NZX;
      const int i1 = erow[e + 1];
      for (int i = erow[e]; i < i1; ++i) {
        const double R = Rw[i];
        if (R == 0.0) continue;
        const double* PR = ae.PAR + (long long)b * ae.pstride + (long long)i * q;
        double h, gs[7];
        int id[7];
        MEAS::eval_slots([&](int c) { return c < n ? xe[c] : Zs[c - n]; }, PR, nz, h, id, gs);
        // a component in two slots gets their sum; zero gradients dropped (as k_big_resid)
#pragma unroll
        for (int k1 = 0; k1 < 7; ++k1)
#pragma unroll
          for (int k2 = k1 + 1; k2 < 7; ++k2)
            if (id[k1] >= 0 && id[k2] == id[k1]) {
              gs[k1] += gs[k2];
              id[k2] = -1;
            }
#pragma unroll
        for (int k1 = 0; k1 < 7; ++k1)
          if (gs[k1] == 0.0) id[k1] = -1;
        const double ev = ae.Y[(long long)b * Mf + i] - h;
        const double Re = R * ev;
        if (u == 0) cost += ev * Re;
        int ia = -1;
        double ga = 0.0;
#pragma unroll
        for (int k1 = 0; k1 < 7; ++k1)
          if (u == k1) {
            ia = id[k1];
            ga = gs[k1];
          }
        if (ia >= 0) {
          if (ia < n) ge[ia] += ga * Re;
          else gz[ia - n] += ga * Re;
#pragma unroll
          for (int v = 0; v < 7; ++v) {
            if (id[v] < 0) continue;
            const int ib = id[v];
            const double w2 = R * (ga * gs[v]);  // the same value at (ia, ib) and (ib, ia)
            if (ia < n && ib < n) G[ia * n + ib] += w2;
            else if (ia < n) Gz[ia * NZX + (ib - n)] += w2;
            else if (ib >= n) Hzz[(ia - n) * NZX + (ib - n)] += w2;
          }
        }
        wave_lds_sync();
      }
    }
  }
  __syncthreads();
  cost += grad_phase<DYN, true, false, false, false>(ae, CL, SL, sm, b);
  return cost;
}

// ------------------------------------------------------------ bordered step
// After factor_forward (U in the accumulator slots, L_kk^-T in DT, y = U^-T b complete in YV):
// the step k_big_border takes, through the forward half of the factor only.  Leaves
// y - V w in YV (backward<SLOTS, true> then gives dx), w = [dz; lambda] in RW.  Returns false
// for a non-finite Sigma or pivot of it (MHE_STATUS_NOT_SPD).  Signs and row order: the KKT
// system in include/mhe.h.
template <int n, int SLOTS>
__device__ __forceinline__ bool fg_border(const GnArgs& ae, const FgConst& FC, const FgSmem& FS, double* sm,
                                          d4 (&acc)[SLOTS], int wave, int lane, int stab, int b, int E) {
  constexpr int NZX = MHE_MAX_EXTRA;
  const SmemLayout& SL = FS.S;
  const int nz = ae.nz, nc = ae.nc, K = nz + nc, KP = (K + 15) / 16 * 16;
  const int NT = ae.NT, dp = 16 * NT, d = ae.d, P = ae.P;
  const double* PhiE = (const double*)(ae.cbuf + FC.C.Phi);
  const int* eq = (const int*)(ae.cbuf + FC.eq);
  const double* eqr = (const double*)(ae.cbuf + FC.eqr);
  double* VP = sm + FS.VP;
  double* YV = sm + SL.YV;
  double* Ms = sm + FS.MS;
  double* rw = sm + FS.RW;
  double* lc = sm + FS.LC;
  int* flg = (int*)(sm + FS.FLG);
  // element (row i, column c) of the border columns / of V
  auto vat = [&](int i, int c) -> double& { return VP[(c >> 4) * dp * 16 + (i >> 4) * 256 + (i & 15) * 16 + (c & 15)]; };
  // (1) Bd = [H_xz C^T], node-major rows (padding rows and the panels' spare columns 0):
  //     column c < nz at row (j, ca): sum_e Phi_E[e][j] GZ_e[ca][c] in epoch order;
  //     column nz + k: +1 at eq[2k], -1 at eq[2k + 1]
  for (int t = threadIdx.x; t < KP * dp; t += NTHREADS) {
    const int c = t / dp, i = t - c * dp;
    double v = 0.0;
    if (i < d && c < K) {
      if (c < nz) {
        const int j = i / n, ca = i - j * n;
        for (int e = 0; e < E; ++e) v += PhiE[(size_t)e * P + j] * sm[FS.GZ + (e * n + ca) * NZX + c];
      } else {
        if (eq[2 * (c - nz)] == i) v += 1.0;
        if (eq[2 * (c - nz) + 1] == i) v -= 1.0;
      }
    }
    vat(i, c) = v;
  }
  if (threadIdx.x == 0) flg[0] = 0;
  __syncthreads();
  // (2) V = U^-T Bd, panel by panel, in place
  for (int p0 = 0; p0 < KP; p0 += 16) {
    d4 unused = {0.0, 0.0, 0.0, 0.0};
    fwd_sweep_panel<SLOTS, true>(NT, sm + SL.DT, VP + p0 * dp, acc, wave, lane, stab, unused);
    __syncthreads();
  }
  // (3) Sigma = S - V^T V (lower triangle, mirrored) and r - V^T y: one wave per entry, lanes
  //     over the rows
  for (int t = wave; t < K * K + K; t += NW) {
    const bool isr = t >= K * K;
    const int r = isr ? t - K * K : t / K, c = isr ? 0 : t - (t / K) * K;
    if (!isr && c > r) continue;
    double s = 0.0;
    for (int i = lane; i < dp; i += 64) s += vat(i, r) * (isr ? YV[i] : vat(i, c));
    s = wave_sum(s);
    if (lane == 0) {
      double base = 0.0;
      if (isr) {
        if (r < nz) {  // -g_z = sum H_z^T R e
          for (int e = 0; e < E; ++e) base += sm[FS.GZV + e * NZX + r];
        } else {  // -c(v)
          const int ia = eq[2 * (r - nz)], ib = eq[2 * (r - nz) + 1];
          base = -(sm[SL.Xs + ia] - (ib >= 0 ? sm[SL.Xs + ib] : 0.0) - eqr[r - nz]);
        }
        rw[r] = base - s;
      } else {
        if (r < nz && c < nz)
          for (int e = 0; e < E; ++e) base += sm[FS.HZZ + e * NZX * NZX + r * NZX + c];
        Ms[r * K + c] = base - s;
        Ms[c * K + r] = base - s;
      }
    }
  }
  __syncthreads();
  // (4) LDL^T without pivoting (quasi-definite; a z no row depends on has an exactly zero
  //     pivot and is held) and the solve, wave 0
  if (wave == 0) {
    bool bad = false;
    for (int t = lane; t < K * K; t += 64) bad |= !isfinite(Ms[t]);
    big_ldl_factor(Ms, lc, K, lane);
    if (lane < K) bad |= !isfinite(Ms[lane * K + lane]);
    if (lane == 0) big_ldl_solve(Ms, rw, K, 1);
    if (bad) flg[0] = 1;
  }
  __syncthreads();
  if (flg[0] != 0) return false;
  // (5) y -= V w;  lambda = w[nz:K]
  for (int i = threadIdx.x; i < dp; i += NTHREADS) {
    double s = YV[i];
    for (int c = 0; c < K; ++c) s -= vat(i, c) * rw[c];
    YV[i] = s;
  }
  if (ae.lam)
    for (int i = threadIdx.x; i < nc; i += NTHREADS) ae.lam[(size_t)b * nc + i] = rw[nz + i];
  __syncthreads();
  return true;
}

// ------------------------------------------------------------ the kernel
// As k_gn (FCL / FSL): every phase recomputes the layouts from opaque copies of the dimensions
// instead of keeping their ~60 offsets live in scalar registers across the factorization.
#define GFC fg_const_layout(opaque_s(a.P), opaque_s(a.M), n, opaque_s(a.NT), opaque_s(a.nc))
#define GFS fg_smem_layout(opaque_s(a.P), opaque_s(ECm), n, opaque_s(a.NT), opaque_s(a.nz), opaque_s(a.nc))
template <class DYN, class MEAS, int SLOTS, int MINW>
__global__ __launch_bounds__(NTHREADS, MINW) void k_gn_general(GnArgs a) {
  constexpr int n = DYN::n, NZX = MHE_MAX_EXTRA;
  static_assert(MEAS::MIXED && n <= 16, "k_gn_general: mixed rows, n <= 16");
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int nz = a.nz, K = a.nz + a.nc;
  const FgConst FC = fg_const_layout(a.P, a.M, n, a.NT, a.nc);
  const int EC = fg_epoch_cap(a.P, a.M > 0 ? a.M : 1, n, a.NT, a.nz, a.nc);
  const int ECm = a.M < EC ? a.M : EC;
  const FgSmem FS = fg_smem_layout(a.P, ECm, n, a.NT, a.nz, a.nc);
  const SmemLayout& SL = FS.S;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.x;
  const int stab = make_slot_table(wave, lane, a.NT);
  init_rowmask<SLOTS>((int*)(sm + SL.ROWM), wave, lane, stab);
  double* Xs = sm + SL.Xs;
  double* Zs = sm + FS.ZS;
  if (threadIdx.x == 0) *(int*)(sm + SL.RED + 4 * NW) = 0;  // NOT_SPD flag
  init_units(sm + SL.UN);
  double* DV = sm + SL.YV;  // delta after backward()
  double* RED = sm + SL.RED;
  d4 acc[SLOTS];
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) acc[s] = d4{0.0, 0.0, 0.0, 0.0};
  // constants built for other dims (or never stamped: more epochs than the LDS layout holds,
  // which mhe_build_constants refuses): compute nothing
  int E = 0;
  bool okc = tag_ok(a);
  if (okc && a.M > 0) {
    E = __builtin_amdgcn_readfirstlane(*(const int*)(a.cbuf + FC.ne));
    okc = E >= 0 && E <= EC && E <= a.M;
  }
  if (!okc) {
    bad_constants(a, b, MODE_SOLVE);
    for (int t = threadIdx.x; t < nz; t += NTHREADS) a.Zout[(size_t)b * nz + t] = a.Z0[(size_t)b * nz + t];
    return;
  }
  GnArgs ae = a;
  ae.M = E;
  const int Mf = a.M;

  for (int t = threadIdx.x; t < a.d; t += NTHREADS) Xs[t] = a.X0[(size_t)b * a.d + t];
  for (int t = threadIdx.x; t < E * a.P; t += NTHREADS) sm[FS.PHE + t] = ((const double*)(a.cbuf + FC.C.Phi))[t];
  if (threadIdx.x < NZX) Zs[threadIdx.x] = threadIdx.x < nz ? a.Z0[(size_t)b * nz + threadIdx.x] : 0.0;
  __syncthreads();

  int status = MHE_STATUS_MAX_ITER;
  int it = 0;
  DIAG_DECL
  for (;;) {
    const double c1 = fg_resid<DYN, MEAS>(ae, GFC, GFS, sm, opaque_s(b), opaque_s(E), Mf);
    {
      // this wave's part of the cost, parked in LDS: read back if the loop exits at this iterate
      const double cwv = wave_sum(c1);
      if (lane == 0) RED[2 * NW + wave] = cwv;
    }
    if (it >= a.max_iter) break;
    build_tiles<DYN, MEAS, SLOTS, false, false, true>(ae, GFC.C, GFS.S, sm, acc, wave, lane, stab, sm + GFS.PHE);
    __syncthreads();
    if (!factor_forward<SLOTS>(ae, GFS.S, sm, acc, wave, lane, stab, DIAG_FARGS)) {
      status = MHE_STATUS_NOT_SPD;
      break;
    }
    // y_{NT-1} (backward() forms it itself otherwise): y is complete before the border reads it
    if (wave == (a.NT - 1) % NW) {
      const SmemLayout S2 = GFS.S;
      block_fwd(sm + S2.DT + (a.NT - 1) * DTS, sm + S2.BV + 16 * (a.NT - 1), sm + S2.YV + 16 * (a.NT - 1), lane);
    }
    __syncthreads();
    if (K > 0 && !fg_border<n, SLOTS>(ae, GFC, GFS, sm, acc, wave, lane, stab, opaque_s(b), opaque_s(E))) {
      status = MHE_STATUS_NOT_SPD;
      break;
    }
    backward<SLOTS, true>(ae, GFS.S, sm, acc, wave, lane, stab);
    // (X, z) += (dx, dz); a non-finite step is flagged (NONFINITE, the iterate untouched)
    const double* dz = sm + GFS.RW;
    double dmax = 0.0, xmax = 0.0;
    const int tid_u = opaque_tid();
    for (int t = tid_u; t < a.d; t += NTHREADS) {
      const double dv = DV[t];
      dmax = isfinite(dv) ? fmax(dmax, fabs(dv)) : INFINITY;
      xmax = fmax(xmax, fabs(Xs[t] + dv));
    }
    if (tid_u < nz) {
      const double dv = dz[tid_u];
      dmax = isfinite(dv) ? fmax(dmax, fabs(dv)) : INFINITY;
      xmax = fmax(xmax, fabs(Zs[tid_u] + dv));
    }
    block_reduce2(RED, dmax, xmax, true);
    if (dmax == INFINITY) {
      status = MHE_STATUS_NONFINITE;
      break;
    }
    for (int t = tid_u; t < a.d; t += NTHREADS) Xs[t] = Xs[t] + DV[t];
    if (tid_u < nz) Zs[tid_u] = Zs[tid_u] + dz[tid_u];
    __syncthreads();
    ++it;
    if (dmax <= a.tol * (1.0 + xmax)) {
      status = MHE_STATUS_CONVERGED;
      double cf = fg_resid<DYN, MEAS>(ae, GFC, GFS, sm, opaque_s(b), opaque_s(E), Mf), z = 0.0;
      block_reduce2(RED, cf, z, false);
      if (threadIdx.x == 0) a.cost[b] = cf;
      goto done;
    }
  }
  {
    // every other exit leaves (Xs, z) at the iterate of the loop's last residual pass
    __syncthreads();
    if (threadIdx.x == 0) {
      double cf = RED[2 * NW];
      for (int w = 1; w < NW; ++w) cf += RED[2 * NW + w];
      a.cost[b] = cf;
    }
  }
done:
  __syncthreads();
  for (int t = threadIdx.x; t < a.d; t += NTHREADS) a.Xout[(size_t)b * a.d + t] = Xs[t];
  for (int t = threadIdx.x; t < nz; t += NTHREADS) a.Zout[(size_t)b * nz + t] = Zs[t];
  if (threadIdx.x == 0) {
    a.iters[b] = it;
    a.status[b] = status;
  }
}
#undef GFC
#undef GFS
