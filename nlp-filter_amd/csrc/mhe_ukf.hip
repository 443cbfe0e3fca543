// libmhe: batched unscented Kalman filter for MI355X (gfx950).
//
// The additive-noise UKF with the scaled unscented transform (include/mhe.h states the
// recursion) over the plug-ins of the batched EKF, by their values only (DYN::f, MEAS::h of
// mhe_ekf_models.h): no Jacobian enters.  ONE WAVEFRONT PER FILTER runs all `steps` updates of
// its instance, four instances per workgroup, per-wave LDS scratch, wave barriers and
// wavefront fences between phases, no workgroup barrier -- the layout of k_ekf.
//   * Cholesky of S / S- (n <= 9): row per lane in registers, right-looking, pivots and L_jc
//     broadcast by v_readlane; true sqrt and division.
//   * sigma points: one per lane (2n+1 <= 19 lanes) for the propagation; the nz x (2n+1)
//     measurement evaluations are strided over the 64 lanes.
//   * S-, Pzz (upper triangles, then mirrored / read as (min, max)) and Pxz: one entry per
//     lane-iteration, each summed over j = 0 .. 2n in that order.
//   * the correction is k_ekf's augmented right-looking sweep, here over [Pzz | Pxz^T | e]:
//     Y = L^-1 Pxz^T, w = L^-1 e, mu = mu- + Y^T w, S = S- - Y^T Y.
//   * k_ukf<.., GATE = true> screens the rows on e_i^2 / Pzz_ii before the sweep (mhe_ukf_run_gated).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "mhe.h"
#include "mhe_ekf_models.h"

namespace mhe_ukf {

using mhe_ekf::readlane_d;

constexpr int NWF = 4;     // filters (waves) per workgroup
constexpr int MAXP = 32;   // measurement rows per step (nz <= pmax <= MAXP; mhe_ukf_run checks pmax)
constexpr int TRI = MAXP * (MAXP + 1) / 2;
constexpr double LOG_2PI = 1.8378770664093454836;

struct UkfArgs {
  int batch, steps, nmeas_rows_max;
  double dt;
  double dp[8];  // static dynamics parameters (mhe_ekf_dims.dyn_par)
  double c, wm0, wc0, wi;  // sqrt(n + lambda) and the weights of point 0 (mean, covariance) and of the others
  double* mu;
  double* S;
  const double* U;
  long long u_bstride;
  const double* Z;
  long long z_bstride;
  const int* nz;
  long long nz_bstride;
  const double* PAR;
  long long par_bstride;
  const double* Q;
  const double* R;
  long long r_bstride, r_sstride;
  double* mu_hist;
  double* S_hist;
  int hist_bi;   // 1: histories batch-innermost, as k_ekf's
  long long es;  // element stride of U / Z / nz / PAR, as k_ekf's
  int* status;
  double* nis;   // per-step statistics, optional: (steps, B) with hist_bi, else (B, steps)
  double* loglik;
};

// the gated instances (k_ukf<.., true>) take these as well; the others keep the kernel
// arguments they had
struct UkfGateArgs : UkfArgs {
  double gate;  // screen threshold on d2_i = e_i^2 / Pzz_ii; +inf: no screening
  int* rej;     // optional, laid out as nis: bit i = row i was screened out
};
template <bool GATE>
struct KArgs { using type = UkfArgs; };
template <>
struct KArgs<true> { using type = UkfGateArgs; };

// bits 0..rows-1 (rows <= 32)
__device__ __forceinline__ unsigned row_bits(int rows) { return rows >= 32 ? 0xffffffffu : (1u << rows) - 1u; }

// element (b, k, e) of a per-step history with `w` entries per step
__device__ __forceinline__ size_t hist_at(const UkfArgs& a, int b, int k, int e, int w) {
  return a.hist_bi ? ((size_t)k * w + e) * a.batch + b : ((size_t)b * a.steps + k) * w + e;
}

// entry t (r <= c) of the upper triangle of an N x N matrix, t < N (N + 1) / 2: row a
// (N - a entries) and the row that completes it to N | 1 entries share one line of a folded
// rectangle, so consecutive t are consecutive entries and no lane draws a skipped one
__device__ __forceinline__ void tri_rc(int t, int N, int& r, int& c) {
  const int w = N | 1;
  const int a = t / w, b = t - a * w;
  if (b < N - a) {
    r = a;
    c = a + b;
  } else {
    r = N - a - ((N & 1) ^ 1);
    c = r + (b - (N - a));
  }
}

// packed upper triangle of a MAXP x MAXP matrix (row stride fixed, whatever nz is)
__device__ __forceinline__ int tri_at(int r, int c) { return r * MAXP - r * (r - 1) / 2 + (c - r); }

// per-wave LDS scratch (doubles).  A holds S, then its factor L, then L of S-; XS the
// propagated points Y_j, then the points redrawn from (mu-, S-); ZS the measurement values
// Zs_j and then Dz_j, point-major with MAXP rows each; PZ the packed upper triangle of Pzz;
// T1 row i of Pxz^T and then of Y; E the vector w.
template <int n>
struct WaveSmem {
  static constexpr int NS = 2 * n + 1;
  static constexpr int MU = 0, MP = MU + n, A = MP + n, SP = A + n * n, XS = SP + n * n, ZS = XS + NS * n,
                       PZ = ZS + NS * MAXP, T1 = PZ + TRI, E = T1 + MAXP * n, total = E + MAXP;
};

#define UKF_PHASE()                  \
  __builtin_amdgcn_wave_barrier();   \
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront")

// M (n x n in LDS, row major) = L L^T in place: lane i < n holds row i in registers; column c's
// pivot and every L_jc come by readlane.  The strict upper triangle of L is written as zeros.
// Returns (wave-uniform) whether every pivot was positive and finite.
template <int n>
__device__ __forceinline__ bool chol_inplace(double* M, int lane) {
  double s[n];
#pragma unroll
  for (int c = 0; c < n; ++c) s[c] = lane < n ? M[lane * n + c] : 0.0;
  bool ok = true;
#pragma unroll
  for (int c = 0; c < n; ++c) {
    const double piv = readlane_d(s[c], c);
    ok &= (piv > 0.0 && piv < INFINITY);
    const double d = sqrt(piv);
    const double l = lane == c ? d : s[c] / d;  // L_ic
#pragma unroll
    for (int j = c + 1; j < n; ++j) s[j] -= l * readlane_d(l, j);
    s[c] = lane >= c ? l : 0.0;
  }
  if (lane < n) {
#pragma unroll
    for (int c = 0; c < n; ++c) M[lane * n + c] = s[c];
  }
  return ok;
}

// sigma point j of (mean, L): X_0 = mean, X_j = mean + c L[:, j-1], X_{n+j} = mean - c L[:, j-1]
template <int n>
__device__ __forceinline__ void sigma_point(const double* mean, const double* L, double c, int j, double* x) {
  const int col = j == 0 ? 0 : (j <= n ? j - 1 : j - n - 1);
  const double sc = j == 0 ? 0.0 : (j <= n ? c : -c);
#pragma unroll
  for (int r = 0; r < n; ++r) x[r] = j == 0 ? mean[r] : mean[r] + sc * L[r * n + col];
}

// GATE: innovation screening (include/mhe.h states it).  Lane i holds e_i and reads Pzz_ii
// from PZ once the phase that writes PZ is over; row i is screened out iff
// e_i^2 / Pzz_ii > a.gate (a NaN or non-positive Pzz_ii keeps the row, and the pivot test then
// reports it).  The kept rows are a wave-uniform ballot mask.  A screened lane holds a zero row
// of [Pzz | Pxz^T | e] and is never a pivot, so the kept lanes run the sweep of the kept
// sub-blocks in their order and the screened rows of Y and w are exact zeros in the two closing
// sums: the step is the ungated one fed the kept rows only.  No kept row: predict-only.
// GATE = false is the code as it was: those instances serve every call without gate and rej.
template <class DYN, class MEAS, bool GATE = false>
__global__ __launch_bounds__(NWF * 64) void k_ukf(typename KArgs<GATE>::type a) {
  constexpr int n = DYN::n, m = DYN::m, q = MEAS::q;
  using WS = WaveSmem<n>;
  constexpr int NS = WS::NS;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int b = blockIdx.x * NWF + wave;
  if (b >= a.batch) return;  // whole wave exits; no workgroup barrier is used below
  double* sw = smem + wave * WS::total;
  double* mu = sw + WS::MU;
  double* MP = sw + WS::MP;
  double* A = sw + WS::A;
  double* SP = sw + WS::SP;
  double* XS = sw + WS::XS;
  double* ZS = sw + WS::ZS;
  double* PZ = sw + WS::PZ;
  double* T1 = sw + WS::T1;
  double* E = sw + WS::E;
  for (int t = lane; t < n; t += 64) mu[t] = a.mu[(size_t)b * n + t];
  for (int t = lane; t < n * n; t += 64) A[t] = a.S[(size_t)b * n * n + t];
  int status = 0;
  bool dead = false;  // a pivot failed: this filter's outputs are NaN from that step on
  UKF_PHASE();
  for (int k = 0; k < a.steps; ++k) {
    // ---- predict: sigma points of (mu, S), one per lane, through the dynamics
    dead |= !chol_inplace<n>(A, lane);
    UKF_PHASE();
    if (lane < NS) {
      double x[n], u[m > 0 ? m : 1], xp[n];
      sigma_point<n>(mu, A, a.c, lane, x);
      for (int c = 0; c < m; ++c) u[c] = a.U[(long long)b * a.u_bstride + ((long long)k * m + c) * a.es];
      DYN::f(x, u, a.dt, a.dp, xp);
      for (int c = 0; c < n; ++c) XS[lane * n + c] = xp[c];
    }
    UKF_PHASE();
    if (lane < n) {  // mu- = sum wm_j Y_j
      double acc = a.wm0 * XS[lane];
      for (int j = 1; j < NS; ++j) acc += a.wi * XS[j * n + lane];
      MP[lane] = acc;
    }
    UKF_PHASE();
    for (int t = lane; t < n * (n + 1) / 2; t += 64) {  // S- = sum wc_j (Y_j - mu-)(Y_j - mu-)^T + Q
      int r, c;
      tri_rc(t, n, r, c);
      const double mr = MP[r], mc = MP[c];
      double acc = a.wc0 * ((XS[r] - mr) * (XS[c] - mc));
      for (int j = 1; j < NS; ++j) acc += a.wi * ((XS[j * n + r] - mr) * (XS[j * n + c] - mc));
      acc += a.Q[r * n + c];
      SP[r * n + c] = acc;
      SP[c * n + r] = acc;
    }
    UKF_PHASE();
    const int nz = a.nz[(long long)b * a.nz_bstride + (long long)k * a.es];
    double nis = 0.0, loglik = 0.0;
    unsigned rejm = 0;  // GATE: the step's screened rows
    // Z / PAR / R hold pmax (<= MAXP) rows per step: a step that claims more is refused
    if (nz > 0 && nz <= a.nmeas_rows_max) {
      // ---- sigma points redrawn from (mu-, S-)
      for (int t = lane; t < n * n; t += 64) A[t] = SP[t];
      UKF_PHASE();
      dead |= !chol_inplace<n>(A, lane);
      UKF_PHASE();
      if (lane < NS) {
        double x[n];
        sigma_point<n>(MP, A, a.c, lane, x);
        for (int c = 0; c < n; ++c) XS[lane * n + c] = x[c];
      }
      UKF_PHASE();
      // ---- Zs_j = h(X_j) - z: centred on the measurement, nz x (2n+1) evaluations
      const long long rk0 = (long long)k * a.nmeas_rows_max;  // first row of the step within the instance
      for (int t = lane; t < nz * NS; t += 64) {
        const int j = t / nz, i = t - j * nz;
        double x[n], par[q > 0 ? q : 1];
        for (int c = 0; c < n; ++c) x[c] = XS[j * n + c];
        for (int c = 0; c < q; ++c) par[c] = a.PAR[(long long)b * a.par_bstride + ((rk0 + i) * q + c) * a.es];
        ZS[j * MAXP + i] = MEAS::template h<n>(x, par, i, nz) - a.Z[(long long)b * a.z_bstride + (rk0 + i) * a.es];
      }
      UKF_PHASE();
      double e = 0.0;
      if (lane < nz) {  // e = -sum wm_j Zs_j; Dz_j = Zs_j + e in place
        double acc = a.wm0 * ZS[lane];
        for (int j = 1; j < NS; ++j) acc += a.wi * ZS[j * MAXP + lane];
        e = -acc;
        for (int j = 0; j < NS; ++j) ZS[j * MAXP + lane] += e;
      }
      UKF_PHASE();
      const double* Rk = a.R + (long long)b * a.r_bstride + (long long)k * a.r_sstride;
      for (int t = lane; t < nz * (nz + 1) / 2; t += 64) {  // Pzz = sum wc_j Dz_j Dz_j^T + R, upper triangle
        int r, c;
        tri_rc(t, nz, r, c);
        double acc = a.wc0 * (ZS[r] * ZS[c]);
        for (int j = 1; j < NS; ++j) acc += a.wi * (ZS[j * MAXP + r] * ZS[j * MAXP + c]);
        PZ[tri_at(r, c)] = acc + Rk[r * a.nmeas_rows_max + c];
      }
      for (int t = lane; t < nz * n; t += 64) {  // Pxz^T = sum wc_j Dz_j (X_j - mu-)^T, row i per measurement
        const int i = t / n, c = t % n;
        const double mc = MP[c];
        double acc = a.wc0 * ((XS[c] - mc) * ZS[i]);
        for (int j = 1; j < NS; ++j) acc += a.wi * ((XS[j * n + c] - mc) * ZS[j * MAXP + i]);
        T1[t] = acc;
      }
      UKF_PHASE();
      // ---- augmented sweep: lane i holds row i of [Pzz | Pxz^T | e]
      const int i = lane;
      bool row = i < nz;
      unsigned km = 0xffffffffu;  // GATE: the kept rows (wave-uniform)
      if constexpr (GATE) {
        const double pd = row ? PZ[tri_at(i, i)] : 0.0;  // nz <= MAXP: a row's lane is below MAXP
        const bool keep = row && !(pd > 0.0 && e * e / pd > a.gate);
        km = (unsigned)__ballot(keep);
        rejm = ~km & row_bits(nz);
        if (!keep) e = 0.0;
        row = keep;  // a screened lane holds no row of the sweep
      }
      double p[MAXP], t1[n];
#pragma unroll
      for (int j = 0; j < MAXP; ++j) {
        const int ii = i < MAXP ? i : 0;
        p[j] = (row && j < nz) ? PZ[j < ii ? tri_at(j, ii) : tri_at(ii, j)] : 0.0;
      }
#pragma unroll
      for (int c = 0; c < n; ++c) t1[c] = row ? T1[i * n + c] : 0.0;
      double idg = 0.0;
      bool bad = false;
#pragma unroll
      for (int c = 0; c < MAXP; ++c) {
        if (c < nz && (!GATE || ((km >> c) & 1u))) {
          const double piv = readlane_d(p[c], c);
          bad |= !(piv > 0.0 && piv < INFINITY);
          const double rs = 1.0 / sqrt(piv);
          const double qv = p[c] * rs;                      // L_ic (i > c)
          const double mm = (i > c && row) ? qv * rs : 0.0;  // A'_ic / A'_cc
          idg = (i == c) ? rs : idg;
#pragma unroll
          for (int j = c + 1; j < MAXP; ++j)
            if (j < nz) p[j] -= qv * readlane_d(qv, j);
#pragma unroll
          for (int cc = 0; cc < n; ++cc) t1[cc] -= mm * readlane_d(t1[cc], c);
          e -= mm * readlane_d(e, c);
        }
      }
      dead |= bad;
      if (row) {
#pragma unroll
        for (int c = 0; c < n; ++c) T1[i * n + c] = t1[c] * idg;  // Y = L^-1 Pxz^T
        E[i] = e * idg;                                          // w = L^-1 e
      } else if (GATE && i < nz) {  // a screened row of Y and w: exact zeros for the sums below
#pragma unroll
        for (int c = 0; c < n; ++c) T1[i * n + c] = 0.0;
        E[i] = 0.0;
      }
      if (a.nis || a.loglik) {  // wave-uniform
        // nis = w^T w, sum log L_ii = -sum log(1 / L_ii): the rows sit in lanes 0..31
        double s2 = row ? (e * idg) * (e * idg) : 0.0;
        double lg = row ? log(idg) : 0.0;
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) {
          s2 += __shfl_xor(s2, off);
          lg += __shfl_xor(lg, off);
        }
        nis = s2;
        if constexpr (GATE) {
          const int cnt = __popc(km);  // rows applied; none: s2 = 0 and loglik = 0
          loglik = cnt ? -0.5 * (s2 - 2.0 * lg + cnt * LOG_2PI) : 0.0;
        } else {
          loglik = -0.5 * (s2 - 2.0 * lg + nz * LOG_2PI);
        }
      }
      UKF_PHASE();
      // mu = mu- + Y^T w ; S = S- - Y^T Y (upper triangle, mirrored)
      for (int t = lane; t < n * (n + 1) / 2; t += 64) {
        int r, c;
        tri_rc(t, n, r, c);
        double acc = 0.0;
        for (int ii = 0; ii < nz; ++ii) acc += T1[ii * n + r] * T1[ii * n + c];
        const double v = SP[r * n + c] - acc;
        A[r * n + c] = v;
        A[c * n + r] = v;
      }
      for (int t = lane; t < n; t += 64) {
        double acc = 0.0;
        for (int ii = 0; ii < nz; ++ii) acc += T1[ii * n + t] * E[ii];
        mu[t] = GATE && km == 0 ? MP[t] : MP[t] + acc;  // every row screened out: mu- itself
      }
    } else {
      if (nz > a.nmeas_rows_max) status = 2;
      for (int t = lane; t < n * n; t += 64) A[t] = SP[t];
      for (int t = lane; t < n; t += 64) mu[t] = MP[t];
    }
    if (dead) {
      nis = loglik = NAN;
      for (int t = lane; t < n * n; t += 64) A[t] = NAN;
      for (int t = lane; t < n; t += 64) mu[t] = NAN;
    }
    UKF_PHASE();
    if (lane == 0) {
      const size_t at = hist_at(a, b, k, 0, 1);
      if (a.nis) a.nis[at] = nis;
      if (a.loglik) a.loglik[at] = loglik;
      if constexpr (GATE) {
        if (a.rej) a.rej[at] = (int)rejm;
      }
    }
    if (a.mu_hist)
      for (int t = lane; t < n; t += 64) a.mu_hist[hist_at(a, b, k, t, n)] = mu[t];
    if (a.S_hist)
      for (int t = lane; t < n * n; t += 64) a.S_hist[hist_at(a, b, k, t, n * n)] = A[t];
  }
  for (int t = lane; t < n; t += 64) a.mu[(size_t)b * n + t] = mu[t];
  for (int t = lane; t < n * n; t += 64) a.S[(size_t)b * n * n + t] = A[t];
  if (a.status && lane == 0) a.status[b] = dead ? 1 : status;
}

#undef UKF_PHASE

template <class DYN, class MEAS>
int launch(const UkfGateArgs& g, hipStream_t st, bool gated) {
  const int smem = NWF * WaveSmem<DYN::n>::total * (int)sizeof(double);
  const dim3 grid((g.batch + NWF - 1) / NWF), block(NWF * 64);
  if (gated) {
    hipLaunchKernelGGL((k_ukf<DYN, MEAS, true>), grid, block, smem, st, g);
  } else {
    const UkfArgs& a = g;
    hipLaunchKernelGGL((k_ukf<DYN, MEAS, false>), grid, block, smem, st, a);
  }
  return hipGetLastError() == hipSuccess ? MHE_OK : MHE_ERR_HIP;
}

// ---------------------------------------------------------------- unscented RTS smoother
// Backward pass over the history k_ukf wrote (include/mhe.h states the recursion), in k_ukf's
// launch shape: one wavefront per filter, NWF per workgroup, per-wave LDS scratch, wave
// barriers and wavefront fences between phases, no workgroup barrier.  Carrying the smoothed
// (mu_s, S_s) of step k+1, step k redoes the forward's prediction from (mu_k, S_k) with
// u_{k+1} -- k_ukf's expressions term by term, so that on a predict-only history (mu-, S-) are
// the history's own entry k+1 bitwise -- and adds the cross covariance C of the same points.
//   * M = S-^-1 C^T: column r of C^T (row r of C) per lane in registers, L- read from LDS
//     (every lane the same address); forward then backward substitution, sums over t
//     increasing, times 1 / L-_ii (one true division per pivot, in lane i, broadcast by
//     v_readlane).  The rows are stored back as G = M^T.
//   * S_s = S_k + G (S_s' - S-) G^T as E = D G^T (n^2 entries over the lanes) and then the
//     upper triangle of S_k + G E, one entry per lane, mirrored: bitwise symmetric.
//   * step k-1's mu, S (upper triangle) and u are loaded into registers before step k's
//     arithmetic and reach LDS at the top of the next iteration: a wave has read step k of the
//     input before it writes step k of the output, so the outputs may alias the inputs.
// The prior, when a smoothed prior is asked for, is one more iteration at k = -1 with u_0.
struct UrtsArgs {
  int batch, steps;
  double dt;
  double dp[8];
  double c, wm0, wc0, wi;  // as UkfArgs
  const double* mu_hist;
  const double* S_hist;
  const double* U;
  long long u_bstride, es;  // as UkfArgs
  const double* Q;
  const double* mu0;  // (B, n) / (B, n, n), batch outermost; read only when a smoothed prior is asked for
  const double* S0;
  double* mu_s;
  double* S_s;
  double* mu0_s;
  double* S0_s;
  int hist_bi;
  int* status;
};

// element e of step k's w-entry record of filter b; k = -1 is the prior's (B, w) array
__device__ __forceinline__ size_t urts_at(const UrtsArgs& a, int b, int k, int e, int w) {
  if (k < 0) return (size_t)b * w + e;
  return a.hist_bi ? ((size_t)k * w + e) * a.batch + b : ((size_t)b * a.steps + k) * w + e;
}

// per-wave LDS scratch (doubles): MU mu_k, MP mu-, XM the carried mu_s, DV mu_s' - mu-;
// A S_k and then its factor L, then E; SK S_k; SP S- and then its factor; CS the carried S_s,
// then D = S_s' - S-, then the new S_s; C the cross covariance and then G; XS the points Y_j
template <int n>
struct RtsSmem {
  static constexpr int NS = 2 * n + 1;
  static constexpr int MU = 0, MP = MU + n, XM = MP + n, DV = XM + n, A = DV + n, SK = A + n * n, SP = SK + n * n,
                       CS = SP + n * n, C = CS + n * n, XS = C + n * n, total = XS + NS * n;
};

#define URTS_PHASE()                 \
  __builtin_amdgcn_wave_barrier();   \
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront")

// waves per SIMD: the n = 9 instance fits 168 VGPRs without a spill, which is three waves
template <class DYN>
__global__ __launch_bounds__(NWF * 64) __attribute__((amdgpu_waves_per_eu(3))) void k_ukf_rts(UrtsArgs a) {
  constexpr int n = DYN::n, m = DYN::m;
  using WS = RtsSmem<n>;
  constexpr int NS = WS::NS, NT = n * (n + 1) / 2;
  static_assert(NT <= 64 && NS <= 64, "one triangle entry and one sigma point per lane");
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int b = blockIdx.x * NWF + wave;
  if (b >= a.batch) return;  // whole wave exits; no workgroup barrier is used below
  double* sw = smem + wave * WS::total;
  double* MU = sw + WS::MU;
  double* MP = sw + WS::MP;
  double* XM = sw + WS::XM;
  double* DV = sw + WS::DV;
  double* A = sw + WS::A;
  double* SK = sw + WS::SK;
  double* SP = sw + WS::SP;
  double* CS = sw + WS::CS;
  double* C = sw + WS::C;
  double* XS = sw + WS::XS;
  const int kmin = (a.mu0_s || a.S0_s) ? -1 : 0;
  int tr = 0, tc = 0;  // this lane's entry of an upper triangle
  if (lane < NT) tri_rc(lane, n, tr, tc);
  bool bad = false;
  // what a lane holds of a step's input: mu[lane], S[tr, tc] and the controls of the step after it
  double pm = 0.0, ps = 0.0, pu[m > 0 ? m : 1] = {};
  auto load = [&](int k) {
    const double* hm = k < 0 ? a.mu0 : a.mu_hist;
    const double* hs = k < 0 ? a.S0 : a.S_hist;
    if (lane < n) pm = hm[urts_at(a, b, k, lane, n)];
    if (lane < NT) ps = hs[urts_at(a, b, k, tr * n + tc, n * n)];
    for (int c = 0; c < m; ++c) pu[c] = a.U[(long long)b * a.u_bstride + ((long long)(k + 1) * m + c) * a.es];
  };
  auto store = [&](int k) {  // the carry (XM, CS) is smoothed step k
    double* om = k < 0 ? a.mu0_s : a.mu_s;
    double* os = k < 0 ? a.S0_s : a.S_s;
    if (om)
      for (int t = lane; t < n; t += 64) om[urts_at(a, b, k, t, n)] = XM[t];
    if (os)
      for (int t = lane; t < n * n; t += 64) os[urts_at(a, b, k, t, n * n)] = CS[t];
  };
  {  // k = T-1: the smoothed values are the filtered ones
    const int k = a.steps - 1;
    if (lane < n) pm = a.mu_hist[urts_at(a, b, k, lane, n)];
    if (lane < NT) ps = a.S_hist[urts_at(a, b, k, tr * n + tc, n * n)];
    double vm = pm, vs = ps;
    bad = __any(!(fabs(vm) < INFINITY) || !(fabs(vs) < INFINITY));
    if (bad) vm = vs = NAN;
    if (lane < n) XM[lane] = vm;
    if (lane < NT) {
      CS[tr * n + tc] = vs;
      CS[tc * n + tr] = vs;
    }
    if (k - 1 >= kmin) load(k - 1);  // else no step follows (and U has no u_{k+1})
    URTS_PHASE();
    store(k);
  }
  for (int k = a.steps - 2; k >= kmin; --k) {
    if (lane < n) MU[lane] = pm;
    if (lane < NT) {
      A[tr * n + tc] = ps;
      A[tc * n + tr] = ps;
      SK[tr * n + tc] = ps;
      SK[tc * n + tr] = ps;
    }
    double u[m > 0 ? m : 1];
    for (int c = 0; c < m; ++c) u[c] = pu[c];
    if (k - 1 >= kmin) load(k - 1);  // arrives under this step's arithmetic
    URTS_PHASE();
    // ---- the forward's prediction: sigma points of (mu_k, S_k), one per lane, through the dynamics
    bool ok = chol_inplace<n>(A, lane);
    URTS_PHASE();
    if (lane < NS) {
      double x[n], xp[n];
      sigma_point<n>(MU, A, a.c, lane, x);
      DYN::f(x, u, a.dt, a.dp, xp);
      for (int c = 0; c < n; ++c) XS[lane * n + c] = xp[c];
    }
    URTS_PHASE();
    if (lane < n) {  // mu- = sum wm_j Y_j
      double acc = a.wm0 * XS[lane];
      for (int j = 1; j < NS; ++j) acc += a.wi * XS[j * n + lane];
      MP[lane] = acc;
    }
    URTS_PHASE();
    for (int t = lane; t < n * (n + 1) / 2; t += 64) {  // S- = sum wc_j (Y_j - mu-)(Y_j - mu-)^T + Q
      int r, c;
      tri_rc(t, n, r, c);
      const double mr = MP[r], mc = MP[c];
      double acc = a.wc0 * ((XS[r] - mr) * (XS[c] - mc));
      for (int j = 1; j < NS; ++j) acc += a.wi * ((XS[j * n + r] - mr) * (XS[j * n + c] - mc));
      acc += a.Q[r * n + c];
      SP[r * n + c] = acc;
      SP[c * n + r] = acc;
      const double dv = CS[r * n + c] - acc;  // D = S_s' - S-, over the carry (bitwise symmetric as both are)
      CS[r * n + c] = dv;
      CS[c * n + r] = dv;
    }
    for (int t = lane; t < n * n; t += 64) {  // C = sum wc_j (X_j - mu_k)(Y_j - mu-)^T, X_j the points above
      const int r = t / n, c = t - r * n;
      const double xr = MU[r], mc = MP[c];
      double acc = a.wc0 * ((xr - xr) * (XS[c] - mc));
      for (int j = 1; j <= n; ++j) acc += a.wi * (((xr + a.c * A[r * n + j - 1]) - xr) * (XS[j * n + c] - mc));
      for (int j = 1; j <= n; ++j) acc += a.wi * (((xr - a.c * A[r * n + j - 1]) - xr) * (XS[(n + j) * n + c] - mc));
      C[t] = acc;
    }
    if (lane < n) DV[lane] = XM[lane] - MP[lane];
    URTS_PHASE();
    ok &= chol_inplace<n>(SP, lane);
    URTS_PHASE();
    // 1 / L-_ii: one division in lane i, broadcast, so that the substitutions below multiply
    const double rdl = 1.0 / SP[(lane < n ? lane : 0) * (n + 1)];
    double rd[n];
#pragma unroll
    for (int i = 0; i < n; ++i) rd[i] = readlane_d(rdl, i);
    if (lane < n) {  // L- y = C[lane, :]^T, L-^T g = y: row `lane` of G = C S-^-1
      double v[n];
#pragma unroll
      for (int i = 0; i < n; ++i) v[i] = C[lane * n + i];
#pragma unroll
      for (int i = 0; i < n; ++i) {
        double s = v[i];
#pragma unroll
        for (int t = 0; t < i; ++t) s -= SP[i * n + t] * v[t];
        v[i] = s * rd[i];
      }
#pragma unroll
      for (int i = n - 1; i >= 0; --i) {
        double s = v[i];
#pragma unroll
        for (int t = i + 1; t < n; ++t) s -= SP[t * n + i] * v[t];
        v[i] = s * rd[i];
      }
#pragma unroll
      for (int i = 0; i < n; ++i) C[lane * n + i] = v[i];
    }
    URTS_PHASE();
    for (int t = lane; t < n * n; t += 64) {  // E = D G^T
      const int i = t / n, c = t - i * n;
      double acc = 0.0;
      for (int j = 0; j < n; ++j) acc += CS[i * n + j] * C[c * n + j];
      A[t] = acc;
    }
    URTS_PHASE();
    // mu_s = mu_k + G (mu_s' - mu-);  S_s = S_k + G E (upper triangle, mirrored)
    double vm = 0.0, vs = 0.0;
    if (lane < n) {
      double acc = 0.0;
      for (int i = 0; i < n; ++i) acc += C[lane * n + i] * DV[i];
      vm = MU[lane] + acc;
    }
    if (lane < NT) {
      double acc = 0.0;
      for (int i = 0; i < n; ++i) acc += C[tr * n + i] * A[i * n + tc];
      vs = SK[tr * n + tc] + acc;
    }
    // a failed filter is NaN from the failing step down; a non-finite value (one met in the
    // history, or the carry of a failed step) is a failure as well
    bad |= !ok;
    bad |= (bool)__any(!(fabs(vm) < INFINITY) || !(fabs(vs) < INFINITY));
    if (bad) vm = vs = NAN;
    if (lane < n) XM[lane] = vm;
    if (lane < NT) {
      CS[tr * n + tc] = vs;
      CS[tc * n + tr] = vs;
    }
    URTS_PHASE();
    store(k);
  }
  if (a.status && lane == 0) a.status[b] = bad ? 1 : 0;
}

#undef URTS_PHASE

template <class DYN>
int launch_rts(const UrtsArgs& a, hipStream_t st) {
  const int smem = NWF * RtsSmem<DYN::n>::total * (int)sizeof(double);
  hipLaunchKernelGGL((k_ukf_rts<DYN>), dim3((a.batch + NWF - 1) / NWF), dim3(NWF * 64), smem, st, a);
  return hipGetLastError() == hipSuccess ? MHE_OK : MHE_ERR_HIP;
}

}  // namespace mhe_ukf

// mhe_ukf_run and mhe_ukf_run_gated behind their struct checks: `args` holds mhe_ukf_args'
// fields; gate 0 and rej NULL run the instances without the screen
static int ukf_run(const mhe_ekf_dims* dims, const mhe_ukf_args* args, double gate, int32_t* rej, void* stream) {
  using namespace mhe_ukf;
  using namespace mhe_ekf;
  const double al = args->alpha, be = args->beta, ka = args->kappa;
  if (!(al > 0.0 && al < INFINITY) || !(fabs(be) < INFINITY) || !(fabs(ka) < INFINITY)) return MHE_ERR_DIMS;
  const double nn = (double)dims->n;
  if (!(nn + ka > 0.0)) return MHE_ERR_DIMS;
  const double lam = al * al * (nn + ka) - nn;  // n + lambda = alpha^2 (n + kappa) > 0
  if (!(nn + lam > 0.0 && nn + lam < INFINITY)) return MHE_ERR_DIMS;  // alpha^2 (n + kappa) under- or overflowed
  const int32_t batch = args->batch, steps = args->steps;
  if (batch < 0 || steps < 0 || dims->pmax < 1 || dims->pmax > MAXP) return MHE_ERR_DIMS;
  if (batch == 0 || steps == 0) return MHE_OK;
  if (!args->mu || !args->S || !args->Q || !args->nz || !args->Z || !args->R || (dims->m > 0 && !args->U))
    return MHE_ERR_NULL;
  if (dims->q != 3) return MHE_ERR_DIMS;
  if (!args->PAR) return MHE_ERR_NULL;
  int (*run)(const UkfGateArgs&, hipStream_t, bool) = nullptr;
  if (dims->dyn_model == MHE_EKF_DYN_GNSS_POS_AND_BIAS) {
    if (dims->n != 5 || dims->m != 3) return MHE_ERR_MODEL;
    if (dims->meas_model == MHE_EKF_MEAS_MULTI_PSEUDORANGE)
      run = launch<EkfGnssPosAndBias, EkfMultiPseudorange<false>>;
    else if (dims->meas_model == MHE_EKF_MEAS_MULTI_PSEUDORANGE_AND_BIAS)
      run = launch<EkfGnssPosAndBias, EkfMultiPseudorange<true>>;
  } else if (dims->dyn_model == MHE_EKF_DYN_DISCRETE_VEHICLE) {
    if (dims->n != 9 || dims->m != 2) return MHE_ERR_MODEL;
    if (!(dims->dyn_par[2] != 0.0 && dims->dyn_par[5] != 0.0)) return MHE_ERR_DIMS;  // M, I_Z unset
    if (dims->meas_model == MHE_EKF_MEAS_VEHICLE_SENSORS) run = launch<EkfDiscreteVehicle, EkfVehicleSensors>;
  }
  if (!run) return MHE_ERR_MODEL;
  UkfGateArgs a = {};
  a.batch = batch; a.steps = steps; a.nmeas_rows_max = dims->pmax; a.dt = dims->dt;
  for (int i = 0; i < 8; ++i) a.dp[i] = dims->dyn_par[i];
  a.c = sqrt(nn + lam);
  a.wm0 = lam / (nn + lam);
  a.wc0 = a.wm0 + 1.0 - al * al + be;
  a.wi = 1.0 / (2.0 * (nn + lam));
  a.mu = args->mu; a.S = args->S; a.U = args->U; a.u_bstride = args->u_bstride; a.Z = args->Z;
  a.z_bstride = args->z_bstride; a.nz = args->nz; a.nz_bstride = args->nz_bstride; a.PAR = args->PAR;
  a.par_bstride = args->par_bstride; a.Q = args->Q; a.R = args->R; a.r_bstride = args->r_bstride;
  a.r_sstride = args->r_sstride; a.mu_hist = args->mu_hist; a.S_hist = args->S_hist; a.status = args->status;
  a.nis = args->nis; a.loglik = args->loglik;
  a.hist_bi = dims->hist_batch_inner != 0;
  a.es = 1;
  if (dims->in_batch_inner) {  // U (steps, m, B), Z (steps, pmax, B), nz (steps, B), PAR (steps, pmax, q, B)
    a.es = batch;
    a.u_bstride = a.z_bstride = a.nz_bstride = a.par_bstride = 1;
  }
  a.gate = gate != 0.0 ? gate : INFINITY;
  a.rej = rej;
  return run(a, (hipStream_t)stream, gate != 0.0 || rej);
}

extern "C" int mhe_ukf_run(const mhe_ekf_dims* dims, const mhe_ukf_args* args, void* stream) {
  if (!dims || !args) return MHE_ERR_NULL;
  if (dims->struct_size != (int32_t)sizeof(mhe_ekf_dims)) return MHE_ERR_DIMS;  // stale / truncated binding
  if (args->struct_size != (int32_t)sizeof(mhe_ukf_args)) return MHE_ERR_DIMS;
  return ukf_run(dims, args, 0.0, nullptr, stream);
}

extern "C" int mhe_ukf_run_gated(const mhe_ekf_dims* dims, const mhe_ukf_gate_args* args, void* stream) {
  static_assert(offsetof(mhe_ukf_gate_args, gate) == sizeof(mhe_ukf_args), "mhe_ukf_args' fields, then gate and rej");
  if (!dims || !args) return MHE_ERR_NULL;
  if (dims->struct_size != (int32_t)sizeof(mhe_ekf_dims)) return MHE_ERR_DIMS;  // stale / truncated binding
  if (args->struct_size != (int32_t)sizeof(mhe_ukf_gate_args)) return MHE_ERR_DIMS;
  if (!(args->gate >= 0.0)) return MHE_ERR_DIMS;  // NaN or negative; 0 = no screening, +inf allowed
  mhe_ukf_args u;
  memcpy(&u, args, sizeof u);  // the leading fields are mhe_ukf_args' in order
  u.struct_size = (int32_t)sizeof u;
  return ukf_run(dims, &u, args->gate, args->rej, stream);
}

extern "C" int mhe_ukf_smooth(const mhe_ekf_dims* dims, const mhe_ukf_smooth_args* args, void* stream) {
  using namespace mhe_ukf;
  using namespace mhe_ekf;
  if (!dims || !args) return MHE_ERR_NULL;
  if (dims->struct_size != (int32_t)sizeof(mhe_ekf_dims)) return MHE_ERR_DIMS;  // stale / truncated binding
  if (args->struct_size != (int32_t)sizeof(mhe_ukf_smooth_args)) return MHE_ERR_DIMS;
  const double al = args->alpha, be = args->beta, ka = args->kappa;  // mhe_ukf_run's conditions
  if (!(al > 0.0 && al < INFINITY) || !(fabs(be) < INFINITY) || !(fabs(ka) < INFINITY)) return MHE_ERR_DIMS;
  const double nn = (double)dims->n;
  if (!(nn + ka > 0.0)) return MHE_ERR_DIMS;
  const double lam = al * al * (nn + ka) - nn;
  if (!(nn + lam > 0.0 && nn + lam < INFINITY)) return MHE_ERR_DIMS;
  const int32_t batch = args->batch, steps = args->steps;
  if (batch < 0 || steps < 0) return MHE_ERR_DIMS;
  if (batch == 0 || steps == 0) return MHE_OK;
  int (*run)(const UrtsArgs&, hipStream_t) = nullptr;
  if (dims->dyn_model == MHE_EKF_DYN_GNSS_POS_AND_BIAS) {
    if (dims->n != 5 || dims->m != 3) return MHE_ERR_MODEL;
    run = launch_rts<EkfGnssPosAndBias>;
  } else if (dims->dyn_model == MHE_EKF_DYN_DISCRETE_VEHICLE) {
    if (dims->n != 9 || dims->m != 2) return MHE_ERR_MODEL;
    if (!(dims->dyn_par[2] != 0.0 && dims->dyn_par[5] != 0.0)) return MHE_ERR_DIMS;  // M, I_Z unset
    run = launch_rts<EkfDiscreteVehicle>;
  } else {
    return MHE_ERR_MODEL;
  }
  if (!args->mu_hist || !args->S_hist || !args->U || !args->Q || !args->mu_s || !args->S_s) return MHE_ERR_NULL;
  if ((args->mu0_s || args->S0_s) && (!args->mu0 || !args->S0)) return MHE_ERR_NULL;
  UrtsArgs a = {};
  a.batch = batch; a.steps = steps; a.dt = dims->dt;
  for (int i = 0; i < 8; ++i) a.dp[i] = dims->dyn_par[i];
  a.c = sqrt(nn + lam);  // the weights as mhe_ukf_run forms them
  a.wm0 = lam / (nn + lam);
  a.wc0 = a.wm0 + 1.0 - al * al + be;
  a.wi = 1.0 / (2.0 * (nn + lam));
  a.mu_hist = args->mu_hist; a.S_hist = args->S_hist; a.U = args->U; a.u_bstride = args->u_bstride; a.es = 1;
  a.Q = args->Q; a.mu0 = args->mu0; a.S0 = args->S0; a.mu_s = args->mu_s; a.S_s = args->S_s;
  a.mu0_s = args->mu0_s; a.S0_s = args->S0_s; a.status = args->status;
  a.hist_bi = dims->hist_batch_inner != 0;
  if (dims->in_batch_inner) {  // U (steps, m, B)
    a.es = batch;
    a.u_bstride = 1;
  }
  return run(a, (hipStream_t)stream);
}
