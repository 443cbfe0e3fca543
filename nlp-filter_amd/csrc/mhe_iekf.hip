// libmhe: batched iterated extended Kalman filter for MI355X (gfx950).
//
// The iterated EKF is the Gauss-Newton solve of a step's MAP problem
//   min_x  (x - mu-)^T S-^-1 (x - mu-) + (z - h(x))^T R^-1 (z - h(x)):
// the measurement model is relinearised at the current iterate and the correction of
// mhe_ekf.hip's k_ekf is redone from the prediction.  Per step, with x_0 = mu-:
//   pass i:  (h, H) = MEAS::row at x_i
//            e = z - h - H (mu- - x_i)                 (pass 0: the subtrahend is an exact zero)
//            P = H S- H^T + R,  augmented sweep of [P | H S- | e] -> Y = L^-1 H S-, w = L^-1 e
//            x_{i+1} = mu- + Y^T w,   step = max_c |x_{i+1,c} - x_{i,c}|
//            stop when !(step > tol) or i + 1 == max_iter
//   after:   mu = x_{i+1},  S = S- - Y^T Y with the Y of the last pass.
// With max_iter = 1 the step is k_ekf's, term by term (S- below its diagonal is mirrored, so S is
// bitwise symmetric).  Launch shape, per-wave LDS layout (plus
// one n-vector for the iterate) and the wave-only barriers are k_ekf's: ONE WAVEFRONT PER
// FILTER, four filters per workgroup.  One instance per plug-in pair serves every mhe_iekf_run call:
// the gate (+inf: no screening) and the optional statistics are k_ekf<.., true>'s, taken in pass 0.
// A second instance per pair, k_iekf<.., ROBUST = true>, serves mhe_iekf_run_robust: the rows
// reweighted in every pass (pseudo-Huber, see the kernel); the plain instances' code is unchanged.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "mhe.h"
#include "mhe_ekf_models.h"

namespace mhe_iekf {

using mhe_ekf::readlane_d;

constexpr int NWF = 4;     // filters (waves) per workgroup
constexpr int MAXP = 32;   // measurement rows per step (nz <= pmax <= MAXP; mhe_iekf_run checks pmax)
constexpr int MAX_ITER = 64;

struct IekfArgs {
  int batch, steps, nmeas_rows_max;
  double dt;
  double dp[8];  // static dynamics parameters (mhe_ekf_dims.dyn_par)
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
  int hist_bi;   // 1: histories and per-step outputs batch-innermost
  long long es;  // element stride of U / Z / nz / PAR: 1 (batch outermost) or batch (batch innermost)
  int* status;
  double gate;   // +inf: no screening
  double* nis;   // per-step outputs, optional: (steps, B) with hist_bi, else (B, steps)
  double* loglik;
  int* rej;
  double tol;    // >= 0
  int* n_iter;   // passes made per step, optional, laid out as nis
  int max_iter;  // 1..MAX_ITER
};

// mhe_iekf_run_robust's: the plain arguments, then the pseudo-Huber rows' (the plain instances'
// kernel argument is IekfArgs itself, unchanged)
struct IekfRobustArgs : IekfArgs {
  double delta;         // every row's delta when DELTA is NULL; > 0, +inf allowed
  const double* DELTA;  // optional, per row, laid out and strided as Z
  double* weights;      // optional, omega of the last pass per row: pmax entries per step, laid out as the histories
};

template <bool ROBUST>
using KernelArgs = std::conditional_t<ROBUST, IekfRobustArgs, IekfArgs>;

constexpr double LOG_2PI = 1.8378770664093454836;

// bits 0..rows-1 (rows <= 32)
__device__ __forceinline__ unsigned row_bits(int rows) { return rows >= 32 ? 0xffffffffu : (1u << rows) - 1u; }

// element (b, k, e) of a per-step history with `w` entries per step
__device__ __forceinline__ size_t hist_at(const IekfArgs& a, int b, int k, int e, int w) {
  return a.hist_bi ? ((size_t)k * w + e) * a.batch + b : ((size_t)b * a.steps + k) * w + e;
}

// per-wave LDS scratch (doubles): k_ekf's layout, then the iterate X.  E holds the innovations
// until the sweep has them in registers, then the n components of |x_{i+1} - x_i|.
template <int n>
struct WaveSmem {
  static_assert(n <= MAXP, "the step components share E");
  static constexpr int MU = 0, S = MU + n, G = S + n * n, SP = G + n * n, MP = SP + n * n, H = MP + n,
                       T1 = H + MAXP * n, E = T1 + MAXP * n, Y = E + MAXP, W = Y + MAXP * n, X = W + MAXP,
                       total = X + n;
};

// Gate: row i is screened out iff d2_i = e_i^2 / P_ii > a.gate in pass 0, i.e. at the prediction
// (k_ekf<.., true>'s rule: a NaN or a non-positive P_ii keeps the row and status 1 reports it).
// The keep mask stays fixed for the later passes: a screened lane holds a zero row of [H S- | e]
// and its column is no pivot.  No row kept: the step is predict-only and counts 0 passes.
// nis, loglik and rej are pass 0's over the kept rows -- the innovation likelihood at the
// prediction, what the EKF reports.  Status: 1 if any pass met a pivot that is not positive and
// finite, 2 if nz > pmax at some step.
//
// ROBUST (mhe_iekf_run_robust): pseudo-Huber rows by iteratively reweighted Gauss-Newton.  In every
// pass row j's residual r_j = z_j - h_j at the iterate gives t_j = r_j / delta_j,
// s_j = sqrt(1 + t_j^2), g_j = sqrt(s_j), and the sweep runs on R~_jl = R_jl (g_j g_l) in place of
// R: the weight omega_j = 1 / s_j as the covariance inflation D^-1/2 R D^-1/2, D = diag omega.  Lane
// j owns g_j; the P build reads g_l from lane l's register.  delta = +inf gives s = g = 1 exactly
// and R~ = R bitwise, so the run is the plain one's.  The gate tests the UNWEIGHTED diagonal
// (H S- H^T)_jj + R_jj, the plain instances' sum, so the mask is the plain run's at the same
// prediction; nis and loglik are pass 0's w and L of the REWEIGHTED model (R~ at x_0).  A zero
// or NaN delta of a counted row makes a non-finite pivot: status 1.
template <class DYN, class MEAS, bool ROBUST>
__global__ __launch_bounds__(NWF * 64) void k_iekf(KernelArgs<ROBUST> a) {
  constexpr int n = DYN::n, m = DYN::m, q = MEAS::q;
  using WS = WaveSmem<n>;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int b = blockIdx.x * NWF + wave;
  if (b >= a.batch) return;  // whole wave exits; no workgroup barrier is used below
  double* sw = smem + wave * WS::total;
  double* mu = sw + WS::MU;
  double* S = sw + WS::S;
  double* G = sw + WS::G;
  double* SP = sw + WS::SP;
  double* MP = sw + WS::MP;
  double* H = sw + WS::H;
  double* T1 = sw + WS::T1;
  double* E = sw + WS::E;
  double* Y = sw + WS::Y;
  double* W = sw + WS::W;
  double* X = sw + WS::X;
  for (int t = lane; t < n; t += 64) mu[t] = a.mu[(size_t)b * n + t];
  for (int t = lane; t < n * n; t += 64) S[t] = a.S[(size_t)b * n * n + t];
  int status = 0;
  __builtin_amdgcn_wave_barrier();
  for (int k = 0; k < a.steps; ++k) {
    // ---- predict: k_ekf's (utils/ekf.py:40-45)
    if (lane == 0) {
      double x[n], u[m > 0 ? m : 1], xp[n], Gl[n * n];
      for (int c = 0; c < n; ++c) x[c] = mu[c];
      for (int c = 0; c < m; ++c) u[c] = a.U[(long long)b * a.u_bstride + ((long long)k * m + c) * a.es];
      DYN::step(x, u, a.dt, a.dp, xp, Gl);
      for (int c = 0; c < n; ++c) MP[c] = xp[c];
      for (int c = 0; c < n; ++c) X[c] = xp[c];  // x_0 = mu-
      for (int c = 0; c < n * n; ++c) G[c] = Gl[c];
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    // S- = G S G^T + Q: k_ekf's sum for the entries on and above the diagonal; an entry below it
    // is computed as its mirror image, so S- (and with it S) is bitwise symmetric.  Only the
    // upper triangle of Q is read.
    for (int t = lane; t < n * n; t += 64) {
      const int r = min(t / n, t % n), c = max(t / n, t % n);
      double acc = 0.0;
      for (int kk = 0; kk < n; ++kk) {
        double gs = 0.0;
        for (int l = 0; l < n; ++l) gs += S[kk * n + l] * G[c * n + l];  // (S G^T)[kk][c]
        acc += G[r * n + kk] * gs;
      }
      SP[t] = acc + a.Q[r * n + c];
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    const int nz = a.nz[(long long)b * a.nz_bstride + (long long)k * a.es];
    // Z / PAR / R hold pmax (<= MAXP) rows per step: a step that claims more is refused
    const bool valid = nz > 0 && nz <= a.nmeas_rows_max;
    bool corrected = valid;
    int it = 0;                 // passes made
    unsigned km = 0xffffffffu;  // the kept rows (wave-uniform), fixed by pass 0
    double s = 1.0, g = 1.0;    // ROBUST: this lane's row, at the pass's iterate
    if (valid) {
      const long long rk = (long long)k * a.nmeas_rows_max + lane;  // row index within the instance
      const double* Rk = a.R + (long long)b * a.r_bstride + (long long)k * a.r_sstride;
      const int i = lane;
      const bool row = i < nz;
      double par[q > 0 ? q : 1], z = 0.0;  // the row's inputs do not change between the passes
      if (row) {
        for (int c = 0; c < q; ++c) par[c] = a.PAR[(long long)b * a.par_bstride + (rk * q + c) * a.es];
        z = a.Z[(long long)b * a.z_bstride + rk * a.es];
      }
      double dl = INFINITY;
      if constexpr (ROBUST) {
        if (row) dl = a.DELTA ? a.DELTA[(long long)b * a.z_bstride + rk * a.es] : a.delta;
      }
      for (;;) {
        // ---- measurement rows at the iterate; e = z - h - H (mu- - x_i)
        if (row) {
          double x[n], h, Hr[n];
          for (int c = 0; c < n; ++c) x[c] = X[c];
          MEAS::template row<n>(x, par, lane, nz, h, Hr);
          double e = z - h;
          if constexpr (ROBUST) {
            const double t = e / dl;
            s = sqrt(1.0 + t * t);
            g = sqrt(s);
          }
          for (int c = 0; c < n; ++c) e -= Hr[c] * (MP[c] - x[c]);
          for (int c = 0; c < n; ++c) H[lane * n + c] = Hr[c];
          E[lane] = e;
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        for (int t = lane; t < nz * n; t += 64) {  // T1 = H S-
          const int ii = t / n, c = t % n;
          double acc = 0.0;
          for (int l = 0; l < n; ++l) acc += H[ii * n + l] * SP[l * n + c];
          T1[t] = acc;
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        // ---- augmented sweep: lane i holds row i of [P | T1 | e], P = T1 H^T + R
        double p[MAXP], t1[n], e = 0.0;
#pragma unroll
        for (int j = 0; j < MAXP; ++j) {
          double acc = 0.0, gg = 1.0;
          if constexpr (ROBUST) gg = g * readlane_d(g, j);  // lanes that hold no row keep g = 1
          if (row && j < nz) {
            for (int l = 0; l < n; ++l) acc += T1[i * n + l] * H[j * n + l];
            if constexpr (ROBUST)
              acc += Rk[i * a.nmeas_rows_max + j] * gg;
            else
              acc += Rk[i * a.nmeas_rows_max + j];
          }
          p[j] = acc;
        }
#pragma unroll
        for (int c = 0; c < n; ++c) t1[c] = row ? T1[i * n + c] : 0.0;
        if (row) e = E[i];
        if (it == 0) {
          // lane i tests its own diagonal entry of P, at the prediction
          double pd = 0.0;
          if constexpr (ROBUST) {
            // the unweighted P_ii, by the plain instances' sum
            if (row) {
              for (int l = 0; l < n; ++l) pd += T1[i * n + l] * H[i * n + l];
              pd += Rk[i * a.nmeas_rows_max + i];
            }
          } else {
#pragma unroll
            for (int j = 0; j < MAXP; ++j) pd = (j == i) ? p[j] : pd;
          }
          km = (unsigned)__ballot(row && !(pd > 0.0 && e * e / pd > a.gate));
          if (km == 0u) {  // every row screened out: predict-only
            corrected = false;
            if (lane == 0) {
              const size_t at = hist_at(a, b, k, 0, 1);
              if (a.nis) a.nis[at] = 0.0;
              if (a.loglik) a.loglik[at] = 0.0;
              if (a.rej) a.rej[at] = (int)row_bits(nz);
            }
            break;
          }
        }
        const bool rowk = row && ((km >> (i & 31)) & 1u);  // this lane holds a row of the sweep
        if (!rowk) {
          e = 0.0;
#pragma unroll
          for (int c = 0; c < n; ++c) t1[c] = 0.0;
        }
        double idg = 0.0;
        bool bad = false;
#pragma unroll
        for (int c = 0; c < MAXP; ++c) {
          if (c < nz && ((km >> c) & 1u)) {
            const double piv = readlane_d(p[c], c);
            bad |= !(piv > 0.0 && piv < INFINITY);
            const double rs = 1.0 / sqrt(piv);
            const double qv = p[c] * rs;                 // L_ic (i > c)
            const double mm = (i > c && rowk) ? qv * rs : 0.0;  // A'_ic / A'_cc
            idg = (i == c) ? rs : idg;
#pragma unroll
            for (int j = c + 1; j < MAXP; ++j)
              if (j < nz) p[j] -= qv * readlane_d(qv, j);
#pragma unroll
            for (int cc = 0; cc < n; ++cc) t1[cc] -= mm * readlane_d(t1[cc], c);
            e -= mm * readlane_d(e, c);
          }
        }
        if (bad) status = 1;
        if (row) {
#pragma unroll
          for (int c = 0; c < n; ++c) Y[i * n + c] = t1[c] * idg;  // Y = L^-1 H S-
          W[i] = e * idg;                                         // w = L^-1 e
        }
        if (it == 0 && (a.nis || a.loglik || a.rej)) {
          // nis = w^T w, log det P_a = -2 sum log(1 / L_ii): the rows sit in lanes 0..31
          double s2 = rowk ? (e * idg) * (e * idg) : 0.0;
          double lg = rowk ? log(idg) : 0.0;
#pragma unroll
          for (int off = 16; off >= 1; off >>= 1) {
            s2 += __shfl_xor(s2, off);
            lg += __shfl_xor(lg, off);
          }
          if (lane == 0) {
            const int cnt = __popc(km);
            const size_t at = hist_at(a, b, k, 0, 1);
            if (a.nis) a.nis[at] = s2;
            if (a.loglik) a.loglik[at] = -0.5 * (s2 - 2.0 * lg + cnt * LOG_2PI);
            if (a.rej) a.rej[at] = (int)(~km & row_bits(nz));
          }
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        // ---- x_{i+1} = mu- + Y^T w (utils/ekf.py:34, 58); E <- |x_{i+1} - x_i| per component
        for (int t = lane; t < n; t += 64) {
          double acc = 0.0;
          for (int ii = 0; ii < nz; ++ii) acc += Y[ii * n + t] * W[ii];
          const double xn = MP[t] + acc;
          E[t] = fabs(xn - X[t]);
          X[t] = xn;
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        ++it;
        // the stop decision is read from LDS by every lane, so it is wave-uniform;
        // !(step > tol) with step the max over the components: a NaN component stops as well.
        // tol = 0 asks for max_iter passes: the step is not tested (an exact zero would stop).
        bool moving = false, nan = false;
        for (int c = 0; c < n; ++c) {
          const double d = E[c];
          moving |= d > a.tol;
          nan |= !(d == d);
        }
        if ((a.tol > 0.0 && (!moving || nan)) || it == a.max_iter) break;
        __builtin_amdgcn_wave_barrier();  // E is read before the next pass rewrites it
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      }
    }
    if (corrected) {
      // mu = x_{i+1};  S = S- - Y^T Y with the last pass's Y   (utils/ekf.py:35, 59)
      for (int t = lane; t < n * n; t += 64) {
        const int r = t / n, c = t % n;
        double acc = 0.0;
        for (int ii = 0; ii < nz; ++ii) acc += Y[ii * n + r] * Y[ii * n + c];
        S[t] = SP[t] - acc;
      }
      for (int t = lane; t < n; t += 64) mu[t] = X[t];
    } else {
      if (nz > a.nmeas_rows_max) status = 2;
      for (int t = lane; t < n * n; t += 64) S[t] = SP[t];
      for (int t = lane; t < n; t += 64) mu[t] = MP[t];
      if (!valid && lane == 0) {
        const size_t at = hist_at(a, b, k, 0, 1);
        if (a.nis) a.nis[at] = 0.0;
        if (a.loglik) a.loglik[at] = 0.0;
        if (a.rej) a.rej[at] = 0;
      }
    }
    if (a.n_iter && lane == 0) a.n_iter[hist_at(a, b, k, 0, 1)] = corrected ? it : 0;
    if constexpr (ROBUST) {
      // omega of the last pass on the rows that were applied, 0 on every other row of the step
      if (a.weights && lane < a.nmeas_rows_max)
        a.weights[hist_at(a, b, k, lane, a.nmeas_rows_max)] =
            (corrected && lane < nz && ((km >> (lane & 31)) & 1u)) ? 1.0 / s : 0.0;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    if (a.mu_hist)
      for (int t = lane; t < n; t += 64) a.mu_hist[hist_at(a, b, k, t, n)] = mu[t];
    if (a.S_hist)
      for (int t = lane; t < n * n; t += 64) a.S_hist[hist_at(a, b, k, t, n * n)] = S[t];
  }
  for (int t = lane; t < n; t += 64) a.mu[(size_t)b * n + t] = mu[t];
  for (int t = lane; t < n * n; t += 64) a.S[(size_t)b * n * n + t] = S[t];
  if (a.status && lane == 0) a.status[b] = status;
}

template <class DYN, class MEAS, bool ROBUST>
int launch(const KernelArgs<ROBUST>& a, hipStream_t st) {
  const int smem = NWF * WaveSmem<DYN::n>::total * (int)sizeof(double);
  hipLaunchKernelGGL((k_iekf<DYN, MEAS, ROBUST>), dim3((a.batch + NWF - 1) / NWF), dim3(NWF * 64), smem, st, a);
  return hipGetLastError() == hipSuccess ? MHE_OK : MHE_ERR_HIP;
}

// mhe_iekf_run (ARGS = mhe_iekf_args) and mhe_iekf_run_robust (mhe_iekf_robust_args: the same
// fields in order, then delta, DELTA, weights): one set of refusals, all before the launch
template <bool ROBUST, class ARGS>
int run(const mhe_ekf_dims* dims, const ARGS* args, void* stream) {
  using namespace mhe_ekf;
  if (!dims || !args) return MHE_ERR_NULL;
  if (dims->struct_size != (int32_t)sizeof(mhe_ekf_dims)) return MHE_ERR_DIMS;  // stale / truncated binding
  if (args->struct_size != (int32_t)sizeof(ARGS)) return MHE_ERR_DIMS;
  if (!(args->gate >= 0.0)) return MHE_ERR_DIMS;  // NaN or negative; 0 = no screening, +inf allowed
  if (!(args->tol >= 0.0)) return MHE_ERR_DIMS;   // NaN or negative
  if (args->max_iter < 1 || args->max_iter > MAX_ITER || args->reserved0 != 0) return MHE_ERR_DIMS;
  if constexpr (ROBUST) {
    // one delta for every row (> 0, +inf allowed), or an array and then delta == 0
    if (args->DELTA ? args->delta != 0.0 : !(args->delta > 0.0)) return MHE_ERR_DIMS;
  }
  const int32_t batch = args->batch, steps = args->steps;
  if (batch < 0 || steps < 0 || dims->pmax < 1 || dims->pmax > MAXP) return MHE_ERR_DIMS;
  if (batch == 0 || steps == 0) return MHE_OK;
  if (!args->mu || !args->S || !args->Q || !args->nz || !args->Z || !args->R || (dims->m > 0 && !args->U))
    return MHE_ERR_NULL;
  KernelArgs<ROBUST> a = {};
  a.batch = batch; a.steps = steps; a.nmeas_rows_max = dims->pmax; a.dt = dims->dt;
  a.mu = args->mu; a.S = args->S; a.U = args->U; a.u_bstride = args->u_bstride; a.Z = args->Z;
  a.z_bstride = args->z_bstride; a.nz = args->nz; a.nz_bstride = args->nz_bstride; a.PAR = args->PAR;
  a.par_bstride = args->par_bstride; a.Q = args->Q; a.R = args->R; a.r_bstride = args->r_bstride;
  a.r_sstride = args->r_sstride; a.mu_hist = args->mu_hist; a.S_hist = args->S_hist; a.status = args->status;
  a.gate = args->gate != 0.0 ? args->gate : INFINITY;
  a.nis = args->nis; a.loglik = args->loglik; a.rej = args->rej;
  a.tol = args->tol; a.n_iter = args->n_iter; a.max_iter = args->max_iter;
  if constexpr (ROBUST) {
    a.delta = args->delta; a.DELTA = args->DELTA; a.weights = args->weights;
  }
  a.hist_bi = dims->hist_batch_inner != 0;
  a.es = 1;
  if (dims->in_batch_inner) {  // U (steps, m, B), Z (steps, pmax, B), nz (steps, B), PAR (steps, pmax, q, B)
    a.es = batch;
    a.u_bstride = a.z_bstride = a.nz_bstride = a.par_bstride = 1;
  }
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < 8; ++i) a.dp[i] = dims->dyn_par[i];
  if (dims->q != 3) return MHE_ERR_DIMS;
  if (!args->PAR) return MHE_ERR_NULL;
  if (dims->dyn_model == MHE_EKF_DYN_GNSS_POS_AND_BIAS) {
    if (dims->n != 5 || dims->m != 3) return MHE_ERR_MODEL;
    switch (dims->meas_model) {
      case MHE_EKF_MEAS_MULTI_PSEUDORANGE:
        return launch<EkfGnssPosAndBias, EkfMultiPseudorange<false>, ROBUST>(a, st);
      case MHE_EKF_MEAS_MULTI_PSEUDORANGE_AND_BIAS:
        return launch<EkfGnssPosAndBias, EkfMultiPseudorange<true>, ROBUST>(a, st);
    }
  } else if (dims->dyn_model == MHE_EKF_DYN_DISCRETE_VEHICLE) {
    if (dims->n != 9 || dims->m != 2) return MHE_ERR_MODEL;
    if (!(dims->dyn_par[2] != 0.0 && dims->dyn_par[5] != 0.0)) return MHE_ERR_DIMS;  // M, I_Z unset
    if (dims->meas_model == MHE_EKF_MEAS_VEHICLE_SENSORS)
      return launch<EkfDiscreteVehicle, EkfVehicleSensors, ROBUST>(a, st);
  }
  return MHE_ERR_MODEL;
}

}  // namespace mhe_iekf

extern "C" int mhe_iekf_run(const mhe_ekf_dims* dims, const mhe_iekf_args* args, void* stream) {
  return mhe_iekf::run<false>(dims, args, stream);
}

extern "C" int mhe_iekf_run_robust(const mhe_ekf_dims* dims, const mhe_iekf_robust_args* args, void* stream) {
  return mhe_iekf::run<true>(dims, args, stream);
}
