// libmhe: EM sufficient statistics of the EKF's noise model for MI355X (gfx950).
//
// Reduces a smoothed history (mu_s, S_s and the lag-one covariances C of mhe_ekf_smooth_args)
// to what the M-step of the Shumway-Stoffer / extended-RTS EM update of Q and R needs
// (Sarkka, Bayesian Filtering and Smoothing, ch. 12), per filter:
//   W_k  = d d^T + Ss_k - C_k F^T - F C_k^T + F Ss_{k-1} F^T,   (f, F) = f(mus_{k-1}, u_k),  d = mus_k - f
//   Qsum = sum_k W_k,   r2[k][i] = (z_i - h_i(mus_k))^2 + H_i Ss_k H_i^T
// ONE FILTER PER LANE, as k_ekf_lane and k_ekf_rts: no LDS, no barrier, no cross-lane traffic,
// every sum in a fixed order (k increasing, the terms of W_k in the order of the loops below), so
// a filter's result is bitwise the same alone or anywhere in any batch.  With batch-innermost
// histories and inputs consecutive lanes read consecutive words.
// Registers: the triangle of Qsum, ONE triangle S (Ss_{k-1} while F Ss_{k-1} F^T is added, then
// overwritten by Ss_k, which the rows use and the next step inherits), F's structural non-zeros,
// and one row of C at a time: C F^T + F C^T = P + P^T with P = C F^T, and row r of P needs row r
// of C alone; P(r, c) and P(c, r) land in the same slot of the triangle, the diagonal twice.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mhe.h"
#include "mhe_ekf_models.h"

namespace mhe_em {

using namespace mhe_ekf;

constexpr int MAXP = 32;  // measurement rows per step (the filters' capacity: bit i of rej is row i)

struct EmArgs {
  int batch, steps, pmax;
  double dt;
  double dp[8];
  const double* mu_s;
  const double* S_s;
  const double* C;
  const double* mu0_s;  // (B, n) / (B, n, n) batch outermost; both or neither
  const double* S0_s;
  const double* U;
  long long u_bstride;
  const double* Z;
  long long z_bstride;
  const int* nz;
  long long nz_bstride;
  const double* PAR;
  long long par_bstride;
  long long es;  // element stride of U / Z / nz / PAR, as mhe_ekf::EkfArgs
  const int* rej;
  double* Qsum;
  int* q_cnt;
  double* r2;
  int* r_cnt;
  int* status;
  int hist_bi;  // mu_s (steps, n, B), S_s / C (steps, n, n, B), rej (steps, B), r2 (steps, pmax, B)
};

// slot of (r, c) = (c, r) in a row-major upper triangle
template <int n>
constexpr int tri(int r, int c) {
  return r <= c ? r * n - r * (r - 1) / 2 + (c - r) : c * n - c * (c - 1) / 2 + (r - c);
}

// where step k's w-entry record of filter b starts and the stride between its entries;
// k = -1 is the prior's (B, w) array
struct Rec {
  long long off, es;
};
__device__ __forceinline__ Rec rec(const EmArgs& a, int b, int k, int w) {
  if (k < 0) return {(long long)b * w, 1};
  if (a.hist_bi) return {(long long)k * w * a.batch + b, a.batch};
  return {((long long)b * a.steps + k) * w, 1};
}

template <class DYN, class MEAS>
__global__ __launch_bounds__(256, DYN::n <= 5 ? 2 : 1) void k_ekf_em(EmArgs a) {
  constexpr int n = DYN::n, m = DYN::m, q = MEAS::q, TS = n * (n + 1) / 2;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.batch) return;  // no barriers below
  const bool prior = a.mu0_s != nullptr;
  double Qs[TS], S[TS], mp[n];
#pragma unroll
  for (int i = 0; i < TS; ++i) Qs[i] = 0.0;
  if (prior) {
    const Rec rm = rec(a, b, -1, n), rs = rec(a, b, -1, n * n);
#pragma unroll
    for (int c = 0; c < n; ++c) mp[c] = a.mu0_s[rm.off + c * rm.es];
#pragma unroll
    for (int r = 0; r < n; ++r)
#pragma unroll
      for (int c = r; c < n; ++c) S[tri<n>(r, c)] = a.S0_s[rs.off + (r * n + c) * rs.es];
  }
  int qc = 0, rcnt = 0;
  bool over = false;
  double chk = 0.0;  // sum of the r2 written: non-finite iff one of them is
  for (int k = 0; k < a.steps; ++k) {
    const Rec rm = rec(a, b, k, n), rs = rec(a, b, k, n * n);
    double mk[n];
#pragma unroll
    for (int c = 0; c < n; ++c) mk[c] = a.mu_s[rm.off + c * rm.es];
    const bool dyn = k > 0 || prior;
    if (dyn) {
      double u[m > 0 ? m : 1], f[n], F[n * n], d[n];
#pragma unroll
      for (int c = 0; c < m; ++c) u[c] = a.U[(long long)b * a.u_bstride + ((long long)k * m + c) * a.es];
      DYN::step(mp, u, a.dt, a.dp, f, F);
#pragma unroll
      for (int c = 0; c < n; ++c) d[c] = mk[c] - f[c];
      // d d^T + F Ss_{k-1} F^T: only the structural non-zeros of F (DYN::gnz) enter the products
#pragma unroll
      for (int c = 0; c < n; ++c) {
        double v[n];  // (Ss_{k-1} F^T)[:, c]
#pragma unroll
        for (int l = 0; l < n; ++l) {
          double acc = 0.0;
#pragma unroll
          for (int kk = 0; kk < n; ++kk)
            if (DYN::gnz(c, kk)) acc += S[tri<n>(l, kk)] * F[c * n + kk];
          v[l] = acc;
        }
#pragma unroll
        for (int r = 0; r < n; ++r) {
          if (r > c) continue;  // a constant trip count: the loop is unrolled for every c
          double acc = 0.0;
#pragma unroll
          for (int l = 0; l < n; ++l)
            if (DYN::gnz(r, l)) acc += F[r * n + l] * v[l];
          Qs[tri<n>(r, c)] += d[r] * d[c] + acc;
        }
      }
      // - (P + P^T), P = C_k F^T, one row of C at a time
#pragma unroll
      for (int r = 0; r < n; ++r) {
        double cr[n];
#pragma unroll
        for (int j = 0; j < n; ++j) cr[j] = a.C[rs.off + (r * n + j) * rs.es];
#pragma unroll
        for (int c = 0; c < n; ++c) {
          double p = 0.0;
#pragma unroll
          for (int j = 0; j < n; ++j)
            if (DYN::gnz(c, j)) p += cr[j] * F[c * n + j];
          Qs[tri<n>(r, c)] -= (r == c) ? 2.0 * p : p;
        }
      }
      ++qc;
    }
    // Ss_k: a term of W_k, the rows' covariance, and the next step's Ss_{k-1}
#pragma unroll
    for (int r = 0; r < n; ++r)
#pragma unroll
      for (int c = r; c < n; ++c) S[tri<n>(r, c)] = a.S_s[rs.off + (r * n + c) * rs.es];
    if (dyn) {
#pragma unroll
      for (int i = 0; i < TS; ++i) Qs[i] += S[i];
    }
#pragma unroll
    for (int c = 0; c < n; ++c) mp[c] = mk[c];
    // ---- measurement rows at mus_k
    const int nz = a.nz[(long long)b * a.nz_bstride + (long long)k * a.es];
    if (nz > a.pmax) over = true;
    const int rows = (nz > 0 && nz <= a.pmax) ? nz : 0;
    const unsigned rj = a.rej ? (unsigned)a.rej[rec(a, b, k, 1).off] : 0u;
    const double* zk = a.Z + (long long)b * a.z_bstride + (long long)k * a.pmax * a.es;
    const double* pk = a.PAR + (long long)b * a.par_bstride + (long long)k * a.pmax * q * a.es;
    const Rec rr = rec(a, b, k, a.pmax);
    // rows in chunks of RCH, a chunk's inputs loaded before its first row (k_ekf_lane's scheme;
    // clamped rows read valid memory and are not counted)
    constexpr int RCH = 8;
    for (int i0 = 0; i0 < a.pmax; i0 += RCH) {
      double zr[RCH], pr[RCH][q > 0 ? q : 1];
      if (i0 < rows) {
#pragma unroll
        for (int u = 0; u < RCH; ++u) {
          const int ic = min(i0 + u, rows - 1);
          zr[u] = zk[ic * a.es];
#pragma unroll
          for (int c = 0; c < q; ++c) pr[u][c] = pk[(ic * q + c) * a.es];
        }
      }
#pragma unroll
      for (int u = 0; u < RCH; ++u) {
        const int i = i0 + u;
        if (i >= a.pmax) break;
        double val = 0.0;
        if (i < rows && !((rj >> i) & 1u)) {
          double h, H[n];
          MEAS::template row<n>(mk, pr[u], i, nz, h, H);
          const double e = zr[u] - h;
          double sv = 0.0;  // H_i Ss_k H_i^T
#pragma unroll
          for (int r = 0; r < n; ++r) {
            double acc = 0.0;
#pragma unroll
            for (int c = 0; c < n; ++c) acc += S[tri<n>(r, c)] * H[c];
            sv += H[r] * acc;
          }
          val = e * e + sv;
          chk += fabs(val);
          ++rcnt;
        }
        a.r2[rr.off + i * rr.es] = val;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < TS; ++i) chk += fabs(Qs[i]);
  const bool bad = !(chk < INFINITY);
  if (bad) {  // a non-finite value was met: this filter's sums say nothing
#pragma unroll
    for (int i = 0; i < TS; ++i) Qs[i] = NAN;
    for (int k = 0; k < a.steps; ++k) {
      const Rec rr = rec(a, b, k, a.pmax);
      for (int i = 0; i < a.pmax; ++i) a.r2[rr.off + i * rr.es] = NAN;
    }
  }
#pragma unroll
  for (int r = 0; r < n; ++r)
#pragma unroll
    for (int c = 0; c < n; ++c) a.Qsum[(size_t)b * n * n + r * n + c] = Qs[tri<n>(r, c)];
  a.q_cnt[b] = qc;
  a.r_cnt[b] = rcnt;
  if (a.status) a.status[b] = bad ? 1 : (over ? 2 : 0);
}

template <class DYN, class MEAS>
int launch(const EmArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((k_ekf_em<DYN, MEAS>), dim3((a.batch + 255) / 256), dim3(256), 0, st, a);
  return hipGetLastError() == hipSuccess ? MHE_OK : MHE_ERR_HIP;
}

}  // namespace mhe_em

extern "C" int mhe_ekf_em_stats(const mhe_ekf_dims* dims, const mhe_em_args* args, void* stream) {
  using namespace mhe_em;
  if (!dims || !args) return MHE_ERR_NULL;
  if (dims->struct_size != (int32_t)sizeof(mhe_ekf_dims)) return MHE_ERR_DIMS;  // stale / truncated binding
  if (args->struct_size != (int32_t)sizeof(mhe_em_args)) return MHE_ERR_DIMS;
  const int32_t batch = args->batch, steps = args->steps;
  if (batch < 0 || steps < 0 || dims->pmax < 1 || dims->pmax > MAXP || dims->q != 3) return MHE_ERR_DIMS;
  if (batch == 0 || steps == 0) return MHE_OK;
  int (*run)(const EmArgs&, hipStream_t) = nullptr;
  if (dims->dyn_model == MHE_EKF_DYN_GNSS_POS_AND_BIAS) {
    if (dims->n != 5 || dims->m != 3) return MHE_ERR_MODEL;
    if (dims->meas_model == MHE_EKF_MEAS_MULTI_PSEUDORANGE) run = launch<EkfGnssPosAndBias, EkfMultiPseudorange<false>>;
    if (dims->meas_model == MHE_EKF_MEAS_MULTI_PSEUDORANGE_AND_BIAS)
      run = launch<EkfGnssPosAndBias, EkfMultiPseudorange<true>>;
  } else if (dims->dyn_model == MHE_EKF_DYN_DISCRETE_VEHICLE) {
    if (dims->n != 9 || dims->m != 2) return MHE_ERR_MODEL;
    if (!(dims->dyn_par[2] != 0.0 && dims->dyn_par[5] != 0.0)) return MHE_ERR_DIMS;  // M, I_Z unset
    if (dims->meas_model == MHE_EKF_MEAS_VEHICLE_SENSORS) run = launch<EkfDiscreteVehicle, EkfVehicleSensors>;
  }
  if (!run) return MHE_ERR_MODEL;
  if (!args->mu_s || !args->S_s || !args->C || !args->U || !args->Z || !args->nz || !args->PAR || !args->Qsum ||
      !args->q_cnt || !args->r2 || !args->r_cnt)
    return MHE_ERR_NULL;
  if ((args->mu0_s == nullptr) != (args->S0_s == nullptr)) return MHE_ERR_NULL;
  EmArgs a = {};
  a.batch = batch; a.steps = steps; a.pmax = dims->pmax; a.dt = dims->dt;
  for (int i = 0; i < 8; ++i) a.dp[i] = dims->dyn_par[i];
  a.mu_s = args->mu_s; a.S_s = args->S_s; a.C = args->C; a.mu0_s = args->mu0_s; a.S0_s = args->S0_s;
  a.U = args->U; a.u_bstride = args->u_bstride; a.Z = args->Z; a.z_bstride = args->z_bstride; a.nz = args->nz;
  a.nz_bstride = args->nz_bstride; a.PAR = args->PAR; a.par_bstride = args->par_bstride; a.rej = args->rej;
  a.Qsum = args->Qsum; a.q_cnt = args->q_cnt; a.r2 = args->r2; a.r_cnt = args->r_cnt; a.status = args->status;
  a.hist_bi = dims->hist_batch_inner != 0;
  a.es = 1;
  if (dims->in_batch_inner) {  // U (steps, m, B), Z (steps, pmax, B), nz (steps, B), PAR (steps, pmax, q, B)
    a.es = batch;
    a.u_bstride = a.z_bstride = a.nz_bstride = a.par_bstride = 1;
  }
  return run(a, (hipStream_t)stream);
}
