// libmhe: batched extended Kalman filter for MI355X (gfx950).
//
// Replaces utils/ekf.py:20-61 (EKF.update -> predict / correct, kingdwd/nlp-filter)
// for many independent filter instances at once: ONE WAVEFRONT PER FILTER runs
// all `steps` updates of its instance; four instances per workgroup.  Per step
//   predict:  mu- = f(mu, u),  S- = G S G^T + Q                (utils/ekf.py:40-45)
//   correct:  P = H S- H^T + R,  K = S- H^T P^-1,
//             mu = mu- + K (z - h(mu-)),  S = S- - K H S-        (utils/ekf.py:47-61)
// The reference forms P^-1 explicitly (utils/ekf.py:55).  Here one augmented
// right-looking Cholesky sweep over [P | H S- | e] (row per lane, pivots and
// L_jc broadcast by v_readlane) gives Y = L^-1 H S- and w = L^-1 e, so that
//   K e = Y^T w   and   K H S- = Y^T Y
// -- no inverse and no back substitution; S stays symmetric by construction.
// Results agree with the reference to floating-point rounding (tests state the
// tolerance).  Plug-ins are the utils/gnss.py models as device functors.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mhe.h"
#include "mhe_ekf_models.h"

namespace mhe_ekf {

constexpr int NWF = 4;     // filters (waves) per workgroup
constexpr int MAXP = 32;   // measurement rows per step (nz <= pmax <= MAXP; mhe_ekf_run checks pmax)

struct EkfArgs {
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
  int hist_bi;  // 1: histories batch-innermost, mu_hist (steps, n, B), S_hist (steps, n, n, B)
  long long es;  // element stride of U / Z / nz / PAR: 1 (batch outermost) or batch (batch innermost,
                 // the b-strides are then 1): entry e of step k of instance b at b*bstride + (k*W + e)*es
  int* status;
};

// the gated instances (k_ekf<.., true>, k_ekf_lane<.., true>) take these as well; the others
// keep the kernel arguments they had
struct EkfGateArgs : EkfArgs {
  double gate;     // screen threshold on d2_i = e_i^2 / (H_i S- H_i^T + R_ii); +inf: no screening
  double* nis;     // per-step statistics, optional: (steps, B) with hist_bi, else (B, steps)
  double* loglik;
  int* rej;        // bit i: row i was screened out
};
template <bool GATE>
struct KArgs { using type = EkfArgs; };
template <>
struct KArgs<true> { using type = EkfGateArgs; };

constexpr double LOG_2PI = 1.8378770664093454836, LOG_2 = 0.69314718055994530942;

// bits 0..rows-1 (rows <= 32)
__device__ __forceinline__ unsigned row_bits(int rows) { return rows >= 32 ? 0xffffffffu : (1u << rows) - 1u; }

// element (b, k, e) of a per-step history with `w` entries per step
__device__ __forceinline__ size_t hist_at(const EkfArgs& a, int b, int k, int e, int w) {
  return a.hist_bi ? ((size_t)k * w + e) * a.batch + b : ((size_t)b * a.steps + k) * w + e;
}

// per-wave LDS scratch (doubles)
template <int n>
struct WaveSmem {
  static constexpr int MU = 0, S = MU + n, G = S + n * n, SP = G + n * n, MP = SP + n * n, H = MP + n,
                       T1 = H + MAXP * n, E = T1 + MAXP * n, Y = E + MAXP, W = Y + MAXP * n, total = W + MAXP;
};

// GATE (k_ekf and k_ekf_lane alike): innovation screening and the per-step statistics.
// Row i of a step is screened out iff d2_i = e_i^2 / (H_i S- H_i^T + R_ii) > a.gate, with
// e_i = z_i - h_i(mu-): marginal and at the prediction, so it depends neither on the row
// order nor on the other rows, and both kernels decide alike.  A NaN or a non-positive
// denominator keeps the row (status 1 then reports it).  The correction is the ungated one
// on the kept rows in their order; rows keep their index (MEAS::row sees the original i, nz).
// nis = e_a^T P_a^-1 e_a, loglik = -(nis + log det P_a + |a| log 2 pi) / 2 over the kept rows a
// (both 0 when there is none), rej = the mask of screened rows.  GATE = false is the code
// as it was: those instances serve every call without a gate or a statistics output.
template <class DYN, class MEAS, bool GATE = false>
__global__ __launch_bounds__(NWF * 64) void k_ekf(typename KArgs<GATE>::type a) {
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
  for (int t = lane; t < n; t += 64) mu[t] = a.mu[(size_t)b * n + t];
  for (int t = lane; t < n * n; t += 64) S[t] = a.S[(size_t)b * n * n + t];
  int status = 0;
  __builtin_amdgcn_wave_barrier();
  for (int k = 0; k < a.steps; ++k) {
    // ---- predict (utils/ekf.py:40-45)
    if (lane == 0) {
      double x[n], u[m > 0 ? m : 1], xp[n], Gl[n * n];
      for (int c = 0; c < n; ++c) x[c] = mu[c];
      for (int c = 0; c < m; ++c) u[c] = a.U[(long long)b * a.u_bstride + ((long long)k * m + c) * a.es];
      DYN::step(x, u, a.dt, a.dp, xp, Gl);
      for (int c = 0; c < n; ++c) MP[c] = xp[c];
      for (int c = 0; c < n * n; ++c) G[c] = Gl[c];
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    for (int t = lane; t < n * n; t += 64) {  // S- = G S G^T + Q
      const int r = t / n, c = t % n;
      double acc = 0.0;
      for (int kk = 0; kk < n; ++kk) {
        double gs = 0.0;
        for (int l = 0; l < n; ++l) gs += S[kk * n + l] * G[c * n + l];  // (S G^T)[kk][c]
        acc += G[r * n + kk] * gs;
      }
      SP[t] = acc + a.Q[t];
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    const int nz = a.nz[(long long)b * a.nz_bstride + (long long)k * a.es];
    // Z / PAR / R hold pmax (<= MAXP) rows per step: a step that claims more is refused
    if (nz > 0 && nz <= a.nmeas_rows_max) {
      // ---- measurement rows at mu- (utils/ekf.py:51)
      const long long rk = (long long)k * a.nmeas_rows_max + lane;  // row index within the instance
      if (lane < nz) {
        double x[n], h, Hr[n], par[q > 0 ? q : 1];
        for (int c = 0; c < n; ++c) x[c] = MP[c];
        for (int c = 0; c < q; ++c) par[c] = a.PAR[(long long)b * a.par_bstride + (rk * q + c) * a.es];
        MEAS::template row<n>(x, par, lane, nz, h, Hr);
        for (int c = 0; c < n; ++c) H[lane * n + c] = Hr[c];
        E[lane] = a.Z[(long long)b * a.z_bstride + rk * a.es] - h;
      }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      for (int t = lane; t < nz * n; t += 64) {  // T1 = H S-
        const int i = t / n, c = t % n;
        double acc = 0.0;
        for (int l = 0; l < n; ++l) acc += H[i * n + l] * SP[l * n + c];
        T1[t] = acc;
      }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      // ---- augmented sweep: lane i holds row i of [P | T1 | e], P = T1 H^T + R
      const double* Rk = a.R + (long long)b * a.r_bstride + (long long)k * a.r_sstride;
      const int i = lane;
      const bool row = i < nz;
      double p[MAXP], t1[n], e = 0.0;
#pragma unroll
      for (int j = 0; j < MAXP; ++j) {
        double acc = 0.0;
        if (row && j < nz) {
          for (int l = 0; l < n; ++l) acc += T1[i * n + l] * H[j * n + l];
          acc += Rk[i * a.nmeas_rows_max + j];
        }
        p[j] = acc;
      }
#pragma unroll
      for (int c = 0; c < n; ++c) t1[c] = row ? T1[i * n + c] : 0.0;
      if (row) e = E[i];
      bool rowk = row;                // this lane holds a row of the sweep
      unsigned km = 0xffffffffu;      // GATE: the kept rows (wave-uniform)
      if constexpr (GATE) {
        // lane i tests its own diagonal entry of P; a screened lane becomes a non-row with a
        // zero row of [T1 | e], so its rows of Y and W below are zeros
        double pd = 0.0;
#pragma unroll
        for (int j = 0; j < MAXP; ++j) pd = (j == i) ? p[j] : pd;
        rowk = row && !(pd > 0.0 && e * e / pd > a.gate);
        km = (unsigned)__ballot(rowk);
        if (!rowk) {
          e = 0.0;
#pragma unroll
          for (int c = 0; c < n; ++c) t1[c] = 0.0;
        }
      }
      double idg = 0.0;
      bool bad = false;
#pragma unroll
      for (int c = 0; c < MAXP; ++c) {
        if (c < nz && (!GATE || ((km >> c) & 1u))) {
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
      if constexpr (GATE) {
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
          if (a.nis) a.nis[at] = cnt ? s2 : 0.0;
          if (a.loglik) a.loglik[at] = cnt ? -0.5 * (s2 - 2.0 * lg + cnt * LOG_2PI) : 0.0;
          if (a.rej) a.rej[at] = (int)(~km & row_bits(nz));
        }
      }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      // mu = mu- + Y^T w ; S = S- - Y^T Y   (utils/ekf.py:34-35, 58-59)
      for (int t = lane; t < n * n; t += 64) {
        const int r = t / n, c = t % n;
        double acc = 0.0;
        for (int ii = 0; ii < nz; ++ii) acc += Y[ii * n + r] * Y[ii * n + c];
        S[t] = SP[t] - acc;
      }
      for (int t = lane; t < n; t += 64) {
        double acc = 0.0;
        for (int ii = 0; ii < nz; ++ii) acc += Y[ii * n + t] * W[ii];
        mu[t] = MP[t] + acc;
      }
    } else {
      if (nz > a.nmeas_rows_max) status = 2;
      for (int t = lane; t < n * n; t += 64) S[t] = SP[t];
      for (int t = lane; t < n; t += 64) mu[t] = MP[t];
      if constexpr (GATE) {
        if (lane == 0) {
          const size_t at = hist_at(a, b, k, 0, 1);
          if (a.nis) a.nis[at] = 0.0;
          if (a.loglik) a.loglik[at] = 0.0;
          if (a.rej) a.rej[at] = 0;
        }
      }
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

// ---------------------------------------------------------------- one filter per lane
// When every step's R is diagonal (dims->r_diag, checked by the caller) the
// correction is done as nz sequential SCALAR updates, all linearised at the
// prediction mu- (row i: h_i, H_i at mu-; innovation e_i = z_i - h_i(mu-) -
// H_i (mu - mu-) against the running mean).  For a linear(ised) measurement
// model with diagonal R this is algebraically the reference's batch update
// (utils/ekf.py:51-59: K = S- H^T P^-1, mu = mu- + K e, S = S- - K H S-):
//   v = S H_i^T,  s = H_i v + R_ii,  mu += v e_i / s,  S -= v v^T / s.
// The whole filter lives in one lane's registers (mu, mu-, S: 35 doubles), so a
// wave runs 64 filters with no broadcasts, barriers or LDS: O(p n^2) work per
// step instead of the sweep's O(p^3), and no lane idles on the row loop.
// S storage in one lane: full n x n for small n; for larger n (the 9-state vehicle)
// the upper triangle only (45 instead of 81 doubles, so S and S- fit the registers).
// The symmetric form reads S[r][c] = S[c][r] = stored (min, max) entry.
template <int n>
struct LaneS {
  static constexpr bool sym = true;
  static constexpr int size = sym ? n * (n + 1) / 2 : n * n;
  static constexpr int at(int r, int c) {
    return sym ? (r <= c ? r * n - r * (r - 1) / 2 + (c - r) : c * n - c * (c - 1) / 2 + (r - c)) : r * n + c;
  }
};

// GATE: the screen needs S- before the first update touches S, so a screening pass over the
// step's rows at (mu-, S-) leaves a keep mask in a register and the update pass skips the
// masked rows.  No second copy of S is held; the update pass re-reads the rows' inputs.  With
// a.gate = +inf (statistics only) the screening pass is skipped.  nis = sum e_i^2 / s_i and
// log det P_a = sum log s_i = log prod s_i of the sequential updates.
template <class DYN, class MEAS, bool GATE = false>
__global__ __launch_bounds__(256, GATE ? MEAS::lane_minw_gate : MEAS::lane_minw)
void k_ekf_lane(typename KArgs<GATE>::type a) {
  constexpr int n = DYN::n, m = DYN::m, q = MEAS::q;
  using LS = LaneS<n>;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.batch) return;  // no barriers below
  double mu[n], S[LS::size];
#pragma unroll
  for (int c = 0; c < n; ++c) mu[c] = a.mu[(size_t)b * n + c];
#pragma unroll
  for (int r = 0; r < n; ++r)
#pragma unroll
    for (int c = 0; c < n; ++c)
      if (!LS::sym || c >= r) S[LS::at(r, c)] = a.S[(size_t)b * n * n + r * n + c];
  int status = 0;
  for (int k = 0; k < a.steps; ++k) {
    // ---- predict: mu- = f(mu, u), S- = G S G^T + Q   (utils/ekf.py:40-45); only the
    // structural non-zeros of G (DYN::gnz, compile time) enter the products
    double u[m > 0 ? m : 1], mp[n], G[n * n];
#pragma unroll
    for (int c = 0; c < m; ++c) u[c] = a.U[(long long)b * a.u_bstride + ((long long)k * m + c) * a.es];
    DYN::step(mu, u, a.dt, a.dp, mp, G);
    double SN[LS::size];
#pragma unroll
    for (int c = 0; c < n; ++c) {
      double v[n];  // (S G^T)[:, c]
#pragma unroll
      for (int l = 0; l < n; ++l) {
        double acc = 0.0;
#pragma unroll
        for (int kk = 0; kk < n; ++kk)
          if (DYN::gnz(c, kk)) acc += S[LS::at(l, kk)] * G[c * n + kk];
        v[l] = acc;
      }
#pragma unroll
      for (int r = 0; r < n; ++r) {
        if (LS::sym && r > c) continue;
        double acc = 0.0;
#pragma unroll
        for (int l = 0; l < n; ++l)
          if (DYN::gnz(r, l)) acc += G[r * n + l] * v[l];
        SN[LS::at(r, c)] = acc + a.Q[r * n + c];
      }
    }
#pragma unroll
    for (int i = 0; i < LS::size; ++i) S[i] = SN[i];
#pragma unroll
    for (int c = 0; c < n; ++c) mu[c] = mp[c];
    // ---- correct: sequential scalar updates at the linearisation point mu-
    const int nz = a.nz[(long long)b * a.nz_bstride + (long long)k * a.es];
    // Z / PAR / R hold pmax (<= MAXP) rows per step: a step that claims more is refused
    if (nz > a.nmeas_rows_max) status = 2;
    const int rows = nz <= a.nmeas_rows_max ? nz : 0;
    // with batch-innermost inputs (es = batch) consecutive lanes read consecutive words
    const double* zk = a.Z + (long long)b * a.z_bstride + (long long)k * a.nmeas_rows_max * a.es;
    const double* pk = a.PAR + (long long)b * a.par_bstride + (long long)k * a.nmeas_rows_max * q * a.es;
    const double* Rk = a.R + (long long)b * a.r_bstride + (long long)k * a.r_sstride;
    // rows in chunks of RCH: all of a chunk's inputs (z, satellite position, R_ii) are
    // loaded before its first update, so a step costs ceil(nz / RCH) memory round
    // trips instead of nz (clamped rows read valid memory and are skipped)
    constexpr int RCH = 8;
    unsigned keep = 0xffffffffu;            // GATE: bit i clear = row i screened out
    double nis = 0.0, lprod = 1.0;          // GATE: sum e_i^2 / s_i and prod s_i over the kept rows
    int lexp = 0, cnt = 0;
    if constexpr (GATE) {
      if (a.gate < INFINITY) {
        for (int i0 = 0; i0 < rows; i0 += RCH) {  // screening pass at (mu-, S-), chunked as below
          double zr[RCH], pr[RCH][q > 0 ? q : 1], rr[RCH];
#pragma unroll
          for (int u = 0; u < RCH; ++u) {
            const int ic = min(i0 + u, rows - 1);
            zr[u] = zk[ic * a.es];
#pragma unroll
            for (int c = 0; c < q; ++c) pr[u][c] = pk[(ic * q + c) * a.es];
            rr[u] = Rk[ic * a.nmeas_rows_max + ic];
          }
#pragma unroll
          for (int u = 0; u < RCH; ++u) {
            if (i0 + u >= rows) break;
            double h, H[n];
            MEAS::template row<n>(mp, pr[u], i0 + u, nz, h, H);
            const double e = zr[u] - h;
            double sv = rr[u];  // H_i S- H_i^T + R_ii
#pragma unroll
            for (int r = 0; r < n; ++r) {
              double acc = 0.0;
#pragma unroll
              for (int c = 0; c < n; ++c) acc += S[LS::at(r, c)] * H[c];
              sv += H[r] * acc;
            }
            if (sv > 0.0 && e * e / sv > a.gate) keep &= ~(1u << (i0 + u));
          }
        }
      }
    }
    for (int i0 = 0; i0 < rows; i0 += RCH) {
      double zr[RCH], pr[RCH][q > 0 ? q : 1], rr[RCH];
#pragma unroll
      for (int u = 0; u < RCH; ++u) {
        const int ic = min(i0 + u, rows - 1);
        zr[u] = zk[ic * a.es];
#pragma unroll
        for (int c = 0; c < q; ++c) pr[u][c] = pk[(ic * q + c) * a.es];
        rr[u] = Rk[ic * a.nmeas_rows_max + ic];
      }
#pragma unroll
      for (int u = 0; u < RCH; ++u) {
        if (i0 + u >= rows) break;
        if constexpr (GATE) {
          if (!((keep >> (i0 + u)) & 1u)) continue;
        }
        double h, H[n];
        MEAS::template row<n>(mp, pr[u], i0 + u, nz, h, H);
        double e = zr[u] - h;
#pragma unroll
        for (int c = 0; c < n; ++c) e -= H[c] * (mu[c] - mp[c]);
        double v[n];
#pragma unroll
        for (int r = 0; r < n; ++r) {
          double acc = 0.0;
#pragma unroll
          for (int c = 0; c < n; ++c) acc += S[LS::at(r, c)] * H[c];
          v[r] = acc;
        }
        double sv = rr[u];
#pragma unroll
        for (int c = 0; c < n; ++c) sv += H[c] * v[c];
        if (!(sv > 0.0 && sv < INFINITY)) status = 1;
        const double inv = 1.0 / sv;
        const double ge = e * inv;
        if constexpr (GATE) {
          nis += e * ge;
          int ex;  // prod s_i as (mantissa product in [2^-32, 1)) x 2^lexp: one log per step, not per row
          lprod *= frexp(sv, &ex);
          lexp += ex;
          ++cnt;
        }
#pragma unroll
        for (int r = 0; r < n; ++r) mu[r] += v[r] * ge;
#pragma unroll
        for (int r = 0; r < n; ++r) {
          const double vr = v[r] * inv;
#pragma unroll
          for (int c = 0; c < n; ++c)
            if (!LS::sym || c >= r) S[LS::at(r, c)] -= vr * v[c];
        }
      }
    }
    if constexpr (GATE) {
      const size_t at = hist_at(a, b, k, 0, 1);
      if (a.nis) a.nis[at] = nis;
      if (a.loglik) a.loglik[at] = cnt ? -0.5 * (nis + (log(lprod) + lexp * LOG_2) + cnt * LOG_2PI) : 0.0;
      if (a.rej) a.rej[at] = (int)(~keep & row_bits(rows));
    }
    // histories: with the batch-innermost layout (hist_bi) consecutive lanes write
    // consecutive words -- one coalesced 512-B store per entry instead of 64 partial lines
    if (a.mu_hist) {
#pragma unroll
      for (int c = 0; c < n; ++c) a.mu_hist[hist_at(a, b, k, c, n)] = mu[c];
    }
    if (a.S_hist) {
#pragma unroll
      for (int r = 0; r < n; ++r)
#pragma unroll
        for (int c = 0; c < n; ++c) a.S_hist[hist_at(a, b, k, r * n + c, n * n)] = S[LS::at(r, c)];
    }
  }
#pragma unroll
  for (int c = 0; c < n; ++c) a.mu[(size_t)b * n + c] = mu[c];
#pragma unroll
  for (int r = 0; r < n; ++r)
#pragma unroll
    for (int c = 0; c < n; ++c) a.S[(size_t)b * n * n + r * n + c] = S[LS::at(r, c)];
  if (a.status) a.status[b] = status;
}

template <class DYN, class MEAS>
int launch(const EkfGateArgs& g, hipStream_t st, bool r_diag, bool gated) {
  const int smem = NWF * WaveSmem<DYN::n>::total * (int)sizeof(double);
  if (gated) {
    const EkfGateArgs& a = g;
    if (r_diag) {
      hipLaunchKernelGGL((k_ekf_lane<DYN, MEAS, true>), dim3((a.batch + 255) / 256), dim3(256), 0, st, a);
    } else {
      hipLaunchKernelGGL((k_ekf<DYN, MEAS, true>), dim3((a.batch + NWF - 1) / NWF), dim3(NWF * 64), smem, st, a);
    }
    return hipGetLastError() == hipSuccess ? MHE_OK : MHE_ERR_HIP;
  }
  const EkfArgs& a = g;
  if (r_diag) {
    hipLaunchKernelGGL((k_ekf_lane<DYN, MEAS>), dim3((a.batch + 255) / 256), dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL((k_ekf<DYN, MEAS>), dim3((a.batch + NWF - 1) / NWF), dim3(NWF * 64), smem, st, a);
  }
  return hipGetLastError() == hipSuccess ? MHE_OK : MHE_ERR_HIP;
}

// ---------------------------------------------------------------- fixed-interval smoother
// Rauch-Tung-Striebel backward pass over a filtered history (mu_k, S_k), one filter per
// lane as k_ekf_lane: no LDS, no barriers, no cross-lane traffic.  Carrying the smoothed
// (xs, Ss) of step k+1, step k recomputes the forward's prediction from its own output,
//   (x-, G) = DYN::step(mu_k, u_{k+1}),  S- = G S_k G^T + Q   (k_ekf_lane's predict, term by term)
// factors S- = L L^T (true sqrt and division: the result is user-facing) and, with
// A = G S_k and M = S-^-1 A (= C_k^T, two triangular solves per column, in place in A),
//   xs_k = mu_k + M^T (xs_{k+1} - x-),   Ss_k = S_k + M^T (Ss_{k+1} - S-) M.
// Measurements and R do not enter.  Registers: S_k, S- / L and the carry are upper triangles
// (LaneS); G is dead once A and S- are formed, L overwrites S-, D = Ss_{k+1} - S- overwrites
// the carry, M overwrites A and the triangle of S_k is the accumulator of Ss_k.  The inputs of
// step k-1 do not depend on the recursion and are loaded before step k's arithmetic.
// The prior (mu0, S0), when asked for, is one more step of the same loop at k = -1 with u_0.
struct RtsArgs {
  int batch, steps;
  double dt;
  double dp[8];
  const double* mu_hist;
  const double* S_hist;
  const double* U;
  long long u_bstride, es;  // as EkfArgs
  const double* Q;
  const double* mu0;        // (B, n) / (B, n, n), batch outermost; read only when a smoothed prior is asked for
  const double* S0;
  double* mu_s;             // may alias mu_hist / S_hist: a lane reads step k-1 before it writes step k
  double* S_s;
  double* mu0_s;
  double* S0_s;
  int hist_bi;
  int* status;
};

// the LAG instances (k_ekf_rts<.., true>) take the lag-one output as well; the others keep the
// kernel arguments they had
struct RtsLagArgs : RtsArgs {
  double* C;  // C_k = Cov(x_k, x_{k-1} | all data) = Ss_k M_{k-1}, all n x n entries, laid out as S_s; no aliasing
};
template <bool LAG>
struct RtsK { using type = RtsArgs; };
template <>
struct RtsK<true> { using type = RtsLagArgs; };

// where step k's w-entry record of filter b starts and the stride between its entries;
// k = -1 is the prior's (B, w) array
struct RtsRec {
  long long off, es;
};
__device__ __forceinline__ RtsRec rts_rec(const RtsArgs& a, int b, int k, int w) {
  if (k < 0) return {(long long)b * w, 1};
  if (a.hist_bi) return {(long long)k * w * a.batch + b, a.batch};
  return {((long long)b * a.steps + k) * w, 1};
}

template <class DYN>
struct RtsIn {
  double mu[DYN::n], S[LaneS<DYN::n>::size], u[DYN::m > 0 ? DYN::m : 1];
};

// (mu_k, upper triangle of S_k, u_{k+1}) of filter b; k = -1 reads the prior.  The last
// step has no u_{k+1} (with_u = false: U holds `steps` controls).
template <class DYN, bool with_u = true>
__device__ __forceinline__ void rts_load(const RtsArgs& a, int b, int k, RtsIn<DYN>& in) {
  constexpr int n = DYN::n, m = DYN::m;
  using LS = LaneS<n>;
  const RtsRec rm = rts_rec(a, b, k, n), rs = rts_rec(a, b, k, n * n);
  const double* pm = (k < 0 ? a.mu0 : a.mu_hist) + rm.off;
  const double* ps = (k < 0 ? a.S0 : a.S_hist) + rs.off;
#pragma unroll
  for (int c = 0; c < n; ++c) in.mu[c] = pm[c * rm.es];
#pragma unroll
  for (int r = 0; r < n; ++r)
#pragma unroll
    for (int c = r; c < n; ++c) in.S[LS::at(r, c)] = ps[(r * n + c) * rs.es];
  if (with_u) {
#pragma unroll
    for (int c = 0; c < m; ++c) in.u[c] = a.U[(long long)b * a.u_bstride + ((long long)(k + 1) * m + c) * a.es];
  }
}

// smoothed step k: S_s(r, c) and S_s(c, r) from one register, so the output is bitwise symmetric
template <int n>
__device__ __forceinline__ void rts_store(const RtsArgs& a, int b, int k, const double* xs, const double* Ss) {
  using LS = LaneS<n>;
  double* pm = k < 0 ? a.mu0_s : a.mu_s;
  double* ps = k < 0 ? a.S0_s : a.S_s;
  const RtsRec rm = rts_rec(a, b, k, n), rs = rts_rec(a, b, k, n * n);
  if (pm) {
#pragma unroll
    for (int c = 0; c < n; ++c) pm[rm.off + c * rm.es] = xs[c];
  }
  if (ps) {
#pragma unroll
    for (int r = 0; r < n; ++r)
#pragma unroll
      for (int c = 0; c < n; ++c) ps[rs.off + (r * n + c) * rs.es] = Ss[LS::at(r, c)];
  }
}

// a failed filter's outputs are NaN from the failing step down; a non-finite entry (a NaN or
// an infinity met in the history) is a failure as well
template <int n>
__device__ __forceinline__ bool rts_finite(const double* xs, const double* Ss) {
  double t = 0.0;
#pragma unroll
  for (int c = 0; c < n; ++c) t += fabs(xs[c]);
#pragma unroll
  for (int i = 0; i < LaneS<n>::size; ++i) t += fabs(Ss[i]);
  return t < INFINITY;
}

// LAG: the lag-one smoothed covariance C_{k+1} = Ss_{k+1} M as one more output of step k.  With
// D = Ss_{k+1} - S- the final sum already forms e = D M(:, c) per column, and S- M is the
// pre-solve A = G S_k, so C_{k+1}(:, c) = e + A(:, c): no second product with Ss_{k+1}.  M has
// overwritten A by then; column c of A is formed again from G (kept live: its structural
// non-zeros only) and column c of S_k, which the accumulation on S_k's triangle has not yet
// touched when column c is reached (it writes (r, c'), r <= c' < c, before).  C_0 needs the
// prior; without one it is written as NaN.  A failing step k leaves C NaN from k+1 down.
// LAG = false is the code as it was.
template <class DYN, bool LAG = false>
__global__ __launch_bounds__(256, DYN::n <= 5 ? 2 : 1) void k_ekf_rts(typename RtsK<LAG>::type a) {
  constexpr int n = DYN::n;
  using LS = LaneS<n>;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.batch) return;  // no barriers below
  const int kmin = (a.mu0_s || a.S0_s) ? -1 : 0;
  bool bad = false;
  double xs[n], Ss[LS::size];
  {  // k = T-1: the smoothed values are the filtered ones
    RtsIn<DYN> last;
    rts_load<DYN, false>(a, b, a.steps - 1, last);
#pragma unroll
    for (int c = 0; c < n; ++c) xs[c] = last.mu[c];
#pragma unroll
    for (int i = 0; i < LS::size; ++i) Ss[i] = last.S[i];
  }
  RtsIn<DYN> in = {};
  if (a.steps - 2 >= kmin) rts_load<DYN>(a, b, a.steps - 2, in);  // else no step follows (and U has no u_{k+1})
  if (!rts_finite<n>(xs, Ss)) {
    bad = true;
#pragma unroll
    for (int c = 0; c < n; ++c) xs[c] = NAN;
#pragma unroll
    for (int i = 0; i < LS::size; ++i) Ss[i] = NAN;
  }
  rts_store<n>(a, b, a.steps - 1, xs, Ss);
  for (int k = a.steps - 2; k >= kmin; --k) {
    // step k-1's inputs do not depend on the recursion: issued ahead of this step's
    // arithmetic, they arrive under it (the last step re-reads its own)
    RtsIn<DYN> nx;
    rts_load<DYN>(a, b, max(k - 1, kmin), nx);
    double xp[n], A[n * n], L[LS::size];
    double Gk[LAG ? n * n : 1];  // LAG: G outlives the block below
    {
      double Gb[LAG ? 1 : n * n];
      double* G = LAG ? Gk : Gb;
      DYN::step(in.mu, in.u, a.dt, a.dp, xp, G);
#pragma unroll
      for (int c = 0; c < n; ++c) {  // row c of A = G S_k, then column c of S- = A G^T + Q
#pragma unroll
        for (int l = 0; l < n; ++l) {
          double acc = 0.0;
#pragma unroll
          for (int kk = 0; kk < n; ++kk)
            if (DYN::gnz(c, kk)) acc += in.S[LS::at(l, kk)] * G[c * n + kk];
          A[c * n + l] = acc;
        }
#pragma unroll
        for (int r = 0; r <= c; ++r) {
          double acc = 0.0;
#pragma unroll
          for (int l = 0; l < n; ++l)
            if (DYN::gnz(r, l)) acc += G[r * n + l] * A[c * n + l];
          L[LS::at(r, c)] = acc + a.Q[r * n + c];
        }
      }
    }
    double d[n];
#pragma unroll
    for (int c = 0; c < n; ++c) d[c] = xs[c] - xp[c];
#pragma unroll
    for (int i = 0; i < LS::size; ++i) Ss[i] -= L[i];  // D = Ss_{k+1} - S-
    // S- = L L^T in place (L(i, j), i > j, in the slot of S-(j, i)); the diagonal slot keeps 1 / L(j, j)
#pragma unroll
    for (int j = 0; j < n; ++j) {
      double piv = L[LS::at(j, j)];
#pragma unroll
      for (int t = 0; t < j; ++t) piv -= L[LS::at(j, t)] * L[LS::at(j, t)];
      bad |= !(piv > 0.0 && piv < INFINITY);
      const double inv = 1.0 / sqrt(piv);
      L[LS::at(j, j)] = inv;
#pragma unroll
      for (int i = j + 1; i < n; ++i) {
        double v = L[LS::at(i, j)];
#pragma unroll
        for (int t = 0; t < j; ++t) v -= L[LS::at(i, t)] * L[LS::at(j, t)];
        L[LS::at(i, j)] = v * inv;
      }
    }
    // M = S-^-1 A, column by column in place: L y = A(:, c), L^T m = y
#pragma unroll
    for (int c = 0; c < n; ++c) {
#pragma unroll
      for (int r = 0; r < n; ++r) {
        double v = A[r * n + c];
#pragma unroll
        for (int t = 0; t < r; ++t) v -= L[LS::at(r, t)] * A[t * n + c];
        A[r * n + c] = v * L[LS::at(r, r)];
      }
#pragma unroll
      for (int r = n - 1; r >= 0; --r) {
        double v = A[r * n + c];
#pragma unroll
        for (int t = r + 1; t < n; ++t) v -= L[LS::at(t, r)] * A[t * n + c];
        A[r * n + c] = v * L[LS::at(r, r)];
      }
    }
    // xs_k = mu_k + M^T d;  Ss_k = S_k + M^T D M, accumulated on S_k's triangle
#pragma unroll
    for (int c = 0; c < n; ++c) {
      double acc = 0.0;
#pragma unroll
      for (int r = 0; r < n; ++r) acc += A[r * n + c] * d[r];
      xs[c] = in.mu[c] + acc;
      double e[n];  // D M(:, c)
#pragma unroll
      for (int l = 0; l < n; ++l) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < n; ++j) s += Ss[LS::at(l, j)] * A[j * n + c];
        e[l] = s;
      }
      if constexpr (LAG) {
        const RtsRec rc = rts_rec(a, b, k + 1, n * n);
#pragma unroll
        for (int r = 0; r < n; ++r) {
          double s = 0.0;  // A(r, c) = (G S_k)(r, c), S_k's column c still as loaded
#pragma unroll
          for (int kk = 0; kk < n; ++kk)
            if (DYN::gnz(r, kk)) s += Gk[r * n + kk] * in.S[LS::at(kk, c)];
          a.C[rc.off + (r * n + c) * rc.es] = bad ? NAN : e[r] + s;
        }
      }
#pragma unroll
      for (int r = 0; r <= c; ++r) {
        double s = 0.0;
#pragma unroll
        for (int l = 0; l < n; ++l) s += A[l * n + r] * e[l];
        in.S[LS::at(r, c)] += s;
      }
    }
#pragma unroll
    for (int i = 0; i < LS::size; ++i) Ss[i] = in.S[i];
    if (bad || !rts_finite<n>(xs, Ss)) {
      if constexpr (LAG) {
        if (!bad) {  // met only now: the record written above goes with the step
          const RtsRec rc = rts_rec(a, b, k + 1, n * n);
#pragma unroll
          for (int i = 0; i < n * n; ++i) a.C[rc.off + i * rc.es] = NAN;
        }
      }
      bad = true;
#pragma unroll
      for (int c = 0; c < n; ++c) xs[c] = NAN;
#pragma unroll
      for (int i = 0; i < LS::size; ++i) Ss[i] = NAN;
    }
    rts_store<n>(a, b, k, xs, Ss);
    in = nx;
  }
  if constexpr (LAG) {
    if (kmin == 0) {  // no prior: C_0 is not formed
      const RtsRec rc = rts_rec(a, b, 0, n * n);
#pragma unroll
      for (int i = 0; i < n * n; ++i) a.C[rc.off + i * rc.es] = NAN;
    }
  }
  if (a.status) a.status[b] = bad ? 1 : 0;
}

template <class DYN>
int launch_rts(const RtsLagArgs& g, hipStream_t st) {
  if (g.C) {
    hipLaunchKernelGGL((k_ekf_rts<DYN, true>), dim3((g.batch + 255) / 256), dim3(256), 0, st, g);
  } else {
    const RtsArgs& a = g;
    hipLaunchKernelGGL((k_ekf_rts<DYN>), dim3((a.batch + 255) / 256), dim3(256), 0, st, a);
  }
  return hipGetLastError() == hipSuccess ? MHE_OK : MHE_ERR_HIP;
}

// [p, p + np) and [q, q + nq) doubles share a byte
inline bool overlaps(const double* p, size_t np, const double* q, size_t nq) {
  return p && q && p < q + nq && q < p + np;
}

// mhe_ekf_smooth (C = nullptr) and mhe_ekf_smooth_args
int smooth(const mhe_ekf_dims* dims, int32_t batch, int32_t steps, const double* mu_hist, const double* S_hist,
           const double* U, int64_t u_bstride, const double* Q, const double* mu0, const double* S0, double* mu_s,
           double* S_s, double* mu0_s, double* S0_s, int32_t* status, double* C, void* stream) {
  if (!dims) return MHE_ERR_NULL;
  if (dims->struct_size != (int32_t)sizeof(mhe_ekf_dims)) return MHE_ERR_DIMS;  // stale / truncated binding
  if (batch < 0 || steps < 0) return MHE_ERR_DIMS;
  if (batch == 0 || steps == 0) return MHE_OK;
  int (*run)(const RtsLagArgs&, hipStream_t) = nullptr;
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
  if (!mu_hist || !S_hist || !U || !Q || !mu_s || !S_s) return MHE_ERR_NULL;
  if ((mu0_s || S0_s) && (!mu0 || !S0)) return MHE_ERR_NULL;
  if (C) {  // C is written while the inputs and the other outputs are still being read and written
    const size_t n = (size_t)dims->n, bt = (size_t)batch * (size_t)steps, nc = bt * n * n;
    const size_t nu = dims->in_batch_inner ? bt * (size_t)dims->m
                                           : (size_t)(batch - 1) * (size_t)u_bstride + (size_t)steps * (size_t)dims->m;
    if (overlaps(C, nc, mu_hist, bt * n) || overlaps(C, nc, S_hist, nc) || overlaps(C, nc, U, nu) ||
        overlaps(C, nc, Q, n * n) || overlaps(C, nc, mu0, batch * n) || overlaps(C, nc, S0, batch * n * n) ||
        overlaps(C, nc, mu_s, bt * n) || overlaps(C, nc, S_s, nc) || overlaps(C, nc, mu0_s, batch * n) ||
        overlaps(C, nc, S0_s, batch * n * n))
      return MHE_ERR_DIMS;
  }
  RtsLagArgs a = {};
  a.batch = batch; a.steps = steps; a.dt = dims->dt;
  for (int i = 0; i < 8; ++i) a.dp[i] = dims->dyn_par[i];
  a.mu_hist = mu_hist; a.S_hist = S_hist; a.U = U; a.u_bstride = u_bstride; a.es = 1; a.Q = Q;
  a.mu0 = mu0; a.S0 = S0; a.mu_s = mu_s; a.S_s = S_s; a.mu0_s = mu0_s; a.S0_s = S0_s; a.status = status;
  a.C = C;
  a.hist_bi = dims->hist_batch_inner != 0;
  if (dims->in_batch_inner) {  // U (steps, m, B)
    a.es = batch;
    a.u_bstride = 1;
  }
  return run(a, (hipStream_t)stream);
}

}  // namespace mhe_ekf

extern "C" int mhe_ekf_smooth(const mhe_ekf_dims* dims, int32_t batch, int32_t steps, const double* mu_hist,
                              const double* S_hist, const double* U, int64_t u_bstride, const double* Q,
                              const double* mu0, const double* S0, double* mu_s, double* S_s, double* mu0_s,
                              double* S0_s, int32_t* status, void* stream) {
  return mhe_ekf::smooth(dims, batch, steps, mu_hist, S_hist, U, u_bstride, Q, mu0, S0, mu_s, S_s, mu0_s, S0_s,
                         status, nullptr, stream);
}

extern "C" int mhe_ekf_smooth_args(const mhe_ekf_dims* dims, const mhe_ekf_lag_args* args, void* stream) {
  if (!dims || !args) return MHE_ERR_NULL;
  if (dims->struct_size != (int32_t)sizeof(mhe_ekf_dims)) return MHE_ERR_DIMS;  // stale / truncated binding
  if (args->struct_size != (int32_t)sizeof(mhe_ekf_lag_args)) return MHE_ERR_DIMS;
  return mhe_ekf::smooth(dims, args->batch, args->steps, args->mu_hist, args->S_hist, args->U, args->u_bstride,
                         args->Q, args->mu0, args->S0, args->mu_s, args->S_s, args->mu0_s, args->S0_s, args->status,
                         args->C, stream);
}

extern "C" int mhe_ekf_run_args(const mhe_ekf_dims* dims, const mhe_ekf_args* args, void* stream) {
  using namespace mhe_ekf;
  if (!dims || !args) return MHE_ERR_NULL;
  if (dims->struct_size != (int32_t)sizeof(mhe_ekf_dims)) return MHE_ERR_DIMS;  // stale / truncated binding
  if (args->struct_size != (int32_t)sizeof(mhe_ekf_args)) return MHE_ERR_DIMS;
  if (!(args->gate >= 0.0)) return MHE_ERR_DIMS;  // NaN or negative; 0 = no screening, +inf allowed
  const int32_t batch = args->batch, steps = args->steps;
  if (batch < 0 || steps < 0 || dims->pmax < 1 || dims->pmax > MAXP) return MHE_ERR_DIMS;
  if (batch == 0 || steps == 0) return MHE_OK;
  if (!args->mu || !args->S || !args->Q || !args->nz || !args->Z || !args->R || (dims->m > 0 && !args->U))
    return MHE_ERR_NULL;
  const double* PAR = args->PAR;
  // the instances without the screen and the statistics serve every call that asks for neither
  const bool gated = args->gate != 0.0 || args->nis || args->loglik || args->rej;
  EkfGateArgs a = {};
  a.batch = batch; a.steps = steps; a.nmeas_rows_max = dims->pmax; a.dt = dims->dt;
  a.mu = args->mu; a.S = args->S; a.U = args->U; a.u_bstride = args->u_bstride; a.Z = args->Z;
  a.z_bstride = args->z_bstride; a.nz = args->nz; a.nz_bstride = args->nz_bstride; a.PAR = PAR;
  a.par_bstride = args->par_bstride; a.Q = args->Q; a.R = args->R; a.r_bstride = args->r_bstride;
  a.r_sstride = args->r_sstride; a.mu_hist = args->mu_hist; a.S_hist = args->S_hist; a.status = args->status;
  a.gate = args->gate != 0.0 ? args->gate : INFINITY;
  a.nis = args->nis; a.loglik = args->loglik; a.rej = args->rej;
  a.hist_bi = dims->hist_batch_inner != 0;
  a.es = 1;
  if (dims->in_batch_inner) {  // U (steps, m, B), Z (steps, pmax, B), nz (steps, B), PAR (steps, pmax, q, B)
    a.es = batch;
    a.u_bstride = a.z_bstride = a.nz_bstride = a.par_bstride = 1;
  }
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < 8; ++i) a.dp[i] = dims->dyn_par[i];
  if (dims->q != 3) return MHE_ERR_DIMS;
  if (!PAR) return MHE_ERR_NULL;
  const bool rd = dims->r_diag != 0;
  if (dims->dyn_model == MHE_EKF_DYN_GNSS_POS_AND_BIAS) {
    if (dims->n != 5 || dims->m != 3) return MHE_ERR_MODEL;
    switch (dims->meas_model) {
      case MHE_EKF_MEAS_MULTI_PSEUDORANGE:
        return launch<EkfGnssPosAndBias, EkfMultiPseudorange<false>>(a, st, rd, gated);
      case MHE_EKF_MEAS_MULTI_PSEUDORANGE_AND_BIAS:
        return launch<EkfGnssPosAndBias, EkfMultiPseudorange<true>>(a, st, rd, gated);
    }
  } else if (dims->dyn_model == MHE_EKF_DYN_DISCRETE_VEHICLE) {
    if (dims->n != 9 || dims->m != 2) return MHE_ERR_MODEL;
    if (!(dims->dyn_par[2] != 0.0 && dims->dyn_par[5] != 0.0)) return MHE_ERR_DIMS;  // M, I_Z unset
    if (dims->meas_model == MHE_EKF_MEAS_VEHICLE_SENSORS)
      return launch<EkfDiscreteVehicle, EkfVehicleSensors>(a, st, rd, gated);
  }
  return MHE_ERR_MODEL;
}

extern "C" int mhe_ekf_run(const mhe_ekf_dims* dims, int32_t batch, int32_t steps, double* mu, double* S,
                           const double* U, int64_t u_bstride, const double* Z, int64_t z_bstride, const int32_t* nz,
                           int64_t nz_bstride, const double* PAR, int64_t par_bstride, const double* Q,
                           const double* R, int64_t r_bstride, int64_t r_sstride, double* mu_hist, double* S_hist,
                           int32_t* status, void* stream) {
  mhe_ekf_args g = {};  // gate 0 and no statistics output: the instances this entry always ran
  g.struct_size = (int32_t)sizeof(mhe_ekf_args);
  g.batch = batch; g.steps = steps; g.mu = mu; g.S = S; g.U = U; g.u_bstride = u_bstride; g.Z = Z;
  g.z_bstride = z_bstride; g.nz = nz; g.nz_bstride = nz_bstride; g.PAR = PAR; g.par_bstride = par_bstride; g.Q = Q;
  g.R = R; g.r_bstride = r_bstride; g.r_sstride = r_sstride; g.mu_hist = mu_hist; g.S_hist = S_hist;
  g.status = status;
  return mhe_ekf_run_args(dims, &g, stream);
}
