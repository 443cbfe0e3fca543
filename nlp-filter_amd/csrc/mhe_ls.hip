// libmhe: batched GNSS least-squares fixes for MI355X (gfx950).
//
// Replaces the per-epoch initialiser of kingdwd/nlp-filter:
//   iterativeLeastSquares     utils/leastsquares.py:19-42  position + clock bias,
//                             GN steps dx = pinv(G) drho, stop at ||dx|| < tol
//   iterativeLeastSquaresVel  utils/leastsquares.py:45-63  velocity + bias rate
//                             (one linear solve at the converged position)
//   runLeastSquares           utils/leastsquares.py:97-141 the per-epoch loop
// for many logs ("chains") at once.  ONE LANE PER TASK: a lane forms the geometry
// rows [-(s - x)/|s - x|, 1] and residuals of its epoch's satellites one after the
// other, accumulates the 4x4 normal equations G^T G dx = G^T drho in registers and
// solves them by a register Cholesky.
// For full-column-rank G this is the pinv(G) drho of the reference; results
// agree to rounding (tests state the tolerance).
//
// warm = 1 reproduces the reference's warm start: the default argument x of
// iterativeLeastSquares is one shared array that every call updates in place,
// so epoch k starts from epoch k-1's fix (b restarts at 0 every call) -- one
// lane walks its chain's epochs in order.  warm = 0 solves every epoch
// independently from x_init (one lane per epoch: all epochs in parallel).
//
// k_ls_multi (mhe_ls_multi_run) is the multi-epoch fix of a stationary receiver:
//   iterativeLeastSquares_multiTimeStep  utils/leastsquares.py:66-94
//   runBatchLeastSquares                 utils/leastsquares.py:144-169
// one x, b0, alpha over ALL rows of a log (hundreds to thousands).  There A GROUP OF
// G LANES OWNS ONE LOG (G = 16: a DPP row, four logs per wave; G = 64: a wave): the
// lanes stride over the rows, sum the 5x5 normal equations across the group by DPP /
// v_permlane swaps, and every lane solves the same system.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mhe.h"
#include "mhe_wave.h"

namespace mhe {
int g_opt_lsm_group = 0;  // mhe_set_option(MHE_OPT_LSM_GROUP): 16 / 64 force k_ls_multi's instance
}

namespace mhe_ls {

struct LsArgs {
  int chains, epochs, slots, max_iter, warm, with_vel;
  double tol;
  const double *sat_pos, *pr, *sat_vel, *pr_rate, *x_init;
  const int32_t* nsat;
  double *x_out, *b_out, *v_out, *bd_out, *x_last;
  int32_t* iters;
};

// Solve the 4x4 SPD system A s = v (A packed upper: 00 01 02 03 11 12 13 22 23 33).
// Returns false on a non-positive pivot (fewer than 4 independent rows).
__device__ bool solve4(const double* A, const double* v, double* s) {
  double L[4][4] = {};
  const int id[4][4] = {{0, 1, 2, 3}, {1, 4, 5, 6}, {2, 5, 7, 8}, {3, 6, 8, 9}};
  for (int j = 0; j < 4; ++j) {
    double d = A[id[j][j]];
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    if (!(d > 0.0)) return false;
    L[j][j] = sqrt(d);
    for (int i = j + 1; i < 4; ++i) {
      double t = A[id[i][j]];
      for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
      L[i][j] = t / L[j][j];
    }
  }
  double y[4];
  for (int i = 0; i < 4; ++i) {
    double t = v[i];
    for (int k = 0; k < i; ++k) t -= L[i][k] * y[k];
    y[i] = t / L[i][i];
  }
  for (int i = 3; i >= 0; --i) {
    double t = y[i];
    for (int k = i + 1; k < 4; ++k) t -= L[k][i] * s[k];
    s[i] = t / L[i][i];
  }
  return true;
}

// One task per LANE: a lane walks its log's epochs (warm) or solves one epoch,
// accumulating the 4x4 normal equations of its satellite rows sequentially in
// registers -- no cross-lane reductions, 64 tasks per wavefront.
__device__ __forceinline__ void row_geom(double sp0, double sp1, double sp2, double x0, double x1, double x2,
                                         double g[4], double& nrm) {
  const double l0 = sp0 - x0, l1 = sp1 - x1, l2 = sp2 - x2;
  nrm = sqrt(l0 * l0 + l1 * l1 + l2 * l2);
  g[0] = -l0 / nrm; g[1] = -l1 / nrm; g[2] = -l2 / nrm; g[3] = 1.0;
}

__device__ __forceinline__ void accum(double A[10], double v[4], const double g[4], double r) {
  int t = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = i; j < 4; ++j) A[t++] += g[i] * g[j];
    v[i] += g[i] * r;
  }
}

__global__ __launch_bounds__(256) void k_ls(LsArgs a) {
  const int task = blockIdx.x * blockDim.x + threadIdx.x;
  const int ntask = a.warm ? a.chains : a.chains * a.epochs;
  if (task >= ntask) return;
  const int c = a.warm ? task : task / a.epochs;
  const int k0 = a.warm ? 0 : task % a.epochs;
  const int k1 = a.warm ? a.epochs : k0 + 1;
  double x0 = a.x_init[3 * c], x1 = a.x_init[3 * c + 1], x2 = a.x_init[3 * c + 2];
  for (int k = k0; k < k1; ++k) {
    const size_t e = (size_t)c * a.epochs + k;
    const int ns = min((int)a.nsat[e], a.slots);  // slots beyond the layout are never read
    const double* S = a.sat_pos + e * a.slots * 3;
    const double* PR = a.pr + e * a.slots;
    double b = 0.0;
    int it = 0;
    // fewer than 4 rows cannot fix 4 unknowns: flagged (a rank-deficient G^T G would
    // otherwise leave the last pivot at rounding level, of either sign)
    bool ok = ns >= 4;
    for (int i = 0; i < a.max_iter && ok; ++i) {
      double A[10] = {}, v[4] = {};
      for (int q = 0; q < ns; ++q) {
        double g[4], nrm;
        row_geom(S[3 * q], S[3 * q + 1], S[3 * q + 2], x0, x1, x2, g, nrm);
        accum(A, v, g, PR[q] - nrm - b);
      }
      double dx[4];
      if (!solve4(A, v, dx)) {
        ok = false;
        break;
      }
      x0 += dx[0]; x1 += dx[1]; x2 += dx[2];
      b += dx[3];
      ++it;
      if (sqrt(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2] + dx[3] * dx[3]) < a.tol) break;
    }
    a.x_out[e * 3] = x0; a.x_out[e * 3 + 1] = x1; a.x_out[e * 3 + 2] = x2;
    a.b_out[e] = b;
    a.iters[e] = ok ? it : -1;
    if (a.with_vel) {  // utils/leastsquares.py:45-63 at the fix just computed
      const double* V = a.sat_vel + e * a.slots * 3;
      const double* RR = a.pr_rate + e * a.slots;
      double A[10] = {}, v[4] = {};
      for (int q = 0; q < ns; ++q) {
        double g[4], nrm;
        row_geom(S[3 * q], S[3 * q + 1], S[3 * q + 2], x0, x1, x2, g, nrm);
        accum(A, v, g, RR[q] - (V[3 * q] * -g[0] + V[3 * q + 1] * -g[1] + V[3 * q + 2] * -g[2]));
      }
      // a singular velocity system leaves v / bd NaN; iters keeps the position fix's
      // count (velocity failure is told apart from position failure by the NaN)
      double sv[4] = {NAN, NAN, NAN, NAN};
      if (ns >= 4) (void)solve4(A, v, sv);  // sv untouched (NaN) when singular
      a.v_out[e * 3] = sv[0]; a.v_out[e * 3 + 1] = sv[1]; a.v_out[e * 3 + 2] = sv[2];
      a.bd_out[e] = sv[3];
    }
  }
  if (a.warm && a.x_last) {
    a.x_last[3 * c] = x0; a.x_last[3 * c + 1] = x1; a.x_last[3 * c + 2] = x2;
  }
}

}  // namespace mhe_ls

extern "C" int mhe_ls_run(const mhe_ls_dims* dims, int32_t chains, int32_t epochs, const double* sat_pos,
                          const double* pr, const int32_t* nsat, const double* sat_vel, const double* pr_rate,
                          const double* x_init, double* x_out, double* b_out, double* v_out, double* bd_out,
                          int32_t* iters_out, double* x_last, void* stream) {
  using namespace mhe_ls;
  if (!dims) return MHE_ERR_NULL;
  if (dims->struct_size != (int32_t)sizeof(mhe_ls_dims)) return MHE_ERR_DIMS;  // stale / truncated binding
  if (chains < 0 || epochs < 0 || dims->slots < 1 || dims->slots > 64 || dims->max_iter < 0 ||
      !(dims->tol >= 0.0))
    return MHE_ERR_DIMS;
  if (chains == 0 || epochs == 0) return MHE_OK;
  if (!sat_pos || !pr || !nsat || !x_init || !x_out || !b_out || !iters_out) return MHE_ERR_NULL;
  if (dims->with_vel && (!sat_vel || !pr_rate || !v_out || !bd_out)) return MHE_ERR_NULL;
  LsArgs a = {};
  a.chains = chains; a.epochs = epochs; a.slots = dims->slots; a.max_iter = dims->max_iter;
  a.warm = dims->warm ? 1 : 0; a.with_vel = dims->with_vel ? 1 : 0; a.tol = dims->tol;
  a.sat_pos = sat_pos; a.pr = pr; a.nsat = nsat; a.sat_vel = sat_vel; a.pr_rate = pr_rate; a.x_init = x_init;
  a.x_out = x_out; a.b_out = b_out; a.v_out = v_out; a.bd_out = bd_out; a.iters = iters_out; a.x_last = x_last;
  const long long ntask = a.warm ? (long long)chains : (long long)chains * epochs;
  const int blocks = (int)((ntask + 255) / 256);
  hipLaunchKernelGGL(k_ls, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? MHE_OK : MHE_ERR_HIP;
}

// ---------------------------------------------------------------------------
// Multi-epoch fix: one position, bias and drift over all rows of a log.
namespace mhe_lsm {

constexpr int BLOCK = 256;
// Logs whose row capacity is at most this run on 16-lane groups, longer ones on a whole
// wave.  Measured: with 16384 logs and more, 16 lanes are 4x faster at 55
// rows and 1.5x at 326, the two are level at 652 and 64 lanes are ahead beyond; with 256 logs or fewer
// 64 lanes are always ahead (tens of microseconds below this size).  The choice is a
// function of the row capacity alone -- never of the number of logs -- so a log's result
// is bitwise the same alone or inside any batch.
constexpr int G16_MAX_ROWS = 512;

struct LsmArgs {
  int chains, row_cap, max_iter;
  double tol;
  const double *sat_pos, *pr, *t, *p_init;
  const int32_t* nrows;
  double* p_out;
  int32_t* iters;
};

// Sum / max over the G lanes of a group in a fixed order; every lane ends with the same bits.
template <int G>
__device__ __forceinline__ double group_sum(double v) {
  if constexpr (G == 64) {
    return mhe::wave_sum(v);
  } else {
    v += mhe::dpp_d<0xB1>(v);   // quad_perm [1,0,3,2]
    v += mhe::dpp_d<0x4E>(v);   // quad_perm [2,3,0,1]
    v += mhe::dpp_d<0x141>(v);  // row_half_mirror
    v += mhe::dpp_d<0x140>(v);  // row_mirror
    return v;
  }
}

template <int G>
__device__ __forceinline__ double group_max(double v) {
  v = fmax(v, mhe::dpp_d<0xB1>(v));
  v = fmax(v, mhe::dpp_d<0x4E>(v));
  v = fmax(v, mhe::dpp_d<0x141>(v));
  v = fmax(v, mhe::dpp_d<0x140>(v));
  if constexpr (G == 64) {
    v = mhe::pair_combine<1, true>(v);
    v = mhe::pair_combine<2, true>(v);
  }
  return v;
}

// packed upper 5x5: 00 01 02 03 04 11 12 13 14 22 23 24 33 34 44
__host__ __device__ constexpr int pk5(int i, int j) {
  return i <= j ? i * 5 - i * (i - 1) / 2 + (j - i) : j * 5 - j * (j - 1) / 2 + (i - j);
}

// Solve the 5x5 SPD system A s = v by a register Cholesky (solve4's scheme).
// Returns false on a non-positive pivot.
__device__ __forceinline__ bool solve5(const double (&A)[15], const double (&v)[5], double (&s)[5]) {
  double L[5][5] = {};
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    double d = A[pk5(j, j)];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    if (!(d > 0.0)) return false;
    L[j][j] = sqrt(d);
#pragma unroll
    for (int i = j + 1; i < 5; ++i) {
      double t = A[pk5(i, j)];
#pragma unroll
      for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
      L[i][j] = t / L[j][j];
    }
  }
  double y[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    double t = v[i];
#pragma unroll
    for (int k = 0; k < i; ++k) t -= L[i][k] * y[k];
    y[i] = t / L[i][i];
  }
#pragma unroll
  for (int i = 4; i >= 0; --i) {
    double t = y[i];
#pragma unroll
    for (int k = i + 1; k < 5; ++k) t -= L[k][i] * s[k];
    s[i] = t / L[i][i];
  }
  return true;
}

// G lanes per log, BLOCK / G logs per workgroup; groups never talk to each other (no
// LDS, no barrier, no atomics).  Lane l of a group takes rows l, l + G, ... (coalesced),
// keeps the 15 + 5 partial sums of G^T G and G^T drho in registers, the group sums them
// in a fixed order, and every lane solves the same 5x5 system -- nothing is broadcast.
// K = 0: the rows are read again every iteration (a log of 326 rows is 13 KB).  K > 0: the
// log has at most G * K rows and a lane holds its K rows in registers across the iterations;
// same operations in the same order, so the same bits as K = 0.
template <int G, int K>
__global__ __launch_bounds__(BLOCK) void k_ls_multi(LsmArgs a) {
  const int gl = threadIdx.x & (G - 1);
  const long long c = (long long)blockIdx.x * (BLOCK / G) + threadIdx.x / G;
  if (c >= a.chains) return;  // a whole group (one DPP row / one wave) leaves together
  const int n = min(max((int)a.nrows[c], 0), a.row_cap);  // rows beyond the layout are never read
  const double* S = a.sat_pos + (size_t)c * a.row_cap * 3;
  const double* PR = a.pr + (size_t)c * a.row_cap;
  const double* TT = a.t + (size_t)c * a.row_cap;
  double p[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) p[i] = a.p_init[c * 5 + i];

  // fewer than 5 rows cannot fix 5 unknowns, and rows that all share one t leave the 1
  // and t columns parallel: the last pivot would sit at rounding level, of either sign
  double tmax = -INFINITY, tmin_neg = -INFINITY;
  for (int r = gl; r < n; r += G) {
    const double tt = TT[r];
    tmax = fmax(tmax, tt);
    tmin_neg = fmax(tmin_neg, -tt);
  }
  tmax = group_max<G>(tmax);
  tmin_neg = group_max<G>(tmin_neg);
  bool ok = n >= 5 && tmax > -tmin_neg;

  double held[K > 0 ? K : 1][5] = {};  // K > 0: sat_pos (3), pr, t of rows gl, gl + G, ...
  if constexpr (K > 0) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const int r = gl + j * G;
      if (r < n) {
        held[j][0] = S[3 * r]; held[j][1] = S[3 * r + 1]; held[j][2] = S[3 * r + 2];
        held[j][3] = PR[r]; held[j][4] = TT[r];
      }
    }
  }

  int it = 0;
  for (int i = 0; i < a.max_iter && ok; ++i) {
    double A[15] = {}, v[5] = {};
    auto add_row = [&](double s0, double s1, double s2, double prv, double tt) {
      const double l0 = s0 - p[0], l1 = s1 - p[1], l2 = s2 - p[2];
      const double nrm = sqrt(l0 * l0 + l1 * l1 + l2 * l2);
      const double g[5] = {-l0 / nrm, -l1 / nrm, -l2 / nrm, 1.0, tt};
      const double res = prv - nrm - p[3] - p[4] * tt;
#pragma unroll
      for (int x = 0; x < 5; ++x) {
#pragma unroll
        for (int y = x; y < 5; ++y) A[pk5(x, y)] += g[x] * g[y];
        v[x] += g[x] * res;
      }
    };
    if constexpr (K > 0) {
#pragma unroll
      for (int j = 0; j < K; ++j)
        if (gl + j * G < n) add_row(held[j][0], held[j][1], held[j][2], held[j][3], held[j][4]);
    } else {
      for (int r = gl; r < n; r += G) add_row(S[3 * r], S[3 * r + 1], S[3 * r + 2], PR[r], TT[r]);
    }
#pragma unroll
    for (int q = 0; q < 15; ++q) A[q] = group_sum<G>(A[q]);
#pragma unroll
    for (int q = 0; q < 5; ++q) v[q] = group_sum<G>(v[q]);
    double dx[5];
    if (!solve5(A, v, dx)) {
      ok = false;
      break;
    }
    double s2 = 0.0;
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      p[q] += dx[q];
      s2 += dx[q] * dx[q];
    }
    ++it;
    if (sqrt(s2) < a.tol) break;
  }
  if (gl == 0) {
#pragma unroll
    for (int i = 0; i < 5; ++i) a.p_out[c * 5 + i] = p[i];
    a.iters[c] = ok ? it : -1;
  }
}

inline int group_for(int row_cap) {
  if (mhe::g_opt_lsm_group) return mhe::g_opt_lsm_group;
  return row_cap <= G16_MAX_ROWS ? 16 : 64;
}

// Rows a lane of the 16-lane instance holds in registers: logs of at most 16 * HOLD_ROWS rows
// (a few epochs) are read once instead of once per iteration.
constexpr int HOLD_ROWS = 4;

}  // namespace mhe_lsm

extern "C" int32_t mhe_ls_multi_group(int32_t row_cap) {
  return row_cap < 0 ? MHE_ERR_DIMS : mhe_lsm::group_for(row_cap);
}

extern "C" int mhe_ls_multi_run(const mhe_lsm_dims* dims, int32_t chains, int32_t row_cap, const double* sat_pos,
                                const double* pr, const double* t, const int32_t* nrows, const double* p_init,
                                double* p_out, int32_t* iters_out, void* stream) {
  using namespace mhe_lsm;
  if (!dims) return MHE_ERR_NULL;
  if (dims->struct_size != (int32_t)sizeof(mhe_lsm_dims)) return MHE_ERR_DIMS;  // stale / truncated binding
  if (chains < 0 || row_cap < 0 || dims->max_iter < 0 || !(dims->tol >= 0.0)) return MHE_ERR_DIMS;
  if (chains == 0) return MHE_OK;
  if (!nrows || !p_init || !p_out || !iters_out) return MHE_ERR_NULL;
  if (row_cap > 0 && (!sat_pos || !pr || !t)) return MHE_ERR_NULL;
  LsmArgs a = {};
  a.chains = chains; a.row_cap = row_cap; a.max_iter = dims->max_iter; a.tol = dims->tol;
  a.sat_pos = sat_pos; a.pr = pr; a.t = t; a.nrows = nrows; a.p_init = p_init;
  a.p_out = p_out; a.iters = iters_out;
  const int G = group_for(row_cap);
  const int blocks = (int)(((long long)chains + BLOCK / G - 1) / (BLOCK / G));
  if (G == 16 && row_cap <= 16 * HOLD_ROWS)
    hipLaunchKernelGGL((k_ls_multi<16, HOLD_ROWS>), dim3(blocks), dim3(BLOCK), 0, (hipStream_t)stream, a);
  else if (G == 16)
    hipLaunchKernelGGL((k_ls_multi<16, 0>), dim3(blocks), dim3(BLOCK), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL((k_ls_multi<64, 0>), dim3(blocks), dim3(BLOCK), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? MHE_OK : MHE_ERR_HIP;
}
