// libmhe: batched collocation Gauss-Newton for MI355X (gfx950, CDNA4) -- the C-ABI
// (include/mhe.h), argument checks, constants building and dispatch to the
// per-pair launch templates (mhe_launch.h, pair_*.hip).
//
// What replaces what (reference kingdwd/nlp-filter):
//   fixedTimeOptimalEstimationNLP objective   nlp/nlp.py:202-286
//   NLP.solve() -> CasADi/IPOPT               nlp/nlp.py:61-83
// is re-built here as ONE fused kernel per batch: one workgroup (8 waves) per
// trajectory runs the whole Gauss-Newton loop
//     residual + Jacobian  ->  J^T W J, J^T W r  ->  Cholesky  ->  2 triangular
//     solves  ->  X += delta  ->  convergence test
// with the d x d normal matrix (d = (N+1) n, padded to 16*NT) held in the MFMA
// accumulator registers of the 8 waves as 16x16 fp64 tiles (off-diagonal tiles,
// 2 KB per tile, 8 VGPRs per lane; diagonal tiles in LDS).  The right-looking blocked Cholesky
// factors one 16-column panel per step in registers (row-per-lane sweep with
// scalar broadcasts), streams the panel through LDS and applies the trailing
// update with v_mfma_f64_16x16x4f64.  The forward solve rides along with the
// panel sweep (augmented column); the backward solve reads L straight from the
// tile registers.  Trajectories are independent: no inter-workgroup traffic.
//
// See DESIGN.md for the data layout, the roofline and the measurements.
#include <cstdio>
#include <string.h>

#include "mhe_core.h"

namespace mhe {

// ------------------------------------------------------------ register-path constants
__global__ void k_copy_consts(int P, int M, int n, int p, int NT, const double* D, const double* cw,
                              const double* Phi, const double* Qw, const double* Rw, const double* Pw,
                              char* cbuf) {
  const ConstLayout CL = const_layout(P, M, n, p, NT);
  double* oD = (double*)(cbuf + CL.D);
  double* oDt = (double*)(cbuf + CL.Dt);
  double* oPhi = (double*)(cbuf + CL.Phi);
  double* oPhiT = (double*)(cbuf + CL.PhiT);
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int stride = gridDim.x * blockDim.x;
  for (int e = gid; e < P * P; e += stride) {
    const int k = e / P, j = e % P;
    oD[e] = D[e];
    oDt[j * P + k] = D[e];
  }
  for (int e = gid; e < M * P; e += stride) {
    const int i = e / P, j = e % P;
    oPhi[e] = Phi[e];
    oPhiT[j * M + i] = Phi[e];
  }
  for (int e = gid; e < P; e += stride) ((double*)(cbuf + CL.cw))[e] = cw[e];
  for (int e = gid; e < n * n; e += stride) {
    ((double*)(cbuf + CL.Qw))[e] = Qw[e];
    ((double*)(cbuf + CL.Pw))[e] = Pw ? Pw[e] : 0.0;
  }
  for (int e = gid; e < M * p * p; e += stride) ((double*)(cbuf + CL.Rw))[e] = Rw[e];
  // The mat-vec streams (const_layout): what lane `lane` of wave w reads as its element u / v.
  // Padding rows hold the clamped row's values, as the clamped index read from the tables.
  double* oN = (double*)(cbuf + CL.NMS);
  for (int e = gid; e < NW * CL.nmu * 64; e += stride) {
    const int lane = e & 63, u = (e >> 6) % CL.nmu, w = (e >> 6) / CL.nmu;
    const int j = (lane >> 4) + TPR * u, r = 16 * w + (lane & 15);
    const int kk = r < P ? r : P - 1, ii = r < M ? r : M - 1;
    oN[2 * e] = j < P ? D[kk * P + j] : 0.0;                 // Dt[j][kk]
    oN[2 * e + 1] = j < P && M > 0 ? Phi[ii * P + j] : 0.0;  // PhiT[j][ii]
  }
  double* oG = (double*)(cbuf + CL.GRS);
  for (int e = gid; e < grs_passes(P) * NW * CL.grv * 64; e += stride) {
    const int lane = e & 63, v = (e >> 6) % CL.grv, pw = (e >> 6) / CL.grv;  // pw = NW pass + wave
    const int q = lane >> 4, node = 16 * pw + (lane & 15), jj = node < P ? node : P - 1;
    const bool phi = q >= TPR / 2;
    const double* T = phi ? Phi : D;
    const int len = phi ? M : P, k0 = q % (TPR / 2) + 4 * v, k1 = k0 + 2;
    oG[2 * e] = k0 < len ? T[k0 * P + jj] : 0.0;
    oG[2 * e + 1] = k1 < len ? T[k1 * P + jj] : 0.0;
  }
}

// ------------------------------------------------------------ large-system path (mhe_big.h)
// Every trajectory starts RUNNING -- or, when the constants buffer's stamp does not
// match these dims, BAD_CONSTANTS: then no kernel of the solve touches the constants
// (X_out keeps X0, cost NaN).
__global__ void k_big_init(BigArgs a, int batch) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < batch) {
    const bool ok = *(const unsigned long long*)a.cbuf == a.tag;
    a.state[b] = ok ? BIG_RUNNING : MHE_STATUS_BAD_CONSTANTS;
    a.iters[b] = 0;
    if (!ok) a.cost[b] = NAN;
  }
}

__global__ void k_big_finish(int batch, int* state) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < batch && state[b] == BIG_RUNNING) state[b] = MHE_STATUS_MAX_ITER;
}

// ------------------------------------------------------------ constants
__global__ void k_big_consts(int P, int M, int n, int p, const double* D, const double* cw, const double* Qw,
                             const double* Rw, const double* Pw, char* cbuf) {
  const BigConst CL = big_const_layout(P, M, n, p);
  const int gid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  double* oD = (double*)(cbuf + CL.D);
  double* oDt = (double*)(cbuf + CL.Dt);
  double* oDCD = (double*)(cbuf + CL.DCD);
  for (int e = gid; e < P * P; e += stride) {
    const int k = e / P, j = e % P;
    oD[e] = D[e];
    oDt[j * P + k] = D[e];
    // (D^T C D)[k][j] with C = diag(cw): element (row k, col j), formed in the same order
    // for (k, j) and (j, k) -- exactly symmetric, so k_big_assemble may read either
    const int lo = k < j ? k : j, hi = k < j ? j : k;
    double s = 0.0;
    for (int t = 0; t < P; ++t) s += D[t * P + lo] * cw[t] * D[t * P + hi];
    oDCD[e] = s;
  }
  for (int e = gid; e < P; e += stride) ((double*)(cbuf + CL.cw))[e] = cw[e];
  for (int e = gid; e < n * n; e += stride) {
    ((double*)(cbuf + CL.Qw))[e] = Qw[e];
    ((double*)(cbuf + CL.Pw))[e] = Pw ? Pw[e] : 0.0;
  }
  for (int e = gid; e < M * p * p; e += stride) ((double*)(cbuf + CL.Rw))[e] = Rw[e];
}

// equality-constraint index pairs, passed by value (kernel arguments) so that
// building constants stays a pure stream-ordered enqueue
struct EqPairs {
  int v[2 * MHE_MAX_EQ];
  double r[MHE_MAX_EQ];
};
__global__ void k_big_eq_consts(int P, int M, int n, int p, int nc, EqPairs e, char* cbuf) {
  const BigConst CL = big_const_layout(P, M, n, p, nc);
  int* o = (int*)(cbuf + CL.eq);
  double* orr = (double*)(cbuf + CL.eqr);
  for (int i = threadIdx.x; i < 2 * nc; i += blockDim.x) o[i] = e.v[i];
  for (int i = threadIdx.x; i < nc; i += blockDim.x) orr[i] = e.r[i];
}

// epoch detection: row i starts an epoch unless its Phi row equals row i-1 bitwise
__global__ void k_big_epoch_flags(int P, int M, int n, int p, const double* Phi, char* cbuf) {
  const BigConst CL = big_const_layout(P, M, n, p);
  int* flag = (int*)(cbuf + CL.flag);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += gridDim.x * blockDim.x) {
    int f = (i == 0);
    if (!f)
      for (int j = 0; j < P; ++j)
        if (__double_as_longlong(Phi[(size_t)i * P + j]) != __double_as_longlong(Phi[(size_t)(i - 1) * P + j])) {
          f = 1;
          break;
        }
    flag[i] = f;
  }
}

__global__ void k_big_epoch_scan(int P, int M, int n, int p, char* cbuf) {
  const BigConst CL = big_const_layout(P, M, n, p);
  const int* flag = (const int*)(cbuf + CL.flag);
  int* erow = (int*)(cbuf + CL.erow);
  int E = 0;
  for (int i = 0; i < M; ++i)
    if (flag[i]) erow[E++] = i;
  erow[E] = M;
  *(int*)(cbuf + CL.ne) = E;
}

__global__ void k_big_epoch_rows(int P, int M, int n, int p, const double* Phi, char* cbuf) {
  const BigConst CL = big_const_layout(P, M, n, p);
  const int* erow = (const int*)(cbuf + CL.erow);
  const int E = *(const int*)(cbuf + CL.ne);
  double* PhiE = (double*)(cbuf + CL.PhiE);
  double* PhiET = (double*)(cbuf + CL.PhiET);
  const int Mr = M > 0 ? M : 1;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < E * P; t += gridDim.x * blockDim.x) {
    const int e = t / P, j = t % P;
    const double v = Phi[(size_t)erow[e] * P + j];
    PhiE[(size_t)e * P + j] = v;
    PhiET[(size_t)j * Mr + e] = v;
  }
}

// ------------------------------------------------------------ fused-general constants (mhe_general.h)
// D, D^T, the weights and the equality rows (the tile tables come from k_build_cc)
__global__ void k_fg_consts(int P, int M, int n, int NT, int nc, EqPairs eqp, const double* D, const double* cw,
                            const double* Qw, const double* Rw, const double* Pw, char* cbuf) {
  const FgConst FC = fg_const_layout(P, M, n, NT, nc);
  const ConstLayout& CL = FC.C;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  double* oD = (double*)(cbuf + CL.D);
  double* oDt = (double*)(cbuf + CL.Dt);
  for (int e = gid; e < P * P; e += stride) {
    const int k = e / P, j = e % P;
    oD[e] = D[e];
    oDt[j * P + k] = D[e];
  }
  for (int e = gid; e < P; e += stride) ((double*)(cbuf + CL.cw))[e] = cw[e];
  for (int e = gid; e < n * n; e += stride) {
    ((double*)(cbuf + CL.Qw))[e] = Qw[e];
    ((double*)(cbuf + CL.Pw))[e] = Pw ? Pw[e] : 0.0;
  }
  for (int e = gid; e < M; e += stride) ((double*)(cbuf + CL.Rw))[e] = Rw[e];
  for (int e = gid; e < 2 * nc; e += stride) ((int*)(cbuf + FC.eq))[e] = eqp.v[e];
  for (int e = gid; e < nc; e += stride) ((double*)(cbuf + FC.eqr))[e] = eqp.r[e];
}

// Epochs as the large path detects them (row i starts one unless its Phi row equals row
// i - 1 bitwise), the epoch rows Phi_E / Phi_E^T and the row -> epoch map; one workgroup.
__global__ void k_fg_epochs(int P, int M, int n, int NT, int nc, const double* Phi, char* cbuf) {
  const FgConst FC = fg_const_layout(P, M, n, NT, nc);
  int* flag = (int*)(cbuf + FC.flag);
  int* erow = (int*)(cbuf + FC.erow);
  int* rowe = (int*)(cbuf + FC.rowe);
  double* PhiE = (double*)(cbuf + FC.C.Phi);
  double* PhiET = (double*)(cbuf + FC.C.PhiT);
  for (int i = threadIdx.x; i < M; i += blockDim.x) {
    int f = (i == 0);
    if (!f)
      for (int j = 0; j < P; ++j)
        if (__double_as_longlong(Phi[(size_t)i * P + j]) != __double_as_longlong(Phi[(size_t)(i - 1) * P + j])) {
          f = 1;
          break;
        }
    flag[i] = f;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int E = 0;
    for (int i = 0; i < M; ++i) {
      if (flag[i]) erow[E++] = i;
      rowe[i] = E - 1;
    }
    erow[E] = M;
    *(int*)(cbuf + FC.ne) = E;
  }
  __syncthreads();
  const int E = *(const int*)(cbuf + FC.ne);
  for (int t = threadIdx.x; t < M * P; t += blockDim.x) {
    const int e = t / P, j = t % P;
    const double v = e < E ? Phi[(size_t)erow[e] * P + j] : 0.0;
    PhiE[(size_t)e * P + j] = v;
    PhiET[(size_t)j * M + e] = v;
  }
}

__global__ void k_write_tag(unsigned long long* p, unsigned long long tag) { *p = tag; }

int g_opt_big_right_looking = 0;
int g_opt_smem_pad = 0;

}  // namespace mhe

// ================================================================ dispatch
using namespace mhe;

#ifdef MHE_DIAG
static unsigned long long* g_dbg = nullptr;
#endif

namespace {

// The (dynamics, measurement) pairs compiled into this library (mhe/registry.py
// COMPILED_PAIRS mirrors this list).
const PairOps* find_pair(const mhe_dims* dm) {
  const PairOps* ops = pairs_vdp(dm->dyn_model, dm->meas_model);
#ifndef MHE_FAST_BUILD  // -DMHE_FAST_BUILD: van der Pol only (kernel development)
  if (!ops) ops = pairs_integrators(dm->dyn_model, dm->meas_model);
  if (!ops) ops = pairs_gnss(dm->dyn_model, dm->meas_model);
  if (!ops) ops = pairs_vehicles(dm->dyn_model, dm->meas_model);
  if (!ops) ops = pairs_autocar(dm->dyn_model, dm->meas_model);
  if (!ops) ops = pairs_receivers(dm->dyn_model, dm->meas_model);
#endif
  return ops;
}

// Every entry point validates the caller's struct first: struct_size must be
// sizeof(mhe_dims) of this build, so a binding that declares an older or truncated
// struct gets MHE_ERR_DIMS before any field past struct_size is read.
int check_dims(const mhe_dims* dm, int* NT_out) {
  if (!dm) return MHE_ERR_NULL;
  if (dm->struct_size != (int32_t)sizeof(mhe_dims)) return MHE_ERR_DIMS;
  int n, m, p, q;
  bool lin;
  if (!dyn_info(dm->dyn_model, n, m)) return MHE_ERR_MODEL;
  if (!meas_info(dm->meas_model, n, p, q, lin)) return MHE_ERR_MODEL;
  if (dm->n != n || dm->m != m || dm->p != p || dm->q != q) return MHE_ERR_DIMS;
  if (dm->N < 1 || dm->M < 0 || !(dm->T > 0.0)) return MHE_ERR_DIMS;
  if (dm->dyn_cost != MHE_COST_L2 && dm->dyn_cost != MHE_COST_HUBER) return MHE_ERR_MODEL;
  if (dm->dyn_cost == MHE_COST_HUBER && !(dm->huber_delta > 0.0)) return MHE_ERR_DIMS;
  if (dm->n_bounds < 0 || dm->n_bounds > 8) return MHE_ERR_DIMS;
  for (int i = 0; i < dm->n_bounds; ++i)
    if (dm->bound_idx[i] < 0 || dm->bound_idx[i] >= n || !(dm->bound_lb[i] <= dm->bound_ub[i])) return MHE_ERR_DIMS;
  if (dm->meas_model == MHE_MEAS_VEHICLE_PSEUDORANGE && dm->dyn_model != MHE_DYN_VEHICLE_GNSS) return MHE_ERR_DIMS;
  for (int i = 0; i < 4; ++i)
    if ((dm->meas_model == MHE_MEAS_PSEUDORANGE && (dm->meas_idx[i] < 0 || dm->meas_idx[i] >= n)) ||
        (dm->meas_model == MHE_MEAS_RANGE_3D && i < 3 && (dm->meas_idx[i] < 0 || dm->meas_idx[i] >= n)))
      return MHE_ERR_DIMS;
  const int P = dm->N + 1;
  if (dm->n_extra < 0 || dm->n_extra > MHE_MAX_EXTRA || dm->n_eq < 0 || dm->n_extra + dm->n_eq > MHE_MAX_EQ)
    return MHE_ERR_DIMS;
  if (dm->n_extra > 0 && dm->meas_model != MHE_MEAS_MIXED) return MHE_ERR_DIMS;  // z enters mixed rows only
  if (dm->n_eq > 0) {
    if (!dm->eq_idx) return MHE_ERR_NULL;
    for (int i = 0; i < dm->n_eq; ++i) {
      const int ia = dm->eq_idx[2 * i], ib = dm->eq_idx[2 * i + 1];
      if (ia < 0 || ia >= P * n || ib < -1 || ib >= P * n || ia == ib) return MHE_ERR_DIMS;
    }
  }
  if (dm->n_bounds > 0 && (dm->n_eq > 0 || dm->n_extra > 0)) return MHE_ERR_UNSUPPORTED;
  int NT = (P * n + 15) / 16;
  if (is_big(dm)) NT = n * big_pp(P) / 16;  // large-system path (mhe_big.h), component-major tiles
  if (NT_out) *NT_out = NT;
  return MHE_OK;
}

// bytes of the constants buffer: the 256-B header (layout stamp at offset 0) and the
// constants proper
size_t const_total_bytes(const mhe_dims* dm, int NT) {
  if (is_big(dm)) return big_const_layout(dm->N + 1, dm->M, dm->n, dm->p, dm->n_eq).total;
  if (fg_eligible(dm)) return fg_const_layout(dm->N + 1, dm->M, dm->n, NT, dm->n_eq).total;
  return const_layout(dm->N + 1, dm->M, dm->n, dm->p, NT).total;
}

// FNV-1a over the dims that define the constants' layout and contents, including the
// equality rows (eq_idx pairs and the bits of eq_rhs), which mhe_build_constants copies
// into the buffer: a solve whose dims carry other rows than the buffer was built with
// is refused (MHE_STATUS_BAD_CONSTANTS) instead of silently using the old rows.
unsigned long long const_tag(const mhe_dims* dm, int NT) {
  unsigned long long h = 1469598103934665603ull;
  auto mix = [&h](long long x) {
    h ^= (unsigned long long)x;
    h *= 1099511628211ull;
  };
  // the path bit: 0 register-resident, 1 large-system, 2 fused-general (k_gn_general's layout)
  // CONST_LAYOUT_REV and NW: a buffer laid out by a library with other tables, or with streams
  // for another wave count, is refused like one of other dims
  const long long v[] = {0x4D4845, is_big(dm) ? 1 : fg_eligible(dm) ? 2 : 0, dm->N, dm->n, dm->m, dm->p, dm->M, dm->q, dm->dyn_model,
                         dm->meas_model, dm->has_prior, dm->dyn_cost, NT, dm->n_eq, dm->n_extra, CONST_LAYOUT_REV, NW};
  for (long long x : v) mix(x);
  if (dm->n_eq > 0 && dm->eq_idx)  // check_dims has validated n_eq <= MHE_MAX_EQ and eq_idx
    for (int i = 0; i < 2 * dm->n_eq; ++i) mix(dm->eq_idx[i]);
  for (int i = 0; i < dm->n_eq; ++i) {  // NULL eq_rhs = all 0 (as the build); -0 and +0 alike
    const double r = (dm->eq_rhs ? dm->eq_rhs[i] : 0.0) + 0.0;
    long long bits;
    memcpy(&bits, &r, sizeof bits);
    mix(bits);
  }
  return h | 1ull;
}

// the equality rows of the dims as a kernel argument (NULL eq_rhs = all 0)
EqPairs eq_pairs(const mhe_dims* dm) {
  EqPairs e = {};
  for (int i = 0; i < 2 * dm->n_eq; ++i) e.v[i] = dm->eq_idx[i];
  for (int i = 0; i < dm->n_eq; ++i) e.r[i] = dm->eq_rhs ? dm->eq_rhs[i] : 0.0;
  return e;
}

// Constants of the large-system path: model-independent (D, D^T, D^T C D, weights,
// the epoch-compressed basis and the equality-constraint pairs).
int build_big_consts(const mhe_dims* dm, const double* D, const double* cw, const double* Phi, const double* Qw,
                     const double* Rw, const double* Pw, char* cbuf, hipStream_t st) {
  const int P = dm->N + 1;
  hipLaunchKernelGGL(k_big_consts, dim3(256), dim3(256), 0, st, P, dm->M, dm->n, dm->p, D, cw, Qw, Rw, Pw, cbuf);
  if (dm->M > 0) {
    hipLaunchKernelGGL(k_big_epoch_flags, dim3((dm->M + 255) / 256), dim3(256), 0, st, P, dm->M, dm->n, dm->p, Phi,
                       cbuf);
    hipLaunchKernelGGL(k_big_epoch_scan, dim3(1), dim3(1), 0, st, P, dm->M, dm->n, dm->p, cbuf);
    hipLaunchKernelGGL(k_big_epoch_rows, dim3(256), dim3(256), 0, st, P, dm->M, dm->n, dm->p, Phi, cbuf);
  }
  if (dm->n_eq > 0)
    hipLaunchKernelGGL(k_big_eq_consts, dim3(1), dim3(128), 0, st, P, dm->M, dm->n, dm->p, dm->n_eq, eq_pairs(dm),
                       cbuf);
  return hipGetLastError() == hipSuccess ? MHE_OK : MHE_ERR_HIP;
}

// The launch arguments both paths derive from the dims and the constants alone (GnArgs and
// BigArgs name them alike).
template <class A>
void set_dims(A& a, const mhe_dims* dm, const void* cbuf, int NT) {
  a.cbuf = (const char*)cbuf;
  a.P = dm->N + 1;
  a.M = dm->M;
  a.NT = NT;
  a.q = dm->q;
  a.has_prior = dm->has_prior;
  a.alpha = 2.0 / dm->T;
  a.huber_delta = dm->huber_delta;
  a.n_bounds = dm->n_bounds;
  a.tag = const_tag(dm, NT);
  for (int i = 0; i < 8; ++i) {
    a.idx[i] = dm->meas_idx[i];
    a.bidx[i] = dm->bound_idx[i];
    a.blb[i] = dm->bound_lb[i];
    a.bub[i] = dm->bound_ub[i];
    a.dpar[i] = dm->dyn_par[i];
  }
  a.nz = dm->n_extra;
  a.nc = dm->n_eq;
}

// The per-solve inputs of an operating point: the only place a launch struct takes them from
// mhe_solve_args (the iterate and the outputs are each call's own).
template <class A>
void set_point(A& a, const mhe_solve_args* at) {
  a.U = at->U; a.ustride = at->u_bstride; a.Y = at->Y; a.PAR = at->PAR; a.pstride = at->par_bstride; a.x0 = at->x0;
  a.Rw = at->Rw; a.rwstride = at->rw_bstride; a.md = at->meas_delta; a.mdstride = at->md_bstride;
  a.Pw = at->Pw; a.pwstride = at->pw_bstride;
}

GnArgs make_args(const mhe_dims* dm, const void* cbuf, int NT) {
  GnArgs a = {};
#ifdef MHE_DIAG
  a.dbg = g_dbg;
#endif
  set_dims(a, dm, cbuf, NT);
  a.d = a.P * dm->n;
  a.ntiles = NT * (NT + 1) / 2;
  return a;
}

// Constants of fused-general dims (fg_const_layout): the register path's tables, the epoch-
// compressed basis and the equality rows.  Phi with more distinct rows than the kernel's LDS
// layout holds (fg_epoch_cap) is refused -- the one host synchronisation of this build.
int build_fg_consts(const mhe_dims* dm, int NT, const PairOps* ops, const double* D, const double* cw,
                    const double* Phi, const double* Qw, const double* Rw, const double* Pw, char* cbuf,
                    hipStream_t st) {
  const int P = dm->N + 1;
  hipLaunchKernelGGL(k_fg_consts, dim3(64), dim3(256), 0, st, P, dm->M, dm->n, NT, dm->n_eq, eq_pairs(dm), D, cw, Qw,
                     Rw, Pw, cbuf);
  int rc = ops->build_cc(dm, NT, D, cw, Phi, Qw, Rw, Pw, cbuf, st);
  if (rc != MHE_OK) return rc;
  if (dm->M > 0) {
    hipLaunchKernelGGL(k_fg_epochs, dim3(1), dim3(256), 0, st, P, dm->M, dm->n, NT, dm->n_eq, Phi, cbuf);
    const FgConst FC = fg_const_layout(P, dm->M, dm->n, NT, dm->n_eq);
    int E = 0;
    if (hipMemcpyAsync(&E, cbuf + FC.ne, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return MHE_ERR_HIP;
    if (E > fg_epoch_cap(P, dm->M, dm->n, NT, dm->n_extra, dm->n_eq)) return MHE_ERR_UNSUPPORTED;
  }
  return hipGetLastError() == hipSuccess ? MHE_OK : MHE_ERR_HIP;
}

// The large-system path's launch arguments that follow from the dims and the
// constants / workspace alone (the per-solve pointers are set by the caller).
BigArgs make_big_args(const mhe_dims* dims, const void* cbuf, int NT, void* workspace) {
  BigArgs A = {};
  set_dims(A, dims, cbuf, NT);
  A.n = dims->n; A.Pp = big_pp(A.P); A.NTc = A.Pp / 16;
  A.ws = (double*)workspace; A.ws_stride = big_ws_doubles(dims, NT);
  A.huber = dims->dyn_cost == MHE_COST_HUBER;
  return A;
}

// The per-solve row inputs of mhe_solve_args: Rw needs a nonlinear measurement model (a
// linear h folds Rw into Cc), meas_delta also scalar rows (p = 1).
int check_row_args(const mhe_dims* dims, const double* Rw, const double* meas_delta) {
  if (!Rw && !meas_delta) return MHE_OK;
  int p, q;
  bool lin;
  meas_info(dims->meas_model, dims->n, p, q, lin);
  if (lin) return MHE_ERR_UNSUPPORTED;
  if (meas_delta && p != 1) return MHE_ERR_UNSUPPORTED;
  return MHE_OK;
}

// The per-solve prior weight of mhe_solve_args needs the addInitialCost term; on the register-
// resident path its block must lie inside diagonal tile 0 (n <= 16: every pair that path has).
int check_pw_arg(const mhe_dims* dims, const double* Pw) {
  if (!Pw) return MHE_OK;
  if (!dims->has_prior || (!is_big(dims) && dims->n > 16)) return MHE_ERR_UNSUPPORTED;
  return MHE_OK;
}

int check_rows(const mhe_dims* dims, const mhe_solve_args* at) {
  const int rc = check_row_args(dims, at->Rw, at->meas_delta);
  return rc != MHE_OK ? rc : check_pw_arg(dims, at->Pw);
}

// The header of a caller's mhe_solve_args, before any other field is read.  batch = false
// leaves the batch to check_point (the assemble calls answer for the row inputs first).
int check_header(const mhe_solve_args* at, bool batch = true) {
  if (!at) return MHE_ERR_NULL;
  if (at->struct_size != (int32_t)sizeof(mhe_solve_args)) return MHE_ERR_DIMS;
  return batch && at->batch < 0 ? MHE_ERR_DIMS : MHE_OK;
}

// An mhe_solve_args as an operating point of checked dims: the header, the inputs the dims
// require (Z0 only where the call reads it: need_z), the call's own pointers (outs_ok) and
// the per-solve row inputs and prior weight.  MHE_OK with at->batch == 0 means "nothing to
// do": the pointers of an empty batch are not looked at.  A call whose own checks come
// between the header and the pointers calls check_header first.
int check_point(const mhe_dims* dims, const void* const_buf, const mhe_solve_args* at, bool need_z, bool outs_ok) {
  const int rc = check_header(at);
  if (rc != MHE_OK || at->batch == 0) return rc;
  if (!const_buf || !at->X0 || !outs_ok || (dims->M > 0 && !at->Y) || (dims->m > 0 && !at->U) ||
      (dims->q > 0 && !at->PAR) || (dims->has_prior && !at->x0) || (need_z && !at->Z0))
    return MHE_ERR_NULL;
  return check_rows(dims, at);
}

// The positional entry points' arguments as an operating point (no per-solve row inputs).
mhe_solve_args pack_point(int32_t batch, const double* X, const double* Z, const double* U, int64_t u_bstride,
                          const double* Y, const double* PAR, int64_t par_bstride, const double* x0, void* workspace,
                          size_t workspace_bytes) {
  mhe_solve_args g = {};
  g.struct_size = (int32_t)sizeof(mhe_solve_args);
  g.batch = batch; g.X0 = X; g.Z0 = Z; g.U = U; g.u_bstride = u_bstride; g.Y = Y; g.PAR = PAR;
  g.par_bstride = par_bstride; g.x0 = x0; g.workspace = workspace; g.workspace_bytes = workspace_bytes;
  return g;
}

}  // namespace

// ------------------------------------------------------------ large-system parity I/O
// mhe_assemble_ws / mhe_chol_solve_ws on the large-system path: the kernels keep H as
// the lower 16x16 tiles (row-major inside a tile) of the COMPONENT-MAJOR system
// (unknown (node j, component c) at row c*Pp + j); the caller sees the dense NODE-MAJOR
// system of mhe_assemble (row j*n + c, j < Pp: the first P*n rows are the oracle's
// order, padding nodes last).  cm(r) maps a node-major row to its component-major one.
namespace mhe {

__device__ __forceinline__ int big_cm(int r, int n, int Pp) { return (r % n) * Pp + r / n; }

// state word per trajectory: running, or BAD_CONSTANTS when the buffer's stamp does
// not match these dims (then nothing of the stage runs and the outputs are NaN)
__global__ void k_big_parity_init(BigArgs a, int batch) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < batch) {
    const bool ok = *(const unsigned long long*)a.cbuf == a.tag;
    a.state[b] = ok ? BIG_RUNNING : MHE_STATUS_BAD_CONSTANTS;
    if (!ok && a.cost) a.cost[b] = NAN;
    // the envelope flags k_big_import_hg sets from the caller's system
    const BigWs WL = big_ws_layout(a.P, a.M, a.n, a.NT, a.nz, a.nc);
    int* EM = big_env_mask(a.ws + (size_t)b * a.ws_stride, WL);
    for (int e = 0; e < a.n * a.n; ++e) EM[e] = 0;
  }
}

__global__ void k_big_parity_finish(int batch, int* state) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < batch && state[b] == BIG_RUNNING) state[b] = MHE_STATUS_CONVERGED;
}

// dense node-major H (full, both triangles) and g = -BV from the tiles into the leading
// dp x dp block of a ld x ld matrix per trajectory (ld = dp, or dp + K for the KKT
// system: k_big_export_border fills the rest); grid (x, batch)
__global__ void k_big_export_hg(BigArgs a, int batch, int ld, double* Hout, double* gout) {
  const int b = blockIdx.y;
  const int dp = a.n * a.Pp;
  const BigWs WL = big_ws_layout(a.P, a.M, a.n, a.NT, a.nz, a.nc);
  const double* ws = a.ws + (size_t)b * a.ws_stride;
  const bool ok = a.state[b] == BIG_RUNNING;
  const size_t nel = (size_t)dp * dp;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < nel; e += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(e / dp), c = (int)(e % dp);
    const int R = big_cm(r, a.n, a.Pp), C = big_cm(c, a.n, a.Pp);
    const int hi = R >= C ? R : C, lo = R >= C ? C : R;
    const double v = ws[WL.H + (size_t)big_tile_index(hi >> 4, lo >> 4, a.NT) * 256 + (hi & 15) * 16 + (lo & 15)];
    Hout[(size_t)b * ld * ld + (size_t)r * ld + c] = ok ? v : NAN;
    if (c == 0) gout[(size_t)b * ld + r] = ok ? -ws[WL.BV + R] : NAN;
  }
}

// The border of the KKT system at X (mhe_assemble_kkt_ws), in the rows / columns dp ..
// dp + K - 1 after the dense H block:  [H  B; B^T  S] and g = [g_x; g_z; c(v) - r], the
// values k_big_border forms for the solve (big_border_col / _s / _rhs); grid (K, batch)
__global__ void k_big_export_border(BigArgs a, int batch, int p, double* Hout, double* gout) {
  const int b = blockIdx.y, col = blockIdx.x;
  const int n = a.n, dp = n * a.Pp, K = a.nz + a.nc, ld = dp + K;
  const BigConst CL = big_const_layout(a.P, a.M, n, p, a.nc);
  const BigWs WL = big_ws_layout(a.P, a.M, n, a.NT, a.nz, a.nc);
  const double* ws = a.ws + (size_t)b * a.ws_stride;
  const double* PhiE = (const double*)(a.cbuf + CL.PhiE);
  const int* eq = (const int*)(a.cbuf + CL.eq);
  const double* eqr = (const double*)(a.cbuf + CL.eqr);
  const int E = a.M > 0 ? *(const int*)(a.cbuf + CL.ne) : 0;
  const double* X = a.X + (size_t)b * a.P * n;
  const bool ok = a.state[b] == BIG_RUNNING;
  double* Hb = Hout + (size_t)b * ld * ld;
  for (int r = threadIdx.x; r < dp; r += blockDim.x) {  // node-major row r = j n + ca
    const int j = r / n, ca = r % n;
    const double v = ok ? big_border_col(a, ws, WL, PhiE, eq, E, n, col, ca, j) : NAN;
    Hb[(size_t)r * ld + dp + col] = v;
    Hb[(size_t)(dp + col) * ld + r] = v;
  }
  for (int c = threadIdx.x; c < K; c += blockDim.x)  // S's lower triangle, as k_big_border's LDL^T reads it
    Hb[(size_t)(dp + col) * ld + dp + c] = ok ? big_border_s(a, ws, WL, E, col >= c ? col : c, col >= c ? c : col) : NAN;
  if (threadIdx.x == 0) gout[(size_t)b * ld + dp + col] = ok ? -big_border_rhs(a, ws, WL, eq, eqr, X, E, col) : NAN;
}

// the caller's dense node-major H (lower triangle read; leading dp x dp block of a ld x ld
// matrix) and g into the tiles and BV = -g; grid (lower tiles, batch), one thread per
// tile element
__global__ void k_big_import_hg(BigArgs a, int batch, int ld, const double* Hin, const double* gin) {
  const int b = blockIdx.y;
  const BigWs WL = big_ws_layout(a.P, a.M, a.n, a.NT, a.nz, a.nc);
  double* ws = a.ws + (size_t)b * a.ws_stride;
  int t = blockIdx.x, J = 0;  // tile t -> (I, J), I >= J, column-major over the lower triangle
  while (t >= a.NT - J) {
    t -= a.NT - J;
    ++J;
  }
  const int I = J + t;
  const int tr = threadIdx.x >> 4, tc = threadIdx.x & 15;
  const int R = 16 * I + tr, C = 16 * J + tc;  // component-major
  const int r = (R % a.Pp) * a.n + R / a.Pp, c = (C % a.Pp) * a.n + C / a.Pp;
  const int hi = r >= c ? r : c, lo = r >= c ? c : r;  // node-major, lower triangle
  const double v = Hin[((size_t)b * ld + hi) * ld + lo];
  ws[WL.H + (size_t)blockIdx.x * 256 + threadIdx.x] = v;
  if (I == J && tr == 0) ws[WL.BV + 16 * I + tc] = -gin[(size_t)b * ld + (C % a.Pp) * a.n + C / a.Pp];
  if (__syncthreads_or(v != 0.0) && threadIdx.x == 0) {  // component pair flags (envelope)
    int* EM = big_env_mask(ws, WL);
    const int ca = I / a.NTc, cb = J / a.NTc;
    EM[ca * a.n + cb] = 1;
    EM[cb * a.n + ca] = 1;
  }
}

// The caller's KKT border (rows dp .. dp + K - 1 of a ld = dp + K system, lower part read:
// B^T and S) into the workspace k_big_border reads with border_import set: the columns
// of B component-major in BM and ZM (the panel padding columns K .. KP - 1 zero), S and
// r = -g_tail in KS; grid (KP, batch)
__global__ void k_big_import_border(BigArgs a, int batch, const double* Hin, const double* gin) {
  const int b = blockIdx.y, col = blockIdx.x;
  const int n = a.n, dp = n * a.Pp, K = a.nz + a.nc, ld = dp + K;
  const BigWs WL = big_ws_layout(a.P, a.M, n, a.NT, a.nz, a.nc);
  double* ws = a.ws + (size_t)b * a.ws_stride;
  const double* Hb = Hin + (size_t)b * ld * ld;
  for (int R = threadIdx.x; R < dp; R += blockDim.x) {  // component-major row R = ca Pp + j
    const int r = (R % a.Pp) * n + R / a.Pp;
    const double v = col < K ? Hb[(size_t)(dp + col) * ld + r] : 0.0;
    if (col < K) ws[WL.BM + (size_t)col * dp + R] = v;
    ws[WL.ZM + (size_t)col * dp + R] = v;
  }
  if (col < K) {
    for (int c = threadIdx.x; c < K; c += blockDim.x) {  // lower triangle of S, mirrored
      const int hi = col >= c ? col : c, lo = col >= c ? c : col;
      ws[WL.KS + (size_t)col * K + c] = Hb[(size_t)(dp + hi) * ld + dp + lo];
    }
    if (threadIdx.x == 0) ws[WL.KS + (size_t)K * K + col] = -gin[(size_t)b * ld + dp + col];
  }
}

// delta (node-major) from YV (component-major), then the border unknowns w = [dz; lambda]
// of the bordered step (K > 0); ld = dp + K per trajectory
__global__ void k_big_export_delta(BigArgs a, int batch, int ld, double* delta) {
  const int dp = a.n * a.Pp;
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)batch * ld) return;
  const int b = (int)(e / ld), r = (int)(e % ld);
  const BigWs WL = big_ws_layout(a.P, a.M, a.n, a.NT, a.nz, a.nc);
  const double* ws = a.ws + (size_t)b * a.ws_stride;
  const int K = a.nz + a.nc;
  const double v = r < dp ? ws[WL.YV + big_cm(r, a.n, a.Pp)] : ws[WL.KS + (size_t)K * K + K + (r - dp)];
  delta[e] = a.state[b] == BIG_RUNNING ? v : NAN;
}

// ------------------------------------------------------------ arrival cost (mhe_arrival)
// After the covariance stage (k_gn<MODE_COV> / BIG_STAGE_COV, one query) has left the n x n
// block C = S_t H^-1 S_t^T of every trajectory in `cov` and its outcome in `status`: one
// wavefront per trajectory, the block in LDS (n <= ARR_NMAX),
//   1. Cholesky C = L L^T, right-looking, with true sqrt and division (n is tiny and the
//      result is the next window's weight: no reciprocal-square-root estimate here);
//   2. L^-1 column by column (lane c: forward substitution of e_c), then A = L^-T L^-1,
//      A_ij = sum_{k >= j} (L^-1)_ki (L^-1)_kj for i <= j in increasing k, written to both
//      (i, j) and (j, i): bitwise symmetric;
//   3. x(t) = sum_j phi_j X_j in node order.
// A pivot that is not > 0 or not finite sets MHE_STATUS_NOT_SPD; wherever the status is
// non-zero x_arr, Pw_arr and the covariance block are NaN.  `cov` may be Pw_arr itself (the
// block is read into LDS before anything is written).  Sums are per trajectory and ordered:
// the result does not depend on the batch.
constexpr int ARR_NMAX = 40;
__global__ __launch_bounds__(64) void k_arrival(int n, int P, int batch, const double* X, const double* phi,
                                                double* cov, double* Pw_arr, double* x_arr, int* status) {
  __shared__ double Ls[ARR_NMAX * ARR_NMAX];  // C, then L (lower triangle)
  __shared__ double Ms[ARR_NMAX * ARR_NMAX];  // L^-1 (lower triangle)
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= batch) return;
  const int nn = n * n;
  double* Cb = cov + (size_t)b * nn;
  double* Ab = Pw_arr + (size_t)b * nn;
  bool ok = status[b] == 0;  // wave-uniform
  if (ok) {
    for (int t = lane; t < nn; t += 64) {
      const int i = t / n, j = t - i * n;
      Ls[t] = Cb[i >= j ? t : j * n + i];  // the lower triangle, mirrored (the block is symmetric)
      Ms[t] = 0.0;
    }
    __syncthreads();
    for (int k = 0; k < n && ok; ++k) {
      const double d = Ls[k * n + k];
      if (!(d > 0.0) || !(d < INFINITY)) {
        ok = false;
        break;
      }
      const double lkk = sqrt(d);
      __syncthreads();  // every lane has read the pivot
      for (int i = k + lane; i < n; i += 64) Ls[i * n + k] = i == k ? lkk : Ls[i * n + k] / lkk;
      __syncthreads();
      const int mrem = n - k - 1;
      for (int t = lane; t < mrem * mrem; t += 64) {
        const int i = k + 1 + t / mrem, j = k + 1 + t % mrem;
        if (j <= i) Ls[i * n + j] -= Ls[i * n + k] * Ls[j * n + k];
      }
      __syncthreads();
    }
  }
  if (ok) {
    for (int c = lane; c < n; c += 64) {  // column c of L^-1
      Ms[c * n + c] = 1.0 / Ls[c * n + c];
      for (int i = c + 1; i < n; ++i) {
        double s = 0.0;
        for (int k = c; k < i; ++k) s += Ls[i * n + k] * Ms[k * n + c];
        Ms[i * n + c] = -s / Ls[i * n + i];
      }
    }
    __syncthreads();
    for (int t = lane; t < nn; t += 64) {
      const int i = t / n, j = t - i * n;
      if (i <= j) {
        double s = 0.0;
        for (int k = j; k < n; ++k) s += Ms[k * n + i] * Ms[k * n + j];
        Ab[i * n + j] = s;
        Ab[j * n + i] = s;
      }
    }
    for (int c = lane; c < n; c += 64) {
      double s = 0.0;
      for (int j = 0; j < P; ++j) s += phi[j] * X[((size_t)b * P + j) * n + c];
      x_arr[(size_t)b * n + c] = s;
    }
  } else {
    for (int t = lane; t < nn; t += 64) {
      Ab[t] = NAN;
      Cb[t] = NAN;
    }
    for (int c = lane; c < n; c += 64) x_arr[(size_t)b * n + c] = NAN;
    if (lane == 0 && status[b] == 0) status[b] = MHE_STATUS_NOT_SPD;
  }
}

}  // namespace mhe

#ifdef MHE_DIAG
extern "C" void mhe_diag_set_buffer(void* p) { g_dbg = (unsigned long long*)p; }
#endif

namespace {

// One stage of the large-system path between the state words' init and finish (A.state);
// pre / post enqueue what a call imports before and exports after the stage.
template <class Pre, class Post>
int run_big_stage(const PairOps* ops, const mhe_dims* dims, BigArgs& A, int batch, int stage, hipStream_t st, Pre pre,
                  Post post) {
  const int nb = (batch + 255) / 256;
  hipLaunchKernelGGL(k_big_parity_init, dim3(nb), dim3(256), 0, st, A, batch);
  pre();
  const int rc = ops->big_stage(dims, A, batch, stage, st);
  if (rc != MHE_OK) return rc;
  post();
  hipLaunchKernelGGL(k_big_parity_finish, dim3(nb), dim3(256), 0, st, batch, A.state);
  return hipGetLastError() == hipSuccess ? MHE_OK : MHE_ERR_HIP;
}

}  // namespace

extern "C" {

int32_t mhe_set_option(int32_t option, int32_t value) {
  int* slot = option == MHE_OPT_BIG_RIGHT_LOOKING ? &g_opt_big_right_looking
              : option == MHE_OPT_DEBUG_SMEM_PAD  ? &g_opt_smem_pad
              : option == MHE_OPT_LSM_GROUP       ? &g_opt_lsm_group
                                                  : nullptr;
  if (!slot || value < 0 || (option == MHE_OPT_DEBUG_SMEM_PAD && value > 160 * 1024)) return MHE_ERR_DIMS;
  if (option == MHE_OPT_LSM_GROUP && value != 0 && value != 16 && value != 64) return MHE_ERR_DIMS;
  const int old = *slot;
  *slot = value;
  return old;
}

const char* mhe_version(void) { return "libmhe 0.3 (gfx950, register-tiled fp64 MFMA Cholesky)"; }

int32_t mhe_padded_dim(const mhe_dims* dims) {
  int NT = 0;
  if (check_dims(dims, &NT) != MHE_OK) return -1;
  return 16 * NT;  // big path: n * Pp (component-major)
}

size_t mhe_workspace_bytes(const mhe_dims* dims, int32_t batch) {
  int NT = 0;
  if (check_dims(dims, &NT) != MHE_OK || batch < 0) return 0;
  if (!is_big(dims)) return 0;
  return sizeof(double) * big_ws_doubles(dims, NT) * (size_t)batch;
}

size_t mhe_const_bytes(const mhe_dims* dims) {
  int NT = 0;
  if (check_dims(dims, &NT) != MHE_OK) return 0;
  return const_total_bytes(dims, NT);
}

int mhe_build_constants(const mhe_dims* dims, const double* D, const double* cw, const double* Phi,
                        const double* Qw, const double* Rw, const double* Pw, void* const_buf, void* stream) {
  int NT = 0;
  int rc = check_dims(dims, &NT);
  if (rc != MHE_OK) return rc;
  if (!D || !cw || !Qw || !const_buf || (dims->M > 0 && (!Phi || !Rw)) || (dims->has_prior && !Pw))
    return MHE_ERR_NULL;
  const PairOps* ops = find_pair(dims);
  if (!ops) return MHE_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  char* cb = (char*)const_buf;
  if (is_big(dims)) {
    rc = build_big_consts(dims, D, cw, Phi, Qw, Rw, Pw, cb, st);
  } else if (fg_eligible(dims)) {
    rc = build_fg_consts(dims, NT, ops, D, cw, Phi, Qw, Rw, Pw, cb, st);
  } else {
    hipLaunchKernelGGL(k_copy_consts, dim3(256), dim3(256), 0, st, dims->N + 1, dims->M, dims->n, dims->p, NT, D,
                       cw, Phi, Qw, Rw, Pw, cb);
    rc = ops->build_cc(dims, NT, D, cw, Phi, Qw, Rw, Pw, cb, st);
  }
  if (rc != MHE_OK) return rc;
  hipLaunchKernelGGL(k_write_tag, dim3(1), dim3(1), 0, st, (unsigned long long*)cb, const_tag(dims, NT));
  return hipGetLastError() == hipSuccess ? MHE_OK : MHE_ERR_HIP;
}

int mhe_gn_solve(const mhe_dims* dims, const void* const_buf, int32_t batch, const double* X0, double* X_out,
                 const double* U, int64_t u_bstride, const double* Y, const double* PAR, int64_t par_bstride,
                 const double* x0, double* cost_out, int32_t* iters_out, int32_t* status_out, int32_t max_iter,
                 double tol, void* stream) {
  return mhe_gn_solve_ws(dims, const_buf, batch, X0, X_out, U, u_bstride, Y, PAR, par_bstride, x0, cost_out,
                         iters_out, status_out, max_iter, tol, nullptr, 0, stream);
}

int mhe_gn_solve_ws(const mhe_dims* dims, const void* const_buf, int32_t batch, const double* X0, double* X_out,
                    const double* U, int64_t u_bstride, const double* Y, const double* PAR, int64_t par_bstride,
                    const double* x0, double* cost_out, int32_t* iters_out, int32_t* status_out, int32_t max_iter,
                    double tol, void* workspace, size_t workspace_bytes, void* stream) {
  return mhe_gn_solve_ext(dims, const_buf, batch, X0, X_out, nullptr, nullptr, U, u_bstride, Y, PAR, par_bstride, x0,
                          cost_out, iters_out, status_out, max_iter, tol, workspace, workspace_bytes, stream);
}

int mhe_gn_solve_ext(const mhe_dims* dims, const void* const_buf, int32_t batch, const double* X0, double* X_out,
                     const double* Z0, double* Z_out, const double* U, int64_t u_bstride, const double* Y,
                     const double* PAR, int64_t par_bstride, const double* x0, double* cost_out, int32_t* iters_out,
                     int32_t* status_out, int32_t max_iter, double tol, void* workspace, size_t workspace_bytes,
                     void* stream) {
  mhe_solve_args g = pack_point(batch, X0, Z0, U, u_bstride, Y, PAR, par_bstride, x0, workspace, workspace_bytes);
  g.X_out = X_out; g.Z_out = Z_out; g.cost_out = cost_out; g.iters_out = iters_out; g.status_out = status_out;
  g.max_iter = max_iter; g.tol = tol;
  return mhe_solve(dims, const_buf, &g, stream);
}

int mhe_solve(const mhe_dims* dims, const void* const_buf, const mhe_solve_args* g, void* stream) {
  int NT = 0;
  int rc = check_dims(dims, &NT);
  if (rc != MHE_OK) return rc;
  rc = check_header(g);
  if (rc == MHE_OK && g->max_iter < 0) rc = MHE_ERR_DIMS;
  if (rc == MHE_OK)
    rc = check_point(dims, const_buf, g, dims->n_extra > 0,
                     g->X_out && g->cost_out && g->iters_out && g->status_out && (dims->n_extra == 0 || g->Z_out));
  if (rc != MHE_OK || g->batch == 0) return rc;
  const int batch = g->batch;
  const PairOps* ops = find_pair(dims);
  if (!ops) return MHE_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const bool fused = fg_eligible(dims);
  if (fused && g->meas_delta) return MHE_ERR_UNSUPPORTED;  // k_gn_general has no robust rows
  if (is_big(dims)) {
    if (!g->workspace || g->workspace_bytes < mhe_workspace_bytes(dims, batch)) return MHE_ERR_NULL;
    BigArgs A = make_big_args(dims, const_buf, NT, g->workspace);
    set_point(A, g);
    A.X = g->X_out; A.cost = g->cost_out; A.iters = g->iters_out; A.state = g->status_out; A.tol = g->tol;
    A.Z = g->Z_out;
    A.lam = dims->n_eq > 0 ? g->lambda_out : nullptr;
    if (A.X != g->X0 &&
        hipMemcpyAsync(A.X, g->X0, sizeof(double) * batch * A.P * A.n, hipMemcpyDeviceToDevice, st) != hipSuccess)
      return MHE_ERR_HIP;
    if (A.nz > 0 && g->Z0 != A.Z &&
        hipMemcpyAsync(A.Z, g->Z0, sizeof(double) * batch * A.nz, hipMemcpyDeviceToDevice, st) != hipSuccess)
      return MHE_ERR_HIP;
    hipLaunchKernelGGL(k_big_init, dim3((batch + 255) / 256), dim3(256), 0, st, A, batch);
    rc = ops->big(dims, A, batch, g->max_iter, st);
    if (rc != MHE_OK) return rc;
    hipLaunchKernelGGL(k_big_finish, dim3((batch + 255) / 256), dim3(256), 0, st, batch, A.state);
    return hipGetLastError() == hipSuccess ? MHE_OK : MHE_ERR_HIP;
  }
  GnArgs a = make_args(dims, const_buf, NT);
  set_point(a, g);
  a.X0 = g->X0; a.Xout = g->X_out; a.cost = g->cost_out; a.iters = g->iters_out; a.status = g->status_out;
  a.max_iter = g->max_iter; a.tol = g->tol;
  if (fused) {
    a.Z0 = g->Z0; a.Zout = g->Z_out;
    a.lam = dims->n_eq > 0 ? g->lambda_out : nullptr;
    return ops->gn_general(dims, a, batch, st);
  }
  return ops->gn(dims, a, batch, MODE_SOLVE, st);
}

// mhe_state_cov's scratch on the large-system path: one cost word per trajectory (the
// residual pass writes it; 256-B aligned), then the query columns, KP dp doubles per trajectory
static size_t cov_cost_doubles(int batch) { return ((size_t)batch + 31) & ~size_t(31); }

size_t mhe_cov_scratch_bytes(const mhe_dims* dims, int32_t batch, int32_t n_query) {
  int NT = 0;
  if (check_dims(dims, &NT) != MHE_OK || batch < 0 || n_query <= 0) return 0;
  if (!is_big(dims)) return 0;
  const size_t KP = ((size_t)n_query * dims->n + 15) / 16 * 16;
  return sizeof(double) * (cov_cost_doubles(batch) + (size_t)batch * KP * 16 * NT);
}

// mixed rows, extra variables or equality rows: the problems mhe_state_cov / mhe_arrival refuse
static bool is_general(const mhe_dims* dims) {
  return dims->n_extra > 0 || dims->n_eq > 0 || dims->meas_model == MHE_MEAS_MIXED;
}

// mhe_state_cov's and mhe_kkt_cov's checks of the operating point and the query
static int check_cov_args(const mhe_dims* dims, const void* const_buf, const mhe_solve_args* at, const double* PhiQ,
                          int32_t n_query, const double* cov_out, const int32_t* status_out) {
  int rc = check_header(at);
  if (rc == MHE_OK && n_query <= 0) rc = MHE_ERR_DIMS;
  if (rc == MHE_OK && (!PhiQ || !cov_out || !status_out)) rc = MHE_ERR_NULL;
  return rc != MHE_OK ? rc : check_point(dims, const_buf, at, dims->n_extra > 0, true);  // rows as mhe_solve
}

// The covariance stage on the large-system path (BIG_STAGE_COV, or BIG_STAGE_KKT_COV at
// (X, Z) with the extra variables' block in covz_out).
static int big_cov(const mhe_dims* dims, const void* const_buf, const mhe_solve_args* at, int NT, const PairOps* ops,
                   int stage, const double* PhiQ, int32_t n_query, double* cov_out, double* covz_out,
                   int32_t* status_out, void* scratch, size_t scratch_bytes, hipStream_t st) {
  const int batch = at->batch;
  if (!at->workspace || at->workspace_bytes < mhe_workspace_bytes(dims, batch)) return MHE_ERR_NULL;
  if (!scratch || scratch_bytes < mhe_cov_scratch_bytes(dims, batch, n_query)) return MHE_ERR_NULL;
  BigArgs A = make_big_args(dims, const_buf, NT, at->workspace);
  A.n_bounds = 0;  // the unconstrained GN model at X, under its equality rows (bounds are not reflected)
  set_point(A, at);
  A.X = const_cast<double*>(at->X0);  // read only by k_big_resid / k_big_assemble
  if (stage == BIG_STAGE_KKT_COV) A.Z = const_cast<double*>(at->Z0);  // read only by k_big_resid
  A.cost = (double*)scratch; A.state = status_out;
  A.PhiQ = PhiQ; A.nq = n_query; A.cov = cov_out; A.cov_scratch = (double*)scratch + cov_cost_doubles(batch);
  A.covz = dims->n_extra > 0 ? covz_out : nullptr;
  return run_big_stage(ops, dims, A, batch, stage, st, [] {}, [] {});
}

int mhe_state_cov(const mhe_dims* dims, const void* const_buf, const mhe_solve_args* at, const double* PhiQ,
                  int32_t n_query, double* cov_out, int32_t* status_out, void* scratch, size_t scratch_bytes,
                  void* stream) {
  int NT = 0;
  int rc = check_dims(dims, &NT);
  if (rc != MHE_OK) return rc;
  // a covariance under constraints is a projected quantity: not this call's
  if (is_general(dims)) return MHE_ERR_UNSUPPORTED;
  rc = check_cov_args(dims, const_buf, at, PhiQ, n_query, cov_out, status_out);
  if (rc != MHE_OK || at->batch == 0) return rc;
  const PairOps* ops = find_pair(dims);
  if (!ops) return MHE_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (is_big(dims))
    return big_cov(dims, const_buf, at, NT, ops, BIG_STAGE_COV, PhiQ, n_query, cov_out, nullptr, status_out, scratch,
                   scratch_bytes, st);
  GnArgs a = make_args(dims, const_buf, NT);
  set_point(a, at);
  a.X0 = at->X0;
  a.status = status_out;
  a.PhiQ = PhiQ; a.nq = n_query; a.cov = cov_out;
  return ops->gn(dims, a, at->batch, MODE_COV, st);
}

size_t mhe_arrival_scratch_bytes(const mhe_dims* dims, int32_t batch) { return mhe_cov_scratch_bytes(dims, batch, 1); }

size_t mhe_kkt_cov_scratch_bytes(const mhe_dims* dims, int32_t batch, int32_t n_query) {
  // the query columns, as mhe_state_cov's; the border columns live in the workspace (ZM)
  return mhe_cov_scratch_bytes(dims, batch, n_query);
}

int mhe_kkt_cov(const mhe_dims* dims, const void* const_buf, const mhe_solve_args* at, const double* PhiQ,
                int32_t n_query, double* cov_out, double* covz_out, int32_t* status_out, void* scratch,
                size_t scratch_bytes, void* stream) {
  int NT = 0;
  int rc = check_dims(dims, &NT);
  if (rc != MHE_OK) return rc;
  if (fg_eligible(dims)) return MHE_ERR_UNSUPPORTED;  // k_gn_general solves only
  if (!is_general(dims))  // no border, typed rows: mhe_state_cov itself (both paths)
    return mhe_state_cov(dims, const_buf, at, PhiQ, n_query, cov_out, status_out, scratch, scratch_bytes, stream);
  if (!is_big(dims)) return MHE_ERR_UNSUPPORTED;  // every general problem takes the large-system path
  rc = check_cov_args(dims, const_buf, at, PhiQ, n_query, cov_out, status_out);
  if (rc != MHE_OK || at->batch == 0) return rc;
  const PairOps* ops = find_pair(dims);
  if (!ops) return MHE_ERR_UNSUPPORTED;
  return big_cov(dims, const_buf, at, NT, ops, BIG_STAGE_KKT_COV, PhiQ, n_query, cov_out, covz_out, status_out,
                 scratch, scratch_bytes, (hipStream_t)stream);
}

// mhe_arrival / mhe_kkt_arrival after their dims checks: the covariance stage of mhe_state_cov
// (kkt: mhe_kkt_cov), one query -- the block into cov_out when the caller wants it, else into
// Pw_arr -- and k_arrival, which inverts it in place.
static int arrival(bool kkt, const mhe_dims* dims, const void* const_buf, const mhe_solve_args* at,
                   const double* phi, double* x_arr, double* Pw_arr, double* cov_out, int32_t* status_out,
                   void* scratch, size_t scratch_bytes, void* stream) {
  int rc = check_header(at);
  if (rc != MHE_OK) return rc;
  if (!phi || !x_arr || !Pw_arr || !status_out) return MHE_ERR_NULL;
  if (at->batch == 0) return MHE_OK;
  double* cov = cov_out ? cov_out : Pw_arr;
  rc = kkt ? mhe_kkt_cov(dims, const_buf, at, phi, 1, cov, nullptr, status_out, scratch, scratch_bytes, stream)
           : mhe_state_cov(dims, const_buf, at, phi, 1, cov, status_out, scratch, scratch_bytes, stream);
  if (rc != MHE_OK) return rc;
  hipLaunchKernelGGL(k_arrival, dim3(at->batch), dim3(64), 0, (hipStream_t)stream, dims->n, dims->N + 1, at->batch,
                     at->X0, phi, cov, Pw_arr, x_arr, status_out);
  return hipGetLastError() == hipSuccess ? MHE_OK : MHE_ERR_HIP;
}

int mhe_arrival(const mhe_dims* dims, const void* const_buf, const mhe_solve_args* at, const double* phi,
                double* x_arr, double* Pw_arr, double* cov_out, int32_t* status_out, void* scratch,
                size_t scratch_bytes, void* stream) {
  const int rc = check_dims(dims, nullptr);
  if (rc != MHE_OK) return rc;
  if (is_general(dims) || dims->n > ARR_NMAX) return MHE_ERR_UNSUPPORTED;
  if (!is_big(dims) && dims->n > 16) return MHE_ERR_UNSUPPORTED;  // as mhe_state_cov: one 16-column panel
  return arrival(false, dims, const_buf, at, phi, x_arr, Pw_arr, cov_out, status_out, scratch, scratch_bytes, stream);
}

int mhe_kkt_arrival(const mhe_dims* dims, const void* const_buf, const mhe_solve_args* at, const double* phi,
                    double* x_arr, double* Pw_arr, double* cov_out, int32_t* status_out, void* scratch,
                    size_t scratch_bytes, void* stream) {
  const int rc = check_dims(dims, nullptr);
  if (rc != MHE_OK) return rc;
  if (fg_eligible(dims)) return MHE_ERR_UNSUPPORTED;  // k_gn_general solves only
  // an equality row between state components makes the block rank-deficient: no inverse
  if (dims->n_eq > 0 || dims->n > ARR_NMAX) return MHE_ERR_UNSUPPORTED;
  if (!is_big(dims) && dims->n > 16) return MHE_ERR_UNSUPPORTED;  // as mhe_arrival
  return arrival(true, dims, const_buf, at, phi, x_arr, Pw_arr, cov_out, status_out, scratch, scratch_bytes, stream);
}

int mhe_resjac(const mhe_dims* dims, const void* const_buf, int32_t batch, const double* X, const double* U,
               int64_t u_bstride, const double* Y, const double* PAR, int64_t par_bstride, double* W, double* F,
               double* E, double* Hm, void* stream) {
  int NT = 0;
  int rc = check_dims(dims, &NT);
  if (rc != MHE_OK) return rc;
  if (dims->meas_model == MHE_MEAS_MIXED) return MHE_ERR_UNSUPPORTED;
  if (batch <= 0) return batch == 0 ? MHE_OK : MHE_ERR_DIMS;
  if (!const_buf || !X || (dims->m > 0 && !U) || (dims->M > 0 && E && !Y) || (dims->q > 0 && dims->M > 0 && !PAR))
    return MHE_ERR_NULL;
  const PairOps* ops = find_pair(dims);
  if (!ops) return MHE_ERR_UNSUPPORTED;
  ResjacArgs a = {};
  a.cbuf = (const char*)const_buf;
  a.P = dims->N + 1; a.M = dims->M; a.big = is_big(dims) ? 1 : 0; a.alpha = 2.0 / dims->T;
  a.X = X; a.U = U; a.ustride = u_bstride; a.Y = Y; a.PAR = PAR; a.pstride = par_bstride;
  a.W = W; a.F = F; a.E = E; a.Hm = Hm;
  for (int i = 0; i < 8; ++i) {
    a.idx[i] = dims->meas_idx[i];
    a.dpar[i] = dims->dyn_par[i];
  }
  a.tag = const_tag(dims, NT);
  return ops->resjac(a, batch, (hipStream_t)stream);
}

// mhe_assemble at an operating point (mhe_assemble_at's register path; the positional call
// passes no per-solve row inputs)
static int assemble_reg(const mhe_dims* dims, const void* const_buf, const mhe_solve_args* at, double* H, double* g,
                        double* cost, void* stream) {
  int NT = 0;
  int rc = check_dims(dims, &NT);
  if (rc != MHE_OK) return rc;
  if (is_big(dims)) return MHE_ERR_UNSUPPORTED;  // kernel-level parity APIs: register path only
  rc = check_point(dims, const_buf, at, false, H && g && cost);
  if (rc != MHE_OK || at->batch == 0) return rc;
  const PairOps* ops = find_pair(dims);
  if (!ops) return MHE_ERR_UNSUPPORTED;
  GnArgs a = make_args(dims, const_buf, NT);
  set_point(a, at);
  a.X0 = at->X0;
  a.Hout = H; a.gout = g; a.cost = cost;
  return ops->gn(dims, a, at->batch, MODE_ASSEMBLE, (hipStream_t)stream);
}

int mhe_assemble(const mhe_dims* dims, const void* const_buf, int32_t batch, const double* X, const double* U,
                 int64_t u_bstride, const double* Y, const double* PAR, int64_t par_bstride, const double* x0,
                 double* H, double* g, double* cost, void* stream) {
  const mhe_solve_args at = pack_point(batch, X, nullptr, U, u_bstride, Y, PAR, par_bstride, x0, nullptr, 0);
  return assemble_reg(dims, const_buf, &at, H, g, cost, stream);
}

int mhe_chol_solve(const mhe_dims* dims, const void* const_buf, int32_t batch, const double* H, const double* g,
                   double* delta, int32_t* status, void* stream) {
  int NT = 0;
  int rc = check_dims(dims, &NT);
  if (rc != MHE_OK) return rc;
  if (is_big(dims)) return MHE_ERR_UNSUPPORTED;  // kernel-level parity APIs: register path only
  if (batch <= 0) return batch == 0 ? MHE_OK : MHE_ERR_DIMS;
  if (!const_buf || !H || !g || !delta || !status) return MHE_ERR_NULL;
  const PairOps* ops = find_pair(dims);
  if (!ops) return MHE_ERR_UNSUPPORTED;
  GnArgs a = make_args(dims, const_buf, NT);
  a.Hin = H; a.gin = g; a.dout = delta; a.status = status;
  return ops->gn(dims, a, batch, MODE_LINSOLVE, (hipStream_t)stream);
}

int mhe_assemble_ws(const mhe_dims* dims, const void* const_buf, int32_t batch, const double* X, const double* U,
                    int64_t u_bstride, const double* Y, const double* PAR, int64_t par_bstride, const double* x0,
                    double* H, double* g, double* cost, int32_t* status, void* workspace, size_t workspace_bytes,
                    void* stream) {
  return mhe_assemble_kkt_ws(dims, const_buf, batch, X, nullptr, U, u_bstride, Y, PAR, par_bstride, x0, H, g, cost,
                             status, workspace, workspace_bytes, stream);
}

int32_t mhe_solve_kernel_name(const mhe_dims* dims, int32_t batch, void* stream, char* buf, int32_t len) {
  int NT = 0;
  const int rc = check_dims(dims, &NT);
  if (rc != MHE_OK) return rc;
  if (!buf || len <= 0) return MHE_ERR_NULL;
  if (is_big(dims)) {
    BigArgs A = make_big_args(dims, nullptr, NT, nullptr);
    const bool wide = A.NT >= BIG_WIDE_NT, split = g_opt_big_right_looking == 0;
    snprintf(buf, len, "large-system path (dyn %d, meas %d, NT %d): k_big_resid, k_big_assemble, %s, k_big_%s",
             dims->dyn_model, dims->meas_model, NT,
             split ? "k_big_chol<8|4, LL, split stages> + k_big_rows" : (wide ? "k_big_chol<8>" : "k_big_chol<4>"),
             dims->n_bounds > 0 ? "linesearch" : "update");
    return MHE_OK;
  }
  if (fg_eligible(dims)) {
    snprintf(buf, len, "k_gn_general<dyn %d, meas %d, SLOTS=%d, MINW=%d> (fused bordered solve, NT %d, K %d)",
             dims->dyn_model, dims->meas_model, MAX_SLOTS, FG_MINW, NT, dims->n_extra + dims->n_eq);
    return MHE_OK;
  }
  const GnChoice c = gn_choice(dims, NT, batch, MODE_SOLVE, (hipStream_t)stream);  // a call without meas_delta
  if (c.smem > REG_LDS_LIMIT) return MHE_ERR_UNSUPPORTED;
  snprintf(buf, len, "mhe::%s<dyn %d, meas %d, SLOTS=%d, MODE_SOLVE, HUBER=%d%s>%s", c.bounded ? "k_gn_bounded" : "k_gn",
           dims->dyn_model, dims->meas_model, c.sb ? SB_SLOTS : MAX_SLOTS, c.huber ? 1 : 0,
           c.sb ? ", MINW=2, SB=true" : "", c.sb ? " (small-batch factorization: batch <= CUs)" : " (two workgroups per CU)");
  return MHE_OK;
}

int32_t mhe_big_envelope(const mhe_dims* dims, const void* workspace, size_t workspace_bytes, int32_t traj,
                         int32_t* first_col, int32_t n_out, void* stream) {
  int NT = 0;
  const int rc = check_dims(dims, &NT);
  if (rc != MHE_OK) return rc;
  if (!is_big(dims)) return MHE_ERR_UNSUPPORTED;
  if (!workspace || !first_col) return MHE_ERR_NULL;
  if (n_out < NT || traj < 0) return MHE_ERR_DIMS;
  const BigArgs A = make_big_args(dims, nullptr, NT, const_cast<void*>(workspace));
  if ((size_t)(traj + 1) * A.ws_stride * sizeof(double) > workspace_bytes) return MHE_ERR_DIMS;
  const BigWs WL = big_ws_layout(A.P, A.M, A.n, A.NT, A.nz, A.nc);
  const int* src = (const int*)(A.ws + (size_t)traj * A.ws_stride + WL.ENV) + A.n * A.n;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemcpyAsync(first_col, src, (size_t)NT * sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return MHE_ERR_HIP;
  return NT;
}

int32_t mhe_kkt_dim(const mhe_dims* dims) {
  const int32_t dp = mhe_padded_dim(dims);
  return dp < 0 ? dp : dp + dims->n_extra + dims->n_eq;
}

// mhe_assemble_kkt_ws at an operating point (mhe_assemble_at; the positional call passes no
// per-solve row inputs).  The row inputs are answered for before the batch and the pointers.
static int assemble_kkt(const mhe_dims* dims, const void* const_buf, const mhe_solve_args* at, double* H, double* g,
                        double* cost, int32_t* status, void* stream) {
  int NT = 0;
  int rc = check_dims(dims, &NT);
  if (rc != MHE_OK) return rc;
  rc = check_header(at, false);
  if (rc == MHE_OK) rc = check_rows(dims, at);
  if (rc != MHE_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int batch = at->batch;
  if (!is_big(dims)) {
    rc = assemble_reg(dims, const_buf, at, H, g, cost, stream);
    if (rc == MHE_OK && status && batch > 0 && hipMemsetAsync(status, 0, sizeof(int32_t) * batch, st) != hipSuccess)
      return MHE_ERR_HIP;
    return rc;
  }
  rc = check_point(dims, const_buf, at, dims->n_extra > 0, H && g && cost && status);
  if (rc != MHE_OK || batch == 0) return rc;
  if (!at->workspace || at->workspace_bytes < mhe_workspace_bytes(dims, batch)) return MHE_ERR_NULL;
  const PairOps* ops = find_pair(dims);
  if (!ops) return MHE_ERR_UNSUPPORTED;
  BigArgs A = make_big_args(dims, const_buf, NT, at->workspace);
  A.n_bounds = 0;  // the plain GN system: the projected method's reduction belongs to the solve
  set_point(A, at);
  A.X = const_cast<double*>(at->X0);  // read only by k_big_resid / k_big_assemble
  A.Z = const_cast<double*>(at->Z0);  // read only by k_big_resid
  A.cost = cost; A.state = status;
  return run_big_stage(ops, dims, A, batch, BIG_STAGE_ASSEMBLE, st, [] {}, [&] {
    const size_t dp = (size_t)A.n * A.Pp;
    const int K = A.nz + A.nc;
    const size_t gx0 = (dp * dp + 255) / 256;
    const unsigned gx = (unsigned)(gx0 < 8192 ? gx0 : 8192);
    hipLaunchKernelGGL(k_big_export_hg, dim3(gx, batch), dim3(256), 0, st, A, batch, (int)dp + K, H, g);
    if (K > 0) hipLaunchKernelGGL(k_big_export_border, dim3(K, batch), dim3(256), 0, st, A, batch, dims->p, H, g);
  });
}

int mhe_assemble_kkt_ws(const mhe_dims* dims, const void* const_buf, int32_t batch, const double* X, const double* Z,
                        const double* U, int64_t u_bstride, const double* Y, const double* PAR, int64_t par_bstride,
                        const double* x0, double* H, double* g, double* cost, int32_t* status, void* workspace,
                        size_t workspace_bytes, void* stream) {
  const mhe_solve_args at = pack_point(batch, X, Z, U, u_bstride, Y, PAR, par_bstride, x0, workspace, workspace_bytes);
  return assemble_kkt(dims, const_buf, &at, H, g, cost, status, stream);
}

int mhe_assemble_at(const mhe_dims* dims, const void* const_buf, const mhe_solve_args* at, double* H, double* g,
                    double* cost, int32_t* status, void* stream) {
  return assemble_kkt(dims, const_buf, at, H, g, cost, status, stream);
}

int mhe_chol_solve_ws(const mhe_dims* dims, const void* const_buf, int32_t batch, const double* H, const double* g,
                      double* delta, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  int NT = 0;
  int rc = check_dims(dims, &NT);
  if (rc != MHE_OK) return rc;
  if (fg_eligible(dims)) return MHE_ERR_UNSUPPORTED;  // k_gn_general solves only
  if (!is_big(dims)) return mhe_chol_solve(dims, const_buf, batch, H, g, delta, status, stream);
  if (batch <= 0) return batch == 0 ? MHE_OK : MHE_ERR_DIMS;
  if (!const_buf || !H || !g || !delta || !status) return MHE_ERR_NULL;
  if (!workspace || workspace_bytes < mhe_workspace_bytes(dims, batch)) return MHE_ERR_NULL;
  const PairOps* ops = find_pair(dims);
  if (!ops) return MHE_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  BigArgs A = make_big_args(dims, const_buf, NT, workspace);
  A.n_bounds = 0;
  A.state = status;
  A.border_import = 1;  // K > 0: the caller's border, not one formed at an iterate
  A.lam = nullptr;
  const int K = A.nz + A.nc, ld = A.n * A.Pp + K;
  return run_big_stage(
      ops, dims, A, batch, BIG_STAGE_FACTOR, st,
      [&] {
        hipLaunchKernelGGL(k_big_import_hg, dim3(NT * (NT + 1) / 2, batch), dim3(256), 0, st, A, batch, ld, H, g);
        if (K > 0)
          hipLaunchKernelGGL(k_big_import_border, dim3((K + 15) / 16 * 16, batch), dim3(256), 0, st, A, batch, H, g);
      },
      [&] {
        const long long ne = (long long)batch * ld;
        hipLaunchKernelGGL(k_big_export_delta, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, A, batch, ld,
                           delta);
      });
}

}  // extern "C"
