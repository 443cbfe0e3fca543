// libmhe host launch layer: model tables, path selection and the launch templates that
// each pair_*.hip instantiates for its (dynamics, measurement) pairs -- host code only,
// included after the kernels (mhe_core.h's last line).  The C-ABI (include/mhe.h) and the
// argument checks live in mhe_gn.hip.
#pragma once
#include <mutex>
#include <type_traits>

#include "mhe_core.h"

namespace mhe {

inline bool dyn_info(int id, int& n, int& m) {
  switch (id) {
    case MHE_DYN_SINGLE_INTEGRATOR: n = 1; m = 1; return true;
    case MHE_DYN_SINGLE_INTEGRATOR_2D: n = 2; m = 2; return true;
    case MHE_DYN_SINGLE_INTEGRATOR_3D: n = 3; m = 3; return true;
    case MHE_DYN_DOUBLE_INTEGRATOR: n = 4; m = 2; return true;
    case MHE_DYN_VAN_DER_POL: n = 2; m = 1; return true;
    case MHE_DYN_GNSS_POS_AND_BIAS: n = 5; m = 3; return true;
    case MHE_DYN_MULTI_RECEIVER: n = 8; m = 0; return true;
    case MHE_DYN_GNSS_TWO_RECEIVER: n = 10; m = 6; return true;
    case MHE_DYN_KINEMATIC_BICYCLE: n = 6; m = 2; return true;
    case MHE_DYN_VEHICLE_GNSS: n = 9; m = 2; return true;
    case MHE_DYN_GNSS_8_RECEIVERS: n = 40; m = 24; return true;
  }
  return false;
}

inline bool meas_info(int id, int n, int& p, int& q, bool& linear) {
  switch (id) {
    case MHE_MEAS_FULL_STATE: p = n; q = 0; linear = true; return true;
    case MHE_MEAS_PSEUDORANGE: p = 1; q = 3; linear = false; return true;
    case MHE_MEAS_VEHICLE_PSEUDORANGE: p = 1; q = 3; linear = false; return true;
    case MHE_MEAS_RANGE_3D: p = 1; q = 3; linear = false; return true;
    case MHE_MEAS_MIXED: p = 1; q = MHE_MIXED_Q; linear = false; return true;
  }
  return false;
}

// Register-resident path iff the node-major padded system fits MAX_NT tiles --
// a function of dims alone.  dims->force_large (tests) routes a problem through
// the large-system path so both paths can be compared on identical inputs.
// Mixed-row problems, extra variables and equality constraints
// always take the large-system path (it carries the bordered KKT step).
inline int smem_bytes(const mhe_dims* dm, int NT, bool bounded = false, bool sb = false, bool cov = false) {
  int p, q;
  bool lin;
  meas_info(dm->meas_model, dm->n, p, q, lin);
  return smem_layout(dm->N + 1, dm->M, dm->n, NT, !lin, bounded, sb, cov).total * (int)sizeof(double);
}

// The register-resident kernel keeps per-row measurement blocks G_i (n x n) in LDS;
// when they do not fit (e.g. autonomous-car.py: 231 rows x 9 x 9) the problem takes
// the large-system path, which groups rows by epoch.
constexpr int REG_LDS_LIMIT = 160 * 1024;
static_assert(FG_LDS_DOUBLES * (int)sizeof(double) == REG_LDS_LIMIT, "k_gn_general sizes its LDS by the same limit");

// Fused-general dims (mhe_dims.force_large == MHE_PATH_FUSED_GENERAL): a mixed-row problem
// (with or without extra variables and equality rows) that k_gn_general takes in one launch --
// L2 dynamics cost, no bounds, n <= 16, the node-major padded system within MAX_NT tiles and
// the kernel's LDS layout (fg_smem_layout, at least one epoch) within REG_LDS_LIMIT.  A
// function of dims alone; for every other dims the value 2 is the value 0.
inline bool fg_eligible(const mhe_dims* dm) {
  if (dm->force_large != MHE_PATH_FUSED_GENERAL || dm->meas_model != MHE_MEAS_MIXED) return false;
  if (dm->dyn_cost != MHE_COST_L2 || dm->n_bounds != 0 || dm->n > 16) return false;
  const int NT = ((dm->N + 1) * dm->n + 15) / 16;
  if (NT > MAX_NT) return false;
  return fg_epoch_cap(dm->N + 1, dm->M > 0 ? dm->M : 1, dm->n, NT, dm->n_extra, dm->n_eq) >= 1;
}

inline bool is_big(const mhe_dims* dm) {
  if (dm->force_large != MHE_PATH_AUTO && dm->force_large != MHE_PATH_FUSED_GENERAL) return true;
  if (fg_eligible(dm)) return false;
  if (dm->meas_model == MHE_MEAS_MIXED || dm->n_extra > 0 || dm->n_eq > 0) return true;
  const int NT = ((dm->N + 1) * dm->n + 15) / 16;
  if (NT > MAX_NT) return true;
  return smem_bytes(dm, NT, true) > REG_LDS_LIMIT;
}

inline size_t big_ws_doubles(const mhe_dims* dm, int NT) {
  return big_ws_layout(dm->N + 1, dm->M, dm->n, NT, dm->n_extra, dm->n_eq).total;
}

template <class DYN, class MEAS>
int launch_resjac(ResjacArgs& a, int batch, hipStream_t st) {
  if constexpr (MEAS::MIXED) {
    return MHE_ERR_UNSUPPORTED;  // mixed rows: see mhe_solve parity tests
  } else {
    const long long nt = (long long)batch * (a.P + a.M);
    hipLaunchKernelGGL((k_resjac<DYN, MEAS>), dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, a, batch);
    return hipGetLastError() == hipSuccess ? MHE_OK : MHE_ERR_HIP;
  }
}

// Per (dynamics, measurement) pair: the launches that depend on the model types.
struct PairOps {
  // register-resident path: the tile tables of the constants buffer (k_build_cc)
  int (*build_cc)(const mhe_dims* dm, int NT, const double* D, const double* cw, const double* Phi,
                  const double* Qw, const double* Rw, const double* Pw, char* cbuf, hipStream_t st);
  // register-resident path: one fused launch (MODE_SOLVE / ASSEMBLE / LINSOLVE / COV)
  int (*gn)(const mhe_dims* dm, GnArgs& a, int batch, int mode, hipStream_t st);
  // large-system path: max_iter iterations of resid -> assemble -> chol (-> border)
  // -> update / line search, then the final residual pass (A.X holds X0 and the
  // state words are initialised by the caller)
  int (*big)(const mhe_dims* dm, BigArgs& A, int batch, int max_iter, hipStream_t st);
  // kernel-level parity: residuals and Jacobians per node / row (mhe_resjac)
  int (*resjac)(ResjacArgs& a, int batch, hipStream_t st);
  // kernel-level parity of the large-system path: one stage (BIG_STAGE_*) on the workspace
  int (*big_stage)(const mhe_dims* dm, BigArgs& A, int batch, int stage, hipStream_t st);
  // fused-general dims (fg_eligible): the whole bordered solve in one launch (k_gn_general)
  int (*gn_general)(const mhe_dims* dm, GnArgs& a, int batch, hipStream_t st);
};

// compute units of the device the launch stream belongs to (not the calling thread's
// current device), cached per device; concurrent callers may both fill a slot, with
// the same value (relaxed atomics: no torn or racy plain accesses)
inline int device_cus(hipStream_t st) {
  static int cus[64] = {0};
  int dev = 0;
  if (hipStreamGetDevice(st, &dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  int c = __atomic_load_n(&cus[dev], __ATOMIC_RELAXED);
  if (c == 0) {
    int v = 0;
    c = hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0 ? v : 256;
    __atomic_store_n(&cus[dev], c, __ATOMIC_RELAXED);
  }
  return c;
}

// Which k_gn instance a register-path launch runs (launch_gn, and mhe_solve_kernel_name
// for the records that name it): a function of the dims, the mode and the batch against
// the launch stream's CU count only.
struct GnChoice {
  bool bounded, huber, sb, mhuber;
  int smem;
};
// mhuber: the call carries meas_delta (robust measurement rows: the MHUBER instances)
inline GnChoice gn_choice(const mhe_dims* dm, int NT, int batch, int mode, hipStream_t st, bool mhuber = false) {
  GnChoice c;
  c.bounded = mode == MODE_SOLVE && dm->n_bounds > 0;
  c.huber = dm->dyn_cost == MHE_COST_HUBER;
  c.mhuber = mhuber;
  // a batch that gives each CU at most one trajectory runs the small-batch instance:
  // 256 VGPRs (no two-workgroups-per-CU register cap) and factor_forward_sb (C2 strong
  // scaling at 4-8 GPUs: 256 / 128 per GPU)
  c.sb = mode == MODE_SOLVE && !c.bounded && !c.huber && !c.mhuber && batch <= device_cus(st) &&
         smem_bytes(dm, NT, false, true) + g_opt_smem_pad <= REG_LDS_LIMIT;
  // pad: mhe_set_option, occupancy A/B only; MODE_COV: the query panel on top (dp x 16)
  c.smem = smem_bytes(dm, NT, c.bounded, c.sb, mode == MODE_COV) + g_opt_smem_pad;
  return c;
}

using GnKernel = void (*)(GnArgs);

// One instance ladder for both kinds of k_gn / k_gn_bounded instance: `pick` names the instance
// of the choice, or nullptr where there is none.  MH selects the MHUBER instances (robust
// measurement rows, meas_delta), which have no small-batch and no PW = false variant and no
// MODE_LINSOLVE.  MODE_LINSOLVE has one instance whatever the dynamics cost; MODE_COV exists
// for DYN::n <= 16 only (a query's n columns must fit one 16-column panel).  The device code is
// emitted in the order the instances are first named here (MH first, the plain L2 solve's
// small-batch and PW instances before its Huber one).
template <class DYN, class MEAS>
int launch_gn(const mhe_dims* dm, GnArgs& a, int batch, int mode, hipStream_t st) {
  if constexpr (MEAS::MIXED) {
    return MHE_ERR_UNSUPPORTED;  // mixed rows: large-system path only
  } else {
    const GnChoice ch = gn_choice(dm, a.NT, batch, mode, st, a.md != nullptr);
    const int smem = ch.smem;
    if (smem > REG_LDS_LIMIT) return MHE_ERR_UNSUPPORTED;
    const bool huber = ch.huber, pw = a.Pw != nullptr;
    auto pick = [&](auto mh) -> GnKernel {
      constexpr bool MH = decltype(mh)::value;
      constexpr int W = MHE_GN_MINW;
      if (ch.bounded)
        return huber ? k_gn_bounded<DYN, MEAS, MAX_SLOTS, true, MH> : k_gn_bounded<DYN, MEAS, MAX_SLOTS, false, MH>;
      if (mode == MODE_SOLVE) {
        if constexpr (!MH) {
          // the plain L2 solve keeps the instance without the per-solve prior weight (PW = false)
          // for calls that pass none; every other instance reads a.Pw behind a branch
          if (!huber && ch.sb)
            return pw ? k_gn<DYN, MEAS, SB_SLOTS, MODE_SOLVE, false, 2, true>
                      : k_gn<DYN, MEAS, SB_SLOTS, MODE_SOLVE, false, 2, true, false, false>;
          if (!huber)
            return pw ? k_gn<DYN, MEAS, MAX_SLOTS, MODE_SOLVE>
                      : k_gn<DYN, MEAS, MAX_SLOTS, MODE_SOLVE, false, W, false, false, false>;
        }
        return huber ? k_gn<DYN, MEAS, MAX_SLOTS, MODE_SOLVE, true, W, false, MH>
                     : k_gn<DYN, MEAS, MAX_SLOTS, MODE_SOLVE, false, W, false, MH>;
      }
      if (mode == MODE_ASSEMBLE)
        return huber ? k_gn<DYN, MEAS, MAX_SLOTS, MODE_ASSEMBLE, true, W, false, MH>
                     : k_gn<DYN, MEAS, MAX_SLOTS, MODE_ASSEMBLE, false, W, false, MH>;
      if (mode == MODE_COV) {
        if constexpr (DYN::n <= 16)
          return huber ? k_gn<DYN, MEAS, MAX_SLOTS, MODE_COV, true, W, false, MH>
                       : k_gn<DYN, MEAS, MAX_SLOTS, MODE_COV, false, W, false, MH>;
        else
          return nullptr;
      }
      if constexpr (MH)
        return nullptr;
      else
        return k_gn<DYN, MEAS, MAX_SLOTS, MODE_LINSOLVE>;
    };
    GnKernel kern = nullptr;
    if (ch.mhuber) {
      // robust measurement rows: scalar rows of a nonlinear model only have these instances
      if constexpr (!MEAS::LINEAR && MEAS::p == 1) kern = pick(std::true_type{});
    } else {
      kern = pick(std::false_type{});
    }
    if (!kern) return MHE_ERR_UNSUPPORTED;
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem) != hipSuccess)
      return MHE_ERR_HIP;
    hipLaunchKernelGGL(kern, dim3(batch), dim3(NTHREADS), smem, st, a);
    return hipGetLastError() == hipSuccess ? MHE_OK : MHE_ERR_HIP;
  }
}

// k_gn_general (mhe_general.h), the instance of the mixed pairs with n <= 16: one launch per
// batch, one workgroup per trajectory.  MINW = 2: with 128 VGPRs (MINW = 4) every instance
// spills (58 .. 405 VGPRs), and the LDS layout of the shapes this path is for (two-receiver
// N = 10: 121 KB used) admits one workgroup per CU anyway.
constexpr int FG_MINW = 2;
template <class DYN, class MEAS>
int launch_gn_general(const mhe_dims* dm, GnArgs& a, int batch, hipStream_t st) {
  if constexpr (MEAS::MIXED && DYN::n <= 16) {
    const int EC = fg_epoch_cap(a.P, a.M > 0 ? a.M : 1, DYN::n, a.NT, a.nz, a.nc);
    const int smem = fg_smem_layout(a.P, a.M < EC ? a.M : EC, DYN::n, a.NT, a.nz, a.nc).total * (int)sizeof(double);
    if (EC < 1 || smem > REG_LDS_LIMIT) return MHE_ERR_UNSUPPORTED;
    void (*kern)(GnArgs) = k_gn_general<DYN, MEAS, MAX_SLOTS, FG_MINW>;
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem) != hipSuccess)
      return MHE_ERR_HIP;
    hipLaunchKernelGGL(kern, dim3(batch), dim3(NTHREADS), smem, st, a);
    return hipGetLastError() == hipSuccess ? MHE_OK : MHE_ERR_HIP;
  } else {
    return MHE_ERR_UNSUPPORTED;
  }
}

template <class DYN, class MEAS>
int launch_build_cc(const mhe_dims* dm, int NT, const double* D, const double* cw, const double* Phi,
                    const double* Qw, const double* Rw, const double* Pw, char* cbuf, hipStream_t st) {
  if constexpr (MEAS::MIXED && DYN::n > 16) {
    return MHE_ERR_UNSUPPORTED;
  } else {  // (mixed rows, n <= 16: the tile tables of k_gn_general -- no measurement term in Cc)
    const int ntiles = NT * (NT + 1) / 2;
    hipLaunchKernelGGL(k_build_cc<MEAS>, dim3((ntiles * 256 + 255) / 256), dim3(256), 0, st, dm->N + 1, dm->M,
                       dm->n, dm->p, NT, dm->has_prior, dm->dyn_cost == MHE_COST_HUBER ? 1 : 0, 2.0 / dm->T, D, cw,
                       Phi, Qw, Rw, Pw, cbuf);
    return hipGetLastError() == hipSuccess ? MHE_OK : MHE_ERR_HIP;
  }
}

// The factorization of the large-system path: left-looking block-column updates (default;
// 38 % less HBM traffic than the right-looking trailing update, C3 +5 %, C4 +7.5 %, C5 +8 %);
// the right-looking form (bitwise-identical iterates, tests/test_gpu_big.py) only when a
// caller selected it with mhe_set_option(MHE_OPT_BIG_RIGHT_LOOKING, 1).  The left-looking
// form is always split: launches per block column (k_big_chol SPLIT = 1, then k_big_rows over
// the rows below, one workgroup per 8 rows) and one for the solve (SPLIT = 2) -- C4 +8.9 %,
// C5 +8.2 % over one launch (profiles/r05_ab_big_split.txt), and since round 6 C3 too.
struct BigCholPlan {
  void (*mono)(BigArgs, int);  // the right-looking factorization and solve, one launch (!split)
  void (*diag)(BigArgs, int);  // split: a block column's diagonal stage
  void (*bwd)(BigArgs, int);   // split: the backward solve
  int smem, smem_rows, smem_diag;
  bool split;  // the left-looking form
};
// prec: the instances with the pivots' second Newton step (BIG_STAGE_COV)
inline int big_chol_plan(const BigArgs& A, BigCholPlan& p, bool prec = false) {
  const bool wide = A.NT >= BIG_WIDE_NT;
  p.smem = big_chol_lds(wide ? 8 : 4) * (int)sizeof(double);
  p.smem_rows = big_rows_lds() * (int)sizeof(double);
  p.split = g_opt_big_right_looking == 0;
  p.mono = wide ? k_big_chol<8> : k_big_chol<4>;
  if (prec) p.mono = wide ? k_big_chol<8, false, 0, true> : k_big_chol<4, false, 0, true>;
  // the split diagonal stage keeps its rows' update in registers and stages small slabs at
  // any width: the 4-wide instance's LDS, two workgroups per CU
  p.diag = prec ? k_big_chol<4, true, 1, true> : k_big_chol<4, true, 1>;
  p.smem_diag = big_chol_lds(4) * (int)sizeof(double);
  p.bwd = wide ? k_big_chol<8, true, 2> : k_big_chol<4, true, 2>;
  for (auto f : {p.mono, p.bwd})
    if (hipFuncSetAttribute((const void*)f, hipFuncAttributeMaxDynamicSharedMemorySize, p.smem) != hipSuccess)
      return -1;
  if (hipFuncSetAttribute((const void*)p.diag, hipFuncAttributeMaxDynamicSharedMemorySize, p.smem_diag) != hipSuccess)
    return -1;
  if (hipFuncSetAttribute((const void*)k_big_rows<>, hipFuncAttributeMaxDynamicSharedMemorySize, p.smem_rows) !=
      hipSuccess)
    return -1;
  return 0;
}
// One half of the batch through the split stages (trajectories boff .. boff + nb - 1);
// after_first (two-stream form): recorded on st after the first diagonal stage.
inline void launch_big_split(const BigCholPlan& p, BigArgs A, int boff, int nb, hipStream_t st,
                             hipEvent_t after_first = nullptr) {
  A.ws += (size_t)boff * A.ws_stride;  // the stages index trajectories by workgroup only
  A.state += boff;
  for (int k0 = 0, kend; k0 < A.NT; k0 = kend) {
    hipLaunchKernelGGL(p.diag, dim3(nb), dim3(BIG_NTHREADS), p.smem_diag, st, A, k0);
    if (k0 == 0 && after_first) (void)hipEventRecord(after_first, st);
    kend = big_split_kend(k0, A.NT);  // the same partition as the stages'

    if (kend < A.NT)
      hipLaunchKernelGGL(k_big_rows<>, dim3((A.NT - kend + BIG_NW - 1) / BIG_NW, nb), dim3(BIG_NTHREADS),
                         p.smem_rows, st, A, k0);
  }
  hipLaunchKernelGGL(p.bwd, dim3(nb), dim3(BIG_NTHREADS), p.smem, st, A, 0);
}

// The second stream and fork / join events of the two-stream split factorization, one set
// per device, created on first use (nullptr: run on one stream).  Concurrent callers:
// launch_big_factor holds `use` from its fork record to its join wait, so no other caller
// re-records the events in between (a stream wait captures the event's last record at
// enqueue time); their second halves share s2 (serialised, each behind its own fork).
struct BigAux {
  hipStream_t s2;
  hipEvent_t fork, join;
  std::mutex use;
};
inline BigAux* big_aux(hipStream_t st) {
  static BigAux aux[16];
  static int made[16] = {0};
  static std::mutex mu;
  int dev = 0, sdev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  // the second stream is created on the current device: only when the launch stream is on it
  if (hipStreamGetDevice(st, &sdev) != hipSuccess || sdev != dev) return nullptr;
  std::lock_guard<std::mutex> lock(mu);
  if (!made[dev]) {
    if (hipStreamCreateWithFlags(&aux[dev].s2, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&aux[dev].fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&aux[dev].join, hipEventDisableTiming) != hipSuccess)
      return nullptr;
    made[dev] = 1;
  }
  return &aux[dev];
}

// The factorization + solve.  Split: the two halves of the batch go through the stages on
// two streams, so one half's latency-bound diagonal stages and solve overlap the other
// half's row launches (what the one-launch kernel gets from trajectories at different
// phases; C5 +6.2 %, C3 +1.5 %, C4 0).
inline void launch_big_factor(const BigCholPlan& p, const BigArgs& A, int batch, hipStream_t st) {
  if (!p.split) {
    hipLaunchKernelGGL(p.mono, dim3(batch), dim3(BIG_NTHREADS), p.smem, st, A, 0);
    return;
  }
  BigAux* aux = batch >= 16 ? big_aux(st) : nullptr;
  if (!aux) {
    launch_big_split(p, A, 0, batch, st);
    return;
  }
  std::lock_guard<std::mutex> hold(aux->use);  // this caller's record -> wait pairs, uninterleaved
  const int h = ((batch / 2) + 7) & ~7;  // a multiple of 8 (k_big_rows' XCD grouping)
  // the second half starts one diagonal stage behind the first, so that the halves'
  // latency-bound diagonal stages alternate with the other half's row launches
  launch_big_split(p, A, 0, h, st, aux->fork);
  if (hipStreamWaitEvent(aux->s2, aux->fork, 0) != hipSuccess) {
    (void)hipStreamSynchronize(st);
  }
  launch_big_split(p, A, h, batch - h, aux->s2);
  if (hipEventRecord(aux->join, aux->s2) != hipSuccess || hipStreamWaitEvent(st, aux->join, 0) != hipSuccess)
    (void)hipStreamSynchronize(aux->s2);  // the join failed: wait on the host instead
}

// k_big_assemble's launch shape: per tile position ceil(nchl / WPB) workgroups of WPB
// live pair chunks (the epoch GEMM's operands staged through LDS, big_asm_lds), then the
// other chunks WPB (position, chunk) items per workgroup
struct BigAsmShape {
  int wpb, blocks, lds;
};
inline BigAsmShape big_asm_shape(const BigArgs& A) {
  const int npos = A.NTc * (A.NTc + 1) / 2;
  BigAsmShape s;
  s.wpb = A.nchl > 0 ? (A.nchl < 4 ? A.nchl : 4) : (A.nch < 4 ? A.nch : 4);
  s.blocks = npos * ((A.nchl + s.wpb - 1) / s.wpb) + (npos * (A.nch - A.nchl) + s.wpb - 1) / s.wpb;
  s.lds = big_asm_lds(s.wpb) * (int)sizeof(double);
  return s;
}

// k_big_resid with its dynamic LDS (X staged: P n doubles; C5 64 KB)
template <class DYN, class MEAS>
inline int launch_big_resid(const BigArgs& A, int batch, int final_pass, hipStream_t st) {
  const int smem = A.P * A.n * (int)sizeof(double);
  void (*kern)(BigArgs, int) = k_big_resid<DYN, MEAS>;
  if (A.md) {  // robust measurement rows (meas_delta): scalar rows of a nonlinear model
    if constexpr (!MEAS::LINEAR && MEAS::p == 1)
      kern = k_big_resid<DYN, MEAS, true>;
    else
      return MHE_ERR_UNSUPPORTED;
  }
  if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem) != hipSuccess)
    return MHE_ERR_HIP;
  hipLaunchKernelGGL(kern, dim3(batch), dim3(BIG_NTHREADS), smem, st, A, final_pass);
  return MHE_OK;
}

// Kernel-level parity stages of the large-system path (mhe_assemble_ws /
// mhe_chol_solve_ws): BIG_STAGE_ASSEMBLE runs k_big_resid + k_big_assemble at A.X (H
// tiles and BV = -g in the workspace, cost; with z also the per-epoch border sums),
// BIG_STAGE_FACTOR runs k_big_chol on the workspace's tiles and BV (delta in YV) and,
// for a bordered system, k_big_border on the border the caller imported (w in KS).
// BIG_STAGE_COV (mhe_state_cov) runs both at A.X -- the factorization plan a solve would
// pick -- and then k_big_cov: the query columns A.PhiQ through the factor, A.cov.
// The state words are set by the caller.
// BIG_STAGE_KKT_COV (mhe_kkt_cov) is BIG_STAGE_COV for any large-system problem: with a
// border (A.nz + A.nc > 0) the last launch is k_big_kkt_cov -- the step's own border through
// the factor and its Schur complement, A.cov and A.covz -- else k_big_cov as it is.
constexpr int BIG_STAGE_ASSEMBLE = 0, BIG_STAGE_FACTOR = 1, BIG_STAGE_COV = 2, BIG_STAGE_KKT_COV = 3;
constexpr int BIG_LDS_LIMIT = 64 * 1024;  // k_big_kkt_cov's dynamic LDS (K = MHE_MAX_EQ, n = 40: 49 KB)
template <class DYN, class MEAS>
int launch_big_stage(const mhe_dims* dm, BigArgs& A, int batch, int stage, hipStream_t st) {
  if (stage == BIG_STAGE_KKT_COV && A.nz + A.nc > 0) {
    const int smem_c = big_kkt_cov_lds(A.nz + A.nc, DYN::n, A.nz) * (int)sizeof(double);
    if (smem_c > BIG_LDS_LIMIT) return MHE_ERR_UNSUPPORTED;  // checked before anything is enqueued
    void (*kern)(BigArgs, int) = k_big_kkt_cov<DYN::n, MEAS::p>;
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem_c) != hipSuccess)
      return MHE_ERR_HIP;
    int rc = launch_big_stage<DYN, MEAS>(dm, A, batch, BIG_STAGE_ASSEMBLE, st);
    if (rc != MHE_OK) return rc;
    BigCholPlan cp;
    if (big_chol_plan(A, cp, true) < 0) return MHE_ERR_HIP;  // refined pivots, as BIG_STAGE_COV
    launch_big_factor(cp, A, batch, st);
    hipLaunchKernelGGL(kern, dim3(batch), dim3(BIG_NTHREADS), smem_c, st, A, cp.split ? 1 : 0);
    return hipGetLastError() == hipSuccess ? MHE_OK : MHE_ERR_HIP;
  }
  if (stage == BIG_STAGE_COV || stage == BIG_STAGE_KKT_COV) {
    if (A.nz + A.nc > 0) return MHE_ERR_UNSUPPORTED;
    int rc = launch_big_stage<DYN, MEAS>(dm, A, batch, BIG_STAGE_ASSEMBLE, st);
    if (rc != MHE_OK) return rc;
    // the plan a solve would pick, its pivots refined once more (rsqrt_pivot<true>): with the
    // solve's pivots the C3 covariance sat at 18 times the conditioning floor of the reference
    BigCholPlan cp;
    if (big_chol_plan(A, cp, true) < 0) return MHE_ERR_HIP;
    launch_big_factor(cp, A, batch, st);
    hipLaunchKernelGGL(k_big_cov<DYN::n>, dim3(batch), dim3(BIG_NTHREADS), 0, st, A, cp.split ? 1 : 0);
    return hipGetLastError() == hipSuccess ? MHE_OK : MHE_ERR_HIP;
  }
  if (stage == BIG_STAGE_ASSEMBLE) {
    big_pair_plan(A, BigGSupport<MEAS>::get(A.idx, A.n));
    const BigAsmShape sh = big_asm_shape(A);
    if (launch_big_resid<DYN, MEAS>(A, batch, 0, st) != MHE_OK) return MHE_ERR_HIP;
    hipLaunchKernelGGL((k_big_assemble<DYN, MEAS>), dim3(sh.blocks, batch), dim3(64 * sh.wpb), sh.lds, st, A);
  } else {
    BigCholPlan cp;
    if (big_chol_plan(A, cp) < 0) return MHE_ERR_HIP;
    launch_big_factor(cp, A, batch, st);
    const int K = A.nz + A.nc;  // the bordered (KKT) step through the factor, as the solve's
    if (K > 0) {
      const int smem_b = (K * K + 2 * K) * (int)sizeof(double);
      if (hipFuncSetAttribute((const void*)k_big_border<DYN::n, MEAS::p>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              smem_b) != hipSuccess)
        return MHE_ERR_HIP;
      hipLaunchKernelGGL((k_big_border<DYN::n, MEAS::p>), dim3(batch), dim3(BIG_NTHREADS), smem_b, st, A);
    }
  }
  return hipGetLastError() == hipSuccess ? MHE_OK : MHE_ERR_HIP;
}

template <class DYN, class MEAS>
int launch_big(const mhe_dims* dm, BigArgs& A, int batch, int max_iter, hipStream_t st) {
  big_pair_plan(A, BigGSupport<MEAS>::get(A.idx, A.n));
  BigCholPlan cp;
  if (big_chol_plan(A, cp) < 0) return MHE_ERR_HIP;
  const int K = A.nz + A.nc;
  const int smem_b = (K * K + 2 * K) * (int)sizeof(double);
  if (K > 0 && hipFuncSetAttribute((const void*)k_big_border<DYN::n, MEAS::p>,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, smem_b) != hipSuccess)
    return MHE_ERR_HIP;
  const bool bounded = A.n_bounds > 0;
  const int smem_ls = A.P * A.n * (int)sizeof(double);
  void (*k_ls)(BigArgs) = k_big_linesearch<DYN, MEAS>;
  if constexpr (!MEAS::LINEAR && MEAS::p == 1)
    if (A.md) k_ls = k_big_linesearch<DYN, MEAS, true>;  // the robust cost along the arc
  if (bounded) {
    if (smem_ls > 128 * 1024) return MHE_ERR_UNSUPPORTED;
    if (hipFuncSetAttribute((const void*)k_ls, hipFuncAttributeMaxDynamicSharedMemorySize, smem_ls) != hipSuccess)
      return MHE_ERR_HIP;
    const size_t nx = (size_t)batch * A.P * A.n;
    hipLaunchKernelGGL(k_big_project<DYN::n>, dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, st, A, batch);
  }
  const BigAsmShape sh = big_asm_shape(A);
  for (int it = 0; it < max_iter; ++it) {
    if (launch_big_resid<DYN, MEAS>(A, batch, 0, st) != MHE_OK) return MHE_ERR_HIP;
    A.asm_zskip = it > 0 && cp.split;  // the previous iteration's factorization left its envelope's zeros
    hipLaunchKernelGGL((k_big_assemble<DYN, MEAS>), dim3(sh.blocks, batch), dim3(64 * sh.wpb), sh.lds, st, A);
    A.asm_zskip = 0;
    launch_big_factor(cp, A, batch, st);
    if (K > 0) hipLaunchKernelGGL((k_big_border<DYN::n, MEAS::p>), dim3(batch), dim3(BIG_NTHREADS), smem_b, st, A);
    if (bounded)
      hipLaunchKernelGGL(k_ls, dim3(batch), dim3(BIG_NTHREADS), smem_ls, st, A);
    else
      hipLaunchKernelGGL((k_big_update<DYN::n>), dim3(batch), dim3(256), 0, st, A);
  }
  if (launch_big_resid<DYN, MEAS>(A, batch, 1, st) != MHE_OK) return MHE_ERR_HIP;
  return hipGetLastError() == hipSuccess ? MHE_OK : MHE_ERR_HIP;
}

template <class DYN, class MEAS>
const PairOps* pair_ops() {
  static const PairOps ops = {&launch_build_cc<DYN, MEAS>, &launch_gn<DYN, MEAS>, &launch_big<DYN, MEAS>,
                              &launch_resjac<DYN, MEAS>, &launch_big_stage<DYN, MEAS>,
                              &launch_gn_general<DYN, MEAS>};
  return &ops;
}

// Pair groups, one translation unit each (pair_*.hip): the ops of (dyn, meas) or nullptr.
const PairOps* pairs_vdp(int dyn, int meas);
const PairOps* pairs_integrators(int dyn, int meas);
const PairOps* pairs_gnss(int dyn, int meas);
const PairOps* pairs_vehicles(int dyn, int meas);
const PairOps* pairs_autocar(int dyn, int meas);
const PairOps* pairs_receivers(int dyn, int meas);

}  // namespace mhe
