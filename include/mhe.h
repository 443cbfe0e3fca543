/*
 * mhe.h -- C-ABI of libmhe.so, the MI355X (gfx950) batched collocation
 * Gauss-Newton estimator.
 *
 * This is the drop-in boundary under the reference's solver facade:
 *
 *   reference                                   replaced by
 *   ------------------------------------------  -----------------------------------
 *   NLP.build()      nlp/nlp.py:61-69           mhe_const_bytes + mhe_build_constants
 *   NLP.solve()      nlp/nlp.py:76-83           mhe_gn_solve  (CasADi Opti + IPOPT ->
 *                                               hand-written HIP Gauss-Newton)
 *   addDynamics/addDynamicsCost/addResidualCost/addInitialCost
 *                    nlp/nlp.py:202-286         the objective those calls record is
 *                                               what mhe_gn_solve minimises; its pieces
 *                                               are exported for kernel-level parity:
 *                                               mhe_assemble (J^T W J, J^T W r, cost)
 *                                               mhe_chol_solve (dense SPD solve)
 *   extractSolution  nlp/nlp.py:99-119          host side (Lagrange interpolation)
 *
 * Conventions
 *   - every pointer argument except `dims` and the host-side constant tables
 *     of mhe_build_constants is a DEVICE pointer owned by the caller (torch
 *     tensors in the Python host; hipMalloc'd memory from C);
 *   - fp64 everywhere, row-major, batch outermost; a batch stride of 0 means
 *     "shared by every trajectory";
 *   - no hidden allocation, no host synchronisation: every call only enqueues
 *     work on `stream` (graph-capturable);
 *   - returns MHE_OK (0) or a negative MHE_ERR_* code; per-trajectory solver
 *     outcomes are reported in `status_out` (MHE_STATUS_*), never by aborting
 *     the batch;
 *   - calls that share a constants buffer may run concurrently on different
 *     streams; a constants buffer is read-only after mhe_build_constants.
 */
#ifndef MHE_H
#define MHE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* return codes */
#define MHE_OK 0
#define MHE_ERR_DIMS (-1)        /* dims inconsistent with the models / limits */
#define MHE_ERR_MODEL (-2)       /* unknown dynamics or measurement model id   */
#define MHE_ERR_HIP (-3)         /* a HIP runtime call failed                  */
#define MHE_ERR_UNSUPPORTED (-4) /* valid request this build does not handle   */
#define MHE_ERR_NULL (-5)        /* required pointer is NULL                   */

/* per-trajectory solver status (status_out) */
#define MHE_STATUS_CONVERGED 0   /* max|delta| <= tol * (1 + max|X|)           */
#define MHE_STATUS_MAX_ITER 1    /* max_iter Gauss-Newton steps taken          */
#define MHE_STATUS_NOT_SPD 2     /* Cholesky pivot <= 0 (J^T W J not SPD)      */
#define MHE_STATUS_NONFINITE 3   /* NaN/Inf in the step                        */
#define MHE_STATUS_BAD_CONSTANTS 4 /* const_buf was not built for these dims (its tag
                                      differs): nothing was computed, X_out = X0     */

/* dynamics plug-ins (reference nlp/dynamics.py) */
#define MHE_DYN_SINGLE_INTEGRATOR 1      /* :4-8    n=1  m=1 */
#define MHE_DYN_SINGLE_INTEGRATOR_2D 2   /* :10-17  n=2  m=2 */
#define MHE_DYN_SINGLE_INTEGRATOR_3D 3   /* :19-27  n=3  m=3 */
#define MHE_DYN_DOUBLE_INTEGRATOR 4      /* :29-38  n=4  m=2 */
#define MHE_DYN_VAN_DER_POL 5            /* :61-66  n=2  m=1 */
#define MHE_DYN_GNSS_POS_AND_BIAS 6      /* :68-79  n=5  m=3 */
#define MHE_DYN_MULTI_RECEIVER 7         /* :81-96  n=8  m=0 */
#define MHE_DYN_GNSS_TWO_RECEIVER 8      /* :98-115 n=10 m=6 */
#define MHE_DYN_KINEMATIC_BICYCLE 9      /* :117-136 n=6 m=2 (kinematic_bycicle_and_bias) */
#define MHE_DYN_GNSS_8_RECEIVERS 11      /* 8 receivers x the :98-115 block [x,y,z,b,alpha]:
                                            n=40 m=24 */
#define MHE_DYN_VEHICLE_GNSS 10          /* :148-174 n=9 m=2 (vehicle_dynamics_and_gnss);
                                            dyn_par = params["car_params"] as
                                            [C_AF, C_AR, M, D_F, D_R, I_Z] */

/* measurement plug-ins (reference nlp/measurements.py) */
#define MHE_MEAS_FULL_STATE 1            /* :4-5   p=n, linear            */
#define MHE_MEAS_PSEUDORANGE 2           /* :56-70 p=1, q=3 (sat_pos), idx[4] */
#define MHE_MEAS_VEHICLE_PSEUDORANGE 3   /* :81-88 p=1, q=3 (x[0], x[1], x[8]; bias x[6]) */
#define MHE_MEAS_RANGE_3D 4              /* :39-54 p=1, q=3 ("y" form), idx[3] */
#define MHE_MEAS_MIXED 5                 /* several scalar plug-ins in one problem (one
                                            addResidualCost call each, nlp/nlp.py:258-277):
                                            p=1, q=MHE_MIXED_Q, every row names its model */

/* MHE_MEAS_MIXED rows: PAR row = [code, i0..i6, v0..v5] (q = 14).  Indices point
 * into the augmented vector [x(t_i) (n) ; z (n_extra)] -- z are the extra decision
 * variables (addVariables beyond the state, e.g. XA in multi-receiver.py:73,99);
 * -1 = unused term.  h per code (reference nlp/measurements.py):
 *   PSEUDORANGE       :56-70  |x[i0..i2] - v0..2| + x[i3]
 *   PSEUDORANGE_RATE  :72-79  (v3..5 - x[i3..i5]) . (v0..2 - x[i0..i2]) / |.| + x[i6]
 *   RANGE_2D          :7-20   sqrt(sum_k (x[i_k] - x[i_{k+2}] - v_k)^2 + 1e-6), k < 2
 *   RANGE_3D          :39-54  sqrt(sum_k (x[i_k] - x[i_{k+3}] - v_k)^2 + 1e-6), k < 3
 *                             (both forms: "idxA/idxB" -> i = A, B; "y" -> i = idx, -1
 *                             and v = y, or with y a decision variable i = idx, n + j)
 *   HEADING_2D        :22-37  atan2(x[i0] - x[i1] + v0, x[i2] - x[i3] + v1)
 *   COMPONENT         :4-5    x[i0] (full_state as scalar rows)
 *   NONE                      h = 0 (padding row; give it R = 0) */
#define MHE_MIXED_Q 14
#define MHE_ROW_NONE 0
#define MHE_ROW_PSEUDORANGE 1
#define MHE_ROW_PSEUDORANGE_RATE 2
#define MHE_ROW_RANGE_2D 3
#define MHE_ROW_RANGE_3D 4
#define MHE_ROW_HEADING_2D 5
#define MHE_ROW_COMPONENT 6
#define MHE_MAX_EXTRA 4   /* extra decision variables per trajectory */
#define MHE_MAX_EQ 48     /* n_extra + n_eq */

/* Every dims struct starts with struct_size: the caller sets it to sizeof() of
 * the struct it declares, and every entry point returns MHE_ERR_DIMS (0 / -1 for
 * the size queries) unless it equals this build's sizeof -- a binding that
 * declares an older or truncated struct is refused before any later field is
 * read.  (mhe/_lib.py sets it in the ctypes constructors.) */
#define MHE_ABI_VERSION 11

typedef struct mhe_dims {
  int32_t struct_size;  /* = sizeof(mhe_dims)                                */
  int32_t N;            /* collocation order; P = N + 1 CGL nodes            */
  int32_t n;            /* state dimension   (must equal the model's)        */
  int32_t m;            /* control dimension (must equal the model's)        */
  int32_t p;            /* rows of one measurement (model's)                 */
  int32_t M;            /* number of measurement times in the window         */
  int32_t q;            /* per-row measurement parameters (0 if none)        */
  int32_t dyn_model;    /* MHE_DYN_*                                         */
  int32_t meas_model;   /* MHE_MEAS_*                                        */
  int32_t has_prior;    /* 1: addInitialCost term present                    */
  int32_t meas_idx[8];  /* static index params (params["idx"]), model-defined */
  double T;             /* window length; node times tau2t(tau)              */
  int32_t dyn_cost;     /* MHE_COST_L2 (weighted_l2_norm) or MHE_COST_HUBER  */
  int32_t n_bounds;     /* addVarBounds: number of bounded state components  */
  double huber_delta;   /* pseudo_huber_loss params["delta"]                 */
  int32_t bound_idx[8]; /* bounded component indices (< n)                   */
  double bound_lb[8];   /* lower / upper bounds (+-inf allowed), every node  */
  double bound_ub[8];
  int32_t n_extra;      /* extra decision variables z (<= MHE_MAX_EXTRA); they
                           enter MHE_MEAS_MIXED rows only                        */
  int32_t n_eq;         /* addEqConstraint(equality_constaint, [a, b]) rows
                           (nlp/nlp.py:52-53, nlp/constraints.py): v[a] - v[b] = 0 */
  const int32_t* eq_idx;/* HOST pointer, 2*n_eq entries (a, b) into the flattened
                           state vector v = X (P*n, node-major: j*n + c); b = -1
                           means v[a] = 0.  Copied into the constants buffer at
                           build time and part of its layout stamp (with eq_rhs):
                           solving with other rows than the buffer was built with
                           returns MHE_STATUS_BAD_CONSTANTS -- rebuild instead.     */
  int32_t force_large;  /* path preference, MHE_PATH_* below.  MHE_PATH_LARGE: take the
                           large-system path even when the problem fits the
                           register-resident kernel (parity tests of the two paths on
                           identical inputs).  MHE_PATH_FUSED_GENERAL: see below.  The
                           path is a function of dims alone; mhe_build_constants stamps
                           it (with the layout-defining dims) into the constants buffer
                           and every solve checks that stamp on the device.        */
  double dyn_par[8];    /* static dynamics parameters (model-defined, e.g.
                           MHE_DYN_VEHICLE_GNSS); 0 for the parameter-free models   */
  const double* eq_rhs; /* HOST pointer, n_eq constants r_i of the rows
                           v[a] - v[b] = r_i, or NULL (all 0: addEqConstraint rows).
                           Non-zero r: the rows an active set imposes (bounds and
                           inequality constraints held at equality by the host) */
} mhe_dims;

/* mhe_dims.force_large.  Any value other than AUTO and FUSED_GENERAL is LARGE.
 *
 * MHE_PATH_FUSED_GENERAL (MHE_HAS_FUSED_GENERAL) is a preference: a MHE_MEAS_MIXED problem
 * (with or without n_extra / n_eq) runs the fused kernel k_gn_general -- one launch per batch,
 * one workgroup per trajectory, no workspace -- when dyn_cost is MHE_COST_L2, n_bounds == 0,
 * n <= 16, the node-major padded system 16 ceil(P n / 16) is at most 208 and the kernel's
 * LDS layout fits (all functions of dims alone).  For every other dims, typed problems
 * included, the value behaves as MHE_PATH_AUTO.  For such fused-general dims
 *   mhe_workspace_bytes = 0, mhe_padded_dim = 16 ceil(P n / 16), mhe_kkt_dim = that + K,
 *   mhe_const_bytes / mhe_build_constants use the fused layout (own stamp),
 *   mhe_solve honours Z0, Rw, Pw and lambda_out and solves the same bordered GN steps as
 *   the large-system path (other summation order: results agree to rounding, not bitwise);
 *   mhe_solve with meas_delta, mhe_chol_solve_ws, mhe_kkt_cov, mhe_kkt_arrival and
 *   mhe_resjac return MHE_ERR_UNSUPPORTED before any launch (as do the register-path
 *   parity calls): build a second set of constants with MHE_PATH_AUTO for those.
 * The kernel groups measurement rows by epoch (bitwise-identical Phi rows) in LDS;
 * mhe_build_constants returns MHE_ERR_UNSUPPORTED when Phi has more distinct rows than the
 * layout holds (it copies one word back and waits for the stream: the only build that
 * synchronises) -- use MHE_PATH_AUTO then. */
#define MHE_PATH_AUTO 0
#define MHE_PATH_LARGE 1
#define MHE_PATH_FUSED_GENERAL 2
#define MHE_HAS_FUSED_GENERAL 1

/* Dynamics cost (addDynamicsCost, nlp/nlp.py:242-245): */
#define MHE_COST_L2 0     /* cost_functions.weighted_l2_norm  (cost_functions.py:20-22) */
#define MHE_COST_HUBER 1  /* cost_functions.pseudo_huber_loss (cost_functions.py:25-31): IRLS
                             weights q_a / sqrt(1 + W_a^2 / delta^2), only diag(Qw) enters */
/* Bounds (addVarBounds, nlp/nlp.py:314-317) are enforced by a projected Newton
 * method on the GN model (Bertsekas 1982): the iterate starts projected onto the
 * box, each step is the GN step reduced to the free unknowns (epsilon-active set)
 * followed by an Armijo search along the projection arc; MHE_STATUS_CONVERGED
 * then means a KKT point of the bounded problem (max|P(X + d) - X| <= tol (1 + max|X|)).
 * Extra variables and equality constraints run on the
 * large-system path: each GN step solves the bordered (KKT) system
 *   [ H    H_xz  C^T ] [dx]   [-g  ]
 *   [ H_zx H_zz  0   ] [dz] = [-g_z]
 *   [ C    0     0   ] [l ]   [-c  ]
 * through the Cholesky factor of H (one multi-RHS solve of the border columns,
 * a small quasi-definite LDL^T of the Schur complement).  Linear constraints are
 * therefore met exactly after every step.  Bounds and constraints together are
 * not supported (MHE_ERR_UNSUPPORTED). */

/* Process-wide A/B options, for measurements and tests only; nothing else (no
 * environment variable) changes what a solve runs.  Returns the previous value, or
 * MHE_ERR_DIMS for an unknown option or a value out of range.
 *   MHE_OPT_BIG_RIGHT_LOOKING  1: the large-system factorization's right-looking
 *                              trailing-update form (bitwise-identical iterates,
 *                              slower); 0 (default): left-looking block columns
 *   MHE_OPT_DEBUG_SMEM_PAD     bytes of LDS added to the fused kernel's launch
 *                              (forces lower occupancy; default 0)
 *   MHE_OPT_LSM_GROUP          16 or 64: mhe_ls_multi_run launches that lane-group
 *                              instance whatever the row capacity; 0 (default): the
 *                              row-capacity rule (mhe_ls_multi_group)
 * Not thread-safe against concurrent launches: set it before enqueueing work. */
#define MHE_OPT_BIG_RIGHT_LOOKING 1
#define MHE_OPT_DEBUG_SMEM_PAD 2
#define MHE_OPT_LSM_GROUP 3
int32_t mhe_set_option(int32_t option, int32_t value);

/* Size in bytes of the device constants buffer for `dims` (0 on bad dims).  The
 * first 256 bytes are a header holding the layout stamp written by
 * mhe_build_constants (offset 0: every solve checks it in bounds). */
size_t mhe_const_bytes(const mhe_dims* dims);

/*
 * Build the per-problem device constants (one-time, NLP.build()).
 *   D    (P,P)    negated CGL differentiation matrix   (collocation.py:42-64)
 *   cw   (P)      (T/2) * w_k, w the reference weights   (nlp/nlp.py:245)
 *   Phi  (M,P)    Lagrange basis at the measurement times (nlp/nlp.py:266)
 *   Qw   (n,n)    dynamics-cost weight = params["Q"] of weighted_l2_norm
 *   Rw   (M,p,p)  measurement information R passed to addResidualCost
 *   Pw   (n,n)    prior weight (may be NULL when !has_prior)
 * All six are DEVICE pointers; `const_buf` is a caller-owned device buffer of
 * mhe_const_bytes(dims) bytes.
 */
int mhe_build_constants(const mhe_dims* dims, const double* D, const double* cw,
                        const double* Phi, const double* Qw, const double* Rw,
                        const double* Pw, void* const_buf, void* stream);

/*
 * Batched Gauss-Newton solve (NLP.solve()).  One trajectory per workgroup;
 * the whole GN loop (residual + Jacobian, J^T W J / J^T W r assembly,
 * Cholesky, triangular solves, update) runs inside one launch.
 *   X0     (B,P,n)    initial iterate (warm start = previous solution)
 *   X_out  (B,P,n)    solution (may alias X0)
 *   U      (B|1,P,m)  controls at the nodes (setControl, nlp/nlp.py:304-308);
 *                     NULL when m == 0
 *   Y      (B,M,p)    measurements
 *   PAR    (B|1,M,q)  per-row measurement params (sat_pos ...); NULL if q == 0
 *   x0     (B,n)      prior mean (addInitialCost); NULL when !has_prior
 *   cost_out (B) objective at X_out; iters_out (B) GN steps; status_out (B)
 */
int mhe_gn_solve(const mhe_dims* dims, const void* const_buf, int32_t batch,
                 const double* X0, double* X_out,
                 const double* U, int64_t u_bstride,
                 const double* Y,
                 const double* PAR, int64_t par_bstride,
                 const double* x0,
                 double* cost_out, int32_t* iters_out, int32_t* status_out,
                 int32_t max_iter, double tol, void* stream);

/* Padded system size used by the kernels: 16 * ceil(P*n / 16) on the
 * register-resident path (<= 208); n * 16 * ceil(P / 16) (component-major
 * ordering) on the large-system path. */
int32_t mhe_padded_dim(const mhe_dims* dims);

/*
 * Workspace the large-system path needs for `batch` trajectories (bytes; 0 when
 * the problem fits the register-resident kernel, which needs none).  Holds the
 * per-trajectory H tiles, L_kk^-T blocks and iteration scratch.
 */
size_t mhe_workspace_bytes(const mhe_dims* dims, int32_t batch);

/*
 * mhe_gn_solve with a caller-owned device workspace of >= mhe_workspace_bytes
 * (required when the padded system exceeds the register-resident limit: C3-C5,
 * d = 1005 / 3006 / 8040).  Same arguments and results as mhe_gn_solve, which is
 * this call with workspace = NULL (and returns MHE_ERR_NULL for such problems).
 * Enqueues max_iter iterations of stream-ordered kernels; trajectories that
 * converge or fail are frozen on the device, so no host synchronisation occurs.
 */
int mhe_gn_solve_ws(const mhe_dims* dims, const void* const_buf, int32_t batch,
                    const double* X0, double* X_out,
                    const double* U, int64_t u_bstride,
                    const double* Y, const double* PAR, int64_t par_bstride,
                    const double* x0,
                    double* cost_out, int32_t* iters_out, int32_t* status_out,
                    int32_t max_iter, double tol, void* workspace, size_t workspace_bytes,
                    void* stream);

/*
 * mhe_gn_solve_ws with extra decision variables: Z0 / Z_out (B, n_extra) device
 * arrays (initial values / solution; NULL when n_extra == 0).  Problems with
 * n_extra > 0, n_eq > 0 or MHE_MEAS_MIXED always take the large-system path
 * (workspace required).  The stopping rule covers z too:
 * max|(dx, dz)| <= tol * (1 + max|(X, z)|).
 */
int mhe_gn_solve_ext(const mhe_dims* dims, const void* const_buf, int32_t batch,
                     const double* X0, double* X_out, const double* Z0, double* Z_out,
                     const double* U, int64_t u_bstride,
                     const double* Y, const double* PAR, int64_t par_bstride,
                     const double* x0,
                     double* cost_out, int32_t* iters_out, int32_t* status_out,
                     int32_t max_iter, double tol, void* workspace, size_t workspace_bytes,
                     void* stream);

/*
 * All solve inputs and outputs in one struct (the entry point new bindings use;
 * mhe_gn_solve / _ws / _ext are this call with Rw = NULL).  Pointers as
 * mhe_gn_solve_ext, plus
 *   Rw  (B|1, M, p, p)  per-solve measurement information, overriding the Rw the
 *                       constants were built with (batch stride rw_bstride, 0 =
 *                       shared; M scalars per trajectory for MHE_MEAS_MIXED).  The
 *                       reference's MHE windows re-set R every window (R = 0 masks
 *                       empty satellite slots, autonomous-car.py:250-263,
 *                       gnss-multi-receiver.py:186-204): passing it here keeps one
 *                       constants buffer for all windows.  Nonlinear measurement
 *                       models only (a linear h has Rw folded into the constant
 *                       part of J^T W J): MHE_ERR_UNSUPPORTED otherwise.
 *
 * Robust measurement rows (ABI v9).  meas_delta (B|1, M) puts the reference's
 * pseudo_huber_loss (cost_functions.py:25-31, Q = R_i) on the scalar measurement rows
 * (p = 1: pseudorange, vehicle_pseudorange, range_3d and every MHE_MEAS_MIXED row code).
 * Row i with weight R_i (Rw or the constants'), residual e_i and scale delta_i (in the
 * row's own units) costs
 *   2 R_i delta_i^2 (sqrt(1 + e_i^2 / delta_i^2) - 1)
 *     = 2 R_i e_i^2 / (1 + sqrt(1 + e_i^2 / delta_i^2))      (the form evaluated)
 * and the solve is IRLS, as for MHE_COST_HUBER: each GN step uses the row weight
 *   lambda_i = R_i / sqrt(1 + e_i^2 / delta_i^2)
 * (GE_i = H_i^T lambda_i e_i, G_i = H_i^T lambda_i H_i; the bounded solve's Armijo noise
 * term uses |lambda_i e_i|).  delta_i = +inf selects the plain quadratic row by a branch:
 * that row is bitwise the row of a call with meas_delta = NULL.  R_i = 0 masks the row
 * whatever delta_i is.  delta_i must be > 0 (NaN excluded): the host wrappers check it,
 * these entry points do NOT.  mhe_solve, mhe_state_cov (the covariance then uses the IRLS
 * weights at X) and mhe_assemble_at honour it; cost_out is the robust objective.  A linear
 * measurement model (MHE_MEAS_FULL_STATE: R is folded into the constants) and p > 1 return
 * MHE_ERR_UNSUPPORTED.  NULL: every call runs exactly the kernels it ran before v9.
 *
 * Per-solve prior weight (ABI v10).  Pw (B|1, n, n) is the weight of the addInitialCost term
 * (x(0) - x0)^T Pw (x(0) - x0) for THIS call, per trajectory: a moving-horizon estimator's
 * arrival cost changes every window and differs between the trajectories of a batch, while
 * the constants buffer stays one for all of them (mhe_arrival below forms the next window's
 * weight on the device).  It needs dims->has_prior == 1 (MHE_ERR_UNSUPPORTED otherwise, as
 * for n > 16 on the register-resident path, which has no such model) and
 * symmetric blocks (the host wrappers check that, these entry points do NOT).  Unlike Rw it
 * works for every measurement model: the prior touches the node-0 block of J^T W J alone.
 * The register-resident kernels add Pw_b - Pw_const to the block the constants carry, so a
 * caller that always passes Pw should build the constants with Pw = 0 (no cancellation of
 * two large weights).  Honoured by mhe_solve (every mode: Huber, meas_delta, bounds and their
 * Armijo cost, bordered and mixed problems), mhe_assemble_at, mhe_state_cov and mhe_arrival;
 * mhe_gn_solve* pass NULL.  NULL: bitwise the results of a build without the field.
 */
typedef struct mhe_solve_args {
  int32_t struct_size;     /* = sizeof(mhe_solve_args) */
  int32_t batch;
  const double* X0;
  double* X_out;
  const double* Z0;        /* extra variables (n_extra > 0), else NULL */
  double* Z_out;
  const double* U;
  int64_t u_bstride;
  const double* Y;
  const double* PAR;
  int64_t par_bstride;
  const double* Rw;        /* optional, see above */
  int64_t rw_bstride;
  const double* Pw;        /* optional (B|1, n, n): prior (arrival-cost) weight of this solve, overriding
                              the Pw the constants were built with (ABI v10, see "Per-solve prior
                              weight" above); NULL = the constants'.  Beside the other per-solve
                              weight; the struct_size check refuses every older binding wherever a
                              field is added */
  int64_t pw_bstride;      /* n*n, or 0 = shared by the batch */
  const double* x0;
  double* cost_out;
  int32_t* iters_out;
  int32_t* status_out;
  int32_t max_iter;
  double tol;
  void* workspace;         /* large-system path: >= mhe_workspace_bytes(dims, batch) */
  size_t workspace_bytes;
  double* lambda_out;      /* optional (B, n_eq): multipliers of the constraint rows from the
                              last bordered step, L = J + lambda^T (C v - r) (their signs
                              drive the host's active set), or NULL */
  const double* meas_delta; /* optional (B|1, M): pseudo-Huber scale per measurement row (ABI v9,
                               see "Robust measurement rows" below), or NULL = quadratic rows */
  int64_t md_bstride;       /* batch stride of meas_delta; 0 = shared by the batch */
} mhe_solve_args;

int mhe_solve(const mhe_dims* dims, const void* const_buf, const mhe_solve_args* args, void* stream);

/*
 * Kernel-level parity of the per-collocation-point evaluation (SURVEY §8(a) a5-a7,
 * nlp/nlp.py:225-235 and :264-273): at X (B,P,n) with the solve's device functors,
 *   W  (B,P,n)    W_k = (2/T) sum_j D_kj X_j - f(X_k, U_k)   (the eliminated defects)
 *   F  (B,P,n,n)  df/dx at (X_k, U_k)
 *   E  (B,M,p)    e_i = y_i - h(x(t_i)),  x(t_i) = sum_j Phi_ij X_j
 *   Hm (B,M,p,n)  dh/dx at x(t_i)
 * Any output may be NULL.  Both paths; not for MHE_MEAS_MIXED (MHE_ERR_UNSUPPORTED).
 * A constants buffer built for other dims leaves the outputs untouched.
 */
int mhe_resjac(const mhe_dims* dims, const void* const_buf, int32_t batch, const double* X, const double* U,
               int64_t u_bstride, const double* Y, const double* PAR, int64_t par_bstride, double* W,
               double* F, double* E, double* Hm, void* stream);

/*
 * Kernel-level parity: assemble the GN normal equations at X.
 *   H (B,dp,dp) full symmetric (dp = mhe_padded_dim; padding rows = identity),
 *   g (B,dp) gradient J^T W r (padding 0), cost (B).
 * Register-resident path only (MHE_ERR_UNSUPPORTED on the large-system path, which
 * needs a workspace: mhe_assemble_ws / mhe_chol_solve_ws below).
 */
int mhe_assemble(const mhe_dims* dims, const void* const_buf, int32_t batch,
                 const double* X, const double* U, int64_t u_bstride,
                 const double* Y, const double* PAR, int64_t par_bstride,
                 const double* x0, double* H, double* g, double* cost, void* stream);

/*
 * Kernel-level parity: solve H delta = -g for a batch of SPD matrices with the
 * solver's register-tiled Cholesky.  H (B,dp,dp) (lower triangle read),
 * g (B,dp), delta (B,dp), status (B).  `const_buf` is any constants buffer
 * built for `dims` (only its tile table is read).
 */
int mhe_chol_solve(const mhe_dims* dims, const void* const_buf, int32_t batch,
                   const double* H, const double* g, double* delta, int32_t* status,
                   void* stream);

/*
 * Both kernel-level parity entry points for EVERY path (ABI v5+): on the register-
 * resident path they are mhe_assemble / mhe_chol_solve (workspace ignored, status
 * set to 0 by the assembly); on the large-system path (C3-C5, mhe_workspace_bytes > 0)
 * they run the solve's own kernels over a caller-owned workspace of
 * >= mhe_workspace_bytes(dims, batch) bytes:
 *   mhe_assemble_ws    k_big_resid + k_big_assemble at X, then H and g copied out of
 *                      the kernels' component-major tiles into the SAME dense node-major
 *                      layout as mhe_assemble: H (B,dp,dp), g (B,dp), dp = mhe_padded_dim
 *                      = n * Pp, row j*n + c for node j < Pp (the first P*n rows are the
 *                      oracle's order; padding nodes last: identity block, zero coupling,
 *                      zero gradient), cost (B), status (B): 0, or
 *                      MHE_STATUS_BAD_CONSTANTS (outputs NaN).  The plain GN system
 *                      (bounds are a solve-time reduction).  n_extra / n_eq > 0: the
 *                      bordered KKT system of mhe_assemble_kkt_ws below (Z = NULL, so
 *                      n_extra > 0 returns MHE_ERR_NULL here: use the _kkt_ form).
 *   mhe_chol_solve_ws  H (lower triangle read, node-major as above) and g into the
 *                      tiles, k_big_chol (blocked Cholesky + both triangular solves),
 *                      delta = -H^-1 g (B,dp) node-major; status 0, MHE_STATUS_NOT_SPD
 *                      (non-positive or non-finite pivot; delta NaN) or BAD_CONSTANTS.
 *                      n_extra / n_eq > 0 (ABI v6): H, g, delta are the KKT system of
 *                      mhe_kkt_dim rows below, solved as every bordered GN step is
 *                      (k_big_chol on the leading block, then k_big_border: the border
 *                      columns through the factor, LDL^T of the Schur complement);
 *                      delta = [dx; dz; lambda].
 */
int mhe_assemble_ws(const mhe_dims* dims, const void* const_buf, int32_t batch,
                    const double* X, const double* U, int64_t u_bstride,
                    const double* Y, const double* PAR, int64_t par_bstride,
                    const double* x0, double* H, double* g, double* cost, int32_t* status,
                    void* workspace, size_t workspace_bytes, void* stream);
int mhe_chol_solve_ws(const mhe_dims* dims, const void* const_buf, int32_t batch,
                      const double* H, const double* g, double* delta, int32_t* status,
                      void* workspace, size_t workspace_bytes, void* stream);

/*
 * Kernel-level parity of the BORDERED system (ABI v6; SURVEY §8 f4: extra decision
 * variables z, nlp/nlp.py:40-47 addVariables used by multi-receiver.py:73,99, and
 * addEqConstraint rows, nlp/nlp.py:49-53 / gnss-multi-receiver.py:76-78).  Each
 * bordered GN step solves, with K = n_extra + n_eq and dk = mhe_kkt_dim = dp + K,
 *   [ H    H_xz  C^T ] [dx]     [ g_x       ]
 *   [ H_zx H_zz  0   ] [dz] = - [ g_z       ]     (rows C v - r of the constraints)
 *   [ C    0     0   ] [l ]     [ C v - r   ]
 * mhe_assemble_kkt_ws exports that matrix (B,dk,dk) and right-hand side g (B,dk) at
 * (X, Z): the leading dp x dp block is mhe_assemble_ws's node-major H, then the z rows,
 * then the constraint rows, in the values the solve's own k_big_resid / k_big_border
 * form (Z (B, n_extra) device array; NULL when n_extra == 0).  K = 0: exactly
 * mhe_assemble_ws.  mhe_chol_solve_ws takes the same shapes back (see above).
 */
int32_t mhe_kkt_dim(const mhe_dims* dims);

/* The kernel(s) a solve of `batch` trajectories on `stream` would run, as text into buf
 * (len bytes, NUL-terminated): the register path's k_gn instance -- chosen by the same
 * function as the launch (batch vs the stream device's CUs, Huber, bounds, LDS fit) --
 * or the large-system path's kernel sequence.  Host-only query; launches nothing.
 * (bench.py names the roofline record's kernel with it.) */
int32_t mhe_solve_kernel_name(const mhe_dims* dims, int32_t batch, void* stream, char* buf, int32_t len);

/* The envelope the large-system path's split factorization used (ABI v7): for
 * trajectory `traj` of the last solve / mhe_chol_solve_ws run on `workspace`
 * (workspace_bytes as passed there), the first nonzero tile column of each of its
 * NT = dp / 16 component-major tile rows (the factor has no nonzero tile left of it;
 * the left-looking updates and the backward solve skip those tiles), NT int32 into
 * first_col (n_out >= NT).  Formed on the device from the component pairs whose block
 * of H has a nonzero element at the iterate.  Synchronises `stream` (a copy to the
 * host); returns NT, MHE_ERR_UNSUPPORTED on the register path or in a build without
 * the envelope (every column then starts at 0), MHE_ERR_NULL / MHE_ERR_DIMS on bad
 * arguments.  Used by tools/bench_big.py for the executed flop count. */
int32_t mhe_big_envelope(const mhe_dims* dims, const void* workspace, size_t workspace_bytes, int32_t traj,
                         int32_t* first_col, int32_t n_out, void* stream);
int mhe_assemble_kkt_ws(const mhe_dims* dims, const void* const_buf, int32_t batch,
                        const double* X, const double* Z, const double* U, int64_t u_bstride,
                        const double* Y, const double* PAR, int64_t par_bstride,
                        const double* x0, double* H, double* g, double* cost, int32_t* status,
                        void* workspace, size_t workspace_bytes, void* stream);

/* mhe_assemble_kkt_ws taking the struct (ABI v9): the kernel-level view of the per-solve
 * inputs the positional mhe_assemble* calls cannot carry.  at->X0 is the point (B, P, n);
 * Z0 (n_extra > 0), U, Y, PAR, Rw, meas_delta, Pw (ABI v10), x0 with their strides, batch and (large-
 * system path) workspace / workspace_bytes are read from the struct; its outputs and
 * max_iter / tol are not.  H, g, cost, status as mhe_assemble_kkt_ws: with meas_delta the
 * IRLS system at X (the weights lambda_i above) and the robust cost. */
int mhe_assemble_at(const mhe_dims* dims, const void* const_buf, const mhe_solve_args* at,
                    double* H, double* g, double* cost, int32_t* status, void* stream);

/* Posterior covariance of the state estimate at query times (ABI v8).
 *
 * The objective is r^T W r, so H = J^T W J at the point X is the information matrix of
 * the whole trajectory, and with S_t = phi(t)^T (x) I_n (the Lagrange row extractSolution
 * uses)  Cov[x(t)] = S_t H^-1 S_t^T.  The call assembles H at X exactly as a solve does
 * (Huber IRLS weights, the per-solve Rw and meas_delta), runs the solve's own Cholesky factorization
 * H = U^T U (on the large-system path with the pivots refined once more) and sweeps the query columns through the factor: Z = U^-T S_t^T, Cov = Z^T Z
 * (a multi-column forward substitution; no back substitution, no inverse).
 *
 * The result is the inverse of the HALF-Hessian J^T W J of the cost: the covariance when
 * the weights (Qw, Rw, Pw) are inverse covariances, as in every reference script.
 * Variable bounds are NOT reflected: the result is the information of the unconstrained
 * GN model at X, whatever n_bounds is.  Bordered problems (n_extra > 0, n_eq > 0) and
 * MHE_MEAS_MIXED return MHE_ERR_UNSUPPORTED (a covariance under constraints is a
 * projected quantity), as does n > 16 on the register-resident path, and a problem
 * whose query panel (dp x 16 doubles of LDS on top of the solve's) does not fit.
 *
 *   at          batch; X0 = the point (B, P, n); U, Y, PAR, x0, Rw, meas_delta, Pw and their strides, and
 *               on the large-system path workspace / workspace_bytes, as for mhe_solve.
 *               The outputs and max_iter / tol of the struct are not read.
 *   PhiQ        (n_query, P) DEVICE: Lagrange basis rows at the query times
 *   cov_out     (B, n_query, n, n), each block symmetric; NaN where status != 0
 *   status_out  (B) 0, MHE_STATUS_NOT_SPD (bad pivot) or MHE_STATUS_BAD_CONSTANTS
 *   scratch     large-system path: mhe_cov_scratch_bytes(dims, batch, n_query) bytes of
 *               device memory, the query columns' storage (the register path keeps them
 *               in LDS: the query returns 0 and scratch may be NULL).  Host-only query.
 * Only enqueues work on `stream`; allocates nothing.  A query's block does not depend
 * on the batch size or on the other query times of the call. */
size_t mhe_cov_scratch_bytes(const mhe_dims* dims, int32_t batch, int32_t n_query);
int mhe_state_cov(const mhe_dims* dims, const void* const_buf, const mhe_solve_args* at,
                  const double* PhiQ, int32_t n_query, double* cov_out, int32_t* status_out,
                  void* scratch, size_t scratch_bytes, void* stream);

/* Arrival cost of the next window (ABI v10): the prior a moving-horizon estimator carries
 * from this window to the one shifted by t (the reference's loop, autonomous-car.py:232-271,
 * with the weight the covariance gives), formed on the device for the whole batch:
 *   x_arr   (B, n)     x(t) = sum_j phi_j X_j, summed in node order      (next prior mean)
 *   Pw_arr  (B, n, n)  inv(S_t H^-1 S_t^T), bitwise symmetric            (next prior weight)
 *   cov_out (B, n, n)  optional: the covariance block S_t H^-1 S_t^T itself (bitwise the
 *                      block of mhe_state_cov for the same query), or NULL
 * so that the next mhe_solve takes x0 = x_arr and Pw = Pw_arr without a copy.  The covariance
 * stage is mhe_state_cov's with n_query = 1 (phi: its Lagrange row (1, P), DEVICE): the same
 * `at` semantics (the per-solve Rw, meas_delta and Pw of the window included), the same
 * refusals (bordered and mixed problems, n > 16 on the register-resident path, a query panel
 * that does not fit) and the same scratch (mhe_arrival_scratch_bytes; 0 on the register
 * path).  Then one wavefront per trajectory inverts the n x n block in LDS: Cholesky
 * C = L L^T with true square roots and divisions, A = L^-T L^-1 written from the upper
 * triangle.  status_out (B): 0, MHE_STATUS_NOT_SPD (a bad pivot in H or in the n x n block)
 * or MHE_STATUS_BAD_CONSTANTS; where it is non-zero x_arr, Pw_arr and cov_out of that
 * trajectory are NaN and no other trajectory is affected.  Only enqueues work on `stream`;
 * allocates nothing. */
size_t mhe_arrival_scratch_bytes(const mhe_dims* dims, int32_t batch);
int mhe_arrival(const mhe_dims* dims, const void* const_buf, const mhe_solve_args* at, const double* phi,
                double* x_arr, double* Pw_arr, double* cov_out, int32_t* status_out, void* scratch,
                size_t scratch_bytes, void* stream);

/* Covariance and arrival cost of mixed-row and bordered problems (ABI v11): what
 * mhe_state_cov and mhe_arrival refuse -- MHE_MEAS_MIXED rows, extra variables z
 * (n_extra > 0) and equality rows C v = r (n_eq > 0).  The covariance of the estimate under
 * its equality rows is the leading block of the inverse of the bordered system every GN step
 * of such a problem solves (mhe_assemble_kkt_ws:  [H Bd; Bd^T G], Bd = [H_xz C^T],
 * G = diag(H_zz, 0), K = n_extra + n_eq border columns).  With H = L L^T (the solve's
 * factorization, pivots refined as for mhe_state_cov), Z_q = L^-1 S_q^T, V = L^-1 Bd,
 * Sigma = G - V^T V (the Schur matrix of the bordered step, factored as L D L^T without
 * pivoting as there) and T_q = V^T Z_q,
 *   Cov[x(t_q)] = Z_q^T Z_q + T_q^T Sigma^-1 T_q         cov_out  (B, n_query, n, n)
 *   Cov[z]      = (Sigma^-1)[0:n_extra, 0:n_extra]        covz_out (B, n_extra, n_extra) or NULL
 * each block written from its upper triangle (bitwise symmetric).  Equality rows take
 * variance away: the blocks are positive SEMI-definite (a row x_a - x_b = r leaves the
 * variance of x_a - x_b at 0).  An extra variable no row depends on is held by the solve
 * (zero Schur pivot) and removed here: its row and column of covz_out are NaN, every other
 * entry is that of the system without it.  eq_rhs does not enter; bounds are not reflected.
 *
 *   at          as for mhe_state_cov, plus Z0 (B, n_extra), required when n_extra > 0
 *               (MHE_ERR_NULL); Rw, meas_delta (IRLS weights at X) and Pw are honoured.
 *   status_out  (B) 0, MHE_STATUS_NOT_SPD (a bad pivot of H, a non-finite Sigma or pivot of
 *               it) or MHE_STATUS_BAD_CONSTANTS; the outputs of such a trajectory are NaN and
 *               no other trajectory is affected.
 *   scratch     mhe_kkt_cov_scratch_bytes(dims, batch, n_query) bytes (the query columns;
 *               the border columns use the workspace); a smaller one is MHE_ERR_NULL.
 * Dims without a border and without mixed rows are forwarded to mhe_state_cov (register path
 * included; covz_out is not written): bitwise its result.
 *
 * mhe_kkt_arrival is mhe_kkt_cov with one query followed by mhe_arrival's inversion: x_arr,
 * Pw_arr, cov_out as there, for mixed rows and extra variables.  n_eq > 0 returns
 * MHE_ERR_UNSUPPORTED (an equality row between state components makes the block rank-
 * deficient: it has no inverse), as does n > 40.  Scratch: mhe_kkt_cov_scratch_bytes(dims,
 * batch, 1).  Both calls only enqueue work on `stream` and allocate nothing. */
size_t mhe_kkt_cov_scratch_bytes(const mhe_dims* dims, int32_t batch, int32_t n_query);
int mhe_kkt_cov(const mhe_dims* dims, const void* const_buf, const mhe_solve_args* at,
                const double* PhiQ, int32_t n_query, double* cov_out, double* covz_out,
                int32_t* status_out, void* scratch, size_t scratch_bytes, void* stream);
int mhe_kkt_arrival(const mhe_dims* dims, const void* const_buf, const mhe_solve_args* at, const double* phi,
                    double* x_arr, double* Pw_arr, double* cov_out, int32_t* status_out, void* scratch,
                    size_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Batched extended Kalman filter.
 * Replaces utils/ekf.py:20-61 (EKF.update / predict / correct) with the
 * utils/gnss.py plug-ins, for `batch` independent filter instances, `steps`
 * updates each, in one launch (one wavefront per instance).
 * ------------------------------------------------------------------------ */
#define MHE_EKF_DYN_GNSS_POS_AND_BIAS 1          /* utils/gnss.py:79-90 (n=5, m=3, params dt) */
#define MHE_EKF_MEAS_MULTI_PSEUDORANGE 1         /* utils/gnss.py:27-45 (q=3: sat ENU position) */
#define MHE_EKF_MEAS_MULTI_PSEUDORANGE_AND_BIAS 2 /* utils/gnss.py:48-61 (last row: bias, zero Jacobian row) */
/* the autonomous-car script's own EKF plug-ins (autonomous-car.py:18-77) */
#define MHE_EKF_DYN_DISCRETE_VEHICLE 2           /* discrete_vehicle_dynamics :18-52 (n=9, m=2; params dt,
                                                    car_params -> dyn_par = [C_AF, C_AR, M, D_F, D_R, I_Z]) */
#define MHE_EKF_MEAS_VEHICLE_SENSORS 3           /* vehicle_sensors_model :54-77 (q=3: sat ENU position;
                                                    rows of multi_pseudorange on x[0, 1, 8, 6, 7]) */

typedef struct mhe_ekf_dims {
  int32_t struct_size; /* = sizeof(mhe_ekf_dims) */
  int32_t n, m;        /* state and control sizes of the dynamics model */
  int32_t pmax;        /* row capacity of Z / PAR / R per step (<= 32) */
  int32_t q;           /* parameters per measurement row (3) */
  int32_t dyn_model;   /* MHE_EKF_DYN_* */
  int32_t meas_model;  /* MHE_EKF_MEAS_* */
  double dt;           /* dyn_func_params["dt"] */
  int32_t r_diag;      /* 1: the caller guarantees every step's R block is diagonal -> the
                          correction runs as sequential scalar updates, one filter per lane
                          (same result as the batch update up to rounding); 0: general R,
                          one wavefront per filter with an augmented Cholesky sweep */
  int32_t hist_batch_inner; /* 1: mu_hist is (steps, n, B) and S_hist (steps, n, n, B) --
                               batch innermost, so a wavefront's history stores coalesce;
                               0: (B, steps, n) / (B, steps, n, n) as below */
  int32_t in_batch_inner;   /* 1: U (steps, m, B), Z (steps, pmax, B), nz (steps, B), PAR
                               (steps, pmax, q, B) -- batch innermost (coalesced reads; the
                               *_bstride arguments are ignored); 0: the layouts below */
  double dyn_par[8];        /* static dynamics parameters (MHE_EKF_DYN_DISCRETE_VEHICLE: the car
                               constants; unused by gnss_pos_and_bias) */
} mhe_ekf_dims;

/*
 * All pointers are device pointers; a batch stride of 0 broadcasts one array to
 * every instance.  Per instance b and step k:
 *   U   (steps, m)                      at U   + b*u_bstride
 *   Z   (steps, pmax), rows 0..nz-1     at Z   + b*z_bstride   (z, utils/ekf.py:20)
 *   nz  (steps) valid rows; 0 = no measurement (predict only, utils/ekf.py:30-38)
 *   PAR (steps, pmax, q)                at PAR + b*par_bstride (meas_func_params)
 *   R   leading nz x nz block of (pmax, pmax) at R + b*r_bstride + k*r_sstride
 *   Q   (n, n) shared.
 * mu (B,n) and S (B,n,n) hold the prior on entry and the final state on exit;
 * mu_hist (B,steps,n) / S_hist (B,steps,n,n) (optional) receive the state after
 * every update; status (B, optional): 0 ok, 1 innovation covariance not SPD,
 * 2 nz > pmax (the step is then predict-only).  Returns MHE_OK or a negative MHE_ERR_*.
 */
int mhe_ekf_run(const mhe_ekf_dims* dims, int32_t batch, int32_t steps, double* mu, double* S,
                const double* U, int64_t u_bstride, const double* Z, int64_t z_bstride,
                const int32_t* nz, int64_t nz_bstride, const double* PAR, int64_t par_bstride,
                const double* Q, const double* R, int64_t r_bstride, int64_t r_sstride,
                double* mu_hist, double* S_hist, int32_t* status, void* stream);

/*
 * Innovation gating and likelihood outputs (added within v11; no existing struct or function
 * changed).  mhe_ekf_run_args takes mhe_ekf_run's arguments as a struct, plus:
 *   gate    0: no screening.  > 0 (+inf allowed): row i (i < nz) of step k is screened out iff
 *           d2_i > gate, d2_i = (z_i - h_i(mu-))^2 / (H_i S- H_i^T + R_ii) -- marginal and at
 *           the prediction, so it depends neither on the row order nor on the other rows, and
 *           is the same for r_diag = 1 and 0.  A NaN or non-positive denominator keeps the row
 *           (status 1 then reports it).  The correction is the one above on the kept rows in
 *           their order, with R's kept sub-block; rows keep their index (the bias row of
 *           MHE_EKF_MEAS_MULTI_PSEUDORANGE_AND_BIAS is row nz-1 and is screened like any other);
 *           a step whose rows are all screened out is predict-only.  NaN or negative: MHE_ERR_DIMS.
 *   nis, loglik, rej   optional per-step outputs, (steps, B) with dims->hist_batch_inner, else
 *           (B, steps): over the accepted rows a, nis = e_a^T P_a^-1 e_a and
 *           loglik = -(nis + log det P_a + |a| log 2 pi) / 2; bit i of rej is set iff row i was
 *           screened out (pmax <= 32: bit 31 is a row like any other).  A step with nz = 0, with
 *           nz > pmax (status 2) or with every row screened out has nis = loglik = 0.
 * gate == 0 with nis, loglik and rej all NULL runs exactly what mhe_ekf_run runs (which is this
 * call with those four fields zero); refusals and return codes are mhe_ekf_run's, and a NULL or
 * wrongly sized args struct is refused like dims.
 */
typedef struct mhe_ekf_args {
  int32_t struct_size; /* = sizeof(mhe_ekf_args) */
  int32_t batch, steps;
  double* mu;
  double* S;
  const double* U;
  int64_t u_bstride;
  const double* Z;
  int64_t z_bstride;
  const int32_t* nz;
  int64_t nz_bstride;
  const double* PAR;
  int64_t par_bstride;
  const double* Q;
  const double* R;
  int64_t r_bstride, r_sstride;
  double* mu_hist;
  double* S_hist;
  int32_t* status;
  double gate;
  double* nis;
  double* loglik;
  int32_t* rej;
} mhe_ekf_args;

int mhe_ekf_run_args(const mhe_ekf_dims* dims, const mhe_ekf_args* args, void* stream);

/*
 * Batched unscented Kalman filter (added within v11; no existing struct or function changed).
 * The additive-noise filter with the scaled unscented transform over the same plug-ins, by
 * their VALUES only: no Jacobian enters, so the bias row of
 * MHE_EKF_MEAS_MULTI_PSEUDORANGE_AND_BIAS (h = x[3]) acts, and MHE_EKF_DYN_DISCRETE_VEHICLE is
 * its Euler step.  One wavefront per filter.  With lambda = alpha^2 (n + kappa) - n,
 * c = sqrt(n + lambda), wm_0 = lambda / (n + lambda), wc_0 = wm_0 + 1 - alpha^2 + beta and
 * wm_j = wc_j = 1 / (2 (n + lambda)), the 2n+1 sigma points of (mu, S = L L^T) are mu and
 * mu +- c L[:, j].  Per step:
 *   predict  Y_j = f(X_j, u),  mu- = sum wm_j Y_j,  S- = sum wc_j (Y_j - mu-)(Y_j - mu-)^T + Q
 *   correct  (0 < nz <= pmax) with sigma points redrawn from (mu-, S-):  Zs_j = h(X_j) - z,
 *            e = -sum wm_j Zs_j,  Dz_j = Zs_j + e,  Pzz = sum wc_j Dz_j Dz_j^T + R,
 *            Pxz = sum wc_j (X_j - mu-) Dz_j^T;  with Pzz = L L^T, Y = L^-1 Pxz^T, w = L^-1 e:
 *            mu = mu- + Y^T w,  S = S- - Y^T Y
 * Every sum runs over j in increasing order, so a filter's result does not depend on the batch
 * or on its place in it.  Only the upper triangles of Q and R are read; S_hist and S are bitwise
 * symmetric.
 * dims, the input layouts and strides and the history layout are mhe_ekf_run's (r_diag is
 * ignored); the fields of mhe_ukf_args up to status are mhe_ekf_args', then
 *   alpha, beta, kappa   1, 0, 0 gives lambda = 0: 2n equally weighted points, no negative
 *           weight.  alpha not finite or <= 0, beta or kappa not finite, n + kappa <= 0:
 *           MHE_ERR_DIMS
 *   nis, loglik   optional per-step outputs laid out as mhe_ekf_args': nis = w^T w,
 *           loglik = -(nis + 2 sum log L_ii + nz log 2 pi) / 2; 0 on a step without a correction.
 * status (B, optional): 0 ok; 1 a Cholesky pivot of S, S- or Pzz was not positive and finite:
 * that filter's history entries (nis and loglik included) from that step on and its final
 * mu / S are NaN, every other filter is untouched; 2 nz > pmax at some step (that step is
 * predict-only).  Refusals and return codes are mhe_ekf_run_args' (batch == 0 or steps == 0:
 * MHE_OK, nothing is read).
 */
typedef struct mhe_ukf_args {
  int32_t struct_size; /* = sizeof(mhe_ukf_args) */
  int32_t batch, steps;
  double* mu;
  double* S;
  const double* U;
  int64_t u_bstride;
  const double* Z;
  int64_t z_bstride;
  const int32_t* nz;
  int64_t nz_bstride;
  const double* PAR;
  int64_t par_bstride;
  const double* Q;
  const double* R;
  int64_t r_bstride, r_sstride;
  double* mu_hist;
  double* S_hist;
  int32_t* status;
  double alpha, beta, kappa;
  double* nis;
  double* loglik;
} mhe_ukf_args;

int mhe_ukf_run(const mhe_ekf_dims* dims, const mhe_ukf_args* args, void* stream);

/*
 * Innovation gating and a rejection mask for the unscented filter (added within v11; no existing
 * struct or function changed).  mhe_ukf_gate_args holds mhe_ukf_args' fields in order, then:
 *   gate    0: no screening.  > 0 (+inf allowed, screens nothing): at a step with 0 < nz <= pmax,
 *           after e and Pzz (R included) are formed from the redrawn sigma points,
 *               d2_i = e_i^2 / Pzz_ii   (i < nz)
 *           and row i is screened out iff d2_i > gate.  A NaN or non-positive Pzz_ii keeps the
 *           row (status 1 then reports it through the pivot, as for the EKF).  The screen is
 *           marginal and taken at the prediction: it depends neither on the row order nor on
 *           the other rows.  The correction is the one above over the kept rows, in their order,
 *           with the kept sub-blocks of Pzz and Pxz.  Every entry of e, Pzz and Pxz is a sum
 *           over the sigma points of that row's own values, so the result is exactly the
 *           ungated filter fed only the kept rows.  Rows keep their index: the bias row of
 *           MHE_EKF_MEAS_MULTI_PSEUDORANGE_AND_BIAS stays row nz-1, keeps h = x[3] and is
 *           screened like any other.  A step whose rows are all screened out is predict-only:
 *           mu = mu-, S = S-, nis = loglik = 0.  NaN or negative: MHE_ERR_DIMS.
 *   rej     optional per-step output laid out as nis / loglik ((steps, B) with
 *           dims->hist_batch_inner, else (B, steps)): bit i is set iff row i was screened out
 *           (pmax <= 32: bit 31 is a row like any other); 0 on a step with nz = 0 or nz > pmax.
 * With a gate, nis and loglik are taken over the kept rows a: nis = w^T w and
 * loglik = -(nis + 2 sum_a log L_ii + |a| log 2 pi) / 2.  The status rules are mhe_ukf_run's.
 * gate == 0 with rej NULL runs exactly what mhe_ukf_run runs; refusals and return codes are
 * mhe_ukf_run's (a NULL or wrongly sized args struct is refused like dims; batch == 0 or
 * steps == 0: MHE_OK, nothing is read).
 */
typedef struct mhe_ukf_gate_args {
  int32_t struct_size; /* = sizeof(mhe_ukf_gate_args) */
  int32_t batch, steps;
  double* mu;
  double* S;
  const double* U;
  int64_t u_bstride;
  const double* Z;
  int64_t z_bstride;
  const int32_t* nz;
  int64_t nz_bstride;
  const double* PAR;
  int64_t par_bstride;
  const double* Q;
  const double* R;
  int64_t r_bstride, r_sstride;
  double* mu_hist;
  double* S_hist;
  int32_t* status;
  double alpha, beta, kappa;
  double* nis;
  double* loglik;
  double gate;
  int32_t* rej;
} mhe_ukf_gate_args;

int mhe_ukf_run_gated(const mhe_ekf_dims* dims, const mhe_ukf_gate_args* args, void* stream);

/*
 * Iterated extended Kalman filter (added within v11; no existing struct or function changed).
 * The Gauss-Newton solve of each step's MAP problem
 *   min_x (x - mu-)^T S-^-1 (x - mu-) + (z - h(x))^T R^-1 (z - h(x)):
 * the measurement model is relinearised at the current iterate and the correction of
 * mhe_ekf_run is redone from the prediction.  The predict is mhe_ekf_run's; at a step with
 * 0 < nz <= pmax, with x_0 = mu-:
 *   pass i:  (h, H) at x_i,  e = z - h - H (mu- - x_i),  P = H S- H^T + R = L L^T,
 *            Y = L^-1 H S-,  w = L^-1 e,  x_{i+1} = mu- + Y^T w,
 *            step = max_c |x_{i+1,c} - x_{i,c}|;  stop when !(step > tol) or i + 1 == max_iter
 *   after:   mu = x_{i+1},  S = S- - Y^T Y with the Y of the last pass.
 * With max_iter = 1 the step is mhe_ekf_run's general-R step, term by term.  Only the upper
 * triangle of Q is read (an entry of S- below the diagonal is computed as its mirror image), so
 * S_hist and S are bitwise symmetric.  One wavefront per filter for every R: dims->r_diag is
 * ignored.  mhe_iekf_args holds mhe_ekf_args' fields in order, then:
 *   tol       >= 0, an absolute max-norm in the state's own units; 0: every corrected step makes
 *             max_iter passes (the step is not tested).  With tol > 0 a NaN step stops the
 *             iteration.  Below the rounding floor of the
 *             rows (about 1e-8 m for pseudoranges of 2e7 m) the counts depend on rounding.
 *   n_iter    optional per-step output laid out as nis: the passes made; 0 on a predict-only
 *             step (nz = 0, nz > pmax, or every row screened out).
 *   max_iter  1..64
 *   reserved0 must be 0
 * gate (0: no screening) is mhe_ekf_args' marginal rule d2_i = e_i^2 / P_ii > gate, evaluated
 * once, in pass 0, at the prediction; the kept rows stay fixed for the later passes.  nis,
 * loglik and rej are pass 0's over the kept rows: the innovation likelihood at the prediction,
 * as mhe_ekf_run_args reports it.  status: 1 if any pass met a pivot that is not positive and
 * finite, 2 if nz > pmax at some step.  Refusals and return codes are mhe_ekf_run_args';
 * in addition MHE_ERR_DIMS for max_iter outside 1..64, a NaN or negative tol, reserved0 != 0.
 */
typedef struct mhe_iekf_args {
  int32_t struct_size; /* = sizeof(mhe_iekf_args) */
  int32_t batch, steps;
  double* mu;
  double* S;
  const double* U;
  int64_t u_bstride;
  const double* Z;
  int64_t z_bstride;
  const int32_t* nz;
  int64_t nz_bstride;
  const double* PAR;
  int64_t par_bstride;
  const double* Q;
  const double* R;
  int64_t r_bstride, r_sstride;
  double* mu_hist;
  double* S_hist;
  int32_t* status;
  double gate;
  double* nis;
  double* loglik;
  int32_t* rej;
  double tol;
  int32_t* n_iter;
  int32_t max_iter;
  int32_t reserved0;
} mhe_iekf_args;

int mhe_iekf_run(const mhe_ekf_dims* dims, const mhe_iekf_args* args, void* stream);

/*
 * Pseudo-Huber measurement rows for the iterated filter (added within v11; no existing struct or
 * function changed): the M-estimate of each step's MAP problem by iteratively reweighted
 * Gauss-Newton, the Huber-type Kalman correction.  The predict, the stop rule, tol, max_iter and
 * the gate's meaning are mhe_iekf_run's.  At a step with 0 < nz <= pmax, with x_0 = mu-:
 *   pass i:  (h, H) at x_i,  r_j = z_j - h_j,  t_j = r_j / delta_j,  s_j = sqrt(1 + t_j^2),
 *            g_j = sqrt(s_j),  e = r - H (mu- - x_i),
 *            P = H S- H^T + R~ = L L^T  with  R~_jl = R_jl * (g_j * g_l),
 *            Y = L^-1 H S-,  w = L^-1 e,  x_{i+1} = mu- + Y^T w,  the same stop rule
 *   after:   mu = x_{i+1},  S = S- - Y^T Y with the Y of the last pass,
 *            omega_j = 1 / s_j of the last pass.
 * For a diagonal R this is IRLS on the cost sum_j 2 (delta_j^2 / R_jj) (s_j - 1) + the prior's
 * term: a row counts fully while |r_j| << delta_j and like |r_j| beyond it; delta is in the
 * measurement's own units, as mhe_solve_args.meas_delta.  For any symmetric positive definite R
 * it is the covariance inflation D^-1/2 R D^-1/2, D = diag omega; no R is refused.
 * delta = +inf gives s = g = 1 exactly: the run is then bitwise mhe_iekf_run's.
 * mhe_iekf_robust_args holds mhe_iekf_args' fields in order, then:
 *   delta    every row's delta when DELTA is NULL: > 0, +inf allowed.  With DELTA given it must be 0.
 *   DELTA    optional: one entry per row, laid out and strided exactly as Z (z_bstride,
 *            dims->in_batch_inner).  Entries are not validated on the device: a zero or NaN entry
 *            of a counted row gives a non-finite pivot, status 1 for that filter alone.
 *   weights  optional output: omega of the last pass per row, pmax entries per step, laid out as
 *            the per-step outputs ((steps, pmax, B) with dims->hist_batch_inner, else
 *            (B, steps, pmax)); 0 for every row that was not applied (beyond nz, screened out, or
 *            on a predict-only step).
 * gate (0: no screening) is evaluated once, in pass 0, on the UNWEIGHTED diagonal
 * pd_j = (H S- H^T)_jj + R_jj, the sum mhe_iekf_run forms: the mask is mhe_iekf_run's at the same
 * prediction, and a screened row is out for every pass.  nis and loglik are pass 0's over the
 * kept rows of the REWEIGHTED model: w and L of the sweep that used R~ at x_0 (not the innovation
 * likelihood under R, unless every delta is +inf).  rej, n_iter and status are mhe_iekf_run's.
 * Refusals and return codes are mhe_iekf_run's; in addition MHE_ERR_DIMS for a delta that is NaN
 * or not > 0 when DELTA is NULL, and for delta != 0 when DELTA is given.  These precede the
 * launch and the MHE_OK of an empty call (batch == 0 or steps == 0).
 */
typedef struct mhe_iekf_robust_args {
  int32_t struct_size; /* = sizeof(mhe_iekf_robust_args) */
  int32_t batch, steps;
  double* mu;
  double* S;
  const double* U;
  int64_t u_bstride;
  const double* Z;
  int64_t z_bstride;
  const int32_t* nz;
  int64_t nz_bstride;
  const double* PAR;
  int64_t par_bstride;
  const double* Q;
  const double* R;
  int64_t r_bstride, r_sstride;
  double* mu_hist;
  double* S_hist;
  int32_t* status;
  double gate;
  double* nis;
  double* loglik;
  int32_t* rej;
  double tol;
  int32_t* n_iter;
  int32_t max_iter;
  int32_t reserved0;
  double delta;
  const double* DELTA;
  double* weights;
} mhe_iekf_robust_args;

int mhe_iekf_run_robust(const mhe_ekf_dims* dims, const mhe_iekf_robust_args* args, void* stream);

/*
 * Fixed-interval (Rauch-Tung-Striebel) smoother over the history mhe_ekf_run wrote
 * (added to ABI v11; no existing struct or function changed).  One filter per lane;
 * a filter's result does not depend on the batch or on its place in it.
 * For k = steps-2 .. 0, with (x-, G) = f(mu_k, u_{k+1}) and S- = G S_k G^T + Q recomputed
 * by the forward pass's own dynamics functor:
 *   C = S_k G^T (S-)^-1,  mu_s[k] = mu_k + C (mu_s[k+1] - x-),  S_s[k] = S_k + C (S_s[k+1] - S-) C^T
 * and mu_s / S_s of the last step are the filtered ones.  S- is factored by Cholesky.
 * Of dims this call reads struct_size, n, m, dyn_model, dt, dyn_par, hist_batch_inner (the
 * layout of mu_hist, S_hist, mu_s and S_s alike) and in_batch_inner (the layout of U);
 * pmax, q, meas_model and r_diag are not read: measurements and R do not enter.
 *   mu_hist, S_hist  filtered histories; only the upper triangle of S_hist is read
 *   U, u_bstride, Q  as mhe_ekf_run
 *   mu0 (B,n), S0 (B,n,n)      optional: the prior the filter started from
 *   mu_s, S_s        smoothed histories, S_s bitwise symmetric.  They may alias mu_hist /
 *                    S_hist (in place): every lane reads a step before it writes it
 *   mu0_s (B,n), S0_s (B,n,n)  optional (need mu0 and S0): the smoothed prior, one more
 *                    step of the recursion from (mu0, S0) with u_0
 *   status (B, optional): 0 ok; 1 a pivot of S- was not positive and finite, or the history
 *                    held a non-finite value: that filter's outputs are NaN from the failing
 *                    step down to step 0 (and its smoothed prior); the steps above it and
 *                    every other filter are untouched.
 * Stream-ordered: no host synchronisation, no allocation.  Returns MHE_OK or MHE_ERR_*
 * (batch == 0 or steps == 0: MHE_OK, nothing is read).
 */
int mhe_ekf_smooth(const mhe_ekf_dims* dims, int32_t batch, int32_t steps, const double* mu_hist,
                   const double* S_hist, const double* U, int64_t u_bstride, const double* Q,
                   const double* mu0, const double* S0, double* mu_s, double* S_s, double* mu0_s,
                   double* S0_s, int32_t* status, void* stream);

/*
 * The smoother above with the lag-one smoothed covariances as one more output (added within
 * ABI v11; no existing struct or function changed).  mhe_ekf_lag_args holds mhe_ekf_smooth's
 * arguments in order, then:
 *   C  optional, laid out as S_s ((steps, n, n, B) with dims->hist_batch_inner, else
 *      (B, steps, n, n)):  C_k = Cov(x_k, x_{k-1} | all data) = S_s[k] G_{k-1}^T  with
 *      G_{k-1} = S_{k-1} F^T (S-)^-1 the smoother gain of step k-1 (k = -1: the prior).  All
 *      n x n entries are written; C_k is not symmetric.  k = 1 .. steps-1, and k = 0 when the
 *      smoothed prior is asked for (mu0_s or S0_s given); otherwise C_0 is written as NaN:
 *      "not formed".  C must not overlap any input or any other output (MHE_ERR_DIMS); mu_s /
 *      S_s may still alias the histories.  A filter that fails at step k (status 1) has C_j
 *      NaN for j <= k + 1, next to its S_s[j] NaN for j <= k; no other filter is touched.
 * C == NULL runs exactly what mhe_ekf_smooth runs.  mu_s, S_s, mu0_s, S0_s and status do not
 * depend on C being asked for (bitwise).  Refusals precede any launch and are mhe_ekf_smooth's;
 * a NULL or wrongly sized args struct is refused like dims.
 */
typedef struct mhe_ekf_lag_args {
  int32_t struct_size; /* = sizeof(mhe_ekf_lag_args) */
  int32_t batch, steps;
  const double* mu_hist;
  const double* S_hist;
  const double* U;
  int64_t u_bstride;
  const double* Q;
  const double* mu0;
  const double* S0;
  double* mu_s;
  double* S_s;
  double* mu0_s;
  double* S0_s;
  int32_t* status;
  double* C;
} mhe_ekf_lag_args;

int mhe_ekf_smooth_args(const mhe_ekf_dims* dims, const mhe_ekf_lag_args* args, void* stream);

/*
 * EM sufficient statistics of the noise model from a smoothed history (added within ABI v11; no
 * existing struct or function changed): what the M-step of the Shumway-Stoffer / extended-RTS EM
 * update of Q and R needs, reduced per filter on the device.  One filter per lane; every sum runs
 * in a fixed order (k increasing), so a filter's result is bitwise the same alone or in any batch.
 * Dynamics, for k in K = {1 .. steps-1}, plus {0} when the smoothed prior is given:
 *   (f, F) = f(mu_s[k-1], u_k)   value and Jacobian at the smoothed mean (k = 0: at mu0_s)
 *   d = mu_s[k] - f
 *   W_k = d d^T + S_s[k] - C_k F^T - F C_k^T + F S_s[k-1] F^T
 *   Qsum = sum_K W_k  (upper triangle accumulated term by term and mirrored),  q_cnt = |K|
 * Measurements, for every step with 0 < nz <= pmax and every row i < nz whose bit in rej is clear,
 * with (h, H) at mu_s[k]:
 *   r2[k][i] = (z_i - h_i)^2 + H_i S_s[k] H_i^T,   r_cnt = number of such rows
 * and r2 = 0 for every other row i < pmax.  Only these diagonal second moments are formed.  The
 * all-zero Jacobian row of MHE_EKF_MEAS_MULTI_PSEUDORANGE_AND_BIAS is kept as the filter has it.
 * Of dims this call reads struct_size, n, m, pmax, q, dyn_model, meas_model, dt, dyn_par,
 * hist_batch_inner (the layout of mu_s, S_s, C, rej and r2 alike) and in_batch_inner (U, Z, nz, PAR).
 *   mu_s, S_s, C     what mhe_ekf_smooth_args wrote; of S_s the upper triangle is read
 *   mu0_s (B,n), S0_s (B,n,n)   optional, together: the smoothed prior; C_0 is then read
 *   U, Z, nz, PAR and their strides   as mhe_ekf_run
 *   rej      optional, the mask mhe_ekf_run_args wrote ((steps, B) with hist_batch_inner, else
 *            (B, steps)): bit i set = row i is not counted
 *   Qsum (B,n,n), q_cnt (B), r_cnt (B)   batch outermost;  r2 (steps, pmax, B) with
 *            hist_batch_inner, else (B, steps, pmax)
 *   status (B, optional): 0 ok; 1 a non-finite value was met in what the sums read: that
 *            filter's Qsum and r2 are NaN, no other filter is touched; 2 nz > pmax at some step
 *            (its rows are skipped, as in the filters).  1 wins over 2.
 * Stream-ordered: no host synchronisation, no allocation.  Refusals precede any launch:
 * MHE_ERR_NULL for a missing struct or required pointer (mu0_s without S0_s or the reverse),
 * MHE_ERR_DIMS for a wrong struct_size, negative batch / steps, pmax outside 1..32, q != 3, the
 * vehicle's M / I_Z unset, MHE_ERR_MODEL for a pair that is not compiled (batch == 0 or
 * steps == 0: MHE_OK, nothing is read).
 */
typedef struct mhe_em_args {
  int32_t struct_size; /* = sizeof(mhe_em_args) */
  int32_t batch, steps;
  const double* mu_s;
  const double* S_s;
  const double* C;
  const double* mu0_s;
  const double* S0_s;
  const double* U;
  int64_t u_bstride;
  const double* Z;
  int64_t z_bstride;
  const int32_t* nz;
  int64_t nz_bstride;
  const double* PAR;
  int64_t par_bstride;
  const int32_t* rej;
  double* Qsum;
  int32_t* q_cnt;
  double* r2;
  int32_t* r_cnt;
  int32_t* status;
} mhe_em_args;

int mhe_ekf_em_stats(const mhe_ekf_dims* dims, const mhe_em_args* args, void* stream);

/*
 * Unscented fixed-interval (Rauch-Tung-Striebel) smoother over the history mhe_ukf_run wrote
 * (added within ABI v11; no existing struct or function changed).  One wavefront per filter, by
 * the dynamics' VALUES only: no Jacobian enters.  c, wm and wc are mhe_ukf_run's, from the same
 * (alpha, beta, kappa).  Carrying (mu_s, S_s) of step k+1, which at step steps-1 are the filtered
 * values, for k = steps-2 .. 0:
 *   S_k = L L^T                   upper triangle of S_hist read and mirrored; true sqrt and division
 *   X_0 = mu_k, X_j = mu_k +- c L[:, j]              the forward's sigma points
 *   Y_j = f(X_j, u_{k+1})                            (history entry k -> k+1 used u_{k+1})
 *   mu- = sum wm_j Y_j,  S- = sum wc_j (Y_j - mu-)(Y_j - mu-)^T + Q    the forward's expressions
 *   C   = sum wc_j (X_j - mu_k)(Y_j - mu-)^T         n x n cross covariance
 *   S-  = L- L-^T,  M = (S-)^-1 C^T                  two triangular solves per column, no inverse
 *   mu_s[k] = mu_k + M^T (mu_s[k+1] - mu-),  S_s[k] = S_k + M^T (S_s[k+1] - S-) M
 * Every sum runs in a fixed order (j increasing), so a filter's result is bitwise the same alone
 * or anywhere in any batch; S_s is computed on its upper triangle and mirrored, so it is bitwise
 * symmetric.  On the history of a run without corrections (nz = 0 throughout) the recomputed
 * (mu-, S-) are the history's own next entry, and the call returns that history bitwise.
 * Of dims this call reads what mhe_ekf_smooth reads; measurements and R do not enter.
 *   mu_hist, S_hist, U, u_bstride, Q, mu0, S0, mu_s, S_s, mu0_s, S0_s   as mhe_ekf_smooth's (layouts,
 *                    optional priors, in-place aliasing: a wave has read step k of the input
 *                    before it writes step k of the output); the smoothed prior is one more
 *                    step of the recursion from (mu0, S0) with u_0
 *   alpha, beta, kappa   as mhe_ukf_args', refused alike
 *   status (B, optional): 0 ok; 1 a pivot of S_k or S- was not positive and finite, or a value
 *                    written at a step was not finite (a NaN or an infinity in the copied last
 *                    step or met in the history): that filter's outputs are NaN from the
 *                    failing step down to step 0 (and its smoothed prior); the steps above it
 *                    and every other filter are bitwise those of the healthy run.
 * Stream-ordered: no host synchronisation, no allocation.  Refusals precede any launch and are
 * mhe_ekf_smooth's, plus mhe_ukf_run's for the struct size and (alpha, beta, kappa)
 * (batch == 0 or steps == 0: MHE_OK, nothing is read).
 */
typedef struct mhe_ukf_smooth_args {
  int32_t struct_size; /* = sizeof(mhe_ukf_smooth_args) */
  int32_t batch, steps;
  const double* mu_hist;
  const double* S_hist;
  const double* U;
  int64_t u_bstride;
  const double* Q;
  const double* mu0;
  const double* S0;
  double* mu_s;
  double* S_s;
  double* mu0_s;
  double* S0_s;
  int32_t* status;
  double alpha, beta, kappa;
} mhe_ukf_smooth_args;

int mhe_ukf_smooth(const mhe_ekf_dims* dims, const mhe_ukf_smooth_args* args, void* stream);

/* ------------------------------------------------------------------------
 * Batched GNSS least-squares fixes (the MHE initialiser).
 * Replaces utils/leastsquares.py:19-42 (iterativeLeastSquares),
 * :45-63 (iterativeLeastSquaresVel) and the per-epoch loop of
 * runLeastSquares (:97-141) for `chains` logs of `epochs` epochs each.
 * ------------------------------------------------------------------------ */
typedef struct mhe_ls_dims {
  int32_t struct_size; /* = sizeof(mhe_ls_dims) */
  int32_t slots;     /* satellite slots per epoch in the arrays (<= 64) */
  int32_t max_iter;  /* maxiter of iterativeLeastSquares (reference default 100); 0 = no position
                        iterations (velocity at x_init: iterativeLeastSquaresVel alone) */
  int32_t warm;      /* 1: epochs of a chain run in order, each starting from the previous fix
                        (the reference's shared default x, utils/leastsquares.py:19,34);
                        0: every epoch starts from x_init (all epochs in parallel) */
  int32_t with_vel;  /* 1: also the velocity / bias-rate solve (utils/leastsquares.py:45-63) */
  double tol;        /* stop when ||dx|| < tol (reference: 1e-7) */
} mhe_ls_dims;

/*
 * Device pointers.  Per chain c and epoch k (e = c*epochs + k):
 *   sat_pos (C,T,slots,3) ECEF, pr (C,T,slots), nsat (C,T): rows 0..nsat-1 valid
 *   sat_vel (C,T,slots,3), pr_rate (C,T,slots): only with with_vel
 *   x_init (C,3): starting position (b starts at 0 every epoch, as the reference)
 * Outputs: x_out (C,T,3), b_out (C,T), v_out (C,T,3) / bd_out (C,T) with with_vel
 * (NaN where the velocity system is singular: velocity failure alone leaves
 * iters_out untouched), iters_out (C,T) position GN steps taken (-1: fewer than 4
 * independent satellites for the position fix),
 * x_last (C,3, optional, warm only) the chain's final position (the value the
 * reference's shared default holds afterwards).  Returns MHE_OK or MHE_ERR_*.
 */
int mhe_ls_run(const mhe_ls_dims* dims, int32_t chains, int32_t epochs, const double* sat_pos,
               const double* pr, const int32_t* nsat, const double* sat_vel, const double* pr_rate,
               const double* x_init, double* x_out, double* b_out, double* v_out, double* bd_out,
               int32_t* iters_out, double* x_last, void* stream);

/* ------------------------------------------------------------------------
 * Multi-epoch least squares of a stationary receiver with a linearly drifting
 * clock (added to ABI v11; no existing struct or function changed).
 * Replaces utils/leastsquares.py:66-94 (iterativeLeastSquares_multiTimeStep), the
 * solve behind runBatchLeastSquares (:144-169), for `chains` logs at once: one
 * position x, a bias b0 at t = 0 and a drift alpha shared by ALL rows of a log,
 * Gauss-Newton on pr_k - |s_k - x| - b0 - alpha t_k with rows [-los, 1, t_k].
 * ------------------------------------------------------------------------ */
typedef struct mhe_lsm_dims {
  int32_t struct_size; /* = sizeof(mhe_lsm_dims) */
  int32_t max_iter;    /* maxiter of the reference (default 100); 0: outputs = p_init */
  double tol;          /* stop after the update when ||dx||_2 < tol, all five components
                          (reference: 1e-7) */
} mhe_lsm_dims;

/*
 * Device pointers; rows are flat, as in the reference function's signature:
 *   sat_pos (C,row_cap,3) ECEF, pr (C,row_cap), t (C,row_cap): row r of log c holds one
 *   pseudorange and the time it was taken; nrows (C): rows 0..nrows[c]-1 are valid
 *   (clamped to row_cap), rows beyond are never read
 *   p_init (C,5): x (3), b0, alpha to start from
 * Outputs: p_out (C,5) in the same order; iters_out (C) GN steps taken, or -1 (flagged)
 * when the log has fewer than 5 rows, all its rows share one value of t (the 1 and t
 * columns are then parallel), or a Cholesky pivot of the 5x5 normal matrix is not positive.
 * A flagged log's p_out is its last complete iterate (p_init if the first step fails).
 * A lane group of 16 or 64 owns one log; which one is a function of row_cap alone
 * (mhe_ls_multi_group), so a log's result is bitwise the same alone or in any batch.
 * Stream-ordered: no host synchronisation, no allocation.  Returns MHE_OK or MHE_ERR_*.
 */
int mhe_ls_multi_run(const mhe_lsm_dims* dims, int32_t chains, int32_t row_cap, const double* sat_pos,
                     const double* pr, const double* t, const int32_t* nrows, const double* p_init,
                     double* p_out, int32_t* iters_out, void* stream);

/* Lanes per log (16 or 64) of the instance mhe_ls_multi_run launches for this row
 * capacity (MHE_OPT_LSM_GROUP, when set, overrides the rule); MHE_ERR_DIMS if row_cap < 0. */
int32_t mhe_ls_multi_group(int32_t row_cap);

/* Library version string. */
const char* mhe_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MHE_H */
