// libmhe: the filter plug-ins as device functors, shared by the batched EKF (mhe_ekf.hip:
// step / row, value and Jacobian) and the batched UKF (mhe_ukf.hip: f / h, value only).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace mhe_ekf {

// ---------------------------------------------------------------- plug-ins
// gnss_pos_and_bias, utils/gnss.py:79-90: x+ = x + dt [u0, u1, u2, x4, 0],
// G = I + dt e_3 e_4^T (the reference updates x in place; G does not depend on x).
// gnz(r, c): structural non-zeros of G (compile-time; the predict skips the rest).
struct EkfGnssPosAndBias {
  static constexpr int n = 5, m = 3;
  static constexpr bool gnz(int r, int c) { return r == c || (r == 3 && c == 4); }
  __device__ static void step(const double* x, const double* u, double dt, const double* /*dp*/, double* xp,
                              double* G) {
    xp[0] = x[0] + dt * u[0];
    xp[1] = x[1] + dt * u[1];
    xp[2] = x[2] + dt * u[2];
    xp[3] = x[3] + dt * x[4];
    xp[4] = x[4] + dt * 0.0;
    for (int i = 0; i < n * n; ++i) G[i] = 0.0;
    for (int i = 0; i < n; ++i) G[i * n + i] = 1.0;
    G[3 * n + 4] = dt;
  }
  // the value alone (k_ukf)
  __device__ static void f(const double* x, const double* u, double dt, const double* /*dp*/, double* xp) {
    xp[0] = x[0] + dt * u[0];
    xp[1] = x[1] + dt * u[1];
    xp[2] = x[2] + dt * u[2];
    xp[3] = x[3] + dt * x[4];
    xp[4] = x[4] + dt * 0.0;
  }
};

// discrete_vehicle_dynamics of autonomous-car.py:18-52 (a script-defined EKF plug-in):
// x = [px, py, psi, vx, vy, r, b, bd, pz], u = [F_xr, delta]; explicit Euler on the
// dynamic bicycle of utils/vehicle_sim.py:72-85 with the linear tyres of :58-66
// (slip angles (vy -+ D r)/vx, no epsilon), plus b+ = b + dt bd.
// dp = car_params as [C_AF, C_AR, M, D_F, D_R, I_Z].  Bug-compatible with the
// reference: x is updated IN PLACE before the Jacobian is formed (autonomous-car.py:23),
// so every entry of G below is evaluated at the PREDICTED state x+, and G holds exactly
// the entries the reference writes.
struct EkfDiscreteVehicle {
  static constexpr int n = 9, m = 2;
  static constexpr bool gnz(int r, int c) {
    return r == c || ((r == 0 || r == 1) && c >= 2 && c <= 4) || (r == 2 && c == 5) ||
           (r >= 3 && r <= 5 && c >= 3 && c <= 5) || (r == 6 && c == 7);
  }
  // the Euler step alone (k_ukf): xd at x, utils/vehicle_sim.py:72-85 with linear_tire_model
  __device__ static void f(const double* x, const double* u, double dt, const double* dp, double* xp) {
    const double C_AF = dp[0], C_AR = dp[1], Mv = dp[2], D_F = dp[3], D_R = dp[4], I_Z = dp[5];
    const double a_r = (x[4] - D_R * x[5]) / x[3];
    const double a_f = (x[4] + D_F * x[5]) / x[3] - u[1];
    const double F_yr = -C_AR * a_r, F_yf = -C_AF * a_f;
    double sp, cp, su, cu;
    sincos(x[2], &sp, &cp);
    sincos(u[1], &su, &cu);
    xp[0] = x[0] + dt * (x[3] * cp - x[4] * sp);
    xp[1] = x[1] + dt * (x[3] * sp + x[4] * cp);
    xp[2] = x[2] + dt * x[5];
    xp[3] = x[3] + dt * ((-F_yf * su + u[0]) / Mv + x[5] * x[4]);
    xp[4] = x[4] + dt * ((F_yf * cu + F_yr) / Mv - x[5] * x[3]);
    xp[5] = x[5] + dt * ((D_F * F_yf * cu - D_R * F_yr) / I_Z);
    xp[6] = x[6] + dt * x[7];
    xp[7] = x[7] + dt * 0.0;
    xp[8] = x[8] + dt * 0.0;
  }
  __device__ static void step(const double* x, const double* u, double dt, const double* dp, double* xp,
                              double* G) {
    const double C_AF = dp[0], C_AR = dp[1], Mv = dp[2], D_F = dp[3], D_R = dp[4], I_Z = dp[5];
    {  // xd at x (utils/vehicle_sim.py:72-85 with linear_tire_model)
      const double a_r = (x[4] - D_R * x[5]) / x[3];
      const double a_f = (x[4] + D_F * x[5]) / x[3] - u[1];
      const double F_yr = -C_AR * a_r, F_yf = -C_AF * a_f;
      double sp, cp, su, cu;
      sincos(x[2], &sp, &cp);
      sincos(u[1], &su, &cu);
      xp[0] = x[0] + dt * (x[3] * cp - x[4] * sp);
      xp[1] = x[1] + dt * (x[3] * sp + x[4] * cp);
      xp[2] = x[2] + dt * x[5];
      xp[3] = x[3] + dt * ((-F_yf * su + u[0]) / Mv + x[5] * x[4]);
      xp[4] = x[4] + dt * ((F_yf * cu + F_yr) / Mv - x[5] * x[3]);
      xp[5] = x[5] + dt * ((D_F * F_yf * cu - D_R * F_yr) / I_Z);
      xp[6] = x[6] + dt * x[7];
      xp[7] = x[7] + dt * 0.0;
      xp[8] = x[8] + dt * 0.0;
    }
    // Jacobian at x+ (autonomous-car.py:27-51)
    const double* y = xp;
    const double ivx = 1.0 / (y[3] * y[3]);
    const double dfyf_dvx = C_AF * (y[4] + D_F * y[5]) * ivx;
    const double dfyf_dvy = -C_AF / y[3];
    const double dfyf_dr = -C_AF * D_F / y[3];
    const double dfyr_dvx = C_AR * (y[4] - D_R * y[5]) * ivx;
    const double dfyr_dvy = -C_AR / y[3];
    const double dfyr_dr = C_AR * D_R / y[3];
    double sp, cp, su, cu;
    sincos(y[2], &sp, &cp);
    sincos(u[1], &su, &cu);
    for (int i = 0; i < n * n; ++i) G[i] = 0.0;
    for (int i = 0; i < n; ++i) G[i * n + i] = 1.0;
    G[0 * n + 2] += dt * (-y[3] * sp - y[4] * cp);
    G[0 * n + 3] += dt * cp;
    G[0 * n + 4] += -dt * sp;
    G[1 * n + 2] += dt * (y[3] * cp - y[4] * sp);
    G[1 * n + 3] += dt * sp;
    G[1 * n + 4] += dt * cp;
    G[2 * n + 5] += dt;
    G[3 * n + 3] += -(dt / Mv) * (su * dfyf_dvx);
    G[3 * n + 4] += dt * (y[5] - (su * dfyf_dvy) / Mv);
    G[3 * n + 5] += dt * (y[4] - (su * dfyf_dr) / Mv);
    G[4 * n + 3] += dt * ((cu * dfyf_dvx + dfyr_dvx) / Mv - y[5]);
    G[4 * n + 4] += (dt / Mv) * (cu * dfyf_dvy + dfyr_dvy);
    G[4 * n + 5] += dt * ((cu * dfyf_dr + dfyr_dr) / Mv - y[3]);
    G[5 * n + 3] += (dt / I_Z) * (D_F * cu * dfyf_dvx - D_R * dfyr_dvx);
    G[5 * n + 4] += (dt / I_Z) * (D_F * cu * dfyf_dvy - D_R * dfyr_dvy);
    G[5 * n + 5] += (dt / I_Z) * (D_F * cu * dfyf_dr - D_R * dfyr_dr);
    G[6 * n + 7] += dt;
  }
};

// Row i of multi_pseudorange (utils/gnss.py:27-45 via pseudorange :4-24):
//   h = |x[:3] - s_i| + x[3],  H = [-(s_i - x[:3]) / |s_i - x[:3]|, 1, 0]
// with_bias (multi_pseudorange_and_bias, :48-61): the extra last row is h = x[3]
// and -- bug-compatible -- an all-zero Jacobian row.
template <bool with_bias>
struct EkfMultiPseudorange {
  static constexpr int q = 3;
  static constexpr int lane_minw = with_bias ? 2 : 4;  // k_ekf_lane waves per SIMD (no spills)
  static constexpr int lane_minw_gate = 2;  // the gated instances' own bound
  template <int n>
  __device__ static void row(const double* x, const double* par, int i, int nz, double& h, double* H) {
    if (with_bias && i == nz - 1) {
      h = x[3];
      for (int c = 0; c < n; ++c) H[c] = 0.0;
      return;
    }
    const double l0 = par[0] - x[0], l1 = par[1] - x[1], l2 = par[2] - x[2];
    const double r = sqrt(l0 * l0 + l1 * l1 + l2 * l2);
    h = sqrt((x[0] - par[0]) * (x[0] - par[0]) + (x[1] - par[1]) * (x[1] - par[1]) +
             (x[2] - par[2]) * (x[2] - par[2])) + x[3];
    for (int c = 0; c < n; ++c) H[c] = 0.0;
    H[0] = -l0 / r;
    H[1] = -l1 / r;
    H[2] = -l2 / r;
    H[3] = 1.0;
  }
  // the value alone (k_ukf): the bias row is h = x[3] and, with no Jacobian in play, acts
  template <int n>
  __device__ static double h(const double* x, const double* par, int i, int nz) {
    if (with_bias && i == nz - 1) return x[3];
    return sqrt((x[0] - par[0]) * (x[0] - par[0]) + (x[1] - par[1]) * (x[1] - par[1]) +
                (x[2] - par[2]) * (x[2] - par[2])) + x[3];
  }
};

// vehicle_sensors_model of autonomous-car.py:54-77: multi_pseudorange on
// x_meas = [px, py, pz, b, bd] = x[0, 1, 8, 6, 7]; row i: h = |p - s_i| + b and the
// 5-column Jacobian scattered back to the 9-state (columns 0, 1, 8, 6, 7).
struct EkfVehicleSensors {
  static constexpr int q = 3;
  static constexpr int lane_minw = 2;
  static constexpr int lane_minw_gate = 1;  // no scratch (spills go to AGPRs); 2 spills to scratch, 1.6x slower
  template <int n>
  __device__ static void row(const double* x, const double* par, int /*i*/, int /*nz*/, double& h, double* H) {
    const double l0 = par[0] - x[0], l1 = par[1] - x[1], l2 = par[2] - x[8];
    const double r = sqrt(l0 * l0 + l1 * l1 + l2 * l2);
    h = sqrt((x[0] - par[0]) * (x[0] - par[0]) + (x[1] - par[1]) * (x[1] - par[1]) +
             (x[8] - par[2]) * (x[8] - par[2])) + x[6];
    for (int c = 0; c < n; ++c) H[c] = 0.0;
    H[0] = -l0 / r;
    H[1] = -l1 / r;
    H[8] = -l2 / r;
    H[6] = 1.0;
  }
  template <int n>
  __device__ static double h(const double* x, const double* par, int /*i*/, int /*nz*/) {
    return sqrt((x[0] - par[0]) * (x[0] - par[0]) + (x[1] - par[1]) * (x[1] - par[1]) +
                (x[8] - par[2]) * (x[8] - par[2])) + x[6];
  }
};

__device__ __forceinline__ double readlane_d(double v, int lane) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)b, lane);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

}  // namespace mhe_ekf
