// libmhe: cross-lane sums over a wavefront without LDS (DPP within a 16-lane row,
// v_permlane16/32_swap across rows).  Shared by the estimator kernels (mhe_core.h)
// and the multi-epoch least-squares kernel (mhe_ls.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace mhe {

// Butterfly step over lanes within a DPP row: quad_perm xor 1 / xor 2,
// row_half_mirror, row_mirror -- each leaves every lane of the row holding the
// combined value of its partner set.  Then v_permlane16/32_swap across rows.
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_mov_dpp((int)b, CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_mov_dpp((int)(b >> 32), CTRL, 0xF, 0xF, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// v_permlane16_swap (XOR16 = 1: row pairs) / v_permlane32_swap (2: wave halves)
// with the same register as both operands leaves the two members of each pair in
// [0] and [1] in every lane; OP combines them (sum / max).
template <int XOR16, bool MAX>
__device__ __forceinline__ double pair_combine(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = (int)b, hi = (int)(b >> 32);
  double x, y;
  if constexpr (XOR16 == 1) {
    auto l = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    auto h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    x = __longlong_as_double(((long long)h[0] << 32) | (unsigned int)l[0]);
    y = __longlong_as_double(((long long)h[1] << 32) | (unsigned int)l[1]);
  } else {
    auto l = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    auto h = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    x = __longlong_as_double(((long long)h[0] << 32) | (unsigned int)l[0]);
    y = __longlong_as_double(((long long)h[1] << 32) | (unsigned int)l[1]);
  }
  return MAX ? fmax(x, y) : x + y;
}

__device__ __forceinline__ double wave_sum(double v) {
  v += dpp_d<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_d<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_d<0x141>(v);  // row_half_mirror
  v += dpp_d<0x140>(v);  // row_mirror
  v = pair_combine<1, false>(v);
  return pair_combine<2, false>(v);
}

}  // namespace mhe
