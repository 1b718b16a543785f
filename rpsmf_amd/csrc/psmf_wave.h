// Wave-level primitives every engine shares: the vector typedefs, lane reads, the DPP / permlane sums and the LDS-only barrier.
// Defines no kernel, so any translation unit may include it.
#pragma once
#include "psmf_device.h"

namespace psmf {

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef float f32x4s __attribute__((ext_vector_type(4)));
typedef float f32x2s __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double readlane_f64(double v, const int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

#define F3_DPP64(x, ctrl)                                                                                  \
  __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(x), ctrl, 0xF, 0xF, true),                \
                   __builtin_amdgcn_update_dpp(0, __double2loint(x), ctrl, 0xF, 0xF, true))

// sum over each 16-lane row, float64, DPP only; every lane of a row ends up with its row's sum
__device__ __forceinline__ double row_sum_f64_dpp(double v) {
  v += F3_DPP64(v, 0xB1);    // quad_perm [1,0,3,2]
  v += F3_DPP64(v, 0x4E);    // quad_perm [2,3,0,1]
  v += F3_DPP64(v, 0x141);   // row_half_mirror
  v += F3_DPP64(v, 0x140);   // row_mirror
  return v;
}

// sum over the 64 lanes, float64, fixed order; result uniform
__device__ __forceinline__ double wave_sum_f64_dpp(double v) {
  v = row_sum_f64_dpp(v);
  return (readlane_f64(v, 0) + readlane_f64(v, 16)) + (readlane_f64(v, 32) + readlane_f64(v, 48));
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains vmcnt: the y_hat coefficients and the
// mean history are stored to global memory inside the step loop, and every barrier behind such a store waited for its
// acknowledgement (~400 cycles per barrier, measured with the stamps).  Nothing in the loop READS global memory written
// in the loop, so LDS order is all the steps need.
__device__ __forceinline__ void f3_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// x + (x of the lane 16 rows over) and x + (x of the lane in the other half): v_permlane16_swap / v_permlane32_swap
// (gfx950) exchange whole 16-lane rows between two registers in the VALU; ds_bpermute costs an LDS round trip.
__device__ __forceinline__ double xor16_sum_f64(double x) {
  const unsigned lo = __double2loint(x), hi = __double2hiint(x);
  const auto l2 = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  const auto h2 = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  return __hiloint2double(h2[0], l2[0]) + __hiloint2double(h2[1], l2[1]);
}
__device__ __forceinline__ double xor32_sum_f64(double x) {
  const unsigned lo = __double2loint(x), hi = __double2hiint(x);
  const auto l2 = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  const auto h2 = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  return __hiloint2double(h2[0], l2[0]) + __hiloint2double(h2[1], l2[1]);
}

}  // namespace psmf
