// The bin of a value and the loads of a lane's run: what the distribution score
// (distribution.hip) and the quantile map's histograms (quantile_map.hip) share, so that the
// two form the same tables from the same values.  srmi.h, "the distribution score", states
// the bin; the operations here are that definition, each rounded once (__f*_rn: no fused form
// whatever the contraction setting of the including file).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace srmi {

namespace {

constexpr int kDistRun = 8;  // consecutive pixels of a lane per step

__device__ inline bool dist_nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// 8 consecutive pixels from i0 (a multiple of 8); past the plane: NaN, which no one uses.
// vec: the plane starts on a 16-byte boundary.
__device__ inline void dist_load_run(const float* __restrict__ p, long long i0, long long HW, bool vec,
                                     float (&v)[kDistRun]) {
  if (i0 + kDistRun <= HW) {
    if (vec) {
      const float4 q0 = *reinterpret_cast<const float4*>(p + i0);
      const float4 q1 = *reinterpret_cast<const float4*>(p + i0 + 4);
      v[0] = q0.x, v[1] = q0.y, v[2] = q0.z, v[3] = q0.w;
      v[4] = q1.x, v[5] = q1.y, v[6] = q1.z, v[7] = q1.w;
    } else {
#pragma unroll
      for (int k = 0; k < kDistRun; ++k) v[k] = p[i0 + k];
    }
  } else {
#pragma unroll
    for (int k = 0; k < kDistRun; ++k) v[k] = i0 + k < HW ? p[i0 + k] : __uint_as_float(0x7fc00000u);
  }
}

// index into the n + 2 entries {under, n bins, over}.  The comparisons decide under and over
// before any conversion, and the converted value is clamped again as an integer.
__device__ inline int dist_bin(float x, float lo, float hi, float scale, int n) {
  if (x < lo) return 0;
  if (x > hi) return n + 1;
  if (x == hi) return n;  // what the formula gives whenever hi > lo; also the bin when hi == lo
  const int k = (int)__fmul_rn(__fsub_rn(x, lo), scale);
  return 1 + min(max(k, 0), n - 1);
}

}  // namespace

}  // namespace srmi
