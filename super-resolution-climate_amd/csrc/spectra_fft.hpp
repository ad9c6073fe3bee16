// What the spectral score (spectra.hip) and the spectral loss (spectral_loss.hip) share:
// the workgroup size, the non-finite test, the overlap plan's origin and the radix-2 LDS
// FFT over lines of P points.
#pragma once
#include <hip/hip_runtime.h>

namespace srmi {

constexpr int kSpecThreads = 256;

__device__ inline bool spec_nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// origin of window i of the axis plan (L, P, Q): min(i Q, L - P)
__device__ inline int spec_origin(int i, int L, int P, int Q) { return min(i * Q, L - P); }

// radix-2 DIT over NL lines of P values at buf[l * LS ..], inputs at bit-reversed
// positions, outputs in natural order.  Ends with a barrier.  The butterflies of a stage
// are disjoint, so a thread reads all of its own before it writes any: the LDS reads of a
// stage are in flight together.  tw[k] = exp(-2 pi i k / P) is the forward transform, its
// conjugate the unnormalised inverse.
template <int P, int NL>
__device__ inline void spec_fft_lines(float2* buf, const float2* tw, int LS) {
  constexpr int HP = P / 2, TOT = NL * HP, NB = (TOT + kSpecThreads - 1) / kSpecThreads;
#pragma unroll 1
  for (int half = 1; half < P; half <<= 1) {
    const int tstep = HP / half;
    float2 t[NB], u[NB], x[NB];
    int i0[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int bfly = min((int)threadIdx.x + i * kSpecThreads, TOT - 1);
      const int l = bfly / HP, k = bfly % HP;
      const int j = k & (half - 1);
      i0[i] = l * LS + ((k - j) << 1) + j;
      t[i] = tw[j * tstep];
      u[i] = buf[i0[i]];
      x[i] = buf[i0[i] + half];
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      if ((int)threadIdx.x + i * kSpecThreads >= TOT) continue;
      const float vr = x[i].x * t[i].x - x[i].y * t[i].y, vi = x[i].x * t[i].y + x[i].y * t[i].x;
      buf[i0[i]] = make_float2(u[i].x + vr, u[i].y + vi);
      buf[i0[i] + half] = make_float2(u[i].x - vr, u[i].y - vi);
    }
    __syncthreads();
  }
}

}  // namespace srmi
