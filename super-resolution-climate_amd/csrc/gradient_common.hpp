// The Sobel derivative at unit scale, shared by the gradient score (gradient.hip) and the
// gradient loss term (gradient_loss.hip) -- no reference counterpart.  srmi.h states the
// definition ("the gradient score"); this header is its device form: the operator on a 3x3
// window, and the staging of a workgroup's rectangle of pixels with its halo in LDS.
//
// A workgroup of kGradThreads threads owns kGradTileH x kGradTileW pixels.  The staged rows
// start kGradPadL = 4 columns left of the rectangle, so that every staged row begins on a
// 16-byte boundary of the plane's row whenever W % 4 == 0: the Vec forms load float4, the
// others one float at a time.  The choice is the caller's, from the shape and the pointers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace srmi {

constexpr int kGradThreads = 256;
constexpr int kGradTileH = 16, kGradTileW = 64;          // the pixels a workgroup owns
constexpr int kGradPadL = 4;                             // staged columns x0 - 4 .. x0 + 67
constexpr int kGradPitch = kGradTileW + 2 * kGradPadL;   // 72 floats
constexpr int kGradQuads = kGradPitch / 4;               // 18 float4 per staged row
constexpr int kGradLanesX = kGradTileW / 4;              // 16 threads across a row, 4 pixels each
static_assert(kGradLanesX * kGradTileH == kGradThreads, "one thread per four pixels of a row");

__device__ inline bool grad_nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }
__device__ inline float grad_nan() { return __uint_as_float(0x7fc00000u); }

// Gx = ((dX(y-1) + dX(y+1)) + 2 dX(y)) / 8, dX(r) = f(r, x+1) - f(r, x-1): differences first.
// The doubling and the division by 8 are exact, so a contraction changes nothing.
__device__ inline float grad_sobel_x(float m0, float m2, float c0, float c2, float p0, float p2) {
  const float dm = m2 - m0, dc = c2 - c0, dp = p2 - p0;
  return ((dm + dp) + 2.0f * dc) * 0.125f;
}
// Gy = ((dY(x-1) + dY(x+1)) + 2 dY(x)) / 8, dY(c) = f(y+1, c) - f(y-1, c)
__device__ inline float grad_sobel_y(float m0, float m1, float m2, float p0, float p1, float p2) {
  const float dl = p0 - m0, dc = p1 - m1, dr = p2 - m2;
  return ((dl + dr) + 2.0f * dc) * 0.125f;
}

// x x + y y (+ eps), every product and sum rounded on its own: device code is compiled with
// contraction allowed, and a compiler free to choose which product it fuses gives equal inputs
// unequal magnitudes.  The pragma takes the contract flag off these operations for good.
__device__ inline float grad_mag2(float x, float y) {
#pragma clang fp contract(off)
  const float xx = x * x, yy = y * y;
  return xx + yy;
}
__device__ inline float grad_mag2_eps(float x, float y, float eps) {
#pragma clang fp contract(off)
  const float xx = x * x, yy = y * y;
  const float s = xx + yy;
  return s + eps;
}

// the six staged values a thread's four windows of one row need: columns o - 1 .. o + 4
struct GradRow6 {
  float v[6];
};
__device__ inline GradRow6 grad_row6(const float* __restrict__ s, int o) {
  GradRow6 r;
  const float4 m = *reinterpret_cast<const float4*>(s + o);  // o % 4 == 0, s 16-byte aligned
  r.v[0] = s[o - 1];
  r.v[1] = m.x;
  r.v[2] = m.y;
  r.v[3] = m.z;
  r.v[4] = m.w;
  r.v[5] = s[o + 4];
  return r;
}
// the same at the ends of a staged row: the column left of quad 0 / right of the last is NaN
__device__ inline GradRow6 grad_row6_edge(const float* __restrict__ s, int q) {
  GradRow6 r;
  const int o = 4 * q;
  const float4 m = *reinterpret_cast<const float4*>(s + o);
  r.v[0] = q > 0 ? s[o - 1] : grad_nan();
  r.v[1] = m.x;
  r.v[2] = m.y;
  r.v[3] = m.z;
  r.v[4] = m.w;
  r.v[5] = q < kGradQuads - 1 ? s[o + 4] : grad_nan();
  return r;
}

// Stage rows ya .. ya + NR - 1, columns xa .. xa + kGradPitch - 1 (xa % 4 == 0) of the planes a
// and b.  put(offset, va[4], vb[4]) receives four neighbouring pixels, NaN in both outside the
// plane.  Vec: W % 4 == 0 and 16-byte aligned planes, so a quad lies inside a row or outside.
template <bool Vec, int NR, class Put>
__device__ inline void grad_stage(const float* __restrict__ a, const float* __restrict__ b, int H, int W, int ya,
                                  int xa, int tid, Put put) {
  for (int e = tid; e < NR * kGradQuads; e += kGradThreads) {
    const int ly = e / kGradQuads, q = e - ly * kGradQuads;
    const int y = ya + ly, x = xa + 4 * q;
    const bool row_in = y >= 0 && y < H;
    float va[4], vb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) va[i] = vb[i] = grad_nan();
    if (Vec) {
      if (row_in && x >= 0 && x < W) {
        const size_t o = (size_t)y * W + x;
        const float4 A = *reinterpret_cast<const float4*>(a + o);
        const float4 B = *reinterpret_cast<const float4*>(b + o);
        va[0] = A.x, va[1] = A.y, va[2] = A.z, va[3] = A.w;
        vb[0] = B.x, vb[1] = B.y, vb[2] = B.z, vb[3] = B.w;
      }
    } else if (row_in) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int xi = x + i;
        if (xi >= 0 && xi < W) {
          const size_t o = (size_t)y * W + xi;
          va[i] = a[o];
          vb[i] = b[o];
        }
      }
    }
    put(ly * kGradPitch + 4 * q, va, vb);
  }
}

inline bool grad_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace srmi
