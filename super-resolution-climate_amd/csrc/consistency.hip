// Consistency of a super-resolved field with its coarse input -- no reference counterpart
// (the reference never starts from a coarse field).  srmi.h states the contract; this file
// is its device form.
//
// With D the task's downsample (F.interpolate at 1/s, align_corners=False) and U its
// upsample, iterative back-projection x <- x + U(lr - D x) never has to iterate at HR size:
// at an even s, D reads only the s x s children of an LR pixel (bicubic: taps s/2 - 2 ..
// s/2 + 1 with [-3, 19, 19, -3] / 32; bilinear: s/2 - 1, s/2 with 1/2, 1/2), so with
// r0 = lr - D x0 and E = I - D U
//     x_K = x0 + U(R_K),   R_K = sum_{k < K} E^k r0,   lr - D x_K = E^K r0,
// and D U, in LR space, is a fixed separable stencil of 5 taps per axis (3 when U is
// bilinear) read at clamped indices -- U's own edge handling.
//
// Three streaming kernels, plain vector loads and stores, no LDS, no atomics:
//   consistency_residual_kernel  one thread per LR cell: the tap rows of its s x s block
//                                (float4 loads along rows where s % 4 == 0), summed in
//                                downsample_kernel's order; r0 and the active mask.
//   consistency_iterate_kernel   one thread per LR cell: R (+)= r, r' = M (r - (D U) r).
//   consistency_apply_kernel     one thread per run of s HR pixels of a row (the children
//                                of one LR cell in that row): its 4 x 5 (2 x 3) LR
//                                neighbourhood of R once, combined along y first; then per
//                                pixel the x weights of srmi_upsample / srmi_interpolate.
//                                Finite pixels are updated, the others never written.
// and the three of the correction's adjoint (training through it), described where they
// stand: consistency_adjoint_gather_kernel (U^T, the one kernel here that uses LDS),
// consistency_adjoint_iterate_kernel and consistency_adjoint_apply_kernel.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "common.hpp"
#include "srmi.h"
#include "srmi_internal.hpp"

namespace srmi {
namespace {

constexpr int kConsThreads = 256;
constexpr int kConsMaxGridY = 65535;

struct ConsStencil {
  float gy[5];  // D U along one axis at LR offsets -2 .. 2 (both axes share it)
  int radius;   // 2 (U bicubic) or 1 (U bilinear: gy[0] = gy[4] = 0)
};

__device__ __forceinline__ bool cons_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ void cons_cubic_w(float t, float* c) {  // small.hip's cubic_w, A = -0.75
  const float A = -0.75f;
  float x1 = t + 1.f;
  c[0] = ((A * x1 - 5.f * A) * x1 + 8.f * A) * x1 - 4.f * A;
  float x = t;
  c[1] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
  x = 1.f - t;
  c[2] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
  float x2 = 2.f - t;
  c[3] = ((A * x2 - 5.f * A) * x2 + 8.f * A) * x2 - 4.f * A;
}

// ---------------------------------------------------------------------- residual
// S > 0: the float4 form for that scale (S % 4 == 0, hr 16-byte aligned); S == 0: any
// even scale, scalar loads of the taps alone.  NT = taps per axis of D (4 bicubic, 2
// bilinear).  The taps lie inside the block, so no index is clamped.
template <int S, int NT>
__global__ void __launch_bounds__(kConsThreads)
    consistency_residual_kernel(const float* __restrict__ hr, const float* __restrict__ lr, int NC, int h, int w,
                                int scale, float* __restrict__ r0, int* __restrict__ active) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= h * w) return;
  const int x = i % w, y = i / w;
  const int s = S > 0 ? S : scale;
  const int a = s / 2 - NT / 2;
  const size_t W = (size_t)w * s, H = (size_t)h * s;
  float k[4];
  if (NT == 4) {
    k[0] = -3.f / 32.f, k[1] = 19.f / 32.f, k[2] = 19.f / 32.f, k[3] = -3.f / 32.f;
  } else {
    k[0] = 0.5f, k[1] = 0.5f, k[2] = 0.f, k[3] = 0.f;
  }
  for (size_t nc = blockIdx.y; nc < (size_t)NC; nc += gridDim.y) {
    const float* src = hr + nc * H * W + ((size_t)y * s + a) * W + (size_t)x * s;
    float acc = 0.f;
    bool ok = true;
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
      float v[NT];
      if (S > 0) {
        float row[S > 0 ? S : 4];
#pragma unroll
        for (int q = 0; q < S / 4; ++q) {
          const float4 f = reinterpret_cast<const float4*>(src + (size_t)ti * W)[q];
          row[4 * q] = f.x, row[4 * q + 1] = f.y, row[4 * q + 2] = f.z, row[4 * q + 3] = f.w;
        }
#pragma unroll
        for (int tj = 0; tj < NT; ++tj) v[tj] = row[(S > 0 ? S : 4) / 2 - NT / 2 + tj];
      } else {
#pragma unroll
        for (int tj = 0; tj < NT; ++tj) v[tj] = src[(size_t)ti * W + a + tj];
      }
      float rsum = 0.f;
#pragma unroll
      for (int tj = 0; tj < NT; ++tj) {
        ok = ok && cons_finite(v[tj]);
        rsum += k[tj] * v[tj];
      }
      acc += k[ti] * rsum;
    }
    const size_t o = nc * h * w + i;
    const float l = lr[o];
    ok = ok && cons_finite(l);
    r0[o] = ok ? l - acc : 0.f;
    active[o] = ok ? 1 : 0;
  }
}

// ----------------------------------------------------------------------- iterate
__global__ void __launch_bounds__(kConsThreads)
    consistency_iterate_kernel(const float* __restrict__ r, const int* __restrict__ active, int NC, int h, int w,
                               ConsStencil st, int first, float* __restrict__ R, float* __restrict__ r_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= h * w) return;
  const int x = i % w, y = i / w;
  const int rad = st.radius;
  for (size_t nc = blockIdx.y; nc < (size_t)NC; nc += gridDim.y) {
    const float* src = r + nc * h * w;
    const size_t o = nc * h * w + i;
    const float c = src[i];
    R[o] = first ? c : R[o] + c;
    float out = 0.f;
    if (active[o]) {
      float acc = 0.f;
      for (int dy = -rad; dy <= rad; ++dy) {
        const int yy = min(max(y + dy, 0), h - 1);
        float rsum = 0.f;
        for (int dx = -rad; dx <= rad; ++dx) {
          const int xx = min(max(x + dx, 0), w - 1);
          rsum += st.gy[dx + 2] * src[(size_t)yy * w + xx];
        }
        acc += st.gy[dy + 2] * rsum;
      }
      out = c - acc;
    }
    r_out[o] = out;
  }
}

// ------------------------------------------------------------------------- apply
// srmi_upsample's (bicubic) / srmi_interpolate's (bilinear) axis arithmetic at output index
// d of an axis of n LR samples: the first tap's UNCLAMPED LR index and the nt weights.
__device__ __forceinline__ int cons_up_axis(int mode, float inv, int d, int n, float* wt) {
  float src = inv * ((float)d + 0.5f) - 0.5f;
  if (mode == 1) {
    if (src < 0.f) src = 0.f;
    const int i0 = min((int)floorf(src), n - 1);
    const float t = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
    wt[0] = 1.f - t;
    wt[1] = t;
    return i0;
  }
  const int i0 = (int)floorf(src);
  cons_cubic_w(src - (float)i0, wt);
  return i0 - 1;
}

__device__ __forceinline__ float cons_pick(const float* v, int k) {  // v[k], k in 0 .. 4, without scratch
  return k == 0 ? v[0] : k == 1 ? v[1] : k == 2 ? v[2] : k == 3 ? v[3] : v[4];
}

// VEC: s % 4 == 0 and hr 16-byte aligned -- float4 loads and, for a quad of finite pixels,
// one float4 store; a quad holding a non-finite pixel is stored pixel by pixel, the
// non-finite ones not at all.
template <bool VEC>
__global__ void __launch_bounds__(kConsThreads)
    consistency_apply_kernel(const float* __restrict__ R, int NC, int h, int w, int s, int umode,
                             float* __restrict__ hr) {
  const int H = h * s;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= H * w) return;
  const int d = i % w, Y = i / w;
  const size_t W = (size_t)w * s;
  const int nt = umode == 1 ? 2 : 4;
  const float inv = 1.f / (float)s;
  float wy[4];
  const int y0 = cons_up_axis(umode, inv, Y, h, wy);
  for (size_t nc = blockIdx.y; nc < (size_t)NC; nc += gridDim.y) {
    const float* src = R + nc * h * w;
    float v[5];
#pragma unroll
    for (int cc = 0; cc < 5; ++cc) {
      const int xx = min(max(d + cc - 2, 0), w - 1);
      float acc = 0.f;
      for (int ti = 0; ti < nt; ++ti) {
        const int yy = min(max(y0 + ti, 0), h - 1);
        acc += wy[ti] * src[(size_t)yy * w + xx];
      }
      v[cc] = acc;
    }
    float* dst = hr + nc * H * W + (size_t)Y * W + (size_t)d * s;
    if (VEC) {
      for (int q = 0; q < s / 4; ++q) {
        float4 f = reinterpret_cast<float4*>(dst)[q];
        float px[4] = {f.x, f.y, f.z, f.w};
        float nw[4];
        bool all = true;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float wx[4];
          const int x0 = cons_up_axis(umode, inv, d * s + 4 * q + e, w, wx);
          const int rel = min(max(x0 - d + 2, 0), 5 - nt);
          float add = 0.f;
          for (int tj = 0; tj < nt; ++tj) add += wx[tj] * cons_pick(v, rel + tj);
          nw[e] = px[e] + add;
          all = all && cons_finite(px[e]);
        }
        if (all) {
          reinterpret_cast<float4*>(dst)[q] = make_float4(nw[0], nw[1], nw[2], nw[3]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (cons_finite(px[e])) dst[4 * q + e] = nw[e];
        }
      }
    } else {
      for (int p = 0; p < s; ++p) {
        const float px = dst[p];
        if (!cons_finite(px)) continue;
        float wx[4];
        const int x0 = cons_up_axis(umode, inv, d * s + p, w, wx);
        const int rel = min(max(x0 - d + 2, 0), 5 - nt);
        float add = 0.f;
        for (int tj = 0; tj < nt; ++tj) add += wx[tj] * cons_pick(v, rel + tj);
        dst[p] = px + add;
      }
    }
  }
}

// ----------------------------------------------------------------------- adjoint
// The correction is linear in x0: x_K = x0 + U P M (lr - D x0), P = sum_{k < K} E^k, E =
// M (I - G), G the clamped D U stencil.  Its transpose applied to a gradient g is
//     q = U^T g;  t_0 = q, t_{k+1} = (I - G^T)(M t_k), Q = sum_{k < K} t_k;  g0 = g - D^T (M Q)
// -- the three kernels below, each a gather with a fixed summation order.

// One axis of U^T as a table: row e holds, for HR index X0 + e (block c = X / s), the
// weight of that pixel on the LR cells c - 2 .. c + 2, the clamped taps of cons_up_axis
// folded onto the cell they read (ascending tap order).  Zero outside the field.
__device__ __forceinline__ void cons_ut_table(float* tab, int count, int X0, int n, int s, int umode, float inv) {
  const int nt = umode == 1 ? 2 : 4;
  for (int e = threadIdx.x; e < count; e += blockDim.x) {
    const int X = X0 + e;
    float o5[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (X >= 0 && X < n * s) {
      float wt[4];
      const int x0 = cons_up_axis(umode, inv, X, n, wt);
      const int c = X / s;
#pragma unroll
      for (int o = 0; o < 5; ++o) {
        float sum = 0.f;
        for (int ti = 0; ti < nt; ++ti)
          if (min(max(x0 + ti, 0), n - 1) == c + o - 2) sum += wt[ti];
        o5[o] = sum;
      }
    }
#pragma unroll
    for (int o = 0; o < 5; ++o) tab[e * 5 + o] = o5[o];
  }
}

// q = U^T g.  One workgroup per (band of TB LR rows, strip of TX LR columns), looping over
// its planes: the two axis tables once, then per plane the band's (TB + 4) s HR rows
// reduced along x into LDS (each LR column from the 5 s pixels of its 5 neighbouring
// blocks, ascending X) and those reduced along y (ascending Y).  The strip bounds the LDS
// whatever w s is.  VEC: s % 4 == 0 and g 16-byte aligned -- a block's pixels as float4.
template <bool VEC>
__global__ void __launch_bounds__(kConsThreads)
    consistency_adjoint_gather_kernel(const float* __restrict__ g, int NC, int h, int w, int s, int umode, int TB,
                                      int TX, int nstrips, float* __restrict__ q) {
  extern __shared__ float cons_lds[];
  const int rows = (TB + 4) * s, cols = (TX + 4) * s;
  float* tabx = cons_lds;           // [cols][5]
  float* taby = tabx + cols * 5;    // [rows][5]
  float* xbuf = taby + rows * 5;    // [rows][TX]
  const int jy0 = (blockIdx.x / nstrips) * TB, jx0 = (blockIdx.x % nstrips) * TX;
  const int nby = min(TB, h - jy0), nbx = min(TX, w - jx0);
  const int Y0 = (jy0 - 2) * s, X0 = (jx0 - 2) * s;
  const int H = h * s;
  const size_t W = (size_t)w * s;
  const int rad = umode == 1 ? 1 : 2;
  const float inv = 1.f / (float)s;
  cons_ut_table(tabx, cols, X0, w, s, umode, inv);
  cons_ut_table(taby, rows, Y0, h, s, umode, inv);
  __syncthreads();
  for (size_t nc = blockIdx.y; nc < (size_t)NC; nc += gridDim.y) {
    const float* src = g + nc * H * W;
    for (int e = threadIdx.x; e < rows * nbx; e += blockDim.x) {
      const int r = e / nbx, jl = e % nbx;
      const int Y = Y0 + r, jx = jx0 + jl;
      if (Y < 0 || Y >= H) continue;  // never read below
      const float* row = src + (size_t)Y * W;
      float acc = 0.f;
      for (int c = max(jx - rad, 0); c <= min(jx + rad, w - 1); ++c) {
        const float* tw = tabx + (c * s - X0) * 5 + (jx - c + 2);
        if (VEC) {
          const float4* p4 = reinterpret_cast<const float4*>(row + (size_t)c * s);
          for (int k = 0; k < s / 4; ++k) {
            const float4 f = p4[k];
            acc += tw[(4 * k) * 5] * f.x;
            acc += tw[(4 * k + 1) * 5] * f.y;
            acc += tw[(4 * k + 2) * 5] * f.z;
            acc += tw[(4 * k + 3) * 5] * f.w;
          }
        } else {
          for (int p = 0; p < s; ++p) acc += tw[p * 5] * row[(size_t)c * s + p];
        }
      }
      xbuf[r * TX + jl] = acc;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nby * nbx; e += blockDim.x) {
      const int jyl = e / nbx, jl = e % nbx;
      const int jy = jy0 + jyl;
      float acc = 0.f;
      for (int c = max(jy - rad, 0); c <= min(jy + rad, h - 1); ++c) {
        const int r0 = c * s - Y0;
        const int o = jy - c + 2;
        for (int p = 0; p < s; ++p) acc += taby[(r0 + p) * 5 + o] * xbuf[(r0 + p) * TX + jl];
      }
      q[nc * h * w + (size_t)jy * w + jx0 + jl] = acc;
    }
    __syncthreads();
  }
}

// Q (+)= t, t_out = M t - G^T (M t): one thread per LR cell.  Along an axis of n cells the
// transposed clamped stencil gathers from i = j - 2 .. j + 2 with w^T[j, i] = sum over o of
// g_o [clamp(i + o) = j] (the edge taps folded, ascending o); x taps summed per row in
// ascending i, rows then in ascending i.  An inactive cell is read as an exact zero.
__global__ void __launch_bounds__(kConsThreads)
    consistency_adjoint_iterate_kernel(const float* __restrict__ t, const int* __restrict__ active, int NC, int h,
                                       int w, ConsStencil st, int first, float* __restrict__ Q,
                                       float* __restrict__ t_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= h * w) return;
  const int x = i % w, y = i / w;
  const int rad = st.radius;
  float wy[5], wx[5];
#pragma unroll
  for (int d = 0; d < 5; ++d) {
    float sy = 0.f, sx = 0.f;
    const int iy = y + d - 2, ix = x + d - 2;
    for (int o = -rad; o <= rad; ++o) {
      if (iy >= 0 && iy < h && min(max(iy + o, 0), h - 1) == y) sy += st.gy[o + 2];
      if (ix >= 0 && ix < w && min(max(ix + o, 0), w - 1) == x) sx += st.gy[o + 2];
    }
    wy[d] = sy;
    wx[d] = sx;
  }
  for (size_t nc = blockIdx.y; nc < (size_t)NC; nc += gridDim.y) {
    const float* src = t + nc * h * w;
    const int* act = active + nc * h * w;
    const size_t o = nc * h * w + i;
    const float c = src[i];
    Q[o] = first ? c : Q[o] + c;
    float acc = 0.f;
#pragma unroll
    for (int dy = 0; dy < 5; ++dy) {
      const int yy = y + dy - 2;
      if (dy < 2 - rad || dy > 2 + rad || yy < 0 || yy >= h) continue;
      float rsum = 0.f;
#pragma unroll
      for (int dx = 0; dx < 5; ++dx) {
        const int xx = x + dx - 2;
        if (dx < 2 - rad || dx > 2 + rad || xx < 0 || xx >= w) continue;
        const int idx = yy * w + xx;
        rsum += wx[dx] * (act[idx] ? src[idx] : 0.f);
      }
      acc += wy[dy] * rsum;
    }
    t_out[o] = (act[i] ? c : 0.f) - acc;
  }
}

// g -= D^T (M Q): one thread per (tap row of D, LR cell) -- the NT tap pixels of that row
// inside the cell's block, g[Y, X] -= (k(Y mod s) k(X mod s)) Q[cell]; the products of two
// taps are exact in fp32.  Rows and pixels at non-tap phases, and the blocks of inactive
// cells, are never touched.  VEC (s % 4 == 0, g 16-byte aligned): taps that fill an
// aligned quad (bicubic at s = 4) go as one float4, an aligned pair as one float2.
template <bool VEC, int NT>
__global__ void __launch_bounds__(kConsThreads)
    consistency_adjoint_apply_kernel(const float* __restrict__ Q, const int* __restrict__ active, int NC, int h, int w,
                                     int s, float* __restrict__ g) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= h * NT * w) return;
  const int d = i % w, tr = i / w;
  const int y = tr / NT, ti = tr % NT;
  const int a = s / 2 - NT / 2;
  const size_t W = (size_t)w * s, H = (size_t)h * s;
  float k[4];
  if (NT == 4) {
    k[0] = -3.f / 32.f, k[1] = 19.f / 32.f, k[2] = 19.f / 32.f, k[3] = -3.f / 32.f;
  } else {
    k[0] = 0.5f, k[1] = 0.5f, k[2] = 0.f, k[3] = 0.f;
  }
  const float ky = k[ti];
  for (size_t nc = blockIdx.y; nc < (size_t)NC; nc += gridDim.y) {
    const size_t o = nc * h * w + (size_t)y * w + d;
    if (!active[o]) continue;
    const float v = Q[o];
    float* dst = g + nc * H * W + ((size_t)y * s + a + ti) * W + (size_t)d * s + a;
    if (VEC && NT == 4 && (a & 3) == 0) {
      float4 f = *reinterpret_cast<float4*>(dst);
      f.x -= (ky * k[0]) * v, f.y -= (ky * k[1]) * v, f.z -= (ky * k[2]) * v, f.w -= (ky * k[3]) * v;
      *reinterpret_cast<float4*>(dst) = f;
    } else if (VEC && (a & 1) == 0) {
#pragma unroll
      for (int p = 0; p < NT / 2; ++p) {
        float2 f = reinterpret_cast<float2*>(dst)[p];
        f.x -= (ky * k[2 * p]) * v, f.y -= (ky * k[2 * p + 1]) * v;
        reinterpret_cast<float2*>(dst)[p] = f;
      }
    } else {
#pragma unroll
      for (int tj = 0; tj < NT; ++tj) dst[tj] -= (ky * k[tj]) * v;
    }
  }
}

// ---------------------------------------------------------------------------- host
double cons_cubic1(double x) { return ((1.25 * x - 2.25) * x) * x + 1.0; }                     // |x| <= 1, A = -0.75
double cons_cubic2(double x) { return ((-0.75 * x + 3.75) * x - 6.0) * x + 3.0; }               // 1 < |x| < 2

bool cons_mode_ok(int m) { return m == SRMI_INTERP_BILINEAR || m == SRMI_INTERP_BICUBIC; }

// even scale; bicubic D needs s >= 4 for its taps to stay inside the block
bool cons_scale_ok(int s, int dmode) { return s >= (dmode == SRMI_INTERP_BICUBIC ? 4 : 2) && s % 2 == 0 && s <= 64; }

int cons_shape(int C, int h, int w, int s, int* gy) {
  if (C < 1 || h < 1 || w < 1) return SRMI_ERR_SHAPE;
  // one plane is indexed in 32 bits: (h s) (w s) < 2^31
  if ((long long)h * s * w * s >= (1ll << 31)) return SRMI_ERR_SHAPE;
  *gy = C < kConsMaxGridY ? C : kConsMaxGridY;
  return 0;
}

// LDS of the adjoint gather at a band of tb LR rows and a strip of tx LR columns: the two
// axis tables and the x-reduced rows.  14.3 KB at tb = 8, tx = 48, s = 4.
constexpr size_t kConsGatherLds = 48 * 1024;
size_t cons_gather_lds(int tb, int tx, int s) {
  const size_t rows = (size_t)(tb + 4) * s, cols = (size_t)(tx + 4) * s;
  return sizeof(float) * (5 * cols + 5 * rows + rows * tx);
}

// D U along one axis, in double from ATen's weights: g[o + 2] = sum over the taps j of D
// (HR phase p_j inside the block) of k_j * (U's weight of LR offset o at phase p_j)
void cons_stencil(int s, int umode, int dmode, ConsStencil* st) {
  double g[5] = {0, 0, 0, 0, 0};
  const int nd = dmode == SRMI_INTERP_BICUBIC ? 4 : 2;
  for (int j = 0; j < nd; ++j) {
    double kj;
    if (nd == 4) {
      kj = (j == 1 || j == 2) ? cons_cubic1(0.5) : cons_cubic2(1.5);
    } else {
      kj = 0.5;
    }
    const int p = s / 2 - nd / 2 + j;
    const double src = (p + 0.5) / s - 0.5;
    const int i0 = (int)floor(src);  // -1 or 0, relative to the block's own LR cell
    const double t = src - i0;
    if (umode == SRMI_INTERP_BICUBIC) {
      const double c[4] = {cons_cubic2(t + 1.0), cons_cubic1(t), cons_cubic1(1.0 - t), cons_cubic2(2.0 - t)};
      for (int q = 0; q < 4; ++q) g[i0 - 1 + q + 2] += kj * c[q];
    } else {
      g[i0 + 2] += kj * (1.0 - t);
      g[i0 + 1 + 2] += kj * t;
    }
  }
  for (int q = 0; q < 5; ++q) st->gy[q] = (float)g[q];
  st->radius = umode == SRMI_INTERP_BICUBIC ? 2 : 1;
}

}  // namespace
}  // namespace srmi

using namespace srmi;

extern "C" {

int srmi_consistency_residual(const float* hr, const float* lr, int C, int h, int w, int scale, int dmode, float* r0,
                              int* active, void* stream) {
  if (!hr || !lr || !r0 || !active || !cons_mode_ok(dmode)) return SRMI_ERR_ARG;
  if (!cons_scale_ok(scale, dmode)) return SRMI_ERR_SHAPE;
  int gy;
  const int rc = cons_shape(C, h, w, scale, &gy);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((h * w + kConsThreads - 1) / kConsThreads, gy), block(kConsThreads);
  const bool vec = ((uintptr_t)hr & 15) == 0;
  const bool cubic = dmode == SRMI_INTERP_BICUBIC;
#define SRMI_CONS_RES(SS, NT) \
  hipLaunchKernelGGL((consistency_residual_kernel<SS, NT>), grid, block, 0, st, hr, lr, C, h, w, scale, r0, active)
  if (vec && scale == 4) {
    if (cubic) SRMI_CONS_RES(4, 4); else SRMI_CONS_RES(4, 2);
  } else if (vec && scale == 8) {
    if (cubic) SRMI_CONS_RES(8, 4); else SRMI_CONS_RES(8, 2);
  } else {
    if (cubic) SRMI_CONS_RES(0, 4); else SRMI_CONS_RES(0, 2);
  }
#undef SRMI_CONS_RES
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_consistency_iterate(const float* r, const int* active, int C, int h, int w, int scale, int umode, int dmode,
                             int first, float* R, float* r_out, void* stream) {
  if (!r || !active || !R || !r_out || r == r_out || r == R || R == r_out || !cons_mode_ok(umode) ||
      !cons_mode_ok(dmode))
    return SRMI_ERR_ARG;
  if (!cons_scale_ok(scale, dmode)) return SRMI_ERR_SHAPE;
  int gy;
  const int rc = cons_shape(C, h, w, scale, &gy);
  if (rc) return rc;
  ConsStencil stc;
  cons_stencil(scale, umode, dmode, &stc);
  hipLaunchKernelGGL(consistency_iterate_kernel, dim3((h * w + kConsThreads - 1) / kConsThreads, gy),
                     dim3(kConsThreads), 0, static_cast<hipStream_t>(stream), r, active, C, h, w, stc, first ? 1 : 0, R,
                     r_out);
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_consistency_apply(const float* R, int C, int h, int w, int scale, int umode, float* hr, void* stream) {
  if (!R || !hr || !cons_mode_ok(umode)) return SRMI_ERR_ARG;
  if (!cons_scale_ok(scale, SRMI_INTERP_BILINEAR)) return SRMI_ERR_SHAPE;
  int gy;
  const int rc = cons_shape(C, h, w, scale, &gy);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((h * scale * w + kConsThreads - 1) / kConsThreads, gy), block(kConsThreads);
  if (scale % 4 == 0 && ((uintptr_t)hr & 15) == 0)
    hipLaunchKernelGGL(consistency_apply_kernel<true>, grid, block, 0, st, R, C, h, w, scale, umode, hr);
  else
    hipLaunchKernelGGL(consistency_apply_kernel<false>, grid, block, 0, st, R, C, h, w, scale, umode, hr);
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_consistency_adjoint_gather(const float* g, int C, int h, int w, int scale, int umode, float* q,
                                    void* stream) {
  if (!g || !q || !cons_mode_ok(umode)) return SRMI_ERR_ARG;
  if (!cons_scale_ok(scale, SRMI_INTERP_BILINEAR)) return SRMI_ERR_SHAPE;
  int gy;
  const int rc = cons_shape(C, h, w, scale, &gy);
  if (rc) return rc;
  // the band / strip: the largest that fits kConsGatherLds, columns first (a strip of 8
  // columns and a band of one row need 31.6 KB at scale 64, so one always fits); then
  // smaller bands while the grid would leave most of the chip idle
  int TB = 1, TX = w < 8 ? w : 8;
  bool found = false;
  const int txs[4] = {64, 32, 16, 8}, tbs[4] = {8, 4, 2, 1};
  for (int b = 0; b < 4 && !found; ++b)
    for (int a = 0; a < 4 && !found; ++a) {
      const int tb = tbs[b] < h ? tbs[b] : h, tx = txs[a] < w ? txs[a] : w;
      if (cons_gather_lds(tb, tx, scale) <= kConsGatherLds) TB = tb, TX = tx, found = true;
    }
  const int nstrips = (w + TX - 1) / TX;
  while (TB > 1 && (long long)gy * ((h + TB - 1) / TB) * nstrips < 256) TB = (TB + 1) / 2;
  const dim3 grid(((h + TB - 1) / TB) * nstrips, gy), block(kConsThreads);
  const size_t lds = cons_gather_lds(TB, TX, scale);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (scale % 4 == 0 && ((uintptr_t)g & 15) == 0)
    hipLaunchKernelGGL(consistency_adjoint_gather_kernel<true>, grid, block, lds, st, g, C, h, w, scale, umode, TB, TX,
                       nstrips, q);
  else
    hipLaunchKernelGGL(consistency_adjoint_gather_kernel<false>, grid, block, lds, st, g, C, h, w, scale, umode, TB,
                       TX, nstrips, q);
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_consistency_adjoint_iterate(const float* t, const int* active, int C, int h, int w, int scale, int umode,
                                     int dmode, int first, float* Q, float* t_out, void* stream) {
  if (!t || !active || !Q || !t_out || t == t_out || t == Q || Q == t_out || !cons_mode_ok(umode) ||
      !cons_mode_ok(dmode))
    return SRMI_ERR_ARG;
  if (!cons_scale_ok(scale, dmode)) return SRMI_ERR_SHAPE;
  int gy;
  const int rc = cons_shape(C, h, w, scale, &gy);
  if (rc) return rc;
  ConsStencil stc;
  cons_stencil(scale, umode, dmode, &stc);
  hipLaunchKernelGGL(consistency_adjoint_iterate_kernel, dim3((h * w + kConsThreads - 1) / kConsThreads, gy),
                     dim3(kConsThreads), 0, static_cast<hipStream_t>(stream), t, active, C, h, w, stc, first ? 1 : 0,
                     Q, t_out);
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_consistency_adjoint_apply(const float* Q, const int* active, int C, int h, int w, int scale, int dmode,
                                   float* g, void* stream) {
  if (!Q || !active || !g || !cons_mode_ok(dmode)) return SRMI_ERR_ARG;
  if (!cons_scale_ok(scale, dmode)) return SRMI_ERR_SHAPE;
  int gy;
  const int rc = cons_shape(C, h, w, scale, &gy);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool cubic = dmode == SRMI_INTERP_BICUBIC;
  const long long cells = (long long)h * (cubic ? 4 : 2) * w;  // < 2^31: at most the plane's pixels
  const dim3 grid((unsigned)((cells + kConsThreads - 1) / kConsThreads), gy), block(kConsThreads);
  const bool vec = scale % 4 == 0 && ((uintptr_t)g & 15) == 0;
#define SRMI_CONS_ADJ(VV, NT) \
  hipLaunchKernelGGL((consistency_adjoint_apply_kernel<VV, NT>), grid, block, 0, st, Q, active, C, h, w, scale, g)
  if (vec) {
    if (cubic) SRMI_CONS_ADJ(true, 4); else SRMI_CONS_ADJ(true, 2);
  } else {
    if (cubic) SRMI_CONS_ADJ(false, 4); else SRMI_CONS_ADJ(false, 2);
  }
#undef SRMI_CONS_ADJ
  SRMI_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
