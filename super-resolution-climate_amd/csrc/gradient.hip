// Gradient score of a super-resolved field: the Sobel gradients of a prediction and a truth,
// [C][H][W] fp32, their mean magnitudes, the sharpness ratio, the RMSE of the magnitudes and of
// the vector difference, the cosine between the two gradient fields, and optionally the two
// magnitude maps -- no reference counterpart.  srmi.h states the definition ("the gradient
// score"); gradient_common.hpp holds the operator.
//
// Launches, no atomics, no host read:
//   gradient_tile_kernel   one workgroup per kGradTileH x kGradTileW rectangle of pixels.  It
//       stages the rectangle with a one-pixel halo of both fields in LDS (a pixel that is not
//       finite in both, or outside the plane, as NaN in both), forms gx, gy and the magnitudes
//       at its pixels, writes the maps (NaN where the position is not used, the border
//       included) and its seven sums and its count in fp64 (a fixed tree) into the workspace.
//   gradient_plane_kernel  one workgroup per channel: the tile sums in a fixed order (256
//       contiguous shares in tile order, then a fixed tree) and the derived values.
//
// LDS of the tile kernel: 2 x 18 x 72 floats staged + 8 x 256 doubles = 26.1 KiB.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cmath>

#include "common.hpp"
#include "gradient_common.hpp"
#include "srmi_internal.hpp"

namespace srmi {

namespace {

constexpr int kGradSums = 7;               // the fp64 sums of srmi_gradient, in its order
constexpr int kGradSlots = kGradSums + 1;  // and the count, a whole number below 2^53
constexpr int kGradRows = kGradTileH + 2;  // staged rows y0 - 1 .. y0 + 16

struct GradPlan {
  int tiles_x, tiles_per_plane;
  size_t stride;  // bytes of a channel's part of the workspace
};

int gradient_plan(int C, int H, int W, GradPlan* p) {
  if (C < 1 || H < 3 || W < 3 || (long long)H * W >= (1LL << 31)) return SRMI_ERR_ARG;
  p->tiles_x = (W + kGradTileW - 1) / kGradTileW;
  p->tiles_per_plane = p->tiles_x * ((H + kGradTileH - 1) / kGradTileH);
  if ((long long)C * p->tiles_per_plane >= (1LL << 31)) return SRMI_ERR_ARG;
  p->stride = (size_t)p->tiles_per_plane * kGradSlots * sizeof(double);
  return 0;
}

template <bool Vec>
__global__ void __launch_bounds__(kGradThreads) gradient_tile_kernel(const float* __restrict__ pred,
                                                                     const float* __restrict__ truth, int H, int W,
                                                                     float inv_dy, float inv_dx, GradPlan plan,
                                                                     char* __restrict__ ws, float* __restrict__ gp,
                                                                     float* __restrict__ gt) {
  __shared__ __align__(16) float sa[kGradRows * kGradPitch];
  __shared__ __align__(16) float sb[kGradRows * kGradPitch];
  __shared__ double red[kGradSlots][kGradThreads];
  const int tid = threadIdx.x;
  const int plane = blockIdx.x / plan.tiles_per_plane, t = blockIdx.x % plan.tiles_per_plane;
  const int y0 = (t / plan.tiles_x) * kGradTileH, x0 = (t % plan.tiles_x) * kGradTileW;
  const size_t pbase = (size_t)plane * (size_t)H * (size_t)W;

  grad_stage<Vec, kGradRows>(pred + pbase, truth + pbase, H, W, y0 - 1, x0 - kGradPadL, tid,
                             [&](int o, const float* va, const float* vb) {
#pragma unroll
                               for (int i = 0; i < 4; ++i) {
                                 const bool bad = grad_nonfinite(va[i]) || grad_nonfinite(vb[i]);
                                 sa[o + i] = bad ? grad_nan() : va[i];
                                 sb[o + i] = bad ? grad_nan() : vb[i];
                               }
                             });
  __syncthreads();

  // ---- four neighbouring pixels of one row per thread; staged row ly is pixel row y - 1
  const int g = tid % kGradLanesX, ly = tid / kGradLanesX;
  const int y = y0 + ly, x = x0 + 4 * g, o = 4 * g + kGradPadL;
  GradRow6 a[3], b[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    a[r] = grad_row6(sa + (ly + r) * kGradPitch, o);
    b[r] = grad_row6(sb + (ly + r) * kGradPitch, o);
  }
  double s[kGradSums];
#pragma unroll
  for (int k = 0; k < kGradSums; ++k) s[k] = 0.0;
  int n = 0;
  float mp[4], mt[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    // staged NaN stands for "not finite in both fields" and for "outside the plane": a window
    // without one lies in the plane, so the position is a valid one
    bool bad = false;
#pragma unroll
    for (int r = 0; r < 3; ++r) bad = bad || grad_nonfinite(a[r].v[i]) || grad_nonfinite(a[r].v[i + 1]) ||
                                      grad_nonfinite(a[r].v[i + 2]);
    const float pgx = grad_sobel_x(a[0].v[i], a[0].v[i + 2], a[1].v[i], a[1].v[i + 2], a[2].v[i], a[2].v[i + 2]) * inv_dx;
    const float pgy = grad_sobel_y(a[0].v[i], a[0].v[i + 1], a[0].v[i + 2], a[2].v[i], a[2].v[i + 1], a[2].v[i + 2]) * inv_dy;
    const float tgx = grad_sobel_x(b[0].v[i], b[0].v[i + 2], b[1].v[i], b[1].v[i + 2], b[2].v[i], b[2].v[i + 2]) * inv_dx;
    const float tgy = grad_sobel_y(b[0].v[i], b[0].v[i + 1], b[0].v[i + 2], b[2].v[i], b[2].v[i + 1], b[2].v[i + 2]) * inv_dy;
    // products and sums rounded one by one: the sequence srmi.h states
    const float p2 = grad_mag2(pgx, pgy);
    const float t2 = grad_mag2(tgx, tgy);
    const float pm = sqrtf(p2), tm = sqrtf(t2);
    mp[i] = bad ? grad_nan() : pm;
    mt[i] = bad ? grad_nan() : tm;
    if (!bad) {
      const double dm = (double)pm - (double)tm;
      const double ex = (double)pgx - (double)tgx, ey = (double)pgy - (double)tgy;
      s[0] += (double)pm;
      s[1] += (double)tm;
      s[2] += dm * dm;
      s[3] += ex * ex + ey * ey;
      s[4] += (double)pgx * (double)tgx + (double)pgy * (double)tgy;
      s[5] += (double)p2;
      s[6] += (double)t2;
      ++n;
    }
  }
  if (y < H) {
    const size_t row = pbase + (size_t)y * W;
    if (Vec) {
      if (x < W) {
        if (gp) *reinterpret_cast<float4*>(gp + row + x) = make_float4(mp[0], mp[1], mp[2], mp[3]);
        if (gt) *reinterpret_cast<float4*>(gt + row + x) = make_float4(mt[0], mt[1], mt[2], mt[3]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (x + i < W) {
          if (gp) gp[row + x + i] = mp[i];
          if (gt) gt[row + x + i] = mt[i];
        }
      }
    }
  }

  // ---- the workgroup's sums and count, a fixed tree
#pragma unroll
  for (int k = 0; k < kGradSums; ++k) red[k][tid] = s[k];
  red[kGradSums][tid] = (double)n;
  __syncthreads();
  for (int w = kGradThreads / 2; w > 0; w >>= 1) {
    if (tid < w) {
#pragma unroll
      for (int k = 0; k < kGradSlots; ++k) red[k][tid] += red[k][tid + w];
    }
    __syncthreads();
  }
  if (tid < kGradSlots) {
    double* tile = reinterpret_cast<double*>(ws + (size_t)plane * plan.stride) + (size_t)t * kGradSlots;
    tile[tid] = red[tid][0];
  }
}

__global__ void __launch_bounds__(kGradThreads) gradient_plane_kernel(const char* __restrict__ ws, GradPlan plan,
                                                                      long long* __restrict__ count,
                                                                      double* __restrict__ sums,
                                                                      double* __restrict__ stats) {
  __shared__ double red[kGradSlots][kGradThreads];
  const int plane = blockIdx.x, tid = threadIdx.x;
  const double* tiles = reinterpret_cast<const double*>(ws + (size_t)plane * plan.stride);
  const int nt = plan.tiles_per_plane;
  const int share = (nt + kGradThreads - 1) / kGradThreads;
  const int t0 = min(tid * share, nt), t1 = min(t0 + share, nt);
  double s[kGradSlots];
#pragma unroll
  for (int k = 0; k < kGradSlots; ++k) s[k] = 0.0;
  for (int t = t0; t < t1; ++t) {
#pragma unroll
    for (int k = 0; k < kGradSlots; ++k) s[k] += tiles[(size_t)t * kGradSlots + k];
  }
#pragma unroll
  for (int k = 0; k < kGradSlots; ++k) red[k][tid] = s[k];
  __syncthreads();
  for (int w = kGradThreads / 2; w > 0; w >>= 1) {
    if (tid < w) {
#pragma unroll
      for (int k = 0; k < kGradSlots; ++k) red[k][tid] += red[k][tid + w];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  const double n = red[kGradSums][0];
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  count[plane] = (long long)n;
  double* su = sums + (size_t)plane * kGradSums;
  double* st = stats + (size_t)plane * 6;
  if (!(n > 0.0)) {  // no used position: NaN in every fp64 value
    for (int k = 0; k < kGradSums; ++k) su[k] = nan;
    for (int k = 0; k < 6; ++k) st[k] = nan;
    return;
  }
  for (int k = 0; k < kGradSums; ++k) su[k] = red[k][0];
  const double mean_p = red[0][0] / n, mean_t = red[1][0] / n;
  st[0] = mean_p;
  st[1] = mean_t;
  st[2] = mean_p / mean_t;
  st[3] = sqrt(red[2][0] / n);
  st[4] = sqrt(red[3][0] / n);
  st[5] = red[4][0] / sqrt(red[5][0] * red[6][0]);
}

bool bad_factor(float v) { return !std::isfinite(v) || !(v > 0.0f); }

}  // namespace
}  // namespace srmi

using namespace srmi;

extern "C" {

int srmi_gradient_workspace(int C, int H, int W, size_t* bytes) {
  GradPlan p;
  if (!bytes) return SRMI_ERR_ARG;
  const int rc = gradient_plan(C, H, W, &p);
  if (rc) return rc;
  *bytes = (size_t)C * p.stride;
  return 0;
}

int srmi_gradient(const float* pred, const float* truth, int C, int H, int W, float inv_dy, float inv_dx,
                  void* workspace, size_t workspace_bytes, long long* count, double* sums, double* stats,
                  float* gmag_pred, float* gmag_truth, void* stream) {
  GradPlan p;
  if (!pred || !truth || !workspace || !grad_aligned16(workspace) || !count || !sums || !stats || bad_factor(inv_dy) ||
      bad_factor(inv_dx))
    return SRMI_ERR_ARG;
  const int rc = gradient_plan(C, H, W, &p);
  if (rc) return rc;
  if (workspace_bytes < (size_t)C * p.stride) return SRMI_ERR_ARG;
  char* w = static_cast<char*>(workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool vec = W % 4 == 0 && grad_aligned16(pred) && grad_aligned16(truth) && grad_aligned16(gmag_pred) &&
                   grad_aligned16(gmag_truth);
  const dim3 grid((unsigned)(C * p.tiles_per_plane)), block(kGradThreads);
  if (vec)
    hipLaunchKernelGGL(gradient_tile_kernel<true>, grid, block, 0, st, pred, truth, H, W, inv_dy, inv_dx, p, w,
                       gmag_pred, gmag_truth);
  else
    hipLaunchKernelGGL(gradient_tile_kernel<false>, grid, block, 0, st, pred, truth, H, W, inv_dy, inv_dx, p, w,
                       gmag_pred, gmag_truth);
  SRMI_CHECK_LAUNCH();
  hipLaunchKernelGGL(gradient_plane_kernel, dim3((unsigned)C), block, 0, st, w, p, count, sums, stats);
  SRMI_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
