// Gradient loss term of the training step: the mean Charbonnier magnitude of the Sobel
// gradient of e = pred - target, [nplanes][H][W] fp32, and its gradient with respect to pred
// -- no reference counterpart.  srmi.h states the definition ("the gradient loss term");
// gradient_common.hpp holds the operator, which is the gradient score's.
//
// Per plane the workspace holds only
//   psum   [tiles] fp64    sum of phi over the used positions of a pixel tile
//   pcnt   [tiles] int32   their number
// one plane after the other (gradient_loss_plan's stride), so a call over a range of planes
// works on its own part of the workspace and gives the bits the whole batch gives.
//
// Launches, no atomics, no host read:
//   gradient_loss_tile_kernel   one workgroup per kGradTileH x kGradTileW rectangle of pixels:
//       stages e with a one-pixel halo in LDS (NaN where a pixel is not finite in both fields
//       or outside the plane), forms a, b and phi at its pixels and writes its sum and count
//       (fp64 / integer, a fixed tree).
//   gradient_loss_plane_kernel  one workgroup per plane: the tile sums in a fixed order,
//       rounded once into parts, the count into cparts (loss_term.hpp's term_plane_reduce).
//   gradient_loss_finalize_kernel  parts and cparts over the planes of the global batch
//       (loss_term.hpp's term_finalize): grad4 and total.
//   gradient_loss_dy_kernel     one workgroup per rectangle of pixels: stages e with a
//       two-pixel halo, forms U = a / phi and V = b / phi on the one-pixel halo (0 where the
//       position is not used) in LDS and gathers Gx^T U + Gy^T V = -(Gx[U] + Gy[V]), the
//       operator applied to the zero-extended maps, into dy: one writer per pixel.  U and V
//       are recomputed here, not stored by the tile kernel: 6 plane-sized transfers over the
//       two launches instead of 8.
//
// Full rows go through 16-byte loads and stores when W % 4 == 0 and the buffers are 16-byte
// aligned (the Vec forms), otherwise through the scalar forms; the results are the same bits.
// LDS: the tile kernel 18 x 72 floats + the tree, 8.1 KiB; the dy kernel 20 x 72 + 2 x 18 x 72
// floats, 15.8 KiB.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cmath>

#include "common.hpp"
#include "gradient_common.hpp"
#include "loss_term.hpp"
#include "srmi_internal.hpp"

namespace srmi {

namespace {

constexpr int kRows1 = kGradTileH + 2;  // staged rows of a one-pixel halo
constexpr int kRows2 = kGradTileH + 4;  // of a two-pixel halo

struct GradLossPlan {
  int tiles_x, tiles_per_plane;
  size_t off_pcnt, stride;  // bytes within a plane's part of the workspace
};

// SRMI_ERR_ARG for a plan outside the definition
int gradient_loss_plan(long long nplanes, int H, int W, GradLossPlan* p) {
  if (nplanes < 1 || H < 3 || W < 3 || (long long)H * W > (1LL << 24)) return SRMI_ERR_ARG;
  p->tiles_x = (W + kGradTileW - 1) / kGradTileW;
  p->tiles_per_plane = p->tiles_x * ((H + kGradTileH - 1) / kGradTileH);
  if (nplanes * p->tiles_per_plane >= (1LL << 31)) return SRMI_ERR_ARG;
  auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
  p->off_pcnt = up((size_t)p->tiles_per_plane * sizeof(double));
  p->stride = p->off_pcnt + up((size_t)p->tiles_per_plane * sizeof(int));
  return 0;
}

// e = pred - target of four neighbouring pixels, NaN where one is not finite in both
__device__ inline void stage_error(float* __restrict__ se, int o, const float* va, const float* vb) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bool bad = grad_nonfinite(va[i]) || grad_nonfinite(vb[i]);
    se[o + i] = bad ? grad_nan() : va[i] - vb[i];
  }
}

// a, b and phi of window i (columns i .. i + 2) of three staged rows; false: not used
__device__ inline bool window_phi(const GradRow6* e, int i, float eps, float* a, float* b, float* phi) {
  bool bad = false;
#pragma unroll
  for (int r = 0; r < 3; ++r) bad = bad || grad_nonfinite(e[r].v[i]) || grad_nonfinite(e[r].v[i + 1]) ||
                                    grad_nonfinite(e[r].v[i + 2]);
  *a = grad_sobel_x(e[0].v[i], e[0].v[i + 2], e[1].v[i], e[1].v[i + 2], e[2].v[i], e[2].v[i + 2]);
  *b = grad_sobel_y(e[0].v[i], e[0].v[i + 1], e[0].v[i + 2], e[2].v[i], e[2].v[i + 1], e[2].v[i + 2]);
  // products and sums rounded one by one: the sequence srmi.h states
  *phi = sqrtf(grad_mag2_eps(*a, *b, eps));
  return !bad;
}

template <bool Vec>
__global__ void __launch_bounds__(kGradThreads) gradient_loss_tile_kernel(const float* __restrict__ pred,
                                                                          const float* __restrict__ target, int H,
                                                                          int W, float eps, GradLossPlan plan,
                                                                          char* __restrict__ ws) {
  __shared__ __align__(16) float se[kRows1 * kGradPitch];
  __shared__ double red[kGradThreads];
  __shared__ int redc[kGradThreads];
  const int tid = threadIdx.x;
  const int plane = blockIdx.x / plan.tiles_per_plane, t = blockIdx.x % plan.tiles_per_plane;
  const int y0 = (t / plan.tiles_x) * kGradTileH, x0 = (t % plan.tiles_x) * kGradTileW;
  const size_t pbase = (size_t)plane * (size_t)H * (size_t)W;
  grad_stage<Vec, kRows1>(pred + pbase, target + pbase, H, W, y0 - 1, x0 - kGradPadL, tid,
                          [&](int o, const float* va, const float* vb) { stage_error(se, o, va, vb); });
  __syncthreads();

  // ---- four neighbouring pixels of one row per thread; staged row ly is pixel row y - 1.  A
  // window without a staged NaN lies in the plane: the position is a valid one
  const int g = tid % kGradLanesX, ly = tid / kGradLanesX, o = 4 * g + kGradPadL;
  GradRow6 e[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) e[r] = grad_row6(se + (ly + r) * kGradPitch, o);
  double s = 0.0;
  int n = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float a, b, phi;
    if (window_phi(e, i, eps, &a, &b, &phi)) {
      s += (double)phi;
      ++n;
    }
  }
  term_tree(s, n, red, redc, tid);
  if (tid == 0) {
    char* pws = ws + (size_t)plane * plan.stride;
    reinterpret_cast<double*>(pws)[t] = red[0];
    reinterpret_cast<int*>(pws + plan.off_pcnt)[t] = redc[0];
  }
}

__global__ void __launch_bounds__(kGradThreads) gradient_loss_plane_kernel(const char* __restrict__ ws,
                                                                           GradLossPlan plan,
                                                                           float* __restrict__ parts,
                                                                           float* __restrict__ cparts) {
  const char* pws = ws + (size_t)blockIdx.x * plan.stride;
  term_plane_reduce(reinterpret_cast<const double*>(pws), reinterpret_cast<const int*>(pws + plan.off_pcnt),
                    plan.tiles_per_plane, blockIdx.x, parts, cparts);
}

__global__ void __launch_bounds__(kGradThreads) gradient_loss_finalize_kernel(const float* __restrict__ parts,
                                                                              const float* __restrict__ cparts,
                                                                              long long nplanes, float weight,
                                                                              const float* base, float* grad4,
                                                                              float* total) {
  term_finalize<false>(parts, cparts, nplanes, 1.0, weight, base, grad4, total);  // L_grad = S / Nused
}

template <bool Vec>
__global__ void __launch_bounds__(kGradThreads) gradient_loss_dy_kernel(const float* __restrict__ pred,
                                                                        const float* __restrict__ target, int H,
                                                                        int W, float eps, float weight,
                                                                        GradLossPlan plan,
                                                                        const float* __restrict__ grad4,
                                                                        float* __restrict__ dy) {
  __shared__ __align__(16) float se[kRows2 * kGradPitch];  // e, rows y0 - 2 .. y0 + 17
  __shared__ __align__(16) float sU[kRows1 * kGradPitch];  // U, V at the positions y0 - 1 .. y0 + 16
  __shared__ __align__(16) float sV[kRows1 * kGradPitch];
  const int tid = threadIdx.x;
  const int plane = blockIdx.x / plan.tiles_per_plane, t = blockIdx.x % plan.tiles_per_plane;
  const int y0 = (t / plan.tiles_x) * kGradTileH, x0 = (t % plan.tiles_x) * kGradTileW;
  const size_t pbase = (size_t)plane * (size_t)H * (size_t)W;
  const float scale = weight * grad4[2];
  grad_stage<Vec, kRows2>(pred + pbase, target + pbase, H, W, y0 - 2, x0 - kGradPadL, tid,
                          [&](int o, const float* va, const float* vb) { stage_error(se, o, va, vb); });
  __syncthreads();

  // ---- U and V of every staged column of the 18 position rows, a quad at a time: position
  // row r reads staged rows r .. r + 2.  The outermost columns have no left / right neighbour
  // staged and come out 0; the gather below never reads them.
  for (int it = tid; it < kRows1 * kGradQuads; it += kGradThreads) {
    const int r = it / kGradQuads, q = it - r * kGradQuads;
    GradRow6 e[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) e[k] = grad_row6_edge(se + (r + k) * kGradPitch, q);
    float u[4], v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float a, b, phi;
      const bool used = window_phi(e, i, eps, &a, &b, &phi);
      u[i] = used ? a / phi : 0.0f;
      v[i] = used ? b / phi : 0.0f;
    }
    *reinterpret_cast<float4*>(sU + r * kGradPitch + 4 * q) = make_float4(u[0], u[1], u[2], u[3]);
    *reinterpret_cast<float4*>(sV + r * kGradPitch + 4 * q) = make_float4(v[0], v[1], v[2], v[3]);
  }
  __syncthreads();

  // ---- gather: pixel row y0 + ly is position row ly + 1 of sU / sV and staged row ly + 2 of se
  const int g = tid % kGradLanesX, ly = tid / kGradLanesX;
  const int y = y0 + ly, x = x0 + 4 * g, o = 4 * g + kGradPadL;
  if (y >= H || x >= W) return;
  GradRow6 U[3], V[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    U[k] = grad_row6(sU + (ly + k) * kGradPitch, o);
    V[k] = grad_row6(sV + (ly + k) * kGradPitch, o);
  }
  float ds[4];
  bool fin[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float gxu = grad_sobel_x(U[0].v[i], U[0].v[i + 2], U[1].v[i], U[1].v[i + 2], U[2].v[i], U[2].v[i + 2]);
    const float gyv = grad_sobel_y(V[0].v[i], V[0].v[i + 1], V[0].v[i + 2], V[2].v[i], V[2].v[i + 1], V[2].v[i + 2]);
    ds[i] = -__fadd_rn(gxu, gyv);
    fin[i] = !grad_nonfinite(se[(ly + 2) * kGradPitch + o + i]);  // NaN also right of the plane
  }
  float* row = dy + pbase + (size_t)y * W;
  if (Vec && fin[0] && fin[1] && fin[2] && fin[3]) {
    float4 d = *reinterpret_cast<const float4*>(row + x);
    d.x = __fmaf_rn(scale, ds[0], d.x);  // one rounding
    d.y = __fmaf_rn(scale, ds[1], d.y);
    d.z = __fmaf_rn(scale, ds[2], d.z);
    d.w = __fmaf_rn(scale, ds[3], d.w);
    *reinterpret_cast<float4*>(row + x) = d;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (fin[i]) row[x + i] = __fmaf_rn(scale, ds[i], row[x + i]);
    }
  }
}

bool bad_weight(float w) { return !(w >= 0.0f) || !std::isfinite(w); }
bool bad_eps(float e) { return !(e > 0.0f) || !std::isfinite(e); }

}  // namespace
}  // namespace srmi

using namespace srmi;

extern "C" {

int srmi_gradient_loss_workspace(long long nplanes, int H, int W, size_t* bytes) {
  GradLossPlan p;
  if (!bytes) return SRMI_ERR_ARG;
  const int rc = gradient_loss_plan(nplanes, H, W, &p);
  if (rc) return rc;
  *bytes = (size_t)nplanes * p.stride;
  return 0;
}

int srmi_gradient_loss_parts(const float* pred, const float* target, long long nplanes, int H, int W, float eps,
                             float* parts, float* cparts, void* workspace, size_t workspace_bytes, void* stream) {
  GradLossPlan p;
  if (!pred || !target || !parts || !cparts || !workspace || !grad_aligned16(workspace) || bad_eps(eps))
    return SRMI_ERR_ARG;
  const int rc = gradient_loss_plan(nplanes, H, W, &p);
  if (rc) return rc;
  if (workspace_bytes < (size_t)nplanes * p.stride) return SRMI_ERR_ARG;
  char* w = static_cast<char*>(workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool vec = W % 4 == 0 && grad_aligned16(pred) && grad_aligned16(target);
  const dim3 grid((unsigned)(nplanes * p.tiles_per_plane)), block(kGradThreads);
  if (vec)
    hipLaunchKernelGGL(gradient_loss_tile_kernel<true>, grid, block, 0, st, pred, target, H, W, eps, p, w);
  else
    hipLaunchKernelGGL(gradient_loss_tile_kernel<false>, grid, block, 0, st, pred, target, H, W, eps, p, w);
  SRMI_CHECK_LAUNCH();
  hipLaunchKernelGGL(gradient_loss_plane_kernel, dim3((unsigned)nplanes), block, 0, st, w, p, parts, cparts);
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_gradient_loss_from_parts(const float* parts, const float* cparts, long long nplanes, float weight,
                                  const float* base, float* grad4, float* total, void* stream) {
  if (!parts || !cparts || !base || !grad4 || !total || nplanes < 1 || bad_weight(weight)) return SRMI_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(gradient_loss_finalize_kernel, dim3(1), dim3(kGradThreads), 0, st, parts, cparts, nplanes,
                     weight, base, grad4, total);
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_gradient_loss_dy(const float* pred, const float* target, long long nplanes, int H, int W, float eps,
                          float weight, const float* grad4, float* dy, void* stream) {
  GradLossPlan p;
  if (!pred || !target || !grad4 || !dy || bad_eps(eps) || bad_weight(weight)) return SRMI_ERR_ARG;
  const int rc = gradient_loss_plan(nplanes, H, W, &p);
  if (rc) return rc;
  if (weight == 0.0f) return 0;  // dy stays as it is, bit for bit
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool vec = W % 4 == 0 && grad_aligned16(pred) && grad_aligned16(target) && grad_aligned16(dy);
  const dim3 grid((unsigned)(nplanes * p.tiles_per_plane)), block(kGradThreads);
  if (vec)
    hipLaunchKernelGGL(gradient_loss_dy_kernel<true>, grid, block, 0, st, pred, target, H, W, eps, weight, p, grad4,
                       dy);
  else
    hipLaunchKernelGGL(gradient_loss_dy_kernel<false>, grid, block, 0, st, pred, target, H, W, eps, weight, p, grad4,
                       dy);
  SRMI_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
