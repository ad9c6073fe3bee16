// SSIM loss term of the training step: 1 - the mean Gaussian-window structural similarity
// of a prediction a against a target b, [nplanes][H][W] fp32, and its gradient with respect
// to a -- no reference counterpart.  srmi.h states the definition ("the SSIM loss term");
// this file is its device form.  The forward is the SSIM score's (ssim.hip): the same taps,
// pivot, mask rule and arithmetic, tiled over the VALID positions instead of the pixels.
//
// A position p = (py, px), py < Hv = H - 10, px < Wv = W - 10, is the window of the pixels
// py .. py + 10, px .. px + 10.  Per plane the workspace holds
//   head   4 floats             {r, L, 0, 0}: the pivot the gradient needs, and the range
//   mm     [nblk][2] fp32       min / max of the target, one pair per workgroup of the range pass
//   psum   [tiles] fp64         sum of ssim over the used positions of a position tile
//   pcnt   [tiles] int32        their number
//   coef   [3][Hv][Wv] fp32     A, B, C of the closed-form gradient, 0 where a position is not used
// one plane after the other (ssim_loss_plan's stride), so a call over a range of planes works
// on its own part of the workspace and gives the bits the whole batch gives.
//
// Launches, no atomics, no host read:
//   ssim_loss_minmax_kernel  a fixed grid of workgroups per plane strides over b: min / max
//       of the finite pixels (fminf / fmaxf started from NaN), one pair per workgroup.
//   ssim_loss_tile_kernel    one workgroup per kTileH x kTileW rectangle of positions.  It
//       folds the plane's min / max pairs (order-independent: r and L are the same bits in
//       every workgroup), stages the rectangle's 34 x 74 pixels of a - r and b - r in LDS (a
//       pixel that is non-finite in a or b, or outside the plane, as the flag a' = NaN, b' =
//       0), runs the horizontal 11-tap pass for the five moment planes and the flag count into
//       LDS and the vertical pass into registers, evaluates ssim and A, B, C, writes the three
//       coefficients of its positions and its sum and count (fp64 / integer, a fixed tree).
//   ssim_loss_plane_kernel   one workgroup per plane: the tile sums in a fixed order, rounded
//       once into parts, the count into cparts (loss_term.hpp's term_plane_reduce).
//   ssim_loss_finalize_kernel  parts and cparts over the planes of the global batch
//       (loss_term.hpp's term_finalize): ssim4 and total.
//   ssim_loss_dy_kernel      one workgroup per kTileH x kTileW rectangle of PIXELS: stages the
//       34 x 74 positions whose windows reach it (0 outside the map: the full correlation),
//       filters A, B and C with the same separable taps, and adds scale (G^T A + a' G^T B + b'
//       G^T C) to dy: every pixel has one writer and one order.  A pixel that is non-finite in
//       a or b is not written.
//
// LDS: the tile kernel is the score's, 34 x 74 x 2 staged + 6 x 34 x 64 horizontal sums =
// 70.7 KiB, two workgroups per CU; the dy kernel stages 3 x 34 x 74 and keeps 3 x 34 x 64
// sums, 55.0 KiB, two workgroups per CU as well.  Every LDS access of a wave is on 64
// consecutive dwords.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cmath>

#include "common.hpp"
#include "loss_term.hpp"
#include "srmi_internal.hpp"
#include "ssim_common.hpp"

namespace srmi {

namespace {

struct SsimLossPlan {
  int Hv, Wv;                     // the valid positions of a plane
  int tiles_x, tiles_per_plane;   // position tiles (parts)
  int dtiles_x, dtiles_per_plane; // pixel tiles (dy)
  int nblk;                       // range-pass workgroups per plane
  size_t off_mm, off_psum, off_pcnt, off_coef, stride;  // bytes within a plane's part of the workspace
};

// SRMI_ERR_ARG for a plan outside the definition
int ssim_loss_plan(long long nplanes, int H, int W, SsimLossPlan* p) {
  if (nplanes < 1 || H < kSsimTaps || W < kSsimTaps || (long long)H * W > (1LL << 24)) return SRMI_ERR_ARG;
  p->Hv = H - 2 * kSsimR;
  p->Wv = W - 2 * kSsimR;
  p->tiles_x = (p->Wv + kTileW - 1) / kTileW;
  p->tiles_per_plane = p->tiles_x * ((p->Hv + kTileH - 1) / kTileH);
  p->dtiles_x = (W + kTileW - 1) / kTileW;
  p->dtiles_per_plane = p->dtiles_x * ((H + kTileH - 1) / kTileH);
  const long long per = (long long)kSsimThreads * kMmPerThread;
  const long long nb = ((long long)H * W + per - 1) / per;
  p->nblk = (int)(nb < kMmBlocks ? nb : kMmBlocks);
  if (nplanes * p->dtiles_per_plane >= (1LL << 31) || nplanes * p->nblk >= (1LL << 31)) return SRMI_ERR_ARG;
  auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
  p->off_mm = 16;
  p->off_psum = p->off_mm + up((size_t)p->nblk * 2 * sizeof(float));
  p->off_pcnt = p->off_psum + up((size_t)p->tiles_per_plane * sizeof(double));
  p->off_coef = p->off_pcnt + up((size_t)p->tiles_per_plane * sizeof(int));
  p->stride = p->off_coef + up((size_t)3 * p->Hv * p->Wv * sizeof(float));
  return 0;
}

__global__ void __launch_bounds__(kSsimThreads) ssim_loss_minmax_kernel(const float* __restrict__ b, int HW, int nblk,
                                                                        char* __restrict__ ws, SsimLossPlan plan) {
  __shared__ float slo[kSsimThreads], shi[kSsimThreads];
  const int plane = blockIdx.x / nblk, blk = blockIdx.x % nblk, tid = threadIdx.x;
  float* mm = reinterpret_cast<float*>(ws + (size_t)plane * plan.stride + plan.off_mm);
  ssim_minmax_block(b + (size_t)plane * (size_t)HW, HW, blk, nblk, slo, shi, tid);
  if (tid == 0) {
    mm[blk * 2 + 0] = slo[0];
    mm[blk * 2 + 1] = shi[0];
  }
}

// two workgroups per CU is what the LDS admits (2 waves per SIMD)
__global__ void __launch_bounds__(kSsimThreads, 2) ssim_loss_tile_kernel(const float* __restrict__ a,
                                                                         const float* __restrict__ b, int H, int W,
                                                                         float data_range, SsimTaps taps,
                                                                         char* __restrict__ ws, SsimLossPlan plan) {
  __shared__ __align__(16) float stage[2 * kHaloH * kHaloW];
  __shared__ float hp[6][kHaloH * kTileW];  // horizontal sums: a', b', a'a', b'b', a'b', unusable count
  float* sa = stage;
  float* sb = stage + kHaloH * kHaloW;
  // the min / max fold runs before hp is written, the final sums after the staged fields are dead
  float* slo = hp[0];
  float* shi = hp[1];
  double* red = reinterpret_cast<double*>(stage);
  int* redc = reinterpret_cast<int*>(stage + 2 * kSsimThreads);
  static_assert(2 * kHaloH * kHaloW >= 3 * kSsimThreads && kHaloH * kTileW >= kSsimThreads, "aliases do not fit");
  const int tid = threadIdx.x;
  const int plane = blockIdx.x / plan.tiles_per_plane, t = blockIdx.x % plan.tiles_per_plane;
  const int y0 = (t / plan.tiles_x) * kTileH, x0 = (t % plan.tiles_x) * kTileW;  // the first position = its first pixel
  char* pws = ws + (size_t)plane * plan.stride;
  const float* mm = reinterpret_cast<const float*>(pws + plan.off_mm);
  const float nan = __uint_as_float(0x7fc00000u);

  // ---- r and L of the plane: min / max do not depend on the order
  ssim_minmax_fold(mm, plan.nblk, slo, shi, tid);
  const float lo = slo[0], hi = shi[0];
  const float r = 0.5f * lo + 0.5f * hi;  // halving is exact: one rounding, no overflow
  const float L = data_range > 0.0f ? data_range : hi - lo;
  // a plane without a finite target pixel (r is NaN) or with a constant target contributes no position
  const bool plane_ok = !ssim_nonfinite(r) && !ssim_nonfinite(L) && L > 0.0f;
  if (t == 0 && tid == 0) {
    float* head = reinterpret_cast<float*>(pws);
    head[0] = r;
    head[1] = L;
    head[2] = 0.0f;
    head[3] = 0.0f;
  }

  // ---- stage a - r, b - r of the rectangle's pixels
  const size_t pbase = (size_t)plane * (size_t)H * (size_t)W;
  for (int e = tid; e < kHaloH * kHaloW; e += kSsimThreads) {
    const int ly = e / kHaloW, lx = e - ly * kHaloW;
    const int y = y0 + ly, x = x0 + lx;
    float va = nan, vb = 0.0f;
    if (y < H && x < W) {
      const size_t o = pbase + (size_t)y * W + x;
      const float fa = a[o], fb = b[o];
      if (!ssim_nonfinite(fa) && !ssim_nonfinite(fb)) {
        va = fa - r;
        vb = fb - r;
      }
    }
    sa[e] = va;
    sb[e] = vb;
  }
  __syncthreads();

  // ---- the score's two passes: horizontal into LDS, vertical into registers; position row i
  // reads staged rows i .. i + 10
  ssim_horizontal_pass(sa, sb, hp, taps, tid);
  __syncthreads();
  const int lx = tid % kTileW, ry = (tid / kTileW) * kRowsPerThread;
  float acc[kRowsPerThread][6];
  ssim_vertical_pass(hp, taps, lx, ry, acc);
  const float k1 = 0.01f * L, k2 = 0.03f * L;
  const float C1 = k1 * k1, C2 = k2 * k2;
  float* coef = reinterpret_cast<float*>(pws + plan.off_coef);
  const size_t cplane = (size_t)plan.Hv * plan.Wv;
  double s_ssim = 0.0;
  int nwin = 0;
#pragma unroll
  for (int i = 0; i < kRowsPerThread; ++i) {
    const int y = y0 + ry + i, x = x0 + lx;
    const float ma = acc[i][0], mb = acc[i][1];
    const float saa = acc[i][2] - ma * ma, sbb = acc[i][3] - mb * mb, sab = acc[i][4] - ma * mb;
    const float Dc = saa + sbb + C2;
    const float cs = (2.0f * sab + C2) / Dc;
    const float mua = ma + r, mub = mb + r;
    const float Dl = mua * mua + mub * mub + C1;
    const float l = (2.0f * mua * mub + C1) / Dl;
    const float ss = l * cs;
    // no unusable pixel in the window: the window lies in the plane too
    const bool used = plane_ok && acc[i][5] == 0.0f;
    if (used) {
      s_ssim += (double)ss;
      ++nwin;
    }
    if (y < plan.Hv && x < plan.Wv) {
      const float Bp = -2.0f * ss / Dc;
      const float Cp = 2.0f * l / Dc;
      const float Ap = 2.0f * cs * (mub - mua * l) / Dl - Bp * ma - Cp * mb;
      const size_t o = (size_t)y * plan.Wv + x;
      coef[o] = used ? Ap : 0.0f;
      coef[cplane + o] = used ? Bp : 0.0f;
      coef[2 * cplane + o] = used ? Cp : 0.0f;
    }
  }

  // ---- the workgroup's sum and count, a fixed tree (stage was last read before the barrier above)
  term_tree(s_ssim, nwin, red, redc, tid);
  if (tid == 0) {
    reinterpret_cast<double*>(pws + plan.off_psum)[t] = red[0];
    reinterpret_cast<int*>(pws + plan.off_pcnt)[t] = redc[0];
  }
}

__global__ void __launch_bounds__(kSsimThreads) ssim_loss_plane_kernel(const char* __restrict__ ws, SsimLossPlan plan,
                                                                       float* __restrict__ parts,
                                                                       float* __restrict__ cparts) {
  const char* pws = ws + (size_t)blockIdx.x * plan.stride;
  term_plane_reduce(reinterpret_cast<const double*>(pws + plan.off_psum),
                    reinterpret_cast<const int*>(pws + plan.off_pcnt), plan.tiles_per_plane, blockIdx.x, parts, cparts);
}

__global__ void __launch_bounds__(kSsimThreads) ssim_loss_finalize_kernel(const float* __restrict__ parts,
                                                                          const float* __restrict__ cparts,
                                                                          long long nplanes, float weight,
                                                                          const float* base, float* ssim4,
                                                                          float* total) {
  term_finalize<true>(parts, cparts, nplanes, 1.0, weight, base, ssim4, total);  // L_ssim = 1 - S / Nused
}

__global__ void __launch_bounds__(kSsimThreads, 2) ssim_loss_dy_kernel(const char* __restrict__ ws, SsimLossPlan plan,
                                                                       const float* __restrict__ a,
                                                                       const float* __restrict__ b, int H, int W,
                                                                       float weight, SsimTaps taps,
                                                                       const float* __restrict__ ssim4,
                                                                       float* __restrict__ dy) {
  __shared__ float st[3][kHaloH * kHaloW];  // A, B, C at the positions whose windows reach the rectangle
  __shared__ float hp[3][kHaloH * kTileW];
  const int tid = threadIdx.x;
  const int plane = blockIdx.x / plan.dtiles_per_plane, t = blockIdx.x % plan.dtiles_per_plane;
  const int y0 = (t / plan.dtiles_x) * kTileH, x0 = (t % plan.dtiles_x) * kTileW;  // the first pixel
  const char* pws = ws + (size_t)plane * plan.stride;
  const float r = reinterpret_cast<const float*>(pws)[0];
  const float* coef = reinterpret_cast<const float*>(pws + plan.off_coef);
  const size_t cplane = (size_t)plan.Hv * plan.Wv;
  const float scale = -(weight * ssim4[2]);

  // ---- positions y0 - 10 .. y0 + 23, x0 - 10 .. x0 + 63; 0 outside the map (the full correlation)
  for (int e = tid; e < kHaloH * kHaloW; e += kSsimThreads) {
    const int ly = e / kHaloW, lx = e - ly * kHaloW;
    const int py = y0 - 2 * kSsimR + ly, px = x0 - 2 * kSsimR + lx;
    float vA = 0.0f, vB = 0.0f, vC = 0.0f;
    if (py >= 0 && py < plan.Hv && px >= 0 && px < plan.Wv) {
      const size_t o = (size_t)py * plan.Wv + px;
      vA = coef[o];
      vB = coef[cplane + o];
      vC = coef[2 * cplane + o];
    }
    st[0][e] = vA;
    st[1][e] = vB;
    st[2][e] = vC;
  }
  __syncthreads();

  // ---- horizontal pass: pixel column lx takes tap k from position column lx + 10 - k, k ascending
  for (int e = tid; e < kHaloH * kTileW; e += kSsimThreads) {
    const int ly = e / kTileW, lx = e % kTileW;
    const int o = ly * kHaloW + lx + 2 * kSsimR;
    float hA = 0.0f, hB = 0.0f, hC = 0.0f;
#pragma unroll
    for (int k = 0; k < kSsimTaps; ++k) {
      const float g = taps.g[k];
      hA = fmaf(g, st[0][o - k], hA);
      hB = fmaf(g, st[1][o - k], hB);
      hC = fmaf(g, st[2][o - k], hC);
    }
    hp[0][e] = hA;
    hp[1][e] = hB;
    hp[2][e] = hC;
  }
  __syncthreads();

  // ---- vertical pass: pixel row i takes tap k from staged row i + 10 - k
  const int lx = tid % kTileW, ry = (tid / kTileW) * kRowsPerThread;
  float acc[kRowsPerThread][3];
#pragma unroll
  for (int i = 0; i < kRowsPerThread; ++i) acc[i][0] = acc[i][1] = acc[i][2] = 0.0f;
#pragma unroll
  for (int j = 0; j < kRowsPerThread + kSsimTaps - 1; ++j) {
    float v[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) v[q] = hp[q][(ry + j) * kTileW + lx];
#pragma unroll
    for (int i = 0; i < kRowsPerThread; ++i) {
      const int k = i + 2 * kSsimR - j;
      if (k >= 0 && k < kSsimTaps) {
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[i][q] = fmaf(taps.g[k], v[q], acc[i][q]);
      }
    }
  }
  const size_t pbase = (size_t)plane * (size_t)H * (size_t)W;
#pragma unroll
  for (int i = 0; i < kRowsPerThread; ++i) {
    const int y = y0 + ry + i, x = x0 + lx;
    if (y < H && x < W) {
      const size_t o = pbase + (size_t)y * W + x;
      const float fa = a[o], fb = b[o];
      if (!ssim_nonfinite(fa) && !ssim_nonfinite(fb)) {
        const float s = fmaf(fb - r, acc[i][2], fmaf(fa - r, acc[i][1], acc[i][0]));
        dy[o] = __fmaf_rn(scale, s, dy[o]);  // one rounding
      }
    }
  }
}

bool bad_weight(float w) { return !(w >= 0.0f) || !std::isfinite(w); }

}  // namespace
}  // namespace srmi

using namespace srmi;

extern "C" {

int srmi_ssim_loss_workspace(long long nplanes, int H, int W, size_t* bytes) {
  SsimLossPlan p;
  if (!bytes) return SRMI_ERR_ARG;
  const int rc = ssim_loss_plan(nplanes, H, W, &p);
  if (rc) return rc;
  *bytes = (size_t)nplanes * p.stride;
  return 0;
}

int srmi_ssim_loss_parts(const float* pred, const float* target, long long nplanes, int H, int W, float data_range,
                         float* parts, float* cparts, void* ws, size_t ws_bytes, void* stream) {
  SsimLossPlan p;
  if (!pred || !target || !parts || !cparts || !ws || ((uintptr_t)ws & 15) != 0 || !std::isfinite(data_range))
    return SRMI_ERR_ARG;
  const int rc = ssim_loss_plan(nplanes, H, W, &p);
  if (rc) return rc;
  if (ws_bytes < (size_t)nplanes * p.stride) return SRMI_ERR_ARG;
  char* w = static_cast<char*>(ws);
  SsimTaps taps;
  ssim_fill_taps(&taps);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(ssim_loss_minmax_kernel, dim3((unsigned)(nplanes * p.nblk)), dim3(kSsimThreads), 0, st, target,
                     H * W, p.nblk, w, p);
  SRMI_CHECK_LAUNCH();
  hipLaunchKernelGGL(ssim_loss_tile_kernel, dim3((unsigned)(nplanes * p.tiles_per_plane)), dim3(kSsimThreads), 0, st,
                     pred, target, H, W, data_range, taps, w, p);
  SRMI_CHECK_LAUNCH();
  hipLaunchKernelGGL(ssim_loss_plane_kernel, dim3((unsigned)nplanes), dim3(kSsimThreads), 0, st, w, p, parts, cparts);
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_ssim_loss_from_parts(const float* parts, const float* cparts, long long nplanes, float weight,
                              const float* base, float* ssim4, float* total, void* stream) {
  if (!parts || !cparts || !base || !ssim4 || !total || nplanes < 1 || bad_weight(weight)) return SRMI_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(ssim_loss_finalize_kernel, dim3(1), dim3(kSsimThreads), 0, st, parts, cparts, nplanes, weight,
                     base, ssim4, total);
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_ssim_loss_dy(const void* ws, size_t ws_bytes, const float* pred, const float* target, long long nplanes,
                      int H, int W, float weight, const float* ssim4, float* dy, void* stream) {
  SsimLossPlan p;
  if (!ws || ((uintptr_t)ws & 15) != 0 || !pred || !target || !ssim4 || !dy || bad_weight(weight)) return SRMI_ERR_ARG;
  const int rc = ssim_loss_plan(nplanes, H, W, &p);
  if (rc) return rc;
  if (ws_bytes < (size_t)nplanes * p.stride) return SRMI_ERR_ARG;
  if (weight == 0.0f) return 0;  // dy stays as it is, bit for bit
  SsimTaps taps;
  ssim_fill_taps(&taps);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(ssim_loss_dy_kernel, dim3((unsigned)(nplanes * p.dtiles_per_plane)), dim3(kSsimThreads), 0, st,
                     static_cast<const char*>(ws), p, pred, target, H, W, weight, taps, ssim4, dy);
  SRMI_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
