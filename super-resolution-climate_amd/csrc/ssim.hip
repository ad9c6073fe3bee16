// SSIM / PSNR score of a super-resolved field: the Gaussian-window structural similarity
// (Wang, Bovik, Sheikh, Simoncelli 2004) of a prediction a against a truth b, [C][H][W]
// fp32, with its per-pixel map, the contrast-structure mean and the mean square error --
// no reference counterpart (the reference scores a field by its RMSE alone).  srmi.h states
// the definition; this file is its device form.
//
// The mask is PER CHANNEL: a position is used for channel c iff the 121 pixels of its
// window are finite in a and in b IN THAT CHANNEL.  (The spectral score, spectra.hip, skips
// a window for all channels at once; this score does not.)
//
// Three launches, no atomics, no host read:
//   ssim_minmax_kernel  a fixed grid of workgroups per channel strides over b's plane:
//                       min / max of the finite pixels (fminf / fmaxf started from NaN, so a
//                       plane without a finite pixel leaves NaN), one pair per workgroup.
//   ssim_tile_kernel    one workgroup per kTileH x kTileW rectangle of output pixels; the
//                       rectangles partition the plane.  It folds the min / max pairs of its
//                       channel (order-independent, so r and L are the same bits in every
//                       workgroup), stages the rectangle plus a 5-pixel halo of a - r and
//                       b - r in LDS, runs the horizontal 11-tap pass for the five moment
//                       planes and the count of unusable pixels into LDS, the vertical pass
//                       into registers, evaluates cs and ssim, writes its part of the map and
//                       its five partial sums (fp64 / integer, summed in a fixed tree).
//   ssim_finish_kernel  one workgroup per channel: the per-rectangle partials in a fixed
//                       order (256 contiguous shares in rectangle order, then a fixed tree),
//                       fp64 and int64, divided by the counts -- bit-identical from run to
//                       run.
//
// Unusable pixels.  A pixel that is non-finite in a or in b, or lies outside the plane, is
// staged as a' = NaN (the flag) and b' = 0.  The horizontal pass counts the flags and reads
// a flagged a' as 0, so every moment sum is finite and a NaN removes exactly the windows that
// hold it: a position is used iff the separable count over its window is 0 (the count is a
// small integer held in fp32, exact).  Positions whose window leaves the plane count the
// outside pixels and so are never used: that is the border of the map.
//
// Tile shape (DESIGN.md "SSIM score"): 24 rows x 64 columns, 256 threads.  The staged halo
// rectangle is 34 x 74 (x 2 fields, 19.7 KiB), the horizontal planes 6 x 34 x 64 fp32
// (51 KiB): 70.7 KiB, two workgroups per CU (the reductions reuse these buffers).  64
// columns keep a staged row at 296 bytes and every LDS access of a wave on 64 consecutive
// dwords (conflict-free); 24 rows are what two workgroups' LDS admit.  Pixels read over
// pixels owned: 34 * 74 / (24 * 64) = 1.64.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cmath>

#include "common.hpp"
#include "srmi_internal.hpp"
#include "ssim_common.hpp"  // the window, the tile shape, the taps and the two passes: shared with ssim_loss.hip

namespace srmi {

namespace {

__global__ void __launch_bounds__(kSsimThreads) ssim_minmax_kernel(const float* __restrict__ b, long long HW,
                                                                   int nblk, float* __restrict__ mm) {
  __shared__ float slo[kSsimThreads], shi[kSsimThreads];
  const int c = blockIdx.y, tid = threadIdx.x;
  ssim_minmax_block(b + (size_t)c * (size_t)HW, HW, blockIdx.x, nblk, slo, shi, tid);
  if (tid == 0) {
    mm[((size_t)c * nblk + blockIdx.x) * 2 + 0] = slo[0];
    mm[((size_t)c * nblk + blockIdx.x) * 2 + 1] = shi[0];
  }
}

// two workgroups per CU is what the LDS admits (2 waves per SIMD)
__global__ void __launch_bounds__(kSsimThreads, 2) ssim_tile_kernel(const float* __restrict__ a,
                                                                    const float* __restrict__ b, int H, int W,
                                                                    int tiles_x, int tiles_per_plane, float data_range,
                                                                    SsimTaps taps, const float* __restrict__ mm,
                                                                    int nblk, double* __restrict__ psum,
                                                                    int* __restrict__ pcnt, float* __restrict__ lout,
                                                                    float* __restrict__ map) {
  __shared__ __align__(16) float stage[2 * kHaloH * kHaloW];
  __shared__ float hp[6][kHaloH * kTileW];  // horizontal sums: a', b', a'a', b'b', a'b', unusable count
  float* sa = stage;
  float* sb = stage + kHaloH * kHaloW;
  // the min / max fold runs before hp is written, the final sums after the staged fields are dead
  float* slo = hp[0];
  float* shi = hp[1];
  double(*red)[kSsimThreads] = reinterpret_cast<double(*)[kSsimThreads]>(stage);
  int(*redc)[kSsimThreads] = reinterpret_cast<int(*)[kSsimThreads]>(stage + 6 * kSsimThreads);
  static_assert(2 * kHaloH * kHaloW >= 8 * kSsimThreads && kHaloH * kTileW >= kSsimThreads, "aliases do not fit");
  const int tid = threadIdx.x;
  const int c = blockIdx.x / tiles_per_plane, t = blockIdx.x % tiles_per_plane;
  const int y0 = (t / tiles_x) * kTileH, x0 = (t % tiles_x) * kTileW;
  const float nan = __uint_as_float(0x7fc00000u);

  // ---- r and L of the channel: min / max do not depend on the order
  ssim_minmax_fold(mm + (size_t)c * nblk * 2, nblk, slo, shi, tid);
  const float lo = slo[0], hi = shi[0];
  const float r = 0.5f * lo + 0.5f * hi;  // halving is exact: one rounding, no overflow
  const float L = data_range > 0.0f ? data_range : hi - lo;
  if (t == 0 && tid == 0) lout[c] = L;

  // ---- stage a - r, b - r with the halo; the own rectangle's squared error on the way
  const size_t plane = (size_t)c * (size_t)H * (size_t)W;
  double sq = 0.0;
  int npix = 0;
  for (int e = tid; e < kHaloH * kHaloW; e += kSsimThreads) {
    const int ly = e / kHaloW, lx = e - ly * kHaloW;
    const int y = y0 - kSsimR + ly, x = x0 - kSsimR + lx;
    float va = nan, vb = 0.0f;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const size_t o = plane + (size_t)y * W + x;
      const float fa = a[o], fb = b[o];
      if (!ssim_nonfinite(fa) && !ssim_nonfinite(fb)) {
        va = fa - r;
        vb = fb - r;
        if (ly >= kSsimR && ly < kSsimR + kTileH && lx >= kSsimR && lx < kSsimR + kTileW) {
          const double d = (double)fa - (double)fb;
          sq += d * d;
          ++npix;
        }
      }
    }
    sa[e] = va;
    sb[e] = vb;
  }
  __syncthreads();

  // ---- horizontal pass: one thread per (staged row, output column), taps in ascending order
  ssim_horizontal_pass(sa, sb, hp, taps, tid);
  __syncthreads();

  // ---- vertical pass: a thread owns kRowsPerThread consecutive rows of one column
  const int lx = tid % kTileW, ry = (tid / kTileW) * kRowsPerThread;
  float acc[kRowsPerThread][6];
  ssim_vertical_pass(hp, taps, lx, ry, acc);
  const float k1 = 0.01f * L, k2 = 0.03f * L;
  const float C1 = k1 * k1, C2 = k2 * k2;
  double s_ssim = 0.0, s_cs = 0.0;
  int nwin = 0;
#pragma unroll
  for (int i = 0; i < kRowsPerThread; ++i) {
    const int y = y0 + ry + i, x = x0 + lx;
    const float ma = acc[i][0], mb = acc[i][1];
    const float saa = acc[i][2] - ma * ma, sbb = acc[i][3] - mb * mb, sab = acc[i][4] - ma * mb;
    const float cs = (2.0f * sab + C2) / (saa + sbb + C2);
    const float mua = ma + r, mub = mb + r;
    const float ss = (2.0f * mua * mub + C1) / (mua * mua + mub * mub + C1) * cs;
    const bool used = acc[i][5] == 0.0f;  // no unusable pixel in the window: the window lies in the plane too
    if (used) {
      s_ssim += (double)ss;
      s_cs += (double)cs;
      ++nwin;
    }
    if (map && y < H && x < W) map[plane + (size_t)y * W + x] = used ? ss : nan;
  }

  // ---- the workgroup's five sums, a fixed tree
  red[0][tid] = s_ssim;
  red[1][tid] = s_cs;
  red[2][tid] = sq;
  redc[0][tid] = nwin;
  redc[1][tid] = npix;
  __syncthreads();
  for (int o = kSsimThreads / 2; o > 0; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int q = 0; q < 3; ++q) red[q][tid] += red[q][tid + o];
      redc[0][tid] += redc[0][tid + o];
      redc[1][tid] += redc[1][tid + o];
    }
    __syncthreads();
  }
  if (tid < 3) psum[(size_t)blockIdx.x * 3 + tid] = red[tid][0];
  if (tid < 2) pcnt[(size_t)blockIdx.x * 2 + tid] = redc[tid][0];
}

// out[c] = {sum ssim / nwin, sum cs / nwin, sum (a - b)^2 / npix, L}, count[c] = {nwin, npix}:
// thread l sums its contiguous share of the channel's rectangles in rectangle order, then a
// fixed tree over the 256 shares.  0 / 0 is the IEEE NaN.
__global__ void __launch_bounds__(kSsimThreads) ssim_finish_kernel(const double* __restrict__ psum,
                                                                   const int* __restrict__ pcnt, int tiles_per_plane,
                                                                   const float* __restrict__ lout,
                                                                   float* __restrict__ out,
                                                                   long long* __restrict__ count) {
  __shared__ double red[3][kSsimThreads];
  __shared__ long long redc[2][kSsimThreads];
  const int c = blockIdx.x, tid = threadIdx.x;
  const int share = (tiles_per_plane + kSsimThreads - 1) / kSsimThreads;
  const int t0 = min(tid * share, tiles_per_plane), t1 = min(t0 + share, tiles_per_plane);
  double s[3] = {0.0, 0.0, 0.0};
  long long n[2] = {0, 0};
  for (int t = t0; t < t1; ++t) {
    const size_t w = (size_t)c * tiles_per_plane + t;
#pragma unroll
    for (int q = 0; q < 3; ++q) s[q] += psum[w * 3 + q];
    n[0] += pcnt[w * 2 + 0];
    n[1] += pcnt[w * 2 + 1];
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) red[q][tid] = s[q];
  redc[0][tid] = n[0];
  redc[1][tid] = n[1];
  __syncthreads();
  for (int o = kSsimThreads / 2; o > 0; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int q = 0; q < 3; ++q) red[q][tid] += red[q][tid + o];
      redc[0][tid] += redc[0][tid + o];
      redc[1][tid] += redc[1][tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double nwin = (double)redc[0][0], npix = (double)redc[1][0];
    out[c * 4 + 0] = (float)(red[0][0] / nwin);
    out[c * 4 + 1] = (float)(red[1][0] / nwin);
    out[c * 4 + 2] = (float)(red[2][0] / npix);
    out[c * 4 + 3] = lout[c];
    count[c * 2 + 0] = redc[0][0];
    count[c * 2 + 1] = redc[1][0];
  }
}

struct SsimPlan {
  int tiles_x, tiles_per_plane, nblk;
  long long ntiles;
  size_t off_cnt, off_mm, off_l, bytes;
};

// SRMI_ERR_ARG for a plan outside the definition
int ssim_plan(int C, int H, int W, SsimPlan* p) {
  if (C < 1 || H < kSsimTaps || W < kSsimTaps || (long long)H * W >= (1LL << 31)) return SRMI_ERR_ARG;
  p->tiles_x = (W + kTileW - 1) / kTileW;
  const long long tpp = (long long)p->tiles_x * ((H + kTileH - 1) / kTileH);
  p->ntiles = tpp * C;
  if (p->ntiles >= (1LL << 31) || C > 65535) return SRMI_ERR_ARG;
  p->tiles_per_plane = (int)tpp;
  const long long per = (long long)kSsimThreads * kMmPerThread;
  const long long nb = ((long long)H * W + per - 1) / per;
  p->nblk = (int)(nb < kMmBlocks ? nb : kMmBlocks);
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  p->off_cnt = up((size_t)p->ntiles * 3 * sizeof(double));
  p->off_mm = p->off_cnt + up((size_t)p->ntiles * 2 * sizeof(int));
  p->off_l = p->off_mm + up((size_t)C * p->nblk * 2 * sizeof(float));
  p->bytes = p->off_l + up((size_t)C * sizeof(float));
  return 0;
}

}  // namespace
}  // namespace srmi

using namespace srmi;

extern "C" {

int srmi_ssim_workspace(int C, int H, int W, size_t* bytes) {
  SsimPlan p;
  if (!bytes) return SRMI_ERR_ARG;
  const int rc = ssim_plan(C, H, W, &p);
  if (rc) return rc;
  *bytes = p.bytes;
  return 0;
}

int srmi_ssim(const float* a, const float* b, int C, int H, int W, float data_range, void* ws, size_t ws_bytes,
              float* out, long long* count, float* map, void* stream) {
  SsimPlan p;
  if (!a || !b || !ws || !out || !count || ((uintptr_t)ws & 15) != 0 || !std::isfinite(data_range)) return SRMI_ERR_ARG;
  const int rc = ssim_plan(C, H, W, &p);
  if (rc) return rc;
  if (ws_bytes < p.bytes) return SRMI_ERR_ARG;
  char* base = static_cast<char*>(ws);
  double* psum = reinterpret_cast<double*>(base);
  int* pcnt = reinterpret_cast<int*>(base + p.off_cnt);
  float* mm = reinterpret_cast<float*>(base + p.off_mm);
  float* lout = reinterpret_cast<float*>(base + p.off_l);
  SsimTaps taps;
  ssim_fill_taps(&taps);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(ssim_minmax_kernel, dim3(p.nblk, C), dim3(kSsimThreads), 0, st, b, (long long)H * W, p.nblk, mm);
  SRMI_CHECK_LAUNCH();
  hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)p.ntiles), dim3(kSsimThreads), 0, st, a, b, H, W, p.tiles_x,
                     p.tiles_per_plane, data_range, taps, mm, p.nblk, psum, pcnt, lout, map);
  SRMI_CHECK_LAUNCH();
  hipLaunchKernelGGL(ssim_finish_kernel, dim3(C), dim3(kSsimThreads), 0, st, psum, pcnt, p.tiles_per_plane, lout, out,
                     count);
  SRMI_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
