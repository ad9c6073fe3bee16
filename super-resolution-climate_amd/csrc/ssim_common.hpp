// What the SSIM score (ssim.hip) and the SSIM loss term (ssim_loss.hip) share: the window,
// the tile shape of a workgroup, the taps, the test for a non-finite pixel, the min / max
// reductions of the range pass and the two passes of the windowed moments.  DESIGN.md "SSIM
// score" derives the tile shape.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace srmi {

constexpr int kSsimThreads = 256;
constexpr int kSsimR = 5, kSsimTaps = 2 * kSsimR + 1;
constexpr int kTileH = 24, kTileW = 64;              // output pixels of a workgroup
constexpr int kHaloH = kTileH + 2 * kSsimR;          // 34 staged rows
constexpr int kHaloW = kTileW + 2 * kSsimR;          // 74 staged columns
constexpr int kRowsPerThread = kTileH / (kSsimThreads / kTileW);  // 6: a thread owns 6 rows of one column
constexpr int kMmBlocks = 512;                       // min / max workgroups per channel, at most
constexpr int kMmPerThread = 16;                     // pixels per thread at which the min / max grid stops growing
static_assert(kSsimThreads % kTileW == 0 && kTileH % (kSsimThreads / kTileW) == 0, "tile does not fit the workgroup");

struct SsimTaps {
  float g[kSsimTaps];
};

// g[k] ~ exp(-(k - 5)^2 / (2 1.5^2)): normalised in fp64, then rounded
inline void ssim_fill_taps(SsimTaps* taps) {
  double g[kSsimTaps], s = 0.0;
  for (int k = 0; k < kSsimTaps; ++k) {
    g[k] = exp(-(double)((k - kSsimR) * (k - kSsimR)) / (2.0 * 1.5 * 1.5));
    s += g[k];
  }
  for (int k = 0; k < kSsimTaps; ++k) taps->g[k] = (float)(g[k] / s);
}

__device__ inline bool ssim_nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// The workgroup's min / max of (lo, hi) over its kSsimThreads threads, left in slo[0] / shi[0]
// (fminf / fmaxf: a NaN operand is ignored, so NaN stands for "nothing yet").
__device__ inline void ssim_minmax_tree(float lo, float hi, float* slo, float* shi, int tid) {
  slo[tid] = lo;
  shi[tid] = hi;
  __syncthreads();
  for (int o = kSsimThreads / 2; o > 0; o >>= 1) {
    if (tid < o) {
      slo[tid] = fminf(slo[tid], slo[tid + o]);
      shi[tid] = fmaxf(shi[tid], shi[tid + o]);
    }
    __syncthreads();
  }
}

// Workgroup blk of nblk strides over a plane p of HW pixels: min / max of its finite pixels
// into slo[0] / shi[0], NaN where it met none.
__device__ inline void ssim_minmax_block(const float* __restrict__ p, long long HW, int blk, int nblk, float* slo,
                                         float* shi, int tid) {
  const float nan = __uint_as_float(0x7fc00000u);
  float lo = nan, hi = nan;
  for (long long i = (long long)blk * kSsimThreads + tid; i < HW; i += (long long)nblk * kSsimThreads) {
    float v = p[i];
    v = ssim_nonfinite(v) ? nan : v;
    lo = fminf(lo, v);  // minNum: a NaN operand is ignored
    hi = fmaxf(hi, v);
  }
  ssim_minmax_tree(lo, hi, slo, shi, tid);
}

// The nblk (min, max) pairs of a plane folded into slo[0] / shi[0]: min / max do not depend on
// the order, so every workgroup of the plane gets the same bits.
__device__ inline void ssim_minmax_fold(const float* __restrict__ mm, int nblk, float* slo, float* shi, int tid) {
  const float nan = __uint_as_float(0x7fc00000u);
  float lo = nan, hi = nan;
  for (int i = tid; i < nblk; i += kSsimThreads) {
    lo = fminf(lo, mm[(size_t)i * 2 + 0]);
    hi = fmaxf(hi, mm[(size_t)i * 2 + 1]);
  }
  ssim_minmax_tree(lo, hi, slo, shi, tid);
}

// Horizontal 11-tap pass over the staged fields sa = a', sb = b' [kHaloH][kHaloW]: one thread
// per (staged row, output column), taps in ascending order, into hp = the sums of a', b',
// a'a', b'b', a'b' and the count of unusable pixels (a' = NaN is the flag and reads as 0).
__device__ inline void ssim_horizontal_pass(const float* sa, const float* sb, float (*hp)[kHaloH * kTileW],
                                            const SsimTaps& taps, int tid) {
  for (int e = tid; e < kHaloH * kTileW; e += kSsimThreads) {
    const int ly = e / kTileW, lx = e % kTileW;
    const float* pa = sa + ly * kHaloW + lx;
    const float* pb = sb + ly * kHaloW + lx;
    float ma = 0.0f, mb = 0.0f, aa = 0.0f, bb = 0.0f, ab = 0.0f, cnt = 0.0f;
#pragma unroll
    for (int k = 0; k < kSsimTaps; ++k) {
      float va = pa[k];
      const float vb = pb[k];
      const bool bad = va != va;
      cnt += bad ? 1.0f : 0.0f;
      va = bad ? 0.0f : va;
      const float g = taps.g[k];
      ma = fmaf(g, va, ma);
      mb = fmaf(g, vb, mb);
      aa = fmaf(g, va * va, aa);
      bb = fmaf(g, vb * vb, bb);
      ab = fmaf(g, va * vb, ab);
    }
    hp[0][e] = ma;
    hp[1][e] = mb;
    hp[2][e] = aa;
    hp[3][e] = bb;
    hp[4][e] = ab;
    hp[5][e] = cnt;
  }
}

// Vertical pass: the thread owns rows ry .. ry + kRowsPerThread - 1 of column lx; output row i
// reads staged rows i .. i + 10, ascending.  acc[i] = the five moments and the count.
__device__ inline void ssim_vertical_pass(const float (*hp)[kHaloH * kTileW], const SsimTaps& taps, int lx, int ry,
                                          float (*acc)[6]) {
#pragma unroll
  for (int i = 0; i < kRowsPerThread; ++i)
#pragma unroll
    for (int q = 0; q < 6; ++q) acc[i][q] = 0.0f;
#pragma unroll
  for (int j = 0; j < kRowsPerThread + kSsimTaps - 1; ++j) {
    float v[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) v[q] = hp[q][(ry + j) * kTileW + lx];
#pragma unroll
    for (int i = 0; i < kRowsPerThread; ++i) {
      const int k = j - i;
      if (k >= 0 && k < kSsimTaps) {
#pragma unroll
        for (int q = 0; q < 5; ++q) acc[i][q] = fmaf(taps.g[k], v[q], acc[i][q]);
        acc[i][5] += v[5];
      }
    }
  }
}

}  // namespace srmi
