// What the auxiliary loss terms of the training step (spectral_loss.hip, ssim_loss.hip,
// gradient_loss.hip) share on the device: the workgroup's fp64-sum / count tree, the reduction
// of a plane's tile sums into parts / cparts, and the finalize of a term from the parts of the
// global batch.  DESIGN.md "The loss-term protocol" states what a term is; every function here
// is for one workgroup of kTermThreads threads, and every sum has one fixed order.
//
// Only fp64 arithmetic and one fp32 fma: nothing here depends on how a file's fp32 divide and
// sqrt are compiled.
#pragma once
#include <hip/hip_runtime.h>

#include "gradient_common.hpp"
#include "spectra_fft.hpp"
#include "ssim_common.hpp"

namespace srmi {

constexpr int kTermThreads = 256;
static_assert(kSpecThreads == kTermThreads && kSsimThreads == kTermThreads && kGradThreads == kTermThreads,
              "the loss terms' workgroups are the 256 threads the trees and shares below are written for");

// The workgroup's sums of s (fp64) and c over its threads, a fixed tree, left in red[0] /
// redc[0]; ends with a barrier.  No barrier comes before the first write: where red / redc
// alias other LDS, the caller's last read of it lies before a barrier of its own.
__device__ inline void term_tree(double s, int c, double* red, int* redc, int tid) {
  red[tid] = s;
  redc[tid] = c;
  __syncthreads();
  for (int o = kTermThreads / 2; o > 0; o >>= 1) {
    if (tid < o) {
      red[tid] += red[tid + o];
      redc[tid] += redc[tid + o];
    }
    __syncthreads();
  }
}

// parts[plane] = a plane's n tile sums, cparts[plane] = its tile counts: a thread sums its
// contiguous share of the tiles in tile order, then the tree over the shares; the sum is
// rounded to fp32 once.
__device__ inline void term_plane_reduce(const double* __restrict__ psum, const int* __restrict__ pcnt, int n,
                                         int plane, float* __restrict__ parts, float* __restrict__ cparts) {
  __shared__ double red[kTermThreads];
  __shared__ int redc[kTermThreads];
  const int tid = threadIdx.x;
  const int share = (n + kTermThreads - 1) / kTermThreads;
  const int t0 = min(tid * share, n), t1 = min(t0 + share, n);
  double s = 0.0;
  int c = 0;
  for (int t = t0; t < t1; ++t) {
    s += psum[t];
    c += pcnt[t];
  }
  term_tree(s, c, red, redc, tid);
  if (tid == 0) {
    parts[plane] = (float)red[0];
    cparts[plane] = (float)redc[0];  // <= H W <= 2^24: exact
  }
}

// term4 = {S, N, 1 / (N m), l} and total = base[0] + weight * l from the parts and counts of
// nplanes planes, fp64: 256 contiguous shares, each summed in plane order, then the shares in
// order (the plain sum in plane order up to 256 planes).  l = S / (N m), or 1 - S / (N m) with
// OneMinus; no used position (N == 0): the term and its gradient scale are 0, not NaN.  base
// is read before anything is written.
template <bool OneMinus>
__device__ inline void term_finalize(const float* __restrict__ parts, const float* __restrict__ cparts,
                                     long long nplanes, double m, float weight, const float* base, float* term4,
                                     float* total) {
  __shared__ double sums[kTermThreads], counts[kTermThreads];
  const int tid = threadIdx.x;
  const long long share = (nplanes + kTermThreads - 1) / kTermThreads;
  const long long i0 = min(tid * share, nplanes), i1 = min(i0 + share, nplanes);
  double s = 0.0, n = 0.0;
  for (long long i = i0; i < i1; ++i) {
    s += (double)parts[i];
    n += (double)cparts[i];
  }
  sums[tid] = s;
  counts[tid] = n;
  __syncthreads();
  if (tid != 0) return;
  s = 0.0;
  n = 0.0;
  for (int i = 0; i < kTermThreads; ++i) {
    s += sums[i];
    n += counts[i];
  }
  const float b0 = base[0];
  float l = 0.0f;
  if (n > 0.0) {
    l = (float)(OneMinus ? 1.0 - s / (n * m) : s / (n * m));
    term4[0] = (float)s;
    term4[1] = (float)n;
    term4[2] = (float)(1.0 / (n * m));
    term4[3] = l;
  } else {
    term4[0] = term4[1] = term4[2] = term4[3] = 0.0f;
  }
  total[0] = __fmaf_rn(weight, l, b0);
}

}  // namespace srmi
