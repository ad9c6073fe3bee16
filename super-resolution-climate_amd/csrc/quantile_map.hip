// Empirical quantile mapping of a super-resolved field: the histograms of a source and of a
// truth accumulated over many fields on a fixed range, the monotone transfer table T =
// F_truth^-1 o F_src built from them, and the pass that maps a field through T -- no
// reference counterpart (the reference never calibrates its output).  srmi.h states the
// definition; this file is its device form.
//
// Launches, none with a global atomic or a host read:
//   qm_hist_kernel    accumulate, 1: a fixed grid of workgroups per channel strides over the
//                     plane, a lane taking 8 consecutive pixels per step, bins src - base and
//                     truth - base (or the values) with the distribution score's own bin
//                     (dist_bin.hpp) into R copies of {hist src, hist truth} in LDS, and
//                     writes one int32 partial table with plain stores.
//   qm_finish_kernel  accumulate, 2: one workgroup per channel, the single writer of hist
//                     and count: the partial tables summed in workgroup order into int64,
//                     stored (first) or added to what is there.
//   qm_fit_kernel     one workgroup per channel: cumulative counts of both tables, an
//                     integer search per knot, one fp64 interpolation, the tie and tail
//                     rules, knots / table / meta.
//   qm_apply_kernel   the channel's table as (value, slope) pairs in LDS, one 8-byte LDS read
//                     per pixel, 16-byte global accesses where the planes allow.
//
// Contention in the histogram is distribution.hip's: the copy is lane % R and a copy's
// stride is 1 mod 32 dwords, so the lanes of a smooth field that share a bin spread over R
// banks.  The apply only READS the table: lanes on one entry broadcast, lanes on many
// entries spread over the banks by the entry's index.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cmath>

#include "common.hpp"
#include "dist_bin.hpp"
#include "srmi_internal.hpp"

// every fp32 and fp64 operation below is a defined one, rounded once: no fused forms
#pragma clang fp contract(off)

namespace srmi {

namespace {

constexpr int kQmThreads = 1024;                // histogram, finish and fit workgroups
constexpr int kQmSpan = kQmThreads * kDistRun;  // 8192 pixels of a histogram workgroup per step
constexpr int kQmBlocks = 256;                  // histogram workgroups per channel, at most
constexpr int kQmMaxCopies = 32;
constexpr int kQmLdsBytes = 56 * 1024;  // the copies' budget
constexpr int kQmWaves = kQmThreads / 64;
constexpr int kQmMaxC = 16;
constexpr int kQmMaxBins = 4096;
constexpr int kQmMaxKnots = kQmMaxBins + 3;                                   // M + 1
constexpr int kQmFitChunk = (kQmMaxKnots + kQmThreads - 1) / kQmThreads;      // knots of a fit thread, at most
constexpr int kQmApplyThreads = 512;
constexpr int kQmApplyRun = 4;                                  // pixels of a lane per step: one 16-byte access
constexpr int kQmApplySpan = kQmApplyThreads * kQmApplyRun;     // 2048 pixels of an apply workgroup per step
constexpr int kQmApplyBlocks = 2048;                            // apply workgroups per channel, at most

struct QmRanges {
  float lo[kQmMaxC], hi[kQmMaxC];
};

// ------------------------------------------------------------------ accumulate
// lds: R copies of `stride` dwords {hist src [B + 2], hist truth [B + 2], pad}
template <bool HasBase>
__global__ void __launch_bounds__(kQmThreads) qm_hist_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                             const float* __restrict__ base, long long HW, int nblk,
                                                             int B, QmRanges rg, int R, int stride, int Wp,
                                                             int* __restrict__ part) {
  extern __shared__ unsigned int lds[];
  const int c = blockIdx.x / nblk, blk = blockIdx.x % nblk, tid = threadIdx.x;
  const int nb2 = B + 2;
  for (int i = tid; i < R * stride; i += kQmThreads) lds[i] = 0u;
  __syncthreads();
  const float lo = rg.lo[c], hi = rg.hi[c];
  const float scale = __fdiv_rn((float)B, __fsub_rn(hi, lo));
  unsigned int* ha = lds + ((tid & 63) & (R - 1)) * stride;
  unsigned int* hb = ha + nb2;
  const float* pa = a + (size_t)c * (size_t)HW;
  const float* pb = b + (size_t)c * (size_t)HW;
  const float* pz = HasBase ? base + (size_t)c * (size_t)HW : nullptr;
  const bool veca = ((uintptr_t)pa & 15) == 0, vecb = ((uintptr_t)pb & 15) == 0, vecz = ((uintptr_t)pz & 15) == 0;
  const long long nruns = (HW + kDistRun - 1) / kDistRun;
  for (long long r = (long long)blk * kQmThreads + tid; r < nruns; r += (long long)nblk * kQmThreads) {
    float va[kDistRun], vb[kDistRun], vz[kDistRun];
    dist_load_run(pa, r * kDistRun, HW, veca, va);
    dist_load_run(pb, r * kDistRun, HW, vecb, vb);
    if (HasBase) dist_load_run(pz, r * kDistRun, HW, vecz, vz);
#pragma unroll
    for (int k = 0; k < kDistRun; ++k) {
      const float xa = HasBase ? __fsub_rn(va[k], vz[k]) : va[k];
      const float xb = HasBase ? __fsub_rn(vb[k], vz[k]) : vb[k];
      if (!dist_nonfinite(xa) && !dist_nonfinite(xb)) {
        atomicAdd(&ha[dist_bin(xa, lo, hi, scale, B)], 1u);
        atomicAdd(&hb[dist_bin(xb, lo, hi, scale, B)], 1u);
      }
    }
  }
  __syncthreads();
  // the workgroup's table: the copies added, plain stores; the pad of the row 0
  for (int w = tid; w < Wp; w += kQmThreads) {
    unsigned int s = 0;
    if (w < 2 * nb2)
      for (int q = 0; q < R; ++q) s += lds[q * stride + w];
    part[(size_t)blockIdx.x * Wp + w] = (int)s;
  }
}

__device__ inline long long qm_wave_sum(long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// hist[c] (=, +=) the partial tables in workgroup order; count[c] (=, +=) the src table's sum
__global__ void __launch_bounds__(kQmThreads) qm_finish_kernel(const int* __restrict__ part, int nblk, int B, int Wp,
                                                               int first, long long* __restrict__ hist,
                                                               long long* __restrict__ count) {
  __shared__ long long wtot[kQmWaves];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nb2 = B + 2;
  const int* p = part + (size_t)c * nblk * Wp;
  long long mine = 0;
  for (int w = tid; w < 2 * nb2; w += kQmThreads) {
    long long s = 0;
    for (int q = 0; q < nblk; ++q) s += p[(size_t)q * Wp + w];
    if (w < nb2) mine += s;
    long long* h = hist + (size_t)c * 2 * nb2 + w;
    *h = first ? s : *h + s;
  }
  mine = qm_wave_sum(mine);
  if (lane == 0) wtot[wave] = mine;
  __syncthreads();
  if (tid == 0) {
    long long S = 0;
    for (int q = 0; q < kQmWaves; ++q) S += wtot[q];
    count[c] = first ? S : count[c] + S;
  }
}

// --------------------------------------------------------------------------- fit
__device__ inline double qm_edge(double lo, double hi, double w, int j, int B) {
  return j == B + 1 ? hi : lo + (double)(j - 1) * w;
}

// T at the cumulative source count a, for the knot whose own edge is ej: F_truth^-1(a) by the
// piecewise-linear quantile over scb[0 .. M] (non-decreasing, scb[0] = 0, scb[M] = N); where a
// meets scb on a stretch k0 .. k1 (empty truth bins) the point of it nearest to ej.
__device__ inline double qm_knot(const long long* scb, long long a, long long N, double ej, double lo, double hi,
                                 double w, int B) {
  const int M = B + 2;
  int l = 0, r = M;  // the smallest k with scb[k] >= a: scb[M] = N >= a
  while (l < r) {
    const int m = (l + r) >> 1;
    if (scb[m] >= a)
      r = m;
    else
      l = m + 1;
  }
  const int k0 = l;
  if (scb[k0] != a) {  // scb[k0 - 1] < a < scb[k0]
    const int k = k0 - 1;
    const long long below = scb[k], h = scb[k0] - below;
    return qm_edge(lo, hi, w, k, B) + w * (double)(a - below) / (double)h;
  }
  l = k0, r = M;  // the largest k with scb[k] <= a
  while (l < r) {
    const int m = (l + r + 1) >> 1;
    if (scb[m] <= a)
      l = m;
    else
      r = m - 1;
  }
  const int k1 = l;
  double t = ej;
  if (a != 0) {
    const double left = qm_edge(lo, hi, w, k0, B);
    t = t < left ? left : t;
  }
  if (a != N) {
    const double right = qm_edge(lo, hi, w, k1, B);
    t = t > right ? right : t;
  }
  return t;
}

__global__ void __launch_bounds__(kQmThreads) qm_fit_kernel(const long long* __restrict__ hist, int B, QmRanges rg,
                                                            long long tail, double* __restrict__ knots,
                                                            float* __restrict__ table, float* __restrict__ meta) {
  __shared__ long long scb[kQmMaxKnots];
  __shared__ long long wtot[2][kQmWaves];
  __shared__ int sj[2];
  __shared__ double sshift[2];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = B + 2, K = M + 1;
  const long long* ha = hist + (size_t)c * 2 * M;
  const long long* hb = ha + M;
  const int chunk = (K + kQmThreads - 1) / kQmThreads;
  const int j0 = min(tid * chunk, K), j1 = min(j0 + chunk, K);  // this thread's knots
  if (tid == 0) sj[0] = K, sj[1] = -1;

  // ---- cumulative counts before entry j: the thread's own entries, then a scan of the sums
  long long la = 0, lb = 0;
  for (int j = j0; j < j1; ++j)
    if (j < M) {
      la += ha[j];
      lb += hb[j];
    }
  long long ia = la, ib = lb;
  for (int o = 1; o < 64; o <<= 1) {
    const long long ta = __shfl_up(ia, o), tb = __shfl_up(ib, o);
    if (lane >= o) {
      ia += ta;
      ib += tb;
    }
  }
  if (lane == 63) {
    wtot[0][wave] = ia;
    wtot[1][wave] = ib;
  }
  __syncthreads();
  long long ca = ia - la, cb = ib - lb, N = 0;
  for (int q = 0; q < kQmWaves; ++q) {
    if (q < wave) {
      ca += wtot[0][q];
      cb += wtot[1][q];
    }
    N += wtot[0][q];
  }
  long long caj[kQmFitChunk];
#pragma unroll
  for (int i = 0; i < kQmFitChunk; ++i) {
    const int j = j0 + i;
    caj[i] = ca;
    if (j < j1) {
      scb[j] = cb;
      if (j < M) {
        ca += ha[j];
        cb += hb[j];
      }
    }
  }
  __syncthreads();

  // ---- the knots, and the first and last trusted one
  const double lo = (double)rg.lo[c], hi = (double)rg.hi[c];
  const double w = (hi - lo) / (double)B;
  double T[kQmFitChunk];
  int tlo = K, thi = -1;
#pragma unroll
  for (int i = 0; i < kQmFitChunk; ++i) {
    const int j = j0 + i;
    T[i] = 0.0;
    if (j < j1) {
      const double ej = qm_edge(lo, hi, w, j, B);
      T[i] = N > 0 ? qm_knot(scb, caj[i], N, ej, lo, hi, w, B) : ej;
      if (N > 0 && caj[i] >= tail && N - caj[i] >= tail) {
        tlo = min(tlo, j);
        thi = max(thi, j);
      }
    }
  }
  if (tlo < K) atomicMin(&sj[0], tlo);
  if (thi >= 0) atomicMax(&sj[1], thi);
  __syncthreads();
  const int f0 = sj[0], f1 = sj[1];
  const bool any = f1 >= 0;
#pragma unroll
  for (int i = 0; i < kQmFitChunk; ++i) {
    const int j = j0 + i;
    if (j < j1 && any) {
      if (j == f0) sshift[0] = T[i] - qm_edge(lo, hi, w, j, B);
      if (j == f1) sshift[1] = T[i] - qm_edge(lo, hi, w, j, B);
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kQmFitChunk; ++i) {
    const int j = j0 + i;
    if (j < j1) {
      const double ej = qm_edge(lo, hi, w, j, B);
      double t = T[i];
      if (!any)
        t = ej;
      else if (j < f0)
        t = ej + sshift[0];
      else if (j > f1)
        t = ej + sshift[1];
      knots[(size_t)c * K + j] = t;
      table[(size_t)c * K + j] = (float)t;
      if (j == 0) {
        meta[c * 4 + 0] = rg.lo[c];
        meta[c * 4 + 1] = rg.hi[c];
        meta[c * 4 + 2] = (float)(t - ej);
      }
      if (j == M) meta[c * 4 + 3] = (float)(t - ej);
    }
  }
}

// ------------------------------------------------------------------------- apply
// one pixel: srmi.h, "srmi_quantile_map_apply", line by line.  Plain operators, on purpose:
// under this file's contract(off) each is one rounded operation, whereas the __f*_rn forms
// of the HIP headers are compiled contractable and a multiply feeding an add fuses.
template <bool HasBase>
__device__ inline float qm_map(float x, float z, const float2* __restrict__ tab, float lo, float scale, float Mf,
                               int M, float strength, float slo, float shi) {
  const float v = HasBase ? x - z : x;
  if (v != v) return x;
  const float d = v - lo;
  const float p = d * scale;
  const float u = p + 1.0f;
  if (u < 0.0f) {
    const float q = strength * slo;
    return x + q;
  }
  if (u >= Mf) {
    const float q = strength * shi;
    return x + q;
  }
  const int k = min(max((int)u, 0), M - 1);
  const float f = u - (float)k;
  const float2 e = tab[k];  // {table[k], table[k + 1] - table[k]}
  const float g = f * e.y;
  const float y = e.x + g;
  const float dv = y - v;
  const float q = strength * dv;
  return x + q;
}

template <bool HasBase>
__global__ void __launch_bounds__(kQmApplyThreads) qm_apply_kernel(const float* x, const float* __restrict__ base,
                                                                   long long HW, int nblk, int B,
                                                                   const float* __restrict__ table,
                                                                   const float* __restrict__ meta, float strength,
                                                                   float* out) {
  extern __shared__ float2 tab[];
  const int c = blockIdx.x / nblk, blk = blockIdx.x % nblk, tid = threadIdx.x;
  const int M = B + 2;
  const float* t = table + (size_t)c * (M + 1);
  for (int k = tid; k < M; k += kQmApplyThreads) {
    const float t0 = t[k], t1 = t[k + 1];
    tab[k] = make_float2(t0, t1 - t0);
  }
  const float lo = meta[c * 4 + 0], hi = meta[c * 4 + 1], slo = meta[c * 4 + 2], shi = meta[c * 4 + 3];
  const float scale = __fdiv_rn((float)B, __fsub_rn(hi, lo));
  const float Mf = (float)M;
  __syncthreads();
  const float* px = x + (size_t)c * (size_t)HW;
  const float* pz = HasBase ? base + (size_t)c * (size_t)HW : nullptr;
  float* po = out + (size_t)c * (size_t)HW;
  const bool vec = (((uintptr_t)px | (uintptr_t)po | (uintptr_t)pz) & 15) == 0;
  const long long nruns = (HW + kQmApplyRun - 1) / kQmApplyRun;
  for (long long r = (long long)blk * kQmApplyThreads + tid; r < nruns; r += (long long)nblk * kQmApplyThreads) {
    const long long i0 = r * kQmApplyRun;
    if (vec && i0 + kQmApplyRun <= HW) {
      const float4 qx = *reinterpret_cast<const float4*>(px + i0);
      float4 qz = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (HasBase) qz = *reinterpret_cast<const float4*>(pz + i0);
      float4 o;
      o.x = qm_map<HasBase>(qx.x, qz.x, tab, lo, scale, Mf, M, strength, slo, shi);
      o.y = qm_map<HasBase>(qx.y, qz.y, tab, lo, scale, Mf, M, strength, slo, shi);
      o.z = qm_map<HasBase>(qx.z, qz.z, tab, lo, scale, Mf, M, strength, slo, shi);
      o.w = qm_map<HasBase>(qx.w, qz.w, tab, lo, scale, Mf, M, strength, slo, shi);
      *reinterpret_cast<float4*>(po + i0) = o;
    } else {
      float vx[kQmApplyRun], vz[kQmApplyRun];
#pragma unroll
      for (int k = 0; k < kQmApplyRun; ++k) {
        const bool in = i0 + k < HW;
        vx[k] = in ? px[i0 + k] : 0.0f;
        vz[k] = in && HasBase ? pz[i0 + k] : 0.0f;
      }
#pragma unroll
      for (int k = 0; k < kQmApplyRun; ++k)
        if (i0 + k < HW) po[i0 + k] = qm_map<HasBase>(vx[k], vz[k], tab, lo, scale, Mf, M, strength, slo, shi);
    }
  }
}

// --------------------------------------------------------------------------- host
struct QmPlan {
  long long HW;
  int nblk, Wp, R, stride;
  size_t bytes;
};

int qm_plan(int C, int H, int W, int B, QmPlan* p) {
  if (C < 1 || C > kQmMaxC || H < 1 || W < 1 || B < 2 || B > kQmMaxBins) return SRMI_ERR_ARG;
  p->HW = (long long)H * W;
  if (p->HW > 2147483647LL) return SRMI_ERR_ARG;
  const long long nb = (p->HW + kQmSpan - 1) / kQmSpan;
  p->nblk = (int)(nb < kQmBlocks ? nb : kQmBlocks);
  const int Wn = 2 * (B + 2);
  p->Wp = (Wn + 3) & ~3;
  p->stride = ((Wn + 30) / 32) * 32 + 1;  // the smallest >= Wn that is 1 mod 32: copy q starts on bank q
  int R = kQmMaxCopies;
  while (R > 1 && (size_t)R * p->stride * 4 > (size_t)kQmLdsBytes) R >>= 1;
  p->R = R;
  p->bytes = (((size_t)C * p->nblk * p->Wp * sizeof(int)) + 255) & ~(size_t)255;
  return 0;
}

// the HOST array range [C][2] -> by-value kernel argument; SRMI_ERR_ARG unless finite, hi > lo
// and hi - lo finite in fp32 (it is the scale's divisor: an overflowed one would give scale 0)
int qm_ranges(const float* range, int C, QmRanges* rg) {
  if (!range) return SRMI_ERR_ARG;
  for (int c = 0; c < kQmMaxC; ++c) {
    const float lo = c < C ? range[2 * c] : 0.0f, hi = c < C ? range[2 * c + 1] : 1.0f;
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(hi > lo) || !std::isfinite(hi - lo)) return SRMI_ERR_ARG;
    rg->lo[c] = lo;
    rg->hi[c] = hi;
  }
  return 0;
}

bool qm_overlap(const float* p, const float* q, size_t n) { return p < q + n && q < p + n; }

}  // namespace
}  // namespace srmi

using namespace srmi;

extern "C" {

int srmi_quantile_map_accumulate_workspace(int C, int H, int W, int nbins, size_t* bytes) {
  QmPlan p;
  if (!bytes) return SRMI_ERR_ARG;
  const int rc = qm_plan(C, H, W, nbins, &p);
  if (rc) return rc;
  *bytes = p.bytes;
  return 0;
}

int srmi_quantile_map_accumulate(const float* src, const float* truth, const float* base, int C, int H, int W,
                                 int nbins, const float* range, int first, void* ws, size_t ws_bytes,
                                 long long* hist, long long* count, void* stream) {
  QmPlan p;
  QmRanges rg;
  if (!src || !truth || !ws || !hist || !count || ((uintptr_t)ws & 15) != 0) return SRMI_ERR_ARG;
  int rc = qm_plan(C, H, W, nbins, &p);
  if (rc) return rc;
  rc = qm_ranges(range, C, &rg);
  if (rc) return rc;
  if (ws_bytes < p.bytes) return SRMI_ERR_ARG;
  int* part = static_cast<int*>(ws);
  const size_t lds = (size_t)p.R * p.stride * sizeof(unsigned int);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (base)
    hipLaunchKernelGGL(qm_hist_kernel<true>, dim3((unsigned)(C * p.nblk)), dim3(kQmThreads), lds, st, src, truth, base,
                       p.HW, p.nblk, nbins, rg, p.R, p.stride, p.Wp, part);
  else
    hipLaunchKernelGGL(qm_hist_kernel<false>, dim3((unsigned)(C * p.nblk)), dim3(kQmThreads), lds, st, src, truth,
                       base, p.HW, p.nblk, nbins, rg, p.R, p.stride, p.Wp, part);
  SRMI_CHECK_LAUNCH();
  hipLaunchKernelGGL(qm_finish_kernel, dim3((unsigned)C), dim3(kQmThreads), 0, st, part, p.nblk, nbins, p.Wp,
                     first ? 1 : 0, hist, count);
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_quantile_map_fit(const long long* hist, const long long* count, int C, int nbins, const float* range,
                          long long tail_count, double* knots, float* table, float* meta, void* stream) {
  QmRanges rg;
  if (!hist || !count || !knots || !table || !meta) return SRMI_ERR_ARG;
  if (C < 1 || C > kQmMaxC || nbins < 2 || nbins > kQmMaxBins || tail_count < 0) return SRMI_ERR_ARG;
  const int rc = qm_ranges(range, C, &rg);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(qm_fit_kernel, dim3((unsigned)C), dim3(kQmThreads), 0, st, hist, nbins, rg, tail_count, knots,
                     table, meta);
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_quantile_map_apply(const float* x, const float* base, int C, int H, int W, int nbins, const float* table,
                            const float* meta, float strength, float* out, void* stream) {
  if (!x || !table || !meta || !out) return SRMI_ERR_ARG;
  if (C < 1 || C > kQmMaxC || H < 1 || W < 1 || nbins < 2 || nbins > kQmMaxBins) return SRMI_ERR_ARG;
  const long long HW = (long long)H * W;
  if (HW > 2147483647LL) return SRMI_ERR_ARG;
  if (!std::isfinite(strength) || strength < 0.0f || strength > 1.0f) return SRMI_ERR_ARG;
  const size_t n = (size_t)C * (size_t)HW;
  if (base && qm_overlap(base, out, n)) return SRMI_ERR_ARG;
  if (out != x && qm_overlap(x, out, n)) return SRMI_ERR_ARG;  // in place or apart, nothing between
  const long long nb = (HW + kQmApplySpan - 1) / kQmApplySpan;
  const int nblk = (int)(nb < kQmApplyBlocks ? nb : kQmApplyBlocks);
  const size_t lds = (size_t)(nbins + 2) * sizeof(float2);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (base)
    hipLaunchKernelGGL(qm_apply_kernel<true>, dim3((unsigned)(C * nblk)), dim3(kQmApplyThreads), lds, st, x, base, HW,
                       nblk, nbins, table, meta, strength, out);
  else
    hipLaunchKernelGGL(qm_apply_kernel<false>, dim3((unsigned)(C * nblk)), dim3(kQmApplyThreads), lds, st, x, base, HW,
                       nblk, nbins, table, meta, strength, out);
  SRMI_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
