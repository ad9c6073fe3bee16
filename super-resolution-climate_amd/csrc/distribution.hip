// Distribution score of a super-resolved field: the histograms of a prediction a and of a
// truth b, [C][H][W] fp32, on the truth's range, their joint histogram, and from those
// integer tables the Perkins skill score, the Wasserstein-1 distance, the under / over
// fractions and a set of quantiles -- no reference counterpart (the reference scores a field
// by its RMSE alone).  srmi.h states the definition; this file is its device form.
//
// Three launches, no global atomics, no host read:
//   dist_range_kernel   a fixed grid of workgroups per channel strides over the plane: min /
//                       max of b over the pixels finite in a AND in b (fminf / fmaxf started
//                       from NaN), one pair per workgroup.  Skipped when the caller gives the
//                       range.
//   dist_hist_kernel    a fixed grid of workgroups per channel.  Each folds the min / max
//                       pairs of its channel (order-independent: the same bits everywhere),
//                       thread 0 forms the two scales with one __fsub_rn and one __fdiv_rn
//                       each, then the workgroup strides over the plane, a lane taking 8
//                       consecutive pixels per step (two 16-byte loads per field), and counts
//                       into LDS with ds_add_u32: R copies of {hist a [B + 2], hist b
//                       [B + 2], joint [J J]}, the copy chosen by the lane.  It adds the
//                       copies and writes one int32 partial table with plain stores.
//   dist_finish_kernel  per channel one workgroup that sums the histograms' part of the
//                       partial tables in workgroup order into int64 and forms the derived
//                       values from those int64 tables alone, and four beside it that sum a
//                       slice of the joint histogram each.
//
// Contention (DESIGN.md "Distribution score" has the figures).  A smooth field puts the 512
// consecutive pixels of a wave's step into one or two bins, and with one copy of the tables
// the 64 lanes of a ds_add meet on one address: measured, the kernel takes 1.8 x its time on
// white noise.  What is kept: the copy is lane % R and a copy's stride is 1 mod 32 dwords, so
// lanes that share a bin spread over R addresses on R banks; with R = 8 (the default tables)
// the smooth field costs what white noise costs.  What was measured and is not the default
// (SRMI_DISTRIBUTION_* keep them selectable): a lane adding a run of equal bins among its 8
// pixels once removes the contention too, but its compares and branches cost more than the
// atomics they save, on both fields; copies chosen by the wave do nothing, because the LDS
// runs one wave-instruction at a time and the conflict is inside it.
//
// Every count a workgroup holds is below 2^31 (H W is), the sums over workgroups are int64:
// the tables are exact and bit-identical from run to run whatever the LDS arrival order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cmath>

#include "common.hpp"
#include "dist_bin.hpp"
#include "srmi_internal.hpp"

// (x - lo) * scale and the fp64 forms below are the defined operations: no fused forms
#pragma clang fp contract(off)

namespace srmi {

namespace {

constexpr int kDistThreads = 1024;                  // histogram and finish workgroups
constexpr int kDistSpan = kDistThreads * kDistRun;  // 8192 pixels of a workgroup per step
constexpr int kDistBlocks = 256;                    // histogram workgroups per channel, at most
constexpr int kRangeThreads = 256;
constexpr int kRangePerThread = 16;                 // pixels per thread at which the range grid stops growing
constexpr int kRangeBlocks = 1024;                  // range workgroups per channel, at most: one per thread of the fold
constexpr int kDistMaxCopies = 32;
constexpr int kDistLdsBytes = 56 * 1024;            // the copies' budget: two workgroups' worth fits a CU
constexpr int kDistMaxProbs = 16;
constexpr int kDistWaves = kDistThreads / 64;
constexpr int kDistJointParts = 4;                  // finish workgroups per channel that sum the joint histogram
static_assert(kRangeBlocks <= kDistThreads, "the fold reads one pair per thread");

struct DistProbs {
  double p[kDistMaxProbs];
};

__global__ void __launch_bounds__(kRangeThreads) dist_range_kernel(const float* __restrict__ a,
                                                                   const float* __restrict__ b, long long HW,
                                                                   int nblk, float* __restrict__ mm) {
  __shared__ float slo[kRangeThreads], shi[kRangeThreads];
  const int c = blockIdx.x / nblk, blk = blockIdx.x % nblk, tid = threadIdx.x;
  const float* pa = a + (size_t)c * (size_t)HW;
  const float* pb = b + (size_t)c * (size_t)HW;
  const bool veca = ((uintptr_t)pa & 15) == 0, vecb = ((uintptr_t)pb & 15) == 0;
  const float nan = __uint_as_float(0x7fc00000u);
  const long long nruns = (HW + kDistRun - 1) / kDistRun;
  float lo = nan, hi = nan;
  for (long long r = (long long)blk * kRangeThreads + tid; r < nruns; r += (long long)nblk * kRangeThreads) {
    float va[kDistRun], vb[kDistRun];
    dist_load_run(pa, r * kDistRun, HW, veca, va);
    dist_load_run(pb, r * kDistRun, HW, vecb, vb);
#pragma unroll
    for (int k = 0; k < kDistRun; ++k) {
      const float v = dist_nonfinite(va[k]) || dist_nonfinite(vb[k]) ? nan : vb[k];
      lo = fminf(lo, v);  // minNum: a NaN operand is ignored
      hi = fmaxf(hi, v);
    }
  }
  slo[tid] = lo;
  shi[tid] = hi;
  __syncthreads();
  for (int o = kRangeThreads / 2; o > 0; o >>= 1) {
    if (tid < o) {
      slo[tid] = fminf(slo[tid], slo[tid + o]);
      shi[tid] = fmaxf(shi[tid], shi[tid + o]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    mm[(size_t)blockIdx.x * 2 + 0] = slo[0];
    mm[(size_t)blockIdx.x * 2 + 1] = shi[0];
  }
}

// one table's counts of a lane's run: equal neighbours once (Merge) or every pixel for itself
template <bool Merge>
__device__ inline void dist_emit(unsigned int* __restrict__ h, const int (&k)[kDistRun], unsigned used) {
  if (Merge) {
    int cur = 0;
    unsigned cnt = 0;
#pragma unroll
    for (int p = 0; p < kDistRun; ++p) {
      if ((used >> p) & 1u) {
        if (cnt != 0 && k[p] != cur) {
          atomicAdd(&h[cur], cnt);
          cnt = 0;
        }
        cur = k[p];
        ++cnt;
      }
    }
    if (cnt != 0) atomicAdd(&h[cur], cnt);
  } else {
#pragma unroll
    for (int p = 0; p < kDistRun; ++p)
      if ((used >> p) & 1u) atomicAdd(&h[k[p]], 1u);
  }
}

// lds: R copies of `stride` dwords {hist a [B + 2], hist b [B + 2], joint [J J], pad}
template <bool Merge>
__global__ void __launch_bounds__(kDistThreads) dist_hist_kernel(const float* __restrict__ a,
                                                                 const float* __restrict__ b, long long HW, int nblk,
                                                                 int B, int J, int given, float glo, float ghi,
                                                                 const float* __restrict__ mm, int nblk_r, int R,
                                                                 int stride, int Wp, int by_wave,
                                                                 int* __restrict__ part, float* __restrict__ range) {
  extern __shared__ unsigned int lds[];
  __shared__ float slo[kDistWaves], shi[kDistWaves], sprm[4];
  const int c = blockIdx.x / nblk, blk = blockIdx.x % nblk, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int nb2 = B + 2;
  for (int i = tid; i < R * stride; i += kDistThreads) lds[i] = 0u;

  // ---- the range of the channel and the two scales, formed once
  {
    const float nan = __uint_as_float(0x7fc00000u);
    float lo = nan, hi = nan;
    if (!given) {
      for (int i = tid; i < nblk_r; i += kDistThreads) {
        lo = fminf(lo, mm[((size_t)c * nblk_r + i) * 2 + 0]);
        hi = fmaxf(hi, mm[((size_t)c * nblk_r + i) * 2 + 1]);
      }
      for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o));
        hi = fmaxf(hi, __shfl_xor(hi, o));
      }
    }
    if (lane == 0) {
      slo[wave] = lo;
      shi[wave] = hi;
    }
    __syncthreads();
    if (tid == 0) {
      if (given) {
        lo = glo, hi = ghi;
      } else {
        for (int w = 0; w < kDistWaves; ++w) {
          lo = fminf(lo, slo[w]);
          hi = fmaxf(hi, shi[w]);
        }
      }
      const bool open = hi > lo;
      const float d = __fsub_rn(hi, lo);
      sprm[0] = lo;
      sprm[1] = hi;
      sprm[2] = open ? __fdiv_rn((float)B, d) : 0.0f;
      sprm[3] = open && J > 0 ? __fdiv_rn((float)J, d) : 0.0f;
      if (blk == 0) {
        range[c * 2 + 0] = lo;
        range[c * 2 + 1] = hi;
      }
    }
    __syncthreads();
  }
  const float lo = sprm[0], hi = sprm[1], scale = sprm[2], scalej = sprm[3];

  const int copy = (by_wave ? wave : lane) & (R - 1);
  unsigned int* ha = lds + copy * stride;
  unsigned int* hb = ha + nb2;
  unsigned int* hj = hb + nb2;
  const float* pa = a + (size_t)c * (size_t)HW;
  const float* pb = b + (size_t)c * (size_t)HW;
  const bool veca = ((uintptr_t)pa & 15) == 0, vecb = ((uintptr_t)pb & 15) == 0;
  const long long nruns = (HW + kDistRun - 1) / kDistRun;
  for (long long r = (long long)blk * kDistThreads + tid; r < nruns; r += (long long)nblk * kDistThreads) {
    float va[kDistRun], vb[kDistRun];
    dist_load_run(pa, r * kDistRun, HW, veca, va);
    dist_load_run(pb, r * kDistRun, HW, vecb, vb);
    int ka[kDistRun], kb[kDistRun], kj[kDistRun];
    unsigned used = 0;
#pragma unroll
    for (int k = 0; k < kDistRun; ++k) {
      const bool u = !dist_nonfinite(va[k]) && !dist_nonfinite(vb[k]);
      used |= (u ? 1u : 0u) << k;
      ka[k] = u ? dist_bin(va[k], lo, hi, scale, B) : 0;
      kb[k] = u ? dist_bin(vb[k], lo, hi, scale, B) : 0;
      kj[k] = 0;
      if (J > 0 && u) {
        const int ja = min(max(dist_bin(va[k], lo, hi, scalej, J) - 1, 0), J - 1);
        const int jb = min(max(dist_bin(vb[k], lo, hi, scalej, J) - 1, 0), J - 1);
        kj[k] = ja * J + jb;
      }
    }
    dist_emit<Merge>(ha, ka, used);
    dist_emit<Merge>(hb, kb, used);
    if (J > 0) dist_emit<Merge>(hj, kj, used);
  }
  __syncthreads();

  // ---- the workgroup's table: the copies added, plain stores.  A row of `part` is {hist a,
  // hist b, pad to 4 entries, joint, pad to 4 entries}, the pads 0.
  const int Jo = (2 * nb2 + 3) & ~3;
  for (int w = tid; w < Wp; w += kDistThreads) {
    const int src = w < 2 * nb2 ? w : (w >= Jo && w - Jo < J * J) ? 2 * nb2 + (w - Jo) : -1;
    unsigned int s = 0;
    if (src >= 0)
      for (int q = 0; q < R; ++q) s += lds[q * stride + src];
    part[(size_t)blockIdx.x * Wp + w] = (int)s;
  }
}

__device__ inline long long dist_wave_sum(long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// hist, joint = the partial tables summed in workgroup order; then, from hist alone, count
// and derived [4 + 2 nprobs] = {pss, w1, under, over, q_pred[], q_truth[]}.  `nparts`
// workgroups per channel: part 0 sums the two histograms and forms the derived values, which
// need nothing else; parts 1 .. nparts - 1 sum a slice of the joint histogram each, beside it.
__global__ void __launch_bounds__(kDistThreads) dist_finish_kernel(const int* __restrict__ part, int nblk, int B, int J,
                                                                   int Wp, int nparts,
                                                                   const float* __restrict__ range, DistProbs probs,
                                                                   int nprobs, long long* hist, long long* joint,
                                                                   long long* __restrict__ count,
                                                                   double* __restrict__ derived) {
  __shared__ long long red[4 * kDistThreads];
  __shared__ long long wtot[2][kDistWaves];
  const int c = blockIdx.x / nparts, role = blockIdx.x % nparts;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nb2 = B + 2, Jo = (2 * nb2 + 3) & ~3;

  // ---- the tables: a thread owns 4 consecutive entries (one 16-byte load per partial table)
  {
    const int QW = Wp / 4, Qh = Jo / 4;  // quads of a row, of its histogram part
    const int per = nparts > 1 ? (QW - Qh + nparts - 2) / (nparts - 1) : 0;
    const int qlo = role == 0 ? 0 : min(Qh + (role - 1) * per, QW), qhi = role == 0 ? Qh : min(qlo + per, QW);
    const int Q = qhi - qlo;
    if (Q <= 0) return;  // the whole workgroup: a joint slice may be empty
    const int Qc = min(Q, kDistThreads), G = kDistThreads / Qc;  // G > 1 shares the partial tables among G groups
    const int4* p4 = reinterpret_cast<const int4*>(part + (size_t)c * nblk * Wp);
    const int g = tid / Qc;
    for (int q0 = 0; q0 < Q; q0 += Qc) {  // one pass whenever G > 1
      const int ql = tid % Qc, q = qlo + q0 + ql;
      const bool mine = g < G && q < qhi;
      long long s[4] = {0, 0, 0, 0};
      if (mine) {
#pragma unroll 4
        for (int p = g; p < nblk; p += G) {
          const int4 v = p4[(size_t)p * QW + q];
          s[0] += v.x, s[1] += v.y, s[2] += v.z, s[3] += v.w;
        }
      }
      if (G > 1) {
        if (mine) {
#pragma unroll
          for (int j = 0; j < 4; ++j) red[(g * Qc + ql) * 4 + j] = s[j];
        }
        __syncthreads();
        if (mine && g == 0) {
          for (int gg = 1; gg < G; ++gg) {
#pragma unroll
            for (int j = 0; j < 4; ++j) s[j] += red[(gg * Qc + ql) * 4 + j];
          }
        }
        __syncthreads();
      }
      if (mine && g == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int w = q * 4 + j;
          if (w < 2 * nb2)
            hist[(size_t)c * 2 * nb2 + w] = s[j];
          else if (w >= Jo && w - Jo < J * J)
            joint[(size_t)c * J * J + (w - Jo)] = s[j];
        }
      }
    }
  }
  if (role != 0) return;
  __threadfence_block();
  __syncthreads();

  // ---- cumulative counts: a thread owns `chunk` consecutive bins
  const long long* ha = hist + (size_t)c * 2 * nb2;
  const long long* hb = ha + nb2;
  const int chunk = (nb2 + kDistThreads - 1) / kDistThreads;
  const int k0 = min(tid * chunk, nb2), k1 = min(k0 + chunk, nb2);
  long long la = 0, lb = 0;
  for (int k = k0; k < k1; ++k) {
    la += ha[k];
    lb += hb[k];
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
  long long ca = ia - la, cb = ib - lb, N = 0;  // exclusive
  for (int w = 0; w < kDistWaves; ++w) {
    if (w < wave) {
      ca += wtot[0][w];
      cb += wtot[1][w];
    }
    N += wtot[0][w];
  }
  __syncthreads();  // wtot is reused below

  const int nd = 4 + 2 * nprobs;
  double* d = derived + (size_t)c * nd;
  const double lo = (double)range[c * 2 + 0], hi = (double)range[c * 2 + 1];
  const double w = (hi - lo) / (double)B;
  const double Nd = (double)N;
  long long spss = 0, sw1 = 0;
  for (int k = k0; k < k1; ++k) {
    const long long xa = ha[k], xb = hb[k];
    const long long pa = ca, pb = cb;
    ca += xa;
    cb += xb;
    spss += xa < xb ? xa : xb;
    sw1 += ca > cb ? ca - cb : cb - ca;
    if (N > 0) {
      const double left = lo + (double)(k - 1) * w;
      for (int i = 0; i < nprobs; ++i) {
        const double r = probs.p[i] * Nd;  // 0 < r < N
        if (xa > 0 && (double)pa < r && r <= (double)ca) d[4 + i] = left + w * (r - (double)pa) / (double)xa;
        if (xb > 0 && (double)pb < r && r <= (double)cb) d[4 + nprobs + i] = left + w * (r - (double)pb) / (double)xb;
      }
    }
  }
  spss = dist_wave_sum(spss);
  sw1 = dist_wave_sum(sw1);
  if (lane == 0) {
    wtot[0][wave] = spss;
    wtot[1][wave] = sw1;
  }
  __syncthreads();
  if (tid == 0) {
    long long S = 0, S1 = 0;
    for (int q = 0; q < kDistWaves; ++q) {
      S += wtot[0][q];
      S1 += wtot[1][q];
    }
    count[c] = N;
    if (N > 0) {
      d[0] = (double)S / Nd;
      d[1] = w * (double)S1 / Nd;
      d[2] = (double)ha[0] / Nd;
      d[3] = (double)ha[B + 1] / Nd;
    } else {
      const double nan = __longlong_as_double(0x7ff8000000000000LL);
      for (int i = 0; i < nd; ++i) d[i] = nan;
    }
  }
}

struct DistPlan {
  long long HW;
  int nblk, nblk_r, Wn, Wp, R, stride;
  size_t off_mm, bytes;
};

// SRMI_ERR_ARG for a plan outside the definition
int dist_plan(int C, int H, int W, int B, int J, DistPlan* p) {
  if (C < 1 || H < 1 || W < 1 || B < 2 || B > 4096 || J < 0 || J > 64) return SRMI_ERR_ARG;
  p->HW = (long long)H * W;
  if (p->HW > 2147483647LL) return SRMI_ERR_ARG;
  const long long nb = (p->HW + kDistSpan - 1) / kDistSpan;
  p->nblk = (int)(nb < kDistBlocks ? nb : kDistBlocks);
  const long long per = (long long)kRangeThreads * kRangePerThread;
  const long long nr = (p->HW + per - 1) / per;
  p->nblk_r = (int)(nr < kRangeBlocks ? nr : kRangeBlocks);
  if ((long long)C * kRangeBlocks >= (1LL << 31)) return SRMI_ERR_ARG;
  p->Wn = 2 * (B + 2) + J * J;
  p->Wp = ((2 * (B + 2) + 3) & ~3) + ((J * J + 3) & ~3);  // a row of the partial tables: both parts padded to 16 bytes
  p->stride = ((p->Wn + 30) / 32) * 32 + 1;  // the smallest >= Wn that is 1 mod 32: copy q starts on bank q
  int R = kDistMaxCopies;
  while (R > 1 && (size_t)R * p->stride * 4 > (size_t)kDistLdsBytes) R >>= 1;
  p->R = R;
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  p->off_mm = up((size_t)C * p->nblk * p->Wp * sizeof(int));
  p->bytes = p->off_mm + up((size_t)C * p->nblk_r * 2 * sizeof(float));
  return 0;
}

}  // namespace
}  // namespace srmi

using namespace srmi;

extern "C" {

int srmi_distribution_workspace(int C, int H, int W, int nbins, int njoint, size_t* bytes) {
  DistPlan p;
  if (!bytes) return SRMI_ERR_ARG;
  const int rc = dist_plan(C, H, W, nbins, njoint, &p);
  if (rc) return rc;
  *bytes = p.bytes;
  return 0;
}

int srmi_distribution(const float* a, const float* b, int C, int H, int W, int nbins, int njoint, const float* lo_hi,
                      const double* probs, int nprobs, void* ws, size_t ws_bytes, long long* hist, long long* joint,
                      float* range, long long* count, double* derived, int flags, void* stream) {
  DistPlan p;
  if (!a || !b || !ws || !hist || !range || !count || !derived || ((uintptr_t)ws & 15) != 0) return SRMI_ERR_ARG;
  if (flags & ~(SRMI_DISTRIBUTION_MERGE_RUNS | SRMI_DISTRIBUTION_ONE_COPY | SRMI_DISTRIBUTION_COPY_BY_WAVE))
    return SRMI_ERR_ARG;
  if (nprobs < 0 || nprobs > kDistMaxProbs || (nprobs > 0 && !probs)) return SRMI_ERR_ARG;
  const int rc = dist_plan(C, H, W, nbins, njoint, &p);
  if (rc) return rc;
  if (njoint > 0 && !joint) return SRMI_ERR_ARG;
  if (ws_bytes < p.bytes) return SRMI_ERR_ARG;
  DistProbs pr;
  for (int i = 0; i < kDistMaxProbs; ++i) {
    pr.p[i] = i < nprobs ? probs[i] : 0.5;
    if (!(pr.p[i] > 0.0 && pr.p[i] < 1.0)) return SRMI_ERR_ARG;
  }
  float glo = 0.0f, ghi = 0.0f;
  if (lo_hi) {
    glo = lo_hi[0], ghi = lo_hi[1];
    if (!std::isfinite(glo) || !std::isfinite(ghi) || !(ghi > glo)) return SRMI_ERR_ARG;
  }
  int R = p.R;
  if (flags & SRMI_DISTRIBUTION_ONE_COPY) R = 1;
  if ((flags & SRMI_DISTRIBUTION_COPY_BY_WAVE) && R > kDistWaves) R = kDistWaves;
  char* base = static_cast<char*>(ws);
  int* part = reinterpret_cast<int*>(base);
  float* mm = reinterpret_cast<float*>(base + p.off_mm);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (!lo_hi) {
    hipLaunchKernelGGL(dist_range_kernel, dim3((unsigned)(C * p.nblk_r)), dim3(kRangeThreads), 0, st, a, b, p.HW,
                       p.nblk_r, mm);
    SRMI_CHECK_LAUNCH();
  }
  const size_t lds = (size_t)R * p.stride * sizeof(unsigned int);
  const int by_wave = (flags & SRMI_DISTRIBUTION_COPY_BY_WAVE) ? 1 : 0;
  if (!(flags & SRMI_DISTRIBUTION_MERGE_RUNS))
    hipLaunchKernelGGL(dist_hist_kernel<false>, dim3((unsigned)(C * p.nblk)), dim3(kDistThreads), lds, st, a, b, p.HW,
                       p.nblk, nbins, njoint, lo_hi ? 1 : 0, glo, ghi, mm, p.nblk_r, R, p.stride, p.Wp, by_wave, part,
                       range);
  else
    hipLaunchKernelGGL(dist_hist_kernel<true>, dim3((unsigned)(C * p.nblk)), dim3(kDistThreads), lds, st, a, b, p.HW,
                       p.nblk, nbins, njoint, lo_hi ? 1 : 0, glo, ghi, mm, p.nblk_r, R, p.stride, p.Wp, by_wave, part,
                       range);
  SRMI_CHECK_LAUNCH();
  const int nparts = njoint > 0 ? 1 + kDistJointParts : 1;
  hipLaunchKernelGGL(dist_finish_kernel, dim3((unsigned)(C * nparts)), dim3(kDistThreads), 0, st, part, p.nblk, nbins,
                     njoint, p.Wp, nparts, range, pr, nprobs, hist, joint, count, derived);
  SRMI_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
