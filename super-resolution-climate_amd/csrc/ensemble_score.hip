// Verification of an ensemble against a truth: CRPS (plain and fair), the rank histogram, the
// spread-skill ratio with a spread-binned reliability table, the spread-|error| correlation and
// a per-pixel CRPS map -- no reference counterpart.  srmi.h states the definition ("the
// ensemble score"); tests/ensemble_score_oracle.py restates it in numpy.  Per pixel everything
// is fp64, each operation rounded once, in the order srmi.h states: written with __d*_rn, and
// the Makefile builds this file with -ffp-contract=off, because the compiler treats those as
// plain operators and would fuse a product into the sum behind it.
//
// Launches, no global atomics, no host read:
//   ens_main_kernel<K>  one read of the K + 1 fields.  A workgroup owns kEnsSpan consecutive
//       pixels of one plane; a lane takes four consecutive pixels per step (one 16-byte load per
//       field where the planes start on 16-byte boundaries).  The integer tables are LDS
//       atomics (integers: exact in any order).  The nine fp64 sums run in a lane's registers in
//       the order of its pixels, then down a fixed xor tree of the wave and over the four waves.
//       The per-bin sums of the bins below the last run in lane-private LDS columns, [slot][lane]
//       doubles: a lane's 8-byte accesses of one slot fall on consecutive bank pairs, so no two
//       lanes of a group meet on a bank whatever their bins; the columns are reduced by the same
//       fixed tree.  The last bin's pair runs in registers beside the nine (30 columns at B = 16
//       are 60 KiB, inside the 64 KiB a launch gets without asking).  A workgroup stores its
//       partials in the workspace.
//   ens_finish_kernel   one workgroup of sixteen waves per channel, a wave per slot: the partials
//       in a fixed order without a barrier, then the tables, the sums, and one thread the derived
//       values.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.hpp"
#include "srmi_internal.hpp"

namespace srmi {

namespace {

typedef unsigned long long u64;

constexpr int kEnsThreads = 256;
constexpr int kEnsWaves = kEnsThreads / 64;
constexpr int kEnsQuad = 4, kEnsSteps = 4;
constexpr int kEnsSpan = kEnsThreads * kEnsQuad * kEnsSteps;  // srmi.ensemble_score.ENS_SPAN
constexpr int kEnsMaxK = 8, kEnsMaxB = 16;
constexpr int kEnsSums = 9;     // crps, crps_fair, a, b, var, e^2, |e|, s, s |e|
constexpr int kEnsRegs = kEnsSums + 2;  // a lane's register sums: those, then var and e^2 of the last bin
constexpr int kEnsDerived = 9;  // srmi.ensemble_score.ENS_DERIVED

struct EnsPlan {
  int blocks;      // workgroups of the main launch per channel
  int nd, ni;      // fp64 and integer slots per workgroup: 9 + 2 B and K + 3 + B
  size_t off_int;  // byte offset of the integer partials behind the fp64 ones
  size_t bytes;
};

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

int ens_plan(int K, int C, int H, int W, int B, EnsPlan* p) {
  if (K < 2 || K > kEnsMaxK || B < 1 || B > kEnsMaxB || C < 1 || H < 1 || W < 1) return SRMI_ERR_ARG;
  const long long HW = (long long)H * W;
  if (HW > 2147483647LL) return SRMI_ERR_SHAPE;
  const long long blocks = (HW + kEnsSpan - 1) / kEnsSpan;
  if (blocks * C >= (1LL << 31)) return SRMI_ERR_ARG;
  p->blocks = (int)blocks;
  p->nd = kEnsSums + 2 * B;
  p->ni = K + 3 + B;
  p->off_int = align16((size_t)C * p->nd * (size_t)blocks * sizeof(double));
  p->bytes = p->off_int + (size_t)C * p->ni * (size_t)blocks * sizeof(uint32_t);
  return 0;
}

__device__ __forceinline__ bool ens_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// t[0] + .. + t[K - 1], ascending j, added pairwise as the blend's ensemble_sum adds: ((t0 + t1)
// + (t2 + t3)) + ((t4 + t5) + (t6 + t7)) with the terms j >= K left out
template <int K>
__device__ __forceinline__ double ens_tree(const double (&t)[kEnsMaxK]) {
  const double s01 = K > 1 ? __dadd_rn(t[0], t[1]) : t[0], s23 = K > 3 ? __dadd_rn(t[2], t[3]) : t[2];
  const double s45 = K > 5 ? __dadd_rn(t[4], t[5]) : t[4], s67 = K > 7 ? __dadd_rn(t[6], t[7]) : t[6];
  const double s03 = K > 2 ? __dadd_rn(s01, s23) : s01, s47 = K > 6 ? __dadd_rn(s45, s67) : s45;
  return K > 4 ? __dadd_rn(s03, s47) : s03;
}

// the same bits in every lane: each level adds a pair both ways round, and a + b == b + a
__device__ __forceinline__ double ens_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = __dadd_rn(v, __shfl_xor(v, o, 64));
  return v;
}

// four consecutive pixels from i (a multiple of 4); past the plane: NaN, which no one uses.
// vec: the plane starts on a 16-byte boundary.
__device__ __forceinline__ void ens_load(const float* __restrict__ p, long long i, long long HW, bool vec,
                                         float (&v)[kEnsQuad]) {
  if (vec && i + kEnsQuad <= HW) {
    const float4 q = *reinterpret_cast<const float4*>(p + i);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (int e = 0; e < kEnsQuad; ++e) v[e] = i + e < HW ? p[i + e] : __uint_as_float(0x7fc00000u);
  }
}

__device__ __forceinline__ bool ens_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// dynamic LDS: col [2 (B - 1)][256] doubles, wred [11][4] doubles, tab [ni] uint32
template <int K>
__global__ void __launch_bounds__(kEnsThreads) ens_main_kernel(const float* __restrict__ members,
                                                               const float* __restrict__ truth,
                                                               const float* __restrict__ edges, int C, long long HW,
                                                               int B, EnsPlan plan, char* __restrict__ ws,
                                                               float* __restrict__ crps_map) {
  extern __shared__ double ens_lds[];
  double* col = ens_lds;
  double* wred = col + 2 * (B - 1) * kEnsThreads;
  uint32_t* tab = reinterpret_cast<uint32_t*>(wred + kEnsRegs * kEnsWaves);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = blockIdx.x / plan.blocks, g = blockIdx.x % plan.blocks;
  const float* tp = truth + (size_t)c * (size_t)HW;
  const float* mp = members + (size_t)c * (size_t)HW;
  const size_t mstride = (size_t)C * (size_t)HW;
  float* cm = crps_map ? crps_map + (size_t)c * (size_t)HW : nullptr;
  bool vec = ens_aligned16(tp) && (!cm || ens_aligned16(cm));
#pragma unroll
  for (int j = 0; j < K; ++j) vec = vec && ens_aligned16(mp + j * mstride);
  // the interior edges of the channel (the same for every lane); past B - 1: never compared
  float ed[kEnsMaxB - 1];
#pragma unroll
  for (int i = 0; i < kEnsMaxB - 1; ++i) ed[i] = i < B - 1 ? edges[(size_t)c * (B - 1) + i] : 0.f;
  for (int s = 0; s < 2 * (B - 1); ++s) col[s * kEnsThreads + tid] = 0.0;  // the lane's own column
  if (tid < plan.ni) tab[tid] = 0;
  __syncthreads();
  double sum[kEnsRegs];
#pragma unroll
  for (int k = 0; k < kEnsRegs; ++k) sum[k] = 0.0;
  uint32_t nused = 0, ntied = 0;
  const double dK = (double)K, dKK = (double)(K * K), dKK1 = (double)(K * (K - 1));
  const float fnan = __uint_as_float(0x7fc00000u);
#pragma unroll 1
  for (int step = 0; step < kEnsSteps; ++step) {
    const long long i0 = (long long)g * kEnsSpan + (long long)(step * kEnsThreads + tid) * kEnsQuad;
    if (i0 >= HW) break;  // later steps lie further on
    float y[kEnsQuad], m[kEnsMaxK][kEnsQuad], out[kEnsQuad];
    ens_load(tp, i0, HW, vec, y);
#pragma unroll
    for (int j = 0; j < K; ++j) ens_load(mp + j * mstride, i0, HW, vec, m[j]);
#pragma unroll
    for (int e = 0; e < kEnsQuad; ++e) {
      bool used = ens_finite(y[e]);
#pragma unroll
      for (int j = 0; j < K; ++j) used = used && ens_finite(m[j][e]);
      out[e] = fnan;
      if (used) {  // a pixel past the plane is NaN in every field
        const double yd = (double)y[e];
        double md[kEnsMaxK], t[kEnsMaxK];
        int rank = 0;
        bool tie = false;
#pragma unroll
        for (int j = 0; j < kEnsMaxK; ++j) md[j] = t[j] = 0.0;
#pragma unroll
        for (int j = 0; j < K; ++j) {
          md[j] = (double)m[j][e];
          t[j] = fabs(__dsub_rn(md[j], yd));
          rank += m[j][e] < y[e] ? 1 : 0;
          tie = tie || m[j][e] == y[e];
        }
        const double a = ens_tree<K>(t);
        double b = 0.0;
#pragma unroll
        for (int j = 0; j < K; ++j) {
#pragma unroll
          for (int l = j + 1; l < K; ++l) b = __dadd_rn(b, fabs(__dsub_rn(md[j], md[l])));
        }
        const double aK = __ddiv_rn(a, dK);
        const double crps = __dsub_rn(aK, __ddiv_rn(b, dKK));
        const double fair = __dsub_rn(aK, __ddiv_rn(b, dKK1));
        const double mean = __ddiv_rn(ens_tree<K>(md), dK);
#pragma unroll
        for (int j = 0; j < K; ++j) {
          const double d = __dsub_rn(md[j], mean);
          t[j] = __dmul_rn(d, d);
        }
        const double var = __ddiv_rn(ens_tree<K>(t), dK);
        const double err = __dsub_rn(mean, yd), aerr = fabs(err), e2 = __dmul_rn(err, err);
        const double sd = __dsqrt_rn(var);
        const float sf = (float)sd;
        int bin = 0;
#pragma unroll
        for (int i = 0; i < kEnsMaxB - 1; ++i) bin += (i < B - 1 && sf >= ed[i]) ? 1 : 0;
        sum[0] = __dadd_rn(sum[0], crps);
        sum[1] = __dadd_rn(sum[1], fair);
        sum[2] = __dadd_rn(sum[2], a);
        sum[3] = __dadd_rn(sum[3], b);
        sum[4] = __dadd_rn(sum[4], var);
        sum[5] = __dadd_rn(sum[5], e2);
        sum[6] = __dadd_rn(sum[6], aerr);
        sum[7] = __dadd_rn(sum[7], sd);
        sum[8] = __dadd_rn(sum[8], __dmul_rn(sd, aerr));
        if (bin == B - 1) {
          sum[9] = __dadd_rn(sum[9], var);
          sum[10] = __dadd_rn(sum[10], e2);
        } else {
          double* cv = col + (2 * bin) * kEnsThreads + tid;
          cv[0] = __dadd_rn(cv[0], var);
          cv[kEnsThreads] = __dadd_rn(cv[kEnsThreads], e2);
        }
        ++nused;
        ntied += tie ? 1u : 0u;
        atomicAdd(&tab[1 + rank], 1u);
        atomicAdd(&tab[K + 3 + bin], 1u);
        out[e] = (float)crps;
      }
    }
    if (cm) {
      if (vec && i0 + kEnsQuad <= HW) {
        *reinterpret_cast<float4*>(cm + i0) = make_float4(out[0], out[1], out[2], out[3]);
      } else {
#pragma unroll
        for (int e = 0; e < kEnsQuad; ++e)
          if (i0 + e < HW) cm[i0 + e] = out[e];
      }
    }
  }
  if (nused) atomicAdd(&tab[0], nused);
  if (ntied) atomicAdd(&tab[K + 2], ntied);
#pragma unroll
  for (int k = 0; k < kEnsRegs; ++k) {
    const double v = ens_wave_sum(sum[k]);
    if (lane == 0) wred[k * kEnsWaves + wave] = v;
  }
  __syncthreads();
  double* pd = reinterpret_cast<double*>(ws) + (size_t)c * plan.nd * (size_t)plan.blocks + g;
  if (tid < kEnsRegs) {  // the last bin's pair behind the columns' slots
    const int slot = tid < kEnsSums ? tid : tid + 2 * (B - 1);
    pd[(size_t)slot * plan.blocks] = __dadd_rn(__dadd_rn(wred[tid * kEnsWaves], wred[tid * kEnsWaves + 1]),
                                               __dadd_rn(wred[tid * kEnsWaves + 2], wred[tid * kEnsWaves + 3]));
  }
  for (int s = wave; s < 2 * (B - 1); s += kEnsWaves) {  // the same for every lane of a wave
    const double* cs = col + s * kEnsThreads + lane;
    const double v = ens_wave_sum(__dadd_rn(__dadd_rn(cs[0], cs[64]), __dadd_rn(cs[128], cs[192])));
    if (lane == 0) pd[(size_t)(kEnsSums + s) * plan.blocks] = v;
  }
  if (tid < plan.ni) {
    uint32_t* pi = reinterpret_cast<uint32_t*>(ws + plan.off_int);
    pi[((size_t)c * plan.ni + tid) * (size_t)plan.blocks + g] = tab[tid];
  }
}

constexpr int kEnsFinThreads = 1024;
constexpr int kEnsFinWaves = kEnsFinThreads / 64;

// a wave per slot, no barrier inside: a lane adds the slot's partials of workgroups lane, lane +
// 64, .. in ascending order, then the wave's fixed tree
__global__ void __launch_bounds__(kEnsFinThreads) ens_finish_kernel(int K, int B, EnsPlan plan,
                                                                    const char* __restrict__ ws,
                                                                    long long* __restrict__ counts,
                                                                    double* __restrict__ sums,
                                                                    double* __restrict__ derived) {
  __shared__ double S[kEnsSums + 2 * kEnsMaxB];
  __shared__ u64 N[kEnsMaxK + 3 + kEnsMaxB];
  const int tid = threadIdx.x, lane = tid & 63, c = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const double* pd = reinterpret_cast<const double*>(ws) + (size_t)c * plan.nd * (size_t)plan.blocks;
  const uint32_t* pi = reinterpret_cast<const uint32_t*>(ws + plan.off_int) + (size_t)c * plan.ni * (size_t)plan.blocks;
  for (int s = wave; s < plan.nd; s += kEnsFinWaves) {
    double v = 0.0;
    for (int g = lane; g < plan.blocks; g += 64) v = __dadd_rn(v, pd[(size_t)s * plan.blocks + g]);
    v = ens_wave_sum(v);
    if (lane == 0) S[s] = v;
  }
  for (int s = wave; s < plan.ni; s += kEnsFinWaves) {
    u64 v = 0;
    for (int g = lane; g < plan.blocks; g += 64) v += pi[(size_t)s * plan.blocks + g];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) N[s] = v;
  }
  __syncthreads();
  if (tid != 0) return;
  long long* cn = counts + (size_t)c * plan.ni;
  double* so = sums + (size_t)c * plan.nd;
  double* d = derived + (size_t)c * (kEnsDerived + 2 * B);
  for (int s = 0; s < plan.ni; ++s) cn[s] = (long long)N[s];
  for (int s = 0; s < plan.nd; ++s) so[s] = S[s];
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  if (N[0] == 0) {  // no used pixel: NaN in every derived entry (the tables and sums are 0 by themselves)
    for (int k = 0; k < kEnsDerived + 2 * B; ++k) d[k] = nan;
    return;
  }
  // the order srmi.h states, each operation rounded once
  const double n = (double)(long long)N[0];
  const double f = __ddiv_rn((double)(K + 1), (double)(K - 1));
  const double mse = __ddiv_rn(S[5], n), mvar = __ddiv_rn(S[4], n);
  const double rmse = __dsqrt_rn(mse);
  d[0] = __ddiv_rn(S[0], n);
  d[1] = __ddiv_rn(S[1], n);
  d[2] = rmse;
  d[3] = __dsqrt_rn(mvar);
  d[4] = __ddiv_rn(__dsqrt_rn(__dmul_rn(f, mvar)), rmse);
  const double ms = __ddiv_rn(S[7], n), ma = __ddiv_rn(S[6], n);
  const double cov = __dsub_rn(__ddiv_rn(S[8], n), __dmul_rn(ms, ma));
  const double vs = __dsub_rn(mvar, __dmul_rn(ms, ms)), va = __dsub_rn(mse, __dmul_rn(ma, ma));
  d[5] = __ddiv_rn(cov, __dsqrt_rn(__dmul_rn(vs, va)));
  d[6] = __ddiv_rn((double)(long long)(N[1] + N[1 + K]), n);
  d[7] = __ddiv_rn(2.0, (double)(K + 1));
  const double u = __ddiv_rn(1.0, (double)(K + 1));
  double ri = 0.0;
  for (int r = 0; r <= K; ++r) ri = __dadd_rn(ri, fabs(__dsub_rn(__ddiv_rn((double)(long long)N[1 + r], n), u)));
  d[8] = ri;
  for (int b = 0; b < B; ++b) {  // an empty bin: 0 / 0 = NaN in both
    const double nb = (double)(long long)N[K + 3 + b];
    d[kEnsDerived + b] = __dsqrt_rn(__dmul_rn(f, __ddiv_rn(S[kEnsSums + 2 * b], nb)));
    d[kEnsDerived + B + b] = __dsqrt_rn(__ddiv_rn(S[kEnsSums + 2 * b + 1], nb));
  }
}

template <int K>
int ens_launch_main(const float* members, const float* truth, const float* edges, int C, long long HW, int B,
                    const EnsPlan& p, char* ws, float* crps_map, hipStream_t st) {
  const size_t lds =
      ((size_t)2 * (B - 1) * kEnsThreads + kEnsRegs * kEnsWaves) * sizeof(double) + (size_t)p.ni * sizeof(uint32_t);
  hipLaunchKernelGGL(ens_main_kernel<K>, dim3((unsigned)(C * p.blocks)), dim3(kEnsThreads), lds, st, members, truth,
                     edges, C, HW, B, p, ws, crps_map);
  SRMI_CHECK_LAUNCH();
  return 0;
}

}  // namespace
}  // namespace srmi

using namespace srmi;

extern "C" {

int srmi_ensemble_score_workspace(int K, int C, int H, int W, int B, size_t* bytes) {
  EnsPlan p;
  if (!bytes) return SRMI_ERR_ARG;
  const int rc = ens_plan(K, C, H, W, B, &p);
  if (rc) return rc;
  *bytes = p.bytes;
  return 0;
}

int srmi_ensemble_score(const float* members, const float* truth, int K, int C, int H, int W, const float* edges,
                        int B, void* workspace, size_t workspace_bytes, long long* counts, double* sums,
                        double* derived, float* crps_map, int launches, void* stream) {
  EnsPlan p;
  if (launches & ~(SRMI_ENSEMBLE_SCORE_MAIN | SRMI_ENSEMBLE_SCORE_FINISH)) return SRMI_ERR_ARG;
  const int rc = ens_plan(K, C, H, W, B, &p);
  if (rc) return rc;
  if (!members || !truth || (B > 1 && !edges) || !workspace || ((uintptr_t)workspace & 15) || !counts || !sums ||
      !derived || workspace_bytes < p.bytes)
    return SRMI_ERR_ARG;
  char* w = static_cast<char*>(workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long HW = (long long)H * W;
  if (!launches) launches = SRMI_ENSEMBLE_SCORE_MAIN | SRMI_ENSEMBLE_SCORE_FINISH;
  if (launches & SRMI_ENSEMBLE_SCORE_MAIN) {
    int r = 0;
    switch (K) {
      case 2: r = ens_launch_main<2>(members, truth, edges, C, HW, B, p, w, crps_map, st); break;
      case 3: r = ens_launch_main<3>(members, truth, edges, C, HW, B, p, w, crps_map, st); break;
      case 4: r = ens_launch_main<4>(members, truth, edges, C, HW, B, p, w, crps_map, st); break;
      case 5: r = ens_launch_main<5>(members, truth, edges, C, HW, B, p, w, crps_map, st); break;
      case 6: r = ens_launch_main<6>(members, truth, edges, C, HW, B, p, w, crps_map, st); break;
      case 7: r = ens_launch_main<7>(members, truth, edges, C, HW, B, p, w, crps_map, st); break;
      default: r = ens_launch_main<8>(members, truth, edges, C, HW, B, p, w, crps_map, st); break;
    }
    if (r) return r;
  }
  if (launches & SRMI_ENSEMBLE_SCORE_FINISH) {
    hipLaunchKernelGGL(ens_finish_kernel, dim3((unsigned)C), dim3(kEnsFinThreads), 0, st, K, B, p, w, counts, sums,
                       derived);
    SRMI_CHECK_LAUNCH();
  }
  return 0;
}

}  // extern "C"
