// Spectral score of a super-resolved field: windowed (Welch) radial power spectra of a
// prediction a and a truth b, [C][H][W] fp32 -- no reference counterpart (the reference
// scores a field by its RMSE alone).  srmi.h states the definition; this file is its
// device form.
//
// Three launches, no atomics, no host read:
//   spectra_flags_kernel   one workgroup per window: skip[w] = 1 where a or b holds a
//                          non-finite value in any channel.
//   spectra_window_kernel  a fixed grid of workgroups strides over the (window, channel)
//                          jobs.  Per job: the fp64 means of both fields, then ONE complex
//                          transform of z = a' + i b' (a', b' the detrended, tapered
//                          windows), unpacked with Fa = (Z(k) + conj Z(-k)) / 2 and
//                          Fb = (Z(k) - conj Z(-k)) / 2i, and the four densities summed
//                          over shells into partial[w][c][4][K] (fp64).
//   spectra_reduce_kernel  per output the used windows in a fixed order (16 contiguous
//                          shares in window order, then the 16 sums in order), in fp64,
//                          divided by nused -- bit-identical from run to run and
//                          independent of the window kernel's grid.
//
// The transform is a radix-2 DIT FFT over lines of P points held contiguously in LDS
// (inputs stored at bit-reversed positions, twiddles from sincospi in fp64).  The LDS
// buffer holds kSlab = 4096 complex values (32 KiB):
//   P <= 64   the whole P x P plane: rows, a transpose through registers, columns.
//   P >= 128  rows in slabs of 4096 / P through a P x P scratch plane of the workgroup's
//             own in global memory (so the scratch is bounded by the grid, not by the
//             window count), then columns in slabs of 2048 / P columns TOGETHER WITH
//             THEIR MIRRORS (P - ix): Z(-k) of every bin of the slab is then in the slab.
// Column lines are padded to P + 1 values so that equal positions of neighbouring lines
// fall in different banks.
//
// Shells without atomics: along a column (fixed kx) the bins of shell j are the run
// |ky| in [ceil sqrt(j^2 - j + 1 - kx^2), floor sqrt(j^2 + j - kx^2)] (integer bounds of
// floor(sqrt(ky^2 + kx^2) + 0.5) == j), so thread j walks, column by column, the short
// runs of its own shell and keeps the four sums in registers across the whole job.
#include <hip/hip_runtime.h>
#include <math.h>

#include "common.hpp"
#include "spectra_fft.hpp"
#include "srmi_internal.hpp"

namespace srmi {

namespace {

constexpr int kSlab = 4096;              // complex values of the LDS buffer
constexpr int kSlabPad = kSlab + 64;     // + one value per line
constexpr int kSpecGridCap = 512;        // workgroups of the window kernel at P >= 128 (2 per CU): one plane each
constexpr int kSpecGridCapLds = 768;     // at P <= 64 (3 per CU is what the LDS admits; P = 64 holds its window in
                                         // registers between the mean and the transform and fits 2)

__global__ void __launch_bounds__(kSpecThreads) spectra_flags_kernel(const float* __restrict__ a,
                                                                     const float* __restrict__ b, int C, int H, int W,
                                                                     int P, int Q, int nx, int* __restrict__ skip) {
  const int w = blockIdx.x;
  const int y0 = spec_origin(w / nx, H, P, Q), x0 = spec_origin(w % nx, W, P, Q);
  int bad = 0;
  for (int c = 0; c < C; ++c) {
    const size_t base = ((size_t)c * H + y0) * W + x0;
    for (int e = threadIdx.x; e < P * P; e += kSpecThreads) {
      const size_t o = base + (size_t)(e / P) * W + (e % P);
      bad |= (int)spec_nonfinite(a[o]) | (int)spec_nonfinite(b[o]);
    }
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) skip[w] = bad ? 1 : 0;
}

__device__ inline int spec_isqrt(int n) {  // floor(sqrt(n)), n >= 0
  int r = (int)sqrtf((float)n);
  while (r * r > n) --r;
  while ((r + 1) * (r + 1) <= n) ++r;
  return r;
}

// The bins of shell j in column slot s (column index ix), their Z(-k) in slot ms: the four
// densities (not yet normalised) times wgt added to acc in fp64.  wgt = 2 serves the mirror
// column as well: both fields are real, so Fa(-k) = conj Fa(k), Fb likewise, -k has k's
// shell, and the bins of column -kx are exactly the mirrors of the bins of column kx.
template <int P>
__device__ inline void spec_shell_column(const float2* buf, int LS, int s, int ms, int ix, int j, double wgt,
                                         double acc[4]) {
  const int kx = ix < P / 2 ? ix : ix - P;
  const int kx2 = kx * kx, hi = j * j + j - kx2;
  if (hi < 0) return;
  const int lo = max(0, (j == 0 ? 0 : j * j - j + 1) - kx2);
  int m0 = spec_isqrt(lo);
  if (m0 * m0 < lo) ++m0;
  const int m1 = min(spec_isqrt(hi), P / 2);
  for (int m = m0; m <= m1; ++m) {
    for (int sign = 0; sign < 2; ++sign) {
      if (sign == 0 ? m > P / 2 - 1 : m < 1) continue;  // ky = +m needs m < P/2; ky = -m needs m >= 1
      const int iy = sign == 0 ? m : P - m;
      const float2 z = buf[s * LS + iy], zm = buf[ms * LS + ((P - iy) & (P - 1))];
      // Fa = (Z + conj Zm) / 2, Fb = (Z - conj Zm) / 2i
      const double far = 0.5 * ((double)z.x + (double)zm.x), fai = 0.5 * ((double)z.y - (double)zm.y);
      const double fbr = 0.5 * ((double)z.y + (double)zm.y), fbi = -0.5 * ((double)z.x - (double)zm.x);
      const double er = far - fbr, ei = fai - fbi;
      acc[0] += wgt * (far * far + fai * fai);
      acc[1] += wgt * (fbr * fbr + fbi * fbi);
      acc[2] += wgt * (er * er + ei * ei);
      acc[3] += wgt * (far * fbr + fai * fbi);
    }
  }
}

// at least 2 workgroups per CU: the grid at P >= 128 is 2 per CU
template <int P>
__global__ void __launch_bounds__(kSpecThreads, 2) spectra_window_kernel(const float* __restrict__ a,
                                                                      const float* __restrict__ b, int C, int H, int W,
                                                                      int Q, int nx, int nwin,
                                                                      const int* __restrict__ skip,
                                                                      double* __restrict__ partial,
                                                                      float2* __restrict__ scratch) {
  constexpr int LOGP = P == 16 ? 4 : P == 32 ? 5 : P == 64 ? 6 : P == 128 ? 7 : 8;
  constexpr int K = P / 2 + 1;
  constexpr bool BIG = P > 64;
  constexpr int LS = P + 1;                   // padded line
  constexpr int R = BIG ? kSlab / P : P;      // lines per slab
  constexpr int M = R / 2;                    // BIG: column pairs per slab
  constexpr int NLD = R * P / kSpecThreads;   // values per thread and slab: 1, 4 or 16
  static_assert(R * LS <= kSlabPad && NLD * kSpecThreads == R * P && (P * P) % (R * P) == 0, "slab does not fit");
  __shared__ float2 buf[kSlabPad];
  __shared__ float2 tw[128];
  __shared__ double hann[256];
  __shared__ double red[2 * kSpecThreads];
  const int tid = threadIdx.x;

  for (int k = tid; k < P / 2; k += kSpecThreads) {
    double s, c;
    sincospi(-2.0 * (double)k / (double)P, &s, &c);
    tw[k] = make_float2((float)c, (float)s);
  }
  for (int p = tid; p < P; p += kSpecThreads) hann[p] = 0.5 - 0.5 * cospi(2.0 * (double)p / (double)P);
  __syncthreads();

  float2* plane = BIG ? scratch + (size_t)blockIdx.x * P * P : nullptr;
  // 1 / (P^2 W2), W2 = (sum_p h(p)^2)^2 = (3 P / 8)^2 for the periodic Hann taper
  const double norm = 1.0 / ((double)P * (double)P * (0.375 * P) * (0.375 * P));
  const long long njobs = (long long)nwin * C;

  for (long long job = blockIdx.x; job < njobs; job += gridDim.x) {
    const int w = (int)(job / C), c = (int)(job % C);
    if (skip[w]) continue;  // uniform over the workgroup
    const int y0 = spec_origin(w / nx, H, P, Q), x0 = spec_origin(w % nx, W, P, Q);
    const size_t base = ((size_t)c * H + y0) * W + x0;

    // ---- the window's means, fp64, fixed order
    double sa = 0.0, sb = 0.0;
#pragma unroll 1
    for (int e0 = tid; e0 < P * P; e0 += NLD * kSpecThreads) {
      float fa[NLD], fb[NLD];  // NLD loads of each field in flight
#pragma unroll
      for (int i = 0; i < NLD; ++i) {
        const int e = e0 + i * kSpecThreads;
        const size_t o = base + (size_t)(e >> LOGP) * W + (e & (P - 1));
        fa[i] = a[o];
        fb[i] = b[o];
      }
#pragma unroll
      for (int i = 0; i < NLD; ++i) {
        sa += (double)fa[i];
        sb += (double)fb[i];
      }
    }
    red[tid] = sa;
    red[kSpecThreads + tid] = sb;
    __syncthreads();
    for (int o = kSpecThreads / 2; o > 0; o >>= 1) {
      if (tid < o) {
        red[tid] += red[tid + o];
        red[kSpecThreads + tid] += red[kSpecThreads + tid + o];
      }
      __syncthreads();
    }
    const double ma = red[0] / (double)(P * P), mb = red[kSpecThreads] / (double)(P * P);

    // ---- rows: z = a' + i b' at bit-reversed x, one slab of R rows at a time
#pragma unroll 1
    for (int r0 = 0; r0 < P; r0 += R) {
      float fa[NLD], fb[NLD];
#pragma unroll
      for (int i = 0; i < NLD; ++i) {
        const int e = tid + i * kSpecThreads;
        const size_t o = base + (size_t)(r0 + (e >> LOGP)) * W + (e & (P - 1));
        fa[i] = a[o];
        fb[i] = b[o];
      }
#pragma unroll
      for (int i = 0; i < NLD; ++i) {
        const int e = tid + i * kSpecThreads;
        const int rl = e >> LOGP, x = e & (P - 1), y = r0 + rl;
        const float da = (float)((double)fa[i] - ma), db = (float)((double)fb[i] - mb);
        const double h2 = hann[y] * hann[x];
        buf[rl * LS + (int)(__brev((unsigned)x) >> (32 - LOGP))] =
            make_float2((float)((double)da * h2), (float)((double)db * h2));
      }
      __syncthreads();
      spec_fft_lines<P, R>(buf, tw, LS);
      if constexpr (BIG) {
        for (int e = tid; e < R * P; e += kSpecThreads)
          plane[(size_t)(r0 + (e >> LOGP)) * P + (e & (P - 1))] = buf[(e >> LOGP) * LS + (e & (P - 1))];
        __syncthreads();  // the slab is free again; the plane's rows are visible to the workgroup
      }
    }

    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if constexpr (!BIG) {
      // ---- transpose through registers: [iy][ix] -> [ix][bitrev(iy)]
      constexpr int NE = P * P / kSpecThreads;
      float2 v[NE];
#pragma unroll
      for (int i = 0; i < NE; ++i) {
        const int e = tid + i * kSpecThreads;
        v[i] = buf[(e >> LOGP) * LS + (e & (P - 1))];
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < NE; ++i) {
        const int e = tid + i * kSpecThreads;
        buf[(e & (P - 1)) * LS + (int)(__brev((unsigned)(e >> LOGP)) >> (32 - LOGP))] = v[i];
      }
      __syncthreads();
      spec_fft_lines<P, P>(buf, tw, LS);
      if (tid < K) {  // columns 0 and P / 2 are their own mirrors; column ix stands for P - ix too
        spec_shell_column<P>(buf, LS, 0, 0, 0, tid, 1.0, acc);
#pragma unroll 1
        for (int ix = 1; ix < P / 2; ++ix) spec_shell_column<P>(buf, LS, ix, P - ix, ix, tid, 2.0, acc);
        spec_shell_column<P>(buf, LS, P / 2, P / 2, P / 2, tid, 1.0, acc);
      }
      __syncthreads();  // the next job overwrites buf
    } else {
      // ---- columns: slab sl holds columns sl M + q (slots 0 .. M-1) and their mirrors
      // P - (sl M + q) (slots M .. 2M-1); column 0 is its own mirror, and its mirror slot
      // carries column P / 2, which is its own mirror too
#pragma unroll 1
      for (int sl = 0; sl < (P / 2) / M; ++sl) {
        float2 z[NLD];
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
          const int e = tid + i * kSpecThreads;
          const int col = sl * M + e % M;
          const int ix = ((e / M) & 1) == 0 ? col : (col == 0 ? P / 2 : P - col);
          z[i] = plane[(size_t)(e / R) * P + ix];
        }
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
          const int e = tid + i * kSpecThreads;
          buf[(e % R) * LS + (int)(__brev((unsigned)(e / R)) >> (32 - LOGP))] = z[i];
        }
        __syncthreads();
        spec_fft_lines<P, R>(buf, tw, LS);
        if (tid < K) {  // slot s stands for its mirror slot s + M too; columns 0 and P / 2 are their own
#pragma unroll 1
          for (int s = 0; s < M; ++s) {
            const int col = sl * M + s;
            if (col == 0) {
              spec_shell_column<P>(buf, LS, 0, 0, 0, tid, 1.0, acc);
              spec_shell_column<P>(buf, LS, M, M, P / 2, tid, 1.0, acc);
            } else {
              spec_shell_column<P>(buf, LS, s, s + M, col, tid, 2.0, acc);
            }
          }
        }
        __syncthreads();  // the next slab (or job) overwrites buf and the plane
      }
    }
    if (tid < K) {
      double* o = partial + ((size_t)job * 4) * K + tid;
#pragma unroll
      for (int q = 0; q < 4; ++q) o[(size_t)q * K] = acc[q] * norm;
    }
  }
}

// out[o] = mean over the used windows of partial[w][o], o over [C][4][K].  A workgroup owns
// 16 outputs; window lane l of 16 sums its contiguous share of the windows in window
// order (a skipped window adds +0.0, its slot is read but never used), and the first lane
// adds the 16 sums in lane order: a fixed order whatever the launch, no atomics.
constexpr int kSpecRedOut = 16, kSpecRedLanes = kSpecThreads / kSpecRedOut;

__global__ void __launch_bounds__(kSpecThreads) spectra_reduce_kernel(const double* __restrict__ partial,
                                                                      const int* __restrict__ skip, int nwin, int n,
                                                                      float* __restrict__ out,
                                                                      int* __restrict__ nused) {
  __shared__ double sums[kSpecRedLanes][kSpecRedOut];
  __shared__ int counts[kSpecRedLanes];
  const int ox = threadIdx.x % kSpecRedOut, l = threadIdx.x / kSpecRedOut;
  const int o = blockIdx.x * kSpecRedOut + ox;
  const int share = (nwin + kSpecRedLanes - 1) / kSpecRedLanes;
  const int w0 = min(l * share, nwin), w1 = min(w0 + share, nwin);
  const size_t oc = (size_t)min(o, n - 1);  // the last workgroup's spare threads stay in bounds
  double s = 0.0;
  int used = 0;
#pragma unroll 8
  for (int w = w0; w < w1; ++w) {
    const int sk = skip[w];
    const double v = partial[(size_t)w * n + oc];
    s += sk ? 0.0 : v;
    used += sk ? 0 : 1;
  }
  sums[l][ox] = s;
  if (ox == 0) counts[l] = used;
  __syncthreads();
  if (l == 0 && o < n) {
    double t = 0.0;
    int u = 0;
    for (int i = 0; i < kSpecRedLanes; ++i) {
      t += sums[i][ox];
      u += counts[i];
    }
    out[o] = u ? (float)(t / (double)u) : __uint_as_float(0x7fc00000u);
    if (o == 0) *nused = u;
  }
}

struct SpecPlan {
  int ny, nx, nwin, grid, K;
  size_t off_partial, off_scratch, bytes;
};

// SRMI_ERR_ARG for a plan outside the definition
int spec_plan(int C, int H, int W, int P, int Q, SpecPlan* p) {
  if (C < 1 || H < 1 || W < 1 || P < 16 || P > 256 || (P & (P - 1)) != 0 || P > H || P > W || Q < 1 || Q > P)
    return SRMI_ERR_ARG;
  p->ny = overlap_count(H, P, Q);
  p->nx = overlap_count(W, P, Q);
  if (p->ny < 1 || p->nx < 1) return SRMI_ERR_ARG;
  const long long nwin = (long long)p->ny * p->nx;
  if (nwin * C > (1LL << 30)) return SRMI_ERR_ARG;
  p->nwin = (int)nwin;
  p->K = P / 2 + 1;
  const long long njobs = nwin * C;
  const int cap = P > 64 ? kSpecGridCap : kSpecGridCapLds;
  p->grid = (int)(njobs < cap ? njobs : cap);
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  p->off_partial = up((size_t)nwin * sizeof(int));
  p->off_scratch = p->off_partial + up((size_t)njobs * 4 * p->K * sizeof(double));
  p->bytes = p->off_scratch + (P > 64 ? (size_t)p->grid * P * P * sizeof(float2) : 0);
  return 0;
}

}  // namespace
}  // namespace srmi

using namespace srmi;

extern "C" {

int srmi_spectra_workspace(int C, int H, int W, int P, int Q, size_t* bytes) {
  SpecPlan p;
  if (!bytes) return SRMI_ERR_ARG;
  const int rc = spec_plan(C, H, W, P, Q, &p);
  if (rc) return rc;
  *bytes = p.bytes;
  return 0;
}

int srmi_spectra(const float* a, const float* b, int C, int H, int W, int P, int Q, void* ws, size_t ws_bytes,
                 float* out, int* nused, void* stream) {
  SpecPlan p;
  if (!a || !b || !ws || !out || !nused || ((uintptr_t)ws & 15) != 0) return SRMI_ERR_ARG;
  const int rc = spec_plan(C, H, W, P, Q, &p);
  if (rc) return rc;
  if (ws_bytes < p.bytes) return SRMI_ERR_ARG;
  int* skip = static_cast<int*>(ws);
  double* partial = reinterpret_cast<double*>(static_cast<char*>(ws) + p.off_partial);
  float2* scratch = reinterpret_cast<float2*>(static_cast<char*>(ws) + p.off_scratch);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(spectra_flags_kernel, dim3(p.nwin), dim3(kSpecThreads), 0, st, a, b, C, H, W, P, Q, p.nx, skip);
  SRMI_CHECK_LAUNCH();
#define SRMI_SPEC_CASE(PP)                                                                                         \
  case PP:                                                                                                         \
    hipLaunchKernelGGL(spectra_window_kernel<PP>, dim3(p.grid), dim3(kSpecThreads), 0, st, a, b, C, H, W, Q, p.nx, \
                       p.nwin, skip, partial, scratch);                                                            \
    break
  switch (P) {
    SRMI_SPEC_CASE(16);
    SRMI_SPEC_CASE(32);
    SRMI_SPEC_CASE(64);
    SRMI_SPEC_CASE(128);
    SRMI_SPEC_CASE(256);
    default:
      return SRMI_ERR_ARG;
  }
#undef SRMI_SPEC_CASE
  SRMI_CHECK_LAUNCH();
  const int n = C * 4 * p.K;
  hipLaunchKernelGGL(spectra_reduce_kernel, dim3((n + kSpecRedOut - 1) / kSpecRedOut), dim3(kSpecThreads), 0, st,
                     partial, skip, p.nwin, n, out, nused);
  SRMI_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
