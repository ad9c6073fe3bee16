// Spectral loss term of the training step: windowed Fourier amplitudes of the error
// p - t of a prediction and a target, [nplanes][H][W] fp32 -- no reference counterpart.
// srmi.h states the definition; this file is its device form.
//
// A job is one window of one plane.  Per plane the workspace holds
//   g      [nwin][P][P] fp32   the job's gradient window h h Re IDFT2(G), not yet scaled
//   jobsum [nwin]       fp64   sum_k A_k of the job (0 for a skipped job)
//   used   [nwin]       int32  1 where no pixel of the window is non-finite in p or in t
// one plane after the other (spec_loss_plan's stride), so a call over a range of planes
// works on its own part of the workspace and gives the bits the whole batch gives.
//
// Launches, no atomics, no host read:
//   spectral_loss_window_kernel  a fixed grid of workgroups strides over PAIRS of jobs, the
//       windows 2 i and 2 i + 1 of one plane (the last window of an odd plan alone), so the
//       pairing does not depend on which planes a call holds.  One complex transform of
//       z = d_a + i d_b (the tapered errors; a skipped or absent partner is 0), unpacked
//       with D_a = (Z(k) + conj Z(-k)) / 2, D_b = (Z(k) - conj Z(-k)) / 2i; the thread that
//       owns the bin pair (k, -k) forms A and G = D / (c A) of both jobs in fp64 and writes
//       X = G_a + i G_b in place (G is Hermitian, so X(-k) = conj G_a + i conj G_b); one
//       inverse transform then holds g_a in its real and g_b in its imaginary part.  The
//       A_k are summed per thread in bin order and over the threads by a tree, in fp64.
//   spectral_loss_plane_kernel   per plane the job sums in window order (fp64, rounded
//       once) and the used-job count into parts / cparts.
//   spectral_loss_finalize_kernel  parts and cparts over the planes of the global batch
//       (loss_term.hpp's term_finalize): spec4 and total.
//   spectral_loss_dy_kernel      a thread per pixel adds the used windows covering it in
//       ascending window index (fp32) and then scale * sum to dy: every pixel has one
//       writer and one order, whatever the grid.  A pixel no used window covers is not
//       written at all.
//
// The transform is spectra.hip's radix-2 LDS FFT (spectra_fft.hpp): rows, a transpose
// through registers, columns, with lines padded to P + 1 values; the inverse runs the
// same butterflies with conjugate twiddles, columns first.  At P = 64 the plane takes
// 32.5 KiB of LDS, the kernel 38 KiB and 225 registers: two workgroups per CU.
#include <hip/hip_runtime.h>
#include <math.h>

#include <cmath>

#include "common.hpp"
#include "loss_term.hpp"
#include "spectra_fft.hpp"
#include "srmi_internal.hpp"

namespace srmi {

namespace {

constexpr int kSpecLossGridCap = 768;  // 3 workgroups per CU
constexpr int kSpecLossDyGridCap = 1 << 20;

struct SpecLossPlan {
  int ny, nx, nwin;
  size_t off_sum, off_used, stride;  // bytes within a plane's part of the workspace
};

// SRMI_ERR_ARG for a plan outside the definition
int spec_loss_plan(long long nplanes, int H, int W, int P, int Q, SpecLossPlan* p) {
  if (nplanes < 1 || (P != 16 && P != 32 && P != 64) || P > H || P > W || Q < 1 || Q > P) return SRMI_ERR_ARG;
  p->ny = overlap_count(H, P, Q);
  p->nx = overlap_count(W, P, Q);
  if (p->ny < 1 || p->nx < 1) return SRMI_ERR_ARG;
  const long long nwin = (long long)p->ny * p->nx;
  if (nwin > (1LL << 24) || nwin * nplanes > (1LL << 30) || nplanes * H * (long long)W > (1LL << 40))
    return SRMI_ERR_ARG;
  p->nwin = (int)nwin;
  p->off_sum = (size_t)nwin * P * P * sizeof(float);
  p->off_used = p->off_sum + (size_t)nwin * sizeof(double);
  p->stride = (p->off_used + (size_t)nwin * sizeof(int) + 15) & ~(size_t)15;
  return 0;
}

template <int P>
__global__ void __launch_bounds__(kSpecThreads, 2) spectral_loss_window_kernel(
    const float* __restrict__ pred, const float* __restrict__ target, long long nplanes, int H, int W, int Q, int nx,
    int nwin, float eps, char* __restrict__ ws, SpecLossPlan plan) {
  constexpr int LOGP = P == 16 ? 4 : P == 32 ? 5 : 6;
  constexpr int LS = P + 1;                    // padded line
  constexpr int NE = P * P / kSpecThreads;     // values per thread: 1, 4 or 16
  static_assert(NE * kSpecThreads == P * P, "a whole number of values per thread");
  __shared__ float2 buf[P * LS];
  __shared__ float2 tw[P / 2], twi[P / 2];
  __shared__ double hann[P];
  __shared__ double red[2 * kSpecThreads];
  const int tid = threadIdx.x;

  for (int k = tid; k < P / 2; k += kSpecThreads) {
    double s, c;
    sincospi(-2.0 * (double)k / (double)P, &s, &c);
    tw[k] = make_float2((float)c, (float)s);
    twi[k] = make_float2((float)c, -(float)s);
  }
  for (int p = tid; p < P; p += kSpecThreads) hann[p] = 0.5 - 0.5 * cospi(2.0 * (double)p / (double)P);
  __syncthreads();

  // c = P^2 W2, W2 = (sum_p h(p)^2)^2 = (3 P / 8)^2 for the periodic Hann taper
  const double c = (double)P * (double)P * (0.375 * P) * (0.375 * P);
  const double invc = 1.0 / c, deps = (double)eps;
  const int npair = (nwin + 1) / 2;
  const long long nunits = nplanes * npair;

  for (long long unit = blockIdx.x; unit < nunits; unit += gridDim.x) {
    const long long plane = unit / npair;
    const int wa = 2 * (int)(unit % npair), wb = wa + 1;
    const bool has_b = wb < nwin;  // uniform over the workgroup
    char* pws = ws + (size_t)plane * plan.stride;
    float* g = reinterpret_cast<float*>(pws);
    double* jobsum = reinterpret_cast<double*>(pws + plan.off_sum);
    int* used = reinterpret_cast<int*>(pws + plan.off_used);
    const size_t pbase = (size_t)plane * H * W;
    const size_t base_a = pbase + (size_t)spec_origin(wa / nx, H, P, Q) * W + spec_origin(wa % nx, W, P, Q);
    const size_t base_b =
        has_b ? pbase + (size_t)spec_origin(wb / nx, H, P, Q) * W + spec_origin(wb % nx, W, P, Q) : base_a;

    // ---- the errors of both windows, and whether either field is non-finite on them
    float da[NE], db[NE];
    int bad_a = 0, bad_b = has_b ? 0 : 1;
    {
      float pa[NE], ta[NE], pb[NE], tb[NE];
#pragma unroll
      for (int i = 0; i < NE; ++i) {
        const int e = tid + i * kSpecThreads;
        const size_t o = (size_t)(e >> LOGP) * W + (e & (P - 1));
        pa[i] = pred[base_a + o];
        ta[i] = target[base_a + o];
        pb[i] = pred[base_b + o];
        tb[i] = target[base_b + o];
      }
#pragma unroll
      for (int i = 0; i < NE; ++i) {
        bad_a |= (int)spec_nonfinite(pa[i]) | (int)spec_nonfinite(ta[i]);
        bad_b |= (int)spec_nonfinite(pb[i]) | (int)spec_nonfinite(tb[i]);
        da[i] = pa[i] - ta[i];
        db[i] = pb[i] - tb[i];
      }
    }
    bad_a = __syncthreads_or(bad_a) ? 1 : 0;
    bad_b = __syncthreads_or(bad_b) ? 1 : 0;
    if (tid == 0) {
      used[wa] = 1 - bad_a;
      if (has_b) used[wb] = 1 - bad_b;
      if (bad_a) jobsum[wa] = 0.0;
      if (has_b && bad_b) jobsum[wb] = 0.0;
    }
    if (bad_a && bad_b) continue;  // uniform: nothing to transform

    // ---- z = h h (d_a + i d_b) at bit-reversed x; a skipped partner is 0
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int e = tid + i * kSpecThreads;
      const int y = e >> LOGP, x = e & (P - 1);
      const double h2 = hann[y] * hann[x];
      const float za = bad_a ? 0.0f : (float)((double)da[i] * h2);
      const float zb = bad_b ? 0.0f : (float)((double)db[i] * h2);
      buf[y * LS + (int)(__brev((unsigned)x) >> (32 - LOGP))] = make_float2(za, zb);
    }
    __syncthreads();
    spec_fft_lines<P, P>(buf, tw, LS);
    float2 v[NE];
    // transpose through registers: [iy][ix] -> [ix][bitrev(iy)]
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
    spec_fft_lines<P, P>(buf, tw, LS);  // buf[ix * LS + iy] = Z(ky = iy, kx = ix)

    // ---- A and G of both jobs, in place: the bin pair (k, -k) has one owner, the bin of
    // the smaller index, which alone reads and writes its two cells
    double sa = 0.0, sb = 0.0;
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int e = tid + i * kSpecThreads;
      const int s = e >> LOGP, q = e & (P - 1);
      const int ms = (P - s) & (P - 1), mq = (P - q) & (P - 1);
      const int me = ms * P + mq;
      if (e > me) continue;
      const float2 z = buf[s * LS + q], zm = buf[ms * LS + mq];
      // D_a = (Z + conj Zm) / 2, D_b = (Z - conj Zm) / 2i
      const double ar = 0.5 * ((double)z.x + (double)zm.x), ai = 0.5 * ((double)z.y - (double)zm.y);
      const double br = 0.5 * ((double)z.y + (double)zm.y), bi = -0.5 * ((double)z.x - (double)zm.x);
      const double Aa = sqrt((ar * ar + ai * ai) * invc + deps), Ab = sqrt((br * br + bi * bi) * invc + deps);
      const double fa = bad_a ? 0.0 : 1.0 / (c * Aa), fb = bad_b ? 0.0 : 1.0 / (c * Ab);
      const double gar = ar * fa, gai = ai * fa, gbr = br * fb, gbi = bi * fb;
      // X(k) = G_a + i G_b, X(-k) = conj G_a + i conj G_b
      buf[s * LS + q] = make_float2((float)(gar - gbi), (float)(gai + gbr));
      if (e != me) buf[ms * LS + mq] = make_float2((float)(gar + gbi), (float)(gbr - gai));
      const double mult = e == me ? 1.0 : 2.0;  // A(-k) = A(k)
      sa += mult * Aa;
      sb += mult * Ab;
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
    if (tid == 0) {
      if (!bad_a) jobsum[wa] = red[0];
      if (!bad_b) jobsum[wb] = red[kSpecThreads];
    }

    // ---- the unnormalised inverse: columns (lines along ky) first, then rows
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int e = tid + i * kSpecThreads;
      v[i] = buf[(e >> LOGP) * LS + (e & (P - 1))];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int e = tid + i * kSpecThreads;
      buf[(e >> LOGP) * LS + (int)(__brev((unsigned)(e & (P - 1))) >> (32 - LOGP))] = v[i];
    }
    __syncthreads();
    spec_fft_lines<P, P>(buf, twi, LS);  // buf[ix * LS + y]
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
    spec_fft_lines<P, P>(buf, twi, LS);  // buf[y * LS + x] = g_a + i g_b

    // ---- tapered again, the two real gradient windows
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int e = tid + i * kSpecThreads;
      const int y = e >> LOGP, x = e & (P - 1);
      const double h2 = hann[y] * hann[x];
      const float2 r = buf[y * LS + x];
      if (!bad_a) g[(size_t)wa * P * P + e] = (float)((double)r.x * h2);
      if (!bad_b) g[(size_t)wb * P * P + e] = (float)((double)r.y * h2);
    }
    __syncthreads();  // the next pair overwrites buf and red
  }
}

__global__ void __launch_bounds__(kSpecThreads) spectral_loss_plane_kernel(const char* __restrict__ ws,
                                                                           SpecLossPlan plan, long long nplanes,
                                                                           float* __restrict__ parts,
                                                                           float* __restrict__ cparts) {
  const long long plane = (long long)blockIdx.x * kSpecThreads + threadIdx.x;
  if (plane >= nplanes) return;
  const char* pws = ws + (size_t)plane * plan.stride;
  const double* jobsum = reinterpret_cast<const double*>(pws + plan.off_sum);
  const int* used = reinterpret_cast<const int*>(pws + plan.off_used);
  double s = 0.0;
  int n = 0;
  for (int w = 0; w < plan.nwin; ++w) {
    const int u = used[w];
    const double v = jobsum[w];
    s += u ? v : 0.0;
    n += u ? 1 : 0;
  }
  parts[plane] = (float)s;
  cparts[plane] = (float)n;
}

__global__ void __launch_bounds__(kSpecThreads) spectral_loss_finalize_kernel(
    const float* __restrict__ parts, const float* __restrict__ cparts, long long nplanes, int P, float weight,
    const float* base, float* spec4, float* total) {
  term_finalize<false>(parts, cparts, nplanes, (double)P, weight, base, spec4, total);  // L_spec = S / (Nused P)
}

__global__ void __launch_bounds__(kSpecThreads) spectral_loss_dy_kernel(const char* __restrict__ ws, SpecLossPlan plan,
                                                                        long long npix, int H, int W, int P, int Q,
                                                                        float weight, const float* __restrict__ spec4,
                                                                        float* __restrict__ dy) {
  const float scale = weight * spec4[2];
  const long long hw = (long long)H * W;
  for (long long o = (long long)blockIdx.x * kSpecThreads + threadIdx.x; o < npix;
       o += (long long)gridDim.x * kSpecThreads) {
    const long long plane = o / hw;
    const int r = (int)(o % hw), y = r / W, x = r % W;
    const char* pws = ws + (size_t)plane * plan.stride;
    const float* g = reinterpret_cast<const float*>(pws);
    const int* used = reinterpret_cast<const int*>(pws + plan.off_used);
    // the windows covering y: i Q + P > y from i = ceil((y - P + 1) / Q) on, while the
    // origin is <= y (the origins do not decrease, and the last, shifted one reaches L - 1)
    const int iy0 = y < P ? 0 : (y - P + Q) / Q, ix0 = x < P ? 0 : (x - P + Q) / Q;
    float acc = 0.0f;
    bool any = false;
    for (int iy = iy0; iy < plan.ny; ++iy) {
      const int y0 = spec_origin(iy, H, P, Q);
      if (y0 > y) break;
      for (int ix = ix0; ix < plan.nx; ++ix) {
        const int x0 = spec_origin(ix, W, P, Q);
        if (x0 > x) break;
        const int w = iy * plan.nx + ix;
        if (!used[w]) continue;
        any = true;
        acc += g[((size_t)w * P + (y - y0)) * P + (x - x0)];
      }
    }
    if (any) dy[o] = __fmaf_rn(scale, acc, dy[o]);  // one rounding
  }
}

}  // namespace
}  // namespace srmi

using namespace srmi;

extern "C" {

int srmi_spectral_loss_workspace(long long nplanes, int H, int W, int P, int Q, size_t* bytes) {
  SpecLossPlan p;
  if (!bytes) return SRMI_ERR_ARG;
  const int rc = spec_loss_plan(nplanes, H, W, P, Q, &p);
  if (rc) return rc;
  *bytes = (size_t)nplanes * p.stride;
  return 0;
}

int srmi_spectral_loss_parts(const float* pred, const float* target, long long nplanes, int H, int W, int P, int Q,
                             float eps, float* parts, float* cparts, void* ws, size_t ws_bytes, void* stream) {
  SpecLossPlan p;
  if (!pred || !target || !parts || !cparts || !ws || ((uintptr_t)ws & 15) != 0 || !(eps > 0.0f) || !std::isfinite(eps))
    return SRMI_ERR_ARG;
  const int rc = spec_loss_plan(nplanes, H, W, P, Q, &p);
  if (rc) return rc;
  if (ws_bytes < (size_t)nplanes * p.stride) return SRMI_ERR_ARG;
  const long long nunits = nplanes * ((p.nwin + 1) / 2);
  const int grid = (int)(nunits < kSpecLossGridCap ? nunits : kSpecLossGridCap);
  char* w = static_cast<char*>(ws);
  hipStream_t st = static_cast<hipStream_t>(stream);
#define SRMI_SPEC_LOSS_CASE(PP)                                                                               \
  case PP:                                                                                                    \
    hipLaunchKernelGGL(spectral_loss_window_kernel<PP>, dim3(grid), dim3(kSpecThreads), 0, st, pred, target, \
                       nplanes, H, W, Q, p.nx, p.nwin, eps, w, p);                                            \
    break
  switch (P) {
    SRMI_SPEC_LOSS_CASE(16);
    SRMI_SPEC_LOSS_CASE(32);
    SRMI_SPEC_LOSS_CASE(64);
    default:
      return SRMI_ERR_ARG;
  }
#undef SRMI_SPEC_LOSS_CASE
  SRMI_CHECK_LAUNCH();
  hipLaunchKernelGGL(spectral_loss_plane_kernel, dim3((unsigned)((nplanes + kSpecThreads - 1) / kSpecThreads)),
                     dim3(kSpecThreads), 0, st, w, p, nplanes, parts, cparts);
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_spectral_loss_from_parts(const float* parts, const float* cparts, long long nplanes, int P, float weight,
                                  const float* base, float* spec4, float* total, void* stream) {
  if (!parts || !cparts || !base || !spec4 || !total || nplanes < 1 || (P != 16 && P != 32 && P != 64) ||
      !(weight >= 0.0f) || !std::isfinite(weight))
    return SRMI_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(spectral_loss_finalize_kernel, dim3(1), dim3(kSpecThreads), 0, st, parts, cparts, nplanes, P,
                     weight, base, spec4, total);
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_spectral_loss_dy(const void* ws, size_t ws_bytes, long long nplanes, int H, int W, int P, int Q,
                          float weight, const float* spec4, float* dy, void* stream) {
  SpecLossPlan p;
  if (!ws || ((uintptr_t)ws & 15) != 0 || !spec4 || !dy || !(weight >= 0.0f) || !std::isfinite(weight)) return SRMI_ERR_ARG;
  const int rc = spec_loss_plan(nplanes, H, W, P, Q, &p);
  if (rc) return rc;
  if (ws_bytes < (size_t)nplanes * p.stride) return SRMI_ERR_ARG;
  if (weight == 0.0f) return 0;  // dy stays as it is, bit for bit
  const long long npix = nplanes * H * (long long)W;
  const long long blocks = (npix + kSpecThreads - 1) / kSpecThreads;
  const int grid = (int)(blocks < kSpecLossDyGridCap ? blocks : kSpecLossDyGridCap);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(spectral_loss_dy_kernel, dim3(grid), dim3(kSpecThreads), 0, st, static_cast<const char*>(ws), p,
                     npix, H, W, P, Q, weight, spec4, dy);
  SRMI_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
