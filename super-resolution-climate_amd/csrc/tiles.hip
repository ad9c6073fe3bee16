// Region <-> tile data path of tiled inference, device side.
//
// region_to_tiles replaces the floor tiling of get_tiles (reference
// sres/base/source/swot/raw.py:216-233) fused with the per-tile, per-channel
// 'lnorm' normalisation of norm() (raw.py:169-181: mean and std over (x, y),
// ddof 0, x' = (x - mean) / std).  One workgroup per (tile, channel): the 2-pass
// statistics are reduced in a fixed order, so the result is deterministic.
//
// batch_prep replaces the training-batch preparation: the
// 'lnorm' branch of norm() (raw.py:169-181) on a selected tile batch, xyflip
// (sres/base/source/batch.py:37-49, applied by load_batch :301) and the
// apply_network input downsample (array.py:72-76) -- one pass over HBM.
//
// batch_prep_norm / region_to_tiles_norm are the two above with the other five
// branches of norm() (raw.py:182-209), and tile_stats the statistics pass they
// need (_compute_normalization, raw.py:89-106, globalize_norm :23-30).
//
// llc_* replace SWOTRawDataLoader.load_file (swot/raw.py:133-145, mds2d
// swot/util.py:3-7, subset_roi raw.py:38-45) and tiles_nonfinite/tiles_gather
// the tiling of get_tiles (raw.py:216-233) -- SURVEY.md §8f row 3, see below.
//
// tiles_to_region replaces denorm (dual_trainer.py:67-77: x * std + mean) fused
// with assemble_images (dual_trainer.py:482-512: tile id -> grid cell
// (tid / gx, tid % gx), cells without a tile are NaN).
//
// region_to_tiles_overlap / tiles_blend generalise the cut and the mosaic to overlapping
// tiles and a feathered blend (srmi.superres).  The reference has no overlapped form.
//
// tiles_dihedral / tiles_blend_ensemble are the geometric self-ensemble of those tiles: the
// xyflip variants (batch.py:37-49) of every tile plane, and the mean and spread of their
// back-transformed, blended outputs.  The reference flips training batches only.
#include <math.h>

#include "common.hpp"
#include "srmi_internal.hpp"

namespace srmi {

__device__ __forceinline__ float block_sum256(float v, float* red) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  const float s = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return s;
}

// grid (C, ntiles): tile t = grid cell t (row-major over gy x gx), cut at the origin
// min(i * stride, length - tile) per axis -- the floor grid's i * tile when the stride is
// the tile (i < length / tile), the overlapped plan's (srmi_region_to_tiles_overlap) else
__global__ void __launch_bounds__(256) region_to_tiles_kernel(const float* __restrict__ region, int C, int H, int W,
                                                              int ty, int tx, int gx, int sy, int sx,
                                                              float* __restrict__ tiles, float* __restrict__ mean,
                                                              float* __restrict__ stdv, int* __restrict__ bad) {
  __shared__ float red[4];
  const int c = blockIdx.x, t = blockIdx.y;
  const int y0 = min((t / gx) * sy, H - ty), x0 = min((t % gx) * sx, W - tx);
  const float* src = region + (size_t)c * H * W + (size_t)y0 * W + x0;
  const int n = ty * tx;
  float s = 0.f;
  int nonfinite = 0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float v = src[(size_t)(i / tx) * W + (i % tx)];
    s += v;
    nonfinite |= !isfinite(v);
  }
  const float m = block_sum256(s, red) / (float)n;
  float q = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float d = src[(size_t)(i / tx) * W + (i % tx)] - m;
    q += d * d;
  }
  const float sd = sqrtf(block_sum256(q, red) / (float)n);
  const float inv = 1.f / sd;
  float* dst = tiles + ((size_t)t * C + c) * n;
  for (int i = threadIdx.x; i < n; i += 256) dst[i] = (src[(size_t)(i / tx) * W + (i % tx)] - m) * inv;
  const int anybad = __syncthreads_or(nonfinite);
  if (threadIdx.x == 0) {
    mean[(size_t)t * C + c] = m;
    stdv[(size_t)t * C + c] = sd;
    if (bad && anybad) atomicOr(&bad[t], 1);  // the reference drops tiles whose mean is not finite
  }
}

// The same with the tile held in registers: 1024 threads, float4 loads, every region
// element read once (the form above reads it three times with scalar loads: 157 us
// for the C5 region, 0.84 TB/s).  Needs tx, W multiples of 4 and ty * tx / 4 <= 1024 * KR.
constexpr int kR2tKR = 12;
__device__ __forceinline__ float block_sum1024(float v, float* red) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 16; i += 2) s += red[i] + red[i + 1];
  __syncthreads();
  return s;
}
__global__ void __launch_bounds__(1024) region_to_tiles_reg_kernel(const float* __restrict__ region, int C, int H,
                                                                   int W, int ty, int tx, int gx, int sy, int sx,
                                                                   float* __restrict__ tiles, float* __restrict__ mean,
                                                                   float* __restrict__ stdv, int* __restrict__ bad) {
  __shared__ float red[16];
  const int c = blockIdx.x, t = blockIdx.y;
  const int y0 = min((t / gx) * sy, H - ty), x0 = min((t % gx) * sx, W - tx);
  const float* src = region + (size_t)c * H * W + (size_t)y0 * W + x0;
  const int tx4 = tx >> 2, n4 = ty * tx4, n = ty * tx;
  float4 v[kR2tKR];
  float s = 0.f;
  int nonfinite = 0;
#pragma unroll
  for (int j = 0; j < kR2tKR; ++j) {
    const int i = threadIdx.x + j * 1024;
    v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < n4) {
      const int r = i / tx4, q = i - r * tx4;
      v[j] = *reinterpret_cast<const float4*>(src + (size_t)r * W + 4 * q);
      s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
      nonfinite |= !(isfinite(v[j].x) && isfinite(v[j].y) && isfinite(v[j].z) && isfinite(v[j].w));
    }
  }
  const float m = block_sum1024(s, red) / (float)n;
  float qs = 0.f;
#pragma unroll
  for (int j = 0; j < kR2tKR; ++j) {
    if (threadIdx.x + j * 1024 < n4) {
      const float a = v[j].x - m, b = v[j].y - m, cc = v[j].z - m, d = v[j].w - m;
      qs += (a * a + b * b) + (cc * cc + d * d);
    }
  }
  const float sd = sqrtf(block_sum1024(qs, red) / (float)n);
  const float inv = 1.f / sd;
  float4* dst = reinterpret_cast<float4*>(tiles + ((size_t)t * C + c) * n);
#pragma unroll
  for (int j = 0; j < kR2tKR; ++j) {
    const int i = threadIdx.x + j * 1024;
    if (i < n4) dst[i] = make_float4((v[j].x - m) * inv, (v[j].y - m) * inv, (v[j].z - m) * inv, (v[j].w - m) * inv);
  }
  const int anybad = __syncthreads_or(nonfinite);
  if (threadIdx.x == 0) {
    mean[(size_t)t * C + c] = m;
    stdv[(size_t)t * C + c] = sd;
    if (bad && anybad) atomicOr(&bad[t], 1);
  }
}

// gy x gx tiles at strides (sy, sx), the caller's validated plan.  The float4 form needs
// every tile origin on a 16-byte boundary: W, tx and the x stride multiples of 4 (the
// shifted last tile starts at W - tx).
static int region_to_tiles_plan_launch(const float* region, int C, int H, int W, int ty, int tx, int gy, int gx,
                                       int sy, int sx, float* tiles, float* mean, float* stdv, int* bad,
                                       hipStream_t st) {
  if (bad) {
    const hipError_t e = hipMemsetAsync(bad, 0, sizeof(int) * (size_t)gy * gx, st);
    if (e != hipSuccess) return -(int)e;
  }
  const bool reg = tx % 4 == 0 && W % 4 == 0 && sx % 4 == 0 && (size_t)ty * (tx / 4) <= (size_t)1024 * kR2tKR &&
                   ((uintptr_t)region & 15) == 0 && ((uintptr_t)tiles & 15) == 0;
  if (reg)
    hipLaunchKernelGGL(region_to_tiles_reg_kernel, dim3(C, gy * gx), dim3(1024), 0, st, region, C, H, W, ty, tx, gx,
                       sy, sx, tiles, mean, stdv, bad);
  else
    hipLaunchKernelGGL(region_to_tiles_kernel, dim3(C, gy * gx), dim3(256), 0, st, region, C, H, W, ty, tx, gx, sy,
                       sx, tiles, mean, stdv, bad);
  SRMI_CHECK_LAUNCH();
  return 0;
}

// out[c][Y][X] = tiles[inv[cell]][c][y][x] * std + mean, NaN where inv[cell] < 0
// (inv == NULL: tile i is grid cell i).  grid (ceil(gx*tx / 256), gy*ty, C)
__global__ void __launch_bounds__(256) tiles_to_region_kernel(const float* __restrict__ tiles,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ stdv,
                                                              const int* __restrict__ inv, int C, int ty, int tx,
                                                              int gx, float* __restrict__ out) {
  const int X = blockIdx.x * 256 + threadIdx.x, Y = blockIdx.y, c = blockIdx.z;
  const int Wo = gx * tx;
  if (X >= Wo) return;
  const int cell = (Y / ty) * gx + X / tx;
  const int t = inv ? inv[cell] : cell;
  float v = __int_as_float(0x7fc00000);  // NaN
  if (t >= 0) {
    const float z = tiles[(((size_t)t * C + c) * ty + (Y % ty)) * tx + (X % tx)];
    v = mean ? z * stdv[(size_t)t * C + c] + mean[(size_t)t * C + c] : z;
  }
  out[((size_t)c * gridDim.y + Y) * Wo + X] = v;
}

// the same, four pixels of one tile row per thread (tx % 4 == 0, 16-byte aligned):
// grid (ceil(gx tx / 1024), gy ty, C)
__global__ void __launch_bounds__(256) tiles_to_region_v4_kernel(const float* __restrict__ tiles,
                                                                 const float* __restrict__ mean,
                                                                 const float* __restrict__ stdv,
                                                                 const int* __restrict__ inv, int C, int ty, int tx,
                                                                 int gx, float* __restrict__ out) {
  const int X = (blockIdx.x * 256 + threadIdx.x) * 4, Y = blockIdx.y, c = blockIdx.z;
  const int Wo = gx * tx;
  if (X >= Wo) return;
  const int cell = (Y / ty) * gx + X / tx;
  const int t = inv ? inv[cell] : cell;
  const float nan = __int_as_float(0x7fc00000);
  float4 v = make_float4(nan, nan, nan, nan);
  if (t >= 0) {
    v = *reinterpret_cast<const float4*>(tiles + (((size_t)t * C + c) * ty + (Y % ty)) * tx + (X % tx));
    if (mean) {
      const float sd = stdv[(size_t)t * C + c], m = mean[(size_t)t * C + c];
      v = make_float4(v.x * sd + m, v.y * sd + m, v.z * sd + m, v.w * sd + m);
    }
  }
  *reinterpret_cast<float4*>(out + ((size_t)c * gridDim.y + Y) * Wo + X) = v;
}

// ------------------------------------------------------------------ batch prep
// One workgroup (1024 threads) per (channel, tile).  The raw tile is read from
// HBM once (float4) into LDS with a padded row pitch (T + 1: the transposed
// reads of flip index >= 4 walk columns without bank conflicts); mean and the
// 2-pass std (ddof 0) are fixed-order block reductions (deterministic) carried
// in fp64, and x - mean is formed in fp64: an fp32 mean of climate fields
// (|mean| ~ 300, ulp 3e-5) would shift a whole normalised tile by ~1e-5.  The
// normalised, flipped HR tile and its bicubic 1/scale LR are written from LDS.
// Tiles too large for LDS (T > 192, e.g. the EDSR x8 256^2 tiles) re-read the
// raw tile through L2 instead.
constexpr int kPrepThreads = 1024;

__device__ __forceinline__ double block_sum1024(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < kPrepThreads / 64; ++i) s += red[i];
  __syncthreads();
  return s;
}

// output pixel (y, x) of xyflip(...) reads source pixel (sy, sx) (square tiles):
// swap (bit 2) first, then flip y (bit 1), then flip x (bit 0) -- the inverse of
// the reference's flip-x, flip-y, transpose sequence.
// The h x w form serves srmi_tiles_dihedral: the flips alone (f < 4) keep a rectangular
// plane's shape, a swap needs h == w.
__device__ __forceinline__ void flip_src(int f, int h, int w, int y, int x, int& sy, int& sx) {
  sy = (f & 4) ? x : y;
  sx = (f & 4) ? y : x;
  if (f & 2) sy = h - 1 - sy;
  if (f & 1) sx = w - 1 - sx;
}
__device__ __forceinline__ void flip_src(int f, int T, int y, int x, int& sy, int& sx) {
  flip_src(f, T, T, y, x, sy, sx);
}

template <bool kLds>
__global__ void __launch_bounds__(kPrepThreads) batch_prep_kernel(const float* __restrict__ raw, int C, int T,
                                                                  int flip, int scale, float* __restrict__ hr,
                                                                  float* __restrict__ lr, float* __restrict__ mean,
                                                                  float* __restrict__ stdv) {
  extern __shared__ float tile[];  // [T][T + 1] when kLds
  __shared__ double red[kPrepThreads / 64];
  const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int n = T * T, P = kLds ? T + 1 : T;
  const float* src = raw + ((size_t)b * C + c) * n;
  const float* buf = kLds ? tile : src;
  double s = 0.0;
  for (int i = 4 * tid; i < n; i += 4 * kPrepThreads) {  // T even -> n % 4 == 0
    const float4 v = *reinterpret_cast<const float4*>(src + i);
    s += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
    if (kLds) {
      const int y = i / T, x = i - y * T;  // a float4 straddles two rows only if T % 4 == 2
      float* d = tile + y * P + x;
      if (x + 3 < T) {
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
      } else {
        const float vv[4] = {v.x, v.y, v.z, v.w};
        for (int e = 0; e < 4; ++e) {
          const int ye = (i + e) / T, xe = (i + e) - ye * T;
          tile[ye * P + xe] = vv[e];
        }
      }
    }
  }
  const double m = block_sum1024(s, red) / (double)n;  // (also orders the LDS stores)
  double q = 0.0;
  for (int i = tid; i < n; i += kPrepThreads) {
    const int y = i / T, x = i - y * T;
    const double d = (double)buf[y * P + x] - m;
    q += d * d;
  }
  const double sd = sqrt(block_sum1024(q, red) / (double)n);
  const double inv = 1.0 / sd;
  auto norm = [&](int y, int x) __attribute__((always_inline)) {
    int sy, sx;
    flip_src(flip, T, y, x, sy, sx);
    return (float)(((double)buf[sy * P + sx] - m) * inv);
  };
  float* dst = hr + ((size_t)b * C + c) * n;
  for (int i = 4 * tid; i < n; i += 4 * kPrepThreads) {
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int y = (i + e) / T, x = (i + e) - y * T;
      o[e] = norm(y, x);
    }
    *reinterpret_cast<float4*>(dst + i) = make_float4(o[0], o[1], o[2], o[3]);
  }
  if (lr) {
    // downsample_kernel's arithmetic (small.hip) on the normalised, flipped tile
    const int t = T / scale;
    const float k[4] = {-3.f / 32.f, 19.f / 32.f, 19.f / 32.f, -3.f / 32.f};
    float* ldst = lr + ((size_t)b * C + c) * t * t;
    for (int i = tid; i < t * t; i += kPrepThreads) {
      const int y = i / t, x = i - y * t;
      const int y0 = y * scale + scale / 2 - 2, x0 = x * scale + scale / 2 - 2;
      float acc = 0.f;
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const int yy = min(max(y0 + a, 0), T - 1);
        float rsum = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) rsum += k[j] * norm(yy, min(max(x0 + j, 0), T - 1));
        acc += k[a] * rsum;
      }
      ldst[i] = acc;
    }
  }
  if (tid == 0) {
    if (mean) mean[(size_t)b * C + c] = (float)m;
    if (stdv) stdv[(size_t)b * C + c] = (float)sd;
  }
}

// ------------------------------------------------- the other task.norm modes
// norm() has six branches (raw.py:169-214).  'lnorm' is the kernels above.
// 'lscale' is (x - min) / (max - min) of the tile; 'gnorm', 'gscale', 'tnorm' and
// 'tscale' are all (x - off) / div with one offset and one divisor per (tile,
// channel) taken from the dataset statistics (srmi.norm.NormStats.offsets): the
// AFFINE mode.  x - off is formed in fp64 for the reason given above
// batch_prep_kernel, the quotient as a product with the fp64 reciprocal (what that
// kernel does with 1 / std; within one fp32 ulp of the division rounded once).
// LSCALE divides by the exact fp64 max - min, so the tile's extremes come out as
// exactly 0 and 1, as the reference's fp32 (max - min) / (max - min) does; the
// divisor it reports is that difference rounded to fp32.
template <int kThreads>
__device__ __forceinline__ void block_minmax(float& mn, float& mx, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  constexpr int kW = kThreads / 64;
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[w] = mn;
    red[kW + w] = mx;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kW; ++i) {
    mn = fminf(mn, red[i]);
    mx = fmaxf(mx, red[kW + i]);
  }
  __syncthreads();
}

// batch_prep_kernel with the plane (b * C + c) on grid.x -- a whole time slice is
// one launch (srmi.norm.normalize_tiles) -- and the statistics of kMode.  The
// flipped HR tile and the LR tile are written exactly as there.
template <bool kLds, int kMode>
__global__ void __launch_bounds__(kPrepThreads) batch_prep_norm_kernel(const float* __restrict__ raw, int T, int flip,
                                                                       int scale, const float* __restrict__ off,
                                                                       const float* __restrict__ dv,
                                                                       float* __restrict__ hr, float* __restrict__ lr,
                                                                       float* __restrict__ off_out,
                                                                       float* __restrict__ div_out) {
  extern __shared__ float tile[];  // [T][T + 1] when kLds
  __shared__ float red[2 * kPrepThreads / 64];
  const size_t p = blockIdx.x;
  const int tid = threadIdx.x;
  const int n = T * T, P = kLds ? T + 1 : T;
  const float* src = raw + p * n;
  const float* buf = kLds ? tile : src;
  float mn = INFINITY, mx = -INFINITY;
  if (kLds || kMode == SRMI_NORM_LSCALE) {
    for (int i = 4 * tid; i < n; i += 4 * kPrepThreads) {  // T even -> n % 4 == 0
      const float4 v = *reinterpret_cast<const float4*>(src + i);
      if (kMode == SRMI_NORM_LSCALE) {
        mn = fminf(fminf(mn, v.x), fminf(v.y, fminf(v.z, v.w)));
        mx = fmaxf(fmaxf(mx, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
      }
      if (kLds) {
        const int y = i / T, x = i - y * T;
        if (x + 3 < T) {
          float* d = tile + y * P + x;
          d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        } else {  // T % 4 == 2: the float4 straddles two rows
          const float vv[4] = {v.x, v.y, v.z, v.w};
          for (int e = 0; e < 4; ++e) {
            const int ye = (i + e) / T, xe = (i + e) - ye * T;
            tile[ye * P + xe] = vv[e];
          }
        }
      }
    }
  }
  double o, inv;
  if (kMode == SRMI_NORM_LSCALE) {
    block_minmax<kPrepThreads>(mn, mx, red);  // (also orders the LDS stores)
    o = (double)mn;
    inv = 1.0 / ((double)mx - (double)mn);
  } else {
    if (kLds) __syncthreads();
    o = (double)off[p];
    inv = 1.0 / (double)dv[p];
  }
  auto norm = [&](int y, int x) __attribute__((always_inline)) {
    int sy, sx;
    flip_src(flip, T, y, x, sy, sx);
    return (float)(((double)buf[sy * P + sx] - o) * inv);
  };
  float* dst = hr + p * n;
  for (int i = 4 * tid; i < n; i += 4 * kPrepThreads) {
    float q[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int y = (i + e) / T, x = (i + e) - y * T;
      q[e] = norm(y, x);
    }
    *reinterpret_cast<float4*>(dst + i) = make_float4(q[0], q[1], q[2], q[3]);
  }
  if (lr) {
    // downsample_kernel's arithmetic (small.hip), tap order as in batch_prep_kernel
    const int t = T / scale;
    const float k[4] = {-3.f / 32.f, 19.f / 32.f, 19.f / 32.f, -3.f / 32.f};
    float* ldst = lr + p * t * t;
    for (int i = tid; i < t * t; i += kPrepThreads) {
      const int y = i / t, x = i - y * t;
      const int y0 = y * scale + scale / 2 - 2, x0 = x * scale + scale / 2 - 2;
      float acc = 0.f;
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const int yy = min(max(y0 + a, 0), T - 1);
        float rsum = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) rsum += k[j] * norm(yy, min(max(x0 + j, 0), T - 1));
        acc += k[a] * rsum;
      }
      ldst[i] = acc;
    }
  }
  if (kMode == SRMI_NORM_LSCALE && tid == 0) {
    if (off_out) off_out[p] = mn;
    if (div_out) div_out[p] = mx - mn;
  }
}

// float4s a thread of the register-resident forms below holds: a 192^2 plane over 1024
// threads (12, as region_to_tiles_reg_kernel, spills next to their fp64 arithmetic)
constexpr int kNormKR = 9;

// region_to_tiles_reg_kernel / region_to_tiles_kernel with the statistics of kMode;
// off / dv are indexed by (grid cell, channel).  kVec: the tile in registers, float4.
template <int kMode, bool kVec>
__global__ void __launch_bounds__(1024) region_to_tiles_norm_kernel(const float* __restrict__ region, int C, int H,
                                                                    int W, int ty, int tx, int gx, int sy, int sx,
                                                                    const float* __restrict__ off,
                                                                    const float* __restrict__ dv,
                                                                    float* __restrict__ tiles,
                                                                    float* __restrict__ off_out,
                                                                    float* __restrict__ div_out,
                                                                    int* __restrict__ bad) {
  __shared__ float red[32];
  const int c = blockIdx.x, t = blockIdx.y;
  const int y0 = min((t / gx) * sy, H - ty), x0 = min((t % gx) * sx, W - tx);
  const float* src = region + (size_t)c * H * W + (size_t)y0 * W + x0;
  const int tx4 = tx >> 2, n4 = ty * tx4, n = ty * tx;
  const size_t p = (size_t)t * C + c;
  float4 v[kVec ? kNormKR : 1];
  float mn = INFINITY, mx = -INFINITY;
  int nonfinite = 0;
  if (kVec) {
#pragma unroll
    for (int j = 0; j < kNormKR; ++j) {
      const int i = threadIdx.x + j * 1024;
      v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (i < n4) {
        const int r = i / tx4, q = i - r * tx4;
        v[j] = *reinterpret_cast<const float4*>(src + (size_t)r * W + 4 * q);
        mn = fminf(fminf(mn, v[j].x), fminf(v[j].y, fminf(v[j].z, v[j].w)));
        mx = fmaxf(fmaxf(mx, v[j].x), fmaxf(v[j].y, fmaxf(v[j].z, v[j].w)));
        nonfinite |= !(isfinite(v[j].x) && isfinite(v[j].y) && isfinite(v[j].z) && isfinite(v[j].w));
      }
    }
  } else {
    for (int i = threadIdx.x; i < n; i += 1024) {
      const float a = src[(size_t)(i / tx) * W + (i % tx)];
      mn = fminf(mn, a);
      mx = fmaxf(mx, a);
      nonfinite |= !isfinite(a);
    }
  }
  double o, inv;
  if (kMode == SRMI_NORM_LSCALE) {
    block_minmax<1024>(mn, mx, red);
    o = (double)mn;
    inv = 1.0 / ((double)mx - (double)mn);
  } else {
    o = (double)off[p];
    inv = 1.0 / (double)dv[p];
  }
  auto norm = [&](float a) __attribute__((always_inline)) { return (float)(((double)a - o) * inv); };
  if (kVec) {
    float4* dst = reinterpret_cast<float4*>(tiles + p * n);
#pragma unroll
    for (int j = 0; j < kNormKR; ++j) {
      const int i = threadIdx.x + j * 1024;
      if (i < n4) dst[i] = make_float4(norm(v[j].x), norm(v[j].y), norm(v[j].z), norm(v[j].w));
    }
  } else {
    float* dst = tiles + p * n;
    for (int i = threadIdx.x; i < n; i += 1024) dst[i] = norm(src[(size_t)(i / tx) * W + (i % tx)]);
  }
  const int anybad = __syncthreads_or(nonfinite);
  if (threadIdx.x == 0) {
    if (kMode == SRMI_NORM_LSCALE) {
      if (off_out) off_out[p] = mn;
      if (div_out) div_out[p] = mx - mn;
    }
    if (bad && anybad) atomicOr(&bad[t], 1);  // as region_to_tiles_kernel: the flag of a dropped tile
  }
}

// LSCALE / AFFINE over gy x gx tiles at strides (sy, sx); the float4 form as in
// region_to_tiles_plan_launch
static int region_to_tiles_norm_plan_launch(const float* region, int C, int H, int W, int ty, int tx, int gy, int gx,
                                            int sy, int sx, int mode, const float* off, const float* dv, float* tiles,
                                            float* off_out, float* div_out, int* bad, hipStream_t st) {
  if (bad) {
    const hipError_t e = hipMemsetAsync(bad, 0, sizeof(int) * (size_t)gy * gx, st);
    if (e != hipSuccess) return -(int)e;
  }
  const bool vec = tx % 4 == 0 && W % 4 == 0 && sx % 4 == 0 && (size_t)ty * (tx / 4) <= (size_t)1024 * kNormKR &&
                   ((uintptr_t)region & 15) == 0 && ((uintptr_t)tiles & 15) == 0;
  const dim3 grid(C, gy * gx), block(1024);
#define SRMI_R2T_NORM(MODE, VEC)                                                                                 \
  hipLaunchKernelGGL((region_to_tiles_norm_kernel<MODE, VEC>), grid, block, 0, st, region, C, H, W, ty, tx, gx, sy, \
                     sx, off, dv, tiles, off_out, div_out, bad)
  if (mode == SRMI_NORM_LSCALE) {
    if (vec) SRMI_R2T_NORM(SRMI_NORM_LSCALE, true);
    else SRMI_R2T_NORM(SRMI_NORM_LSCALE, false);
  } else {
    if (vec) SRMI_R2T_NORM(SRMI_NORM_AFFINE, true);
    else SRMI_R2T_NORM(SRMI_NORM_AFFINE, false);
  }
#undef SRMI_R2T_NORM
  SRMI_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------ overlapped tiles, blended mosaic
// No reference counterpart: get_tiles (raw.py:216-233) cuts the disjoint floor grid and
// assemble_images (dual_trainer.py:482-512) concatenates it.  Here an axis of length L
// is covered by n = ceil((L - t) / S) + 1 tiles of size t at stride S (1 <= S <= t <= L),
// tile i at the origin min(i S, L - t): the last tile is shifted inward, so the axis is
// covered completely.  Three scalars per axis are the whole plan; the kernels compute
// the origins themselves.
int overlap_count(long long L, long long t, long long S) {
  if (S < 1 || t < S || L < t || L > 0x7fffffffLL) return SRMI_ERR_ARG;
  const long long n = (L - t + S - 1) / S + 1;
  return n > 0x7fffffffLL ? SRMI_ERR_ARG : (int)n;
}

// the tiles i with origin(i) <= p < origin(i) + t are lo .. hi, without a gap: tiles
// 0 .. n-2 sit at i S < L - t, the last one at L - t
__device__ __forceinline__ void overlap_cover(int p, int L, int t, int S, int n, int& lo, int& hi) {
  lo = p < t ? 0 : min((p - t) / S + 1, n - 1);
  hi = p >= L - t ? n - 1 : p / S;
}
// blend weight at tile-local position q: the integer ramp min(q + 1, t - q, R + 1) with
// R = t - S, so two regularly overlapping tiles weigh (R - q) / (R + 1) and (q + 1) /
// (R + 1) across their overlap (never zero), and R = 0 weighs everything 1
__device__ __forceinline__ int overlap_weight(int q, int t, int R) { return min(min(q + 1, t - q), R + 1); }
// the de-normalisation of a tile value, one expression for tiles_blend_kernel and
// tiles_blend_ensemble_kernel: whatever the compiler makes of it, it makes in both
__device__ __forceinline__ float blend_denorm(float x, float sd, float m) { return x * sd + m; }

// out[c][Y][X] = sum_k w_k v_k / sum_k w_k over the non-bad tiles k covering (Y, X), v =
// tile value * div + off (off == NULL: as stored), w = wy wx.  Gather form: a thread owns
// kV pixels of one row and walks the covering tiles in ascending (iy, ix) order (up to
// ceil(t / S) + 1 per axis), fp32 sums, integer weight sums, one division -- no atomics,
// deterministic.  A bad tile is skipped before anything of it is read; no cover left: NaN;
// exactly one: its value, copied (so S == T on a divisible region is tiles_to_region,
// bit for bit).  kV == 4: Tx, Sx, Wo multiples of 4 put every tile edge on a quad
// boundary, so the quad has one cover and its tile rows are 16-byte aligned.
// grid (ceil(Wo / kV / 256), Ho, C)
// kMask (srmi_tiles_blend_masked): a pixel whose parent mask_src[c][Y / scale][X / scale]
// is not finite is the canonical NaN, decided before any tile is read; every other pixel
// runs the code below unchanged.  kV == 4 there also needs scale % 4 == 0: the quad then
// has one parent.
template <int kV, bool kMask>
__global__ void __launch_bounds__(256) tiles_blend_kernel(const float* __restrict__ tiles,
                                                          const float* __restrict__ off,
                                                          const float* __restrict__ dv, const int* __restrict__ bad,
                                                          int C, int Ty, int Tx, int Sy, int Sx, int ny, int nx,
                                                          int Ho, int Wo, const float* __restrict__ mask_src,
                                                          int scale, float* __restrict__ out) {
  const int X = (blockIdx.x * 256 + threadIdx.x) * kV, Y = blockIdx.y, c = blockIdx.z;
  if (X >= Wo) return;
  if constexpr (kMask) {
    if (!isfinite(mask_src[((size_t)c * (Ho / scale) + Y / scale) * (Wo / scale) + X / scale])) {
      const float nan = __int_as_float(0x7fc00000);
      float* dst = out + ((size_t)c * Ho + Y) * Wo + X;
      if constexpr (kV == 4) *reinterpret_cast<float4*>(dst) = make_float4(nan, nan, nan, nan);
      else dst[0] = nan;
      return;
    }
  }
  const int Ry = Ty - Sy, Rx = Tx - Sx;
  int ylo, yhi, xlo, xhi;
  overlap_cover(Y, Ho, Ty, Sy, ny, ylo, yhi);
  overlap_cover(X, Wo, Tx, Sx, nx, xlo, xhi);
  float acc[kV], one[kV];
  int wsum[kV], cnt = 0;
#pragma unroll
  for (int e = 0; e < kV; ++e) {
    acc[e] = 0.f;
    one[e] = 0.f;
    wsum[e] = 0;
  }
  for (int iy = ylo; iy <= yhi; ++iy) {
    const int qy = Y - min(iy * Sy, Ho - Ty);
    const int wy = overlap_weight(qy, Ty, Ry);
    for (int ix = xlo; ix <= xhi; ++ix) {
      const int t = iy * nx + ix;
      if (bad && bad[t]) continue;
      const int qx = X - min(ix * Sx, Wo - Tx);
      const size_t p = (size_t)t * C + c;
      const float* src = tiles + (p * Ty + qy) * Tx + qx;
      float v[kV];
      if constexpr (kV == 4) {
        const float4 f = *reinterpret_cast<const float4*>(src);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
      } else {
        v[0] = src[0];
      }
      if (off) {
        const float sd = dv[p], m = off[p];
#pragma unroll
        for (int e = 0; e < kV; ++e) v[e] = blend_denorm(v[e], sd, m);
      }
      ++cnt;
#pragma unroll
      for (int e = 0; e < kV; ++e) {
        const int w = wy * overlap_weight(qx + e, Tx, Rx);
        acc[e] = fmaf((float)w, v[e], acc[e]);
        wsum[e] += w;
        one[e] = v[e];
      }
    }
  }
  float r[kV];
#pragma unroll
  for (int e = 0; e < kV; ++e)
    r[e] = cnt == 0 ? __int_as_float(0x7fc00000) : cnt == 1 ? one[e] : acc[e] / (float)wsum[e];
  float* dst = out + ((size_t)c * Ho + Y) * Wo + X;
  if constexpr (kV == 4) *reinterpret_cast<float4*>(dst) = make_float4(r[0], r[1], r[2], r[3]);
  else dst[0] = r[0];
}

// mask_src == NULL: srmi_tiles_blend; else srmi_tiles_blend_masked (scale >= 1 divides Ho, Wo)
static int tiles_blend_any_launch(const float* tiles, const float* off, const float* dv, const int* bad, int C, int Ty,
                                  int Tx, int Sy, int Sx, int Ho, int Wo, const float* mask_src, int scale, float* out,
                                  hipStream_t st) {
  if (C < 1 || C > 65535) return SRMI_ERR_ARG;  // grid.z
  const int ny = overlap_count(Ho, Ty, Sy), nx = overlap_count(Wo, Tx, Sx);
  if (ny < 0 || nx < 0) return SRMI_ERR_ARG;
  // grid.y; the tile index and a pixel's integer weight sum (at most t / S + 2 covering
  // tiles per axis, each weighing at most R + 1 there) stay in int
  const long long wy = (long long)(Ty / Sy + 2) * (Ty - Sy + 1), wx = (long long)(Tx / Sx + 2) * (Tx - Sx + 1);
  if (Ho > 65535 || (long long)ny * nx > 0x7fffffffLL || wy * wx > 0x7fffffffLL) return SRMI_ERR_SHAPE;
  if (!tiles || !out || (off && !dv)) return SRMI_ERR_ARG;
  const bool vec = Tx % 4 == 0 && Sx % 4 == 0 && Wo % 4 == 0 && ((uintptr_t)tiles & 15) == 0 &&
                   ((uintptr_t)out & 15) == 0 && (!mask_src || scale % 4 == 0);
#define SRMI_BLEND(V, MASK)                                                                                          \
  hipLaunchKernelGGL((tiles_blend_kernel<V, MASK>), dim3((Wo / V + 255) / 256, Ho, C), dim3(256), 0, st, tiles, off, \
                     dv, bad, C, Ty, Tx, Sy, Sx, ny, nx, Ho, Wo, mask_src, scale, out)
  if (mask_src) {
    if (vec) SRMI_BLEND(4, true);
    else SRMI_BLEND(1, true);
  } else {
    if (vec) SRMI_BLEND(4, false);
    else SRMI_BLEND(1, false);
  }
#undef SRMI_BLEND
  SRMI_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------ geometric self-ensemble (the "+" variant)
// No reference counterpart.  The model runs on the dihedral variants of every tile --
// variant f is xyflip's (flip_src above: bit 0 flips x, bit 1 flips y, bit 2 swaps the
// axes), a bit mask selects which, stored in ascending f -- and the blend averages the
// back-transformed outputs and takes their spread.
//
// tiles_dihedral: in [nplanes][h][w] -> out [K][nplanes][h][w], a pure permutation.  One
// workgroup owns one 64 x 64 block of one SOURCE plane: the block is read from HBM once,
// row by row, into LDS with a padded pitch (65: the column walks of the swapping variants
// hit distinct banks), and written once per variant to where that variant puts it, row by
// row again -- no lane walks a column of HBM.  The plane index shares grid.x with the
// blocks (a region's K n C planes do not fit grid.y).
constexpr int kDihB = 64, kDihP = kDihB + 1;

template <bool kVec>
__global__ void __launch_bounds__(256) tiles_dihedral_kernel(const float* __restrict__ in, int h, int w, int nby,
                                                             int nbx, int variants, size_t slab,
                                                             float* __restrict__ out) {
  __shared__ float blk[kDihB * kDihP];
  const int bid = (int)blockIdx.x, tid = threadIdx.x;
  const int bx = bid % nbx, by = (bid / nbx) % nby;
  const size_t plane = (size_t)(bid / (nbx * nby)) * h * w;
  const int y0 = by * kDihB, x0 = bx * kDihB;
  const int bh = min(kDihB, h - y0), bw = min(kDihB, w - x0);
  const float* src = in + plane;
  if (kVec) {  // w % 4 == 0: x0 and bw are multiples of 4
    const int bw4 = bw >> 2;
    for (int i = tid; i < bh * bw4; i += 256) {
      const int r = i / bw4, q = i - r * bw4;
      const float4 v = *reinterpret_cast<const float4*>(src + (size_t)(y0 + r) * w + x0 + 4 * q);
      float* d = blk + r * kDihP + 4 * q;
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
  } else {
    for (int i = tid; i < bh * bw; i += 256) {
      const int r = i / bw, q = i - r * bw;
      blk[r * kDihP + q] = src[(size_t)(y0 + r) * w + x0 + q];
    }
  }
  __syncthreads();
  int j = 0;
  for (int rem = variants; rem; rem &= rem - 1, ++j) {
    const int f = __ffs(rem) - 1;
    // where the block lands: the inverse of flip_src on its corner (a swap has h == w)
    const int a0 = (f & 2) ? h - y0 - bh : y0, b0 = (f & 1) ? w - x0 - bw : x0;
    const int oy0 = (f & 4) ? b0 : a0, ox0 = (f & 4) ? a0 : b0;
    const int oh = (f & 4) ? bw : bh, ow = (f & 4) ? bh : bw;
    float* dst = out + (size_t)j * slab + plane;
    if (kVec) {  // h == w for a swap, so ox0 and ow are multiples of 4 there too
      const int ow4 = ow >> 2;
      for (int i = tid; i < oh * ow4; i += 256) {
        const int r = i / ow4, q = i - r * ow4;
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          int sy, sx;
          flip_src(f, h, w, oy0 + r, ox0 + 4 * q + e, sy, sx);
          o[e] = blk[(sy - y0) * kDihP + (sx - x0)];
        }
        *reinterpret_cast<float4*>(dst + (size_t)(oy0 + r) * w + ox0 + 4 * q) = make_float4(o[0], o[1], o[2], o[3]);
      }
    } else {
      for (int i = tid; i < oh * ow; i += 256) {
        const int r = i / ow, q = i - r * ow;
        int sy, sx;
        flip_src(f, h, w, oy0 + r, ox0 + q, sy, sx);
        dst[(size_t)(oy0 + r) * w + ox0 + q] = blk[(sy - y0) * kDihP + (sx - x0)];
      }
    }
  }
}

// kV values of slab `s` ([Ty][Tx], stored in variant f's frame) at tile-local (qy, qx ..
// qx + kV - 1) of the back-transformed tile: the inverse of flip_src.  kV == 4 (qx, Tx
// multiples of 4): one float4 for the variants that keep the axes (reversed where x is
// flipped), four reads down one column for those that swap them.
template <int kV>
__device__ __forceinline__ void ensemble_read(const float* __restrict__ s, int f, int Ty, int Tx, int qy, int qx,
                                              float (&v)[kV]) {
  const int a = (f & 2) ? Ty - 1 - qy : qy;
  if (f & 4) {  // (y, x) = (b, a), Ty == Tx
#pragma unroll
    for (int e = 0; e < kV; ++e) {
      const int b = (f & 1) ? Tx - 1 - (qx + e) : qx + e;
      v[e] = s[(size_t)b * Tx + a];
    }
  } else if constexpr (kV == 4) {
    const float4 q = *reinterpret_cast<const float4*>(s + (size_t)a * Tx + ((f & 1) ? Tx - 4 - qx : qx));
    if (f & 1) {
      v[0] = q.w; v[1] = q.z; v[2] = q.y; v[3] = q.x;
    } else {
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
  } else {
    v[0] = s[(size_t)a * Tx + ((f & 1) ? Tx - 1 - qx : qx)];
  }
}

// a[0] + .. + a[K - 1] in fp32, ascending j, added pairwise: ((a0 + a1) + (a2 + a3)) +
// ((a4 + a5) + (a6 + a7)) with the terms j >= K left out (not added as zeros: -0 stays -0).
// K equal values then sum to K times the value exactly for K = 1, 2, 4, 8, so identical
// variants average to themselves bit for bit (a running sum rounds at 3 x, 5 x, 7 x).
__device__ __forceinline__ float ensemble_sum(const float (&a)[8], int K) {
  const float s01 = K > 1 ? __fadd_rn(a[0], a[1]) : a[0], s23 = K > 3 ? __fadd_rn(a[2], a[3]) : a[2];
  const float s45 = K > 5 ? __fadd_rn(a[4], a[5]) : a[4], s67 = K > 7 ? __fadd_rn(a[6], a[7]) : a[6];
  const float s03 = K > 2 ? __fadd_rn(s01, s23) : s01, s47 = K > 6 ? __fadd_rn(s45, s67) : s45;
  return K > 4 ? __fadd_rn(s03, s47) : s03;
}

// tiles [K][ny*nx][C][Ty][Tx]: per output pixel and slab j the value B_j of
// tiles_blend_kernel on the back-transformed slab -- the same cover, weights, order, fmaf
// chain, copy at one cover and division, the read address alone differs -- then in fp32
// (ensemble_sum) mean = (B_0 + ...) / K and spread = sqrtf(((B_0 - mean)^2 + ...) / K).  The
// covering tiles are the outer loop (weights, bad flags, off and div are shared by the
// variants), the K slabs the inner one; the K accumulators live in registers.
// A workgroup owns 16 output rows x 16 kV pixels.  kV == 4: a wave is all 16 rows of four
// neighbouring quads (lane = row + 16 quad), so a load of a slab that keeps the axes
// covers 16 rows x 64 bytes and each of the four column reads of a swapped slab 4 rows x
// 64 bytes -- whole 64-byte segments either way, where the row-per-workgroup footprint of
// tiles_blend_kernel would walk a swapped slab as 64 dwords a row pitch apart.  kV == 1:
// a wave is 8 x 8 pixels, 32-byte runs for both kinds.
// grid (ceil(Wo / kV / 16), ceil(Ho / 16), C)
template <int kV, bool kMask>
__global__ void __launch_bounds__(256) tiles_blend_ensemble_kernel(
    const float* __restrict__ tiles, int variants, int K, const float* __restrict__ off, const float* __restrict__ dv,
    const int* __restrict__ bad, int C, int Ty, int Tx, int Sy, int Sx, int ny, int nx, int Ho, int Wo,
    const float* __restrict__ mask_src, int scale, float* __restrict__ mean, float* __restrict__ spread) {
  const int l = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int ly = kV == 4 ? (l & 15) : 8 * (wv >> 1) + (l & 7);
  const int lx = kV == 4 ? 4 * wv + (l >> 4) : 8 * (wv & 1) + (l >> 3);
  const int X = (blockIdx.x * 16 + lx) * kV, Y = blockIdx.y * 16 + ly, c = blockIdx.z;
  if (X >= Wo || Y >= Ho) return;
  const float nan = __int_as_float(0x7fc00000);
  const size_t o = ((size_t)c * Ho + Y) * Wo + X;
  if constexpr (kMask) {
    if (!isfinite(mask_src[((size_t)c * (Ho / scale) + Y / scale) * (Wo / scale) + X / scale])) {
      if constexpr (kV == 4) {
        *reinterpret_cast<float4*>(mean + o) = make_float4(nan, nan, nan, nan);
        if (spread) *reinterpret_cast<float4*>(spread + o) = make_float4(nan, nan, nan, nan);
      } else {
        mean[o] = nan;
        if (spread) spread[o] = nan;
      }
      return;
    }
  }
  const int Ry = Ty - Sy, Rx = Tx - Sx;
  const size_t slab = (size_t)ny * nx * C * Ty * Tx;
  int ylo, yhi, xlo, xhi;
  overlap_cover(Y, Ho, Ty, Sy, ny, ylo, yhi);
  overlap_cover(X, Wo, Tx, Sx, nx, xlo, xhi);
  float acc[8][kV], one[8][kV];
  int wsum[kV], cnt = 0;
#pragma unroll
  for (int e = 0; e < kV; ++e) wsum[e] = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
#pragma unroll
    for (int e = 0; e < kV; ++e) {
      acc[j][e] = 0.f;
      one[j][e] = 0.f;
    }
  }
  for (int iy = ylo; iy <= yhi; ++iy) {
    const int qy = Y - min(iy * Sy, Ho - Ty);
    const int wy = overlap_weight(qy, Ty, Ry);
    for (int ix = xlo; ix <= xhi; ++ix) {
      const int t = iy * nx + ix;
      if (bad && bad[t]) continue;
      const int qx = X - min(ix * Sx, Wo - Tx);
      const size_t p = (size_t)t * C + c;
      const float* src = tiles + p * Ty * Tx;
      float sd = 1.f, m = 0.f;
      if (off) {
        sd = dv[p];
        m = off[p];
      }
      int w[kV];
#pragma unroll
      for (int e = 0; e < kV; ++e) {
        w[e] = wy * overlap_weight(qx + e, Tx, Rx);
        wsum[e] += w[e];
      }
      ++cnt;
      int rem = variants;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (j < K) {
          const int f = __ffs(rem) - 1;
          rem &= rem - 1;
          float v[kV];
          ensemble_read<kV>(src + (size_t)j * slab, f, Ty, Tx, qy, qx, v);
          if (off) {
#pragma unroll
            for (int e = 0; e < kV; ++e) v[e] = blend_denorm(v[e], sd, m);
          }
#pragma unroll
          for (int e = 0; e < kV; ++e) {
            acc[j][e] = fmaf((float)w[e], v[e], acc[j][e]);
            one[j][e] = v[e];
          }
        }
      }
    }
  }
  float mu[kV], sp[kV];
  const float fk = (float)K;
#pragma unroll
  for (int e = 0; e < kV; ++e) {
    float B[8], D[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) B[j] = j >= K ? 0.f : cnt == 1 ? one[j][e] : acc[j][e] / (float)wsum[e];
    mu[e] = ensemble_sum(B, K) / fk;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float d = __fsub_rn(B[j], mu[e]);
      D[j] = __fmul_rn(d, d);
    }
    sp[e] = sqrtf(ensemble_sum(D, K) / fk);
    if (cnt == 0) mu[e] = sp[e] = nan;  // no cover left: the canonical NaN, as tiles_blend_kernel
  }
  if constexpr (kV == 4) {
    *reinterpret_cast<float4*>(mean + o) = make_float4(mu[0], mu[1], mu[2], mu[3]);
    if (spread) *reinterpret_cast<float4*>(spread + o) = make_float4(sp[0], sp[1], sp[2], sp[3]);
  } else {
    mean[o] = mu[0];
    if (spread) spread[o] = sp[0];
  }
}

// ------------------------------------------------------ dataset tile statistics
// _compute_normalization (raw.py:89-106) walks every (tile, variable) plane of every
// time slice on the host: NormData.add_entry (raw.py:55-60) appends the plane's mean
// and variance and folds its max and min.  Here one workgroup owns one plane of the
// [n][C][ty][tx] tensor srmi.llc.get_tiles returns: the plane is read from HBM once
// (float4) and held in registers, mean and the 2-pass variance (ddof 0) are fp64
// fixed-order block reductions (as batch_prep_kernel, and for its reason), and the
// owner adds them to its acc row {sum of means, sum of variances, max, min} with plain
// stores: no atomics, so the result does not depend on the schedule.  The plane index
// is on grid.x (a time slice at 16^2 tiles has ~875 000 planes).
template <int kThreads>
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  constexpr int kW = kThreads / 64;
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < kW; ++i) s += red[i];
  __syncthreads();
  return s;
}

__device__ __forceinline__ void tile_stats_commit(double* __restrict__ a, int first, double m, double var, float mn,
                                                  float mx) {
  // first: the row is initialised (max from -inf, min from +inf), whatever it held
  a[0] = first ? m : a[0] + m;
  a[1] = first ? var : a[1] + var;
  a[2] = first ? (double)mx : fmax(a[2], (double)mx);
  a[3] = first ? (double)mn : fmin(a[3], (double)mn);
}

// n4 = plane elements / 4 <= kThreads * kPer
template <int kThreads, int kPer>
__global__ void __launch_bounds__(kThreads) tile_stats_reg_kernel(const float* __restrict__ tiles, int n4,
                                                                  double* __restrict__ acc, int first) {
  __shared__ double red[kThreads / 64];
  __shared__ float redf[2 * kThreads / 64];
  const size_t p = blockIdx.x;
  const float4* src = reinterpret_cast<const float4*>(tiles + p * 4 * n4);
  float4 v[kPer];
  double s = 0.0;
  float mn = INFINITY, mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int i = threadIdx.x + j * kThreads;
    if (i < n4) {
      v[j] = src[i];
      s += ((double)v[j].x + (double)v[j].y) + ((double)v[j].z + (double)v[j].w);
      mn = fminf(fminf(mn, v[j].x), fminf(v[j].y, fminf(v[j].z, v[j].w)));
      mx = fmaxf(fmaxf(mx, v[j].x), fmaxf(v[j].y, fmaxf(v[j].z, v[j].w)));
    }
  }
  const double nn = 4.0 * (double)n4;
  const double m = block_sum_f64<kThreads>(s, red) / nn;
  double q = 0.0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    if (threadIdx.x + j * kThreads < n4) {
      const double a = (double)v[j].x - m, b = (double)v[j].y - m, c = (double)v[j].z - m, d = (double)v[j].w - m;
      q += (a * a + b * b) + (c * c + d * d);
    }
  }
  const double var = block_sum_f64<kThreads>(q, red) / nn;
  block_minmax<kThreads>(mn, mx, redf);
  if (threadIdx.x == 0) tile_stats_commit(acc + p * 4, first, m, var, mn, mx);
}

// any plane size or alignment: scalar loads, the variance pass re-reads the plane (L2)
__global__ void __launch_bounds__(256) tile_stats_kernel(const float* __restrict__ tiles, int n,
                                                         double* __restrict__ acc, int first) {
  __shared__ double red[4];
  __shared__ float redf[8];
  const size_t p = blockIdx.x;
  const float* src = tiles + p * n;
  double s = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float a = src[i];
    s += (double)a;
    mn = fminf(mn, a);
    mx = fmaxf(mx, a);
  }
  const double m = block_sum_f64<256>(s, red) / (double)n;
  double q = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double d = (double)src[i] - m;
    q += d * d;
  }
  const double var = block_sum_f64<256>(q, red) / (double)n;
  block_minmax<256>(mn, mx, redf);
  if (threadIdx.x == 0) tile_stats_commit(acc + p * 4, first, m, var, mn, mx);
}

// get_norm_stats (raw.py:62-63): row (tile, channel) -> {mean of the means, mean of
// the variances, max, min}, the reference's STATS order
__global__ void __launch_bounds__(256) tile_stats_rows_kernel(const double* __restrict__ acc, long long rows,
                                                              double ntimes, float* __restrict__ tstats) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const double* a = acc + r * 4;
  *reinterpret_cast<float4*>(tstats + r * 4) =
      make_float4((float)(a[0] / ntimes), (float)(a[1] / ntimes), (float)a[2], (float)a[3]);
}

// globalize_norm (raw.py:23-30) of channel c = blockIdx.x: each thread folds its tiles
// t = tid, tid + 1024, ... in order, then fixed-order block reductions.  One workgroup
// (one CU) per channel walks all n rows at a stride of C * 32 bytes: 28 MB at the
// 874 800 tiles of an LLC4320 time slice at 16^2.  It runs once per dataset and keeps
// the order fixed; its time at that size was not measured.
__global__ void __launch_bounds__(1024) tile_stats_global_kernel(const double* __restrict__ acc, long long n, int C,
                                                                 double ntimes, float* __restrict__ gstats) {
  __shared__ double red[16];
  __shared__ float redf[32];
  const int c = blockIdx.x;
  double sm = 0.0, sv = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  for (long long t = threadIdx.x; t < n; t += 1024) {
    const double* a = acc + (t * C + c) * 4;
    sm += a[0] / ntimes;
    sv += a[1] / ntimes;
    mx = fmaxf(mx, (float)a[2]);  // max / min are fp32 values held in fp64: exact
    mn = fminf(mn, (float)a[3]);
  }
  sm = block_sum_f64<1024>(sm, red);
  sv = block_sum_f64<1024>(sv, red);
  block_minmax<1024>(mn, mx, redf);
  if (threadIdx.x == 0)
    *reinterpret_cast<float4*>(gstats + 4 * c) = make_float4((float)(sm / (double)n), (float)(sv / (double)n), mx, mn);
}

// --------------------------------------------------- land-aware overlapped cut
// No reference counterpart: get_tiles (raw.py:216-233) drops every tile that holds a
// non-finite value, and so does region_to_tiles_overlap above.  Here the non-finite
// ("dry": land, ice) pixels of a tile are masked out of its statistics and filled from
// the wet ones, so a coastal tile rides through the forward like any other; the masked
// blend puts the NaN back.  One workgroup (1024 threads) per (channel, tile), grid
// (C, ny * nx) as the unmasked cut.  The plane is read from HBM once into LDS (values
// fp32 + a 16-bit pass stamp per pixel: 6 bytes a pixel, 54 KiB at 96 x 96; planes of more
// than kLandMaxPix pixels are refused), normalised there, filled there, written once.
//
// Statistics over the wet pixels only.  LNORM: mean and the 2-pass variance (ddof 0, over
// nwet) are fp64 fixed-order block reductions (block_sum_f64, as tile_stats and
// batch_prep), x - mean is formed in fp64 and multiplied by the fp64 1 / std --
// deliberately NOT the fp32 two-pass of region_to_tiles_kernel: a coastal tile's few wet
// pixels sit far from 0, where an fp32 mean costs the most.  LSCALE / AFFINE: the
// arithmetic of region_to_tiles_norm_kernel, so an all-finite region gives its bits.
//
// Fill, in normalised space (the neighbour averaging of ocean regridding tools): pass
// j = 1, 2, ... gives every pixel not filled before pass j that has a filled 8-neighbour
// inside the tile the mean of those neighbours -- fp32 adds from 0.0f in the order
// (-1,-1) (-1,0) (-1,1) (0,-1) (0,1) (1,-1) (1,0) (1,1), one fp32 multiply by
// kLandRecip[count - 1] -- and stamps it j.  A neighbour counts iff its stamp < j, so the
// update is Jacobi though it runs in place: a pixel stamped j in this pass is ignored by
// the others whether they see the stamp before or after the store.  One barrier per pass
// (__syncthreads_count, which is also the termination test: nothing unfilled); with
// nwet >= 1 at most max(ty, tx) - 1 passes.  No host read: the sequence stays capturable.
//
// The bad flag is per TILE (some channel has nwet < min_wet) but a workgroup owns one
// channel, so each counts the finite pixels of the tile's other channels too (L2 reads,
// nothing for C == 1); channel 0's workgroup stores the flag, so this cut needs neither
// the memset nor the atomicOr of the unmasked one.  A bad tile's planes are 0.0f.
constexpr int kLandThreads = 1024;
constexpr int kLandMaxPix = 25600;  // 6 bytes a pixel in 150 KiB of LDS (160 x 160)
constexpr unsigned short kLandDry = 0xffffu;
__constant__ float kLandRecip[8] = {1.f, 1.f / 2.f, 1.f / 3.f, 1.f / 4.f, 1.f / 5.f, 1.f / 6.f, 1.f / 7.f, 1.f / 8.f};

static_assert(kPrepThreads == kLandThreads, "block_sum_i32 also serves the kPrepThreads kernels");
__device__ __forceinline__ int block_sum_i32(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int i = 0; i < kLandThreads / 64; ++i) s += red[i];
  __syncthreads();
  return s;
}

// The flood fill described above, on a ty x tx plane in LDS (val, and stamp: 0 = wet,
// kLandDry = not filled yet), by the kLandThreads threads of a workgroup; a thread owns
// the pixels tid, tid + kLandThreads, ...  The caller has a barrier between its last
// store to the plane and this call; the stores of the last pass are ordered by the
// barrier that ends it.  Needs a wet pixel.  Returns the number of passes that filled
// something (1 for a plane without a dry pixel: the one pass that finds nothing to do).
// Shared by the masked cut and srmi_tiles_fill, so the two fill bit for bit alike.
__device__ __forceinline__ int land_fill(float* val, unsigned short* stamp, int ty, int tx) {
  const int n = ty * tx, tid = threadIdx.x;
  const int jmax = max(ty, tx);
  int j = 1;
  for (; j < jmax; ++j) {
    int left = 0;
    for (int i = tid; i < n; i += kLandThreads) {
      if (stamp[i] != kLandDry) continue;
      const int y = i / tx, x = i - y * tx;
      float acc = 0.f;
      int cnt = 0;
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          if (dy == 0 && dx == 0) continue;
          const int yy = y + dy, xx = x + dx;
          if (yy < 0 || yy >= ty || xx < 0 || xx >= tx) continue;
          const int q = yy * tx + xx;
          if ((int)stamp[q] < j) {
            acc += val[q];
            ++cnt;
          }
        }
      }
      if (cnt) {
        val[i] = acc * kLandRecip[cnt - 1];
        stamp[i] = (unsigned short)j;
      } else {
        left = 1;
      }
    }
    if (__syncthreads_count(left) == 0) break;
  }
  return j;
}

template <int kMode, bool kVec>
__global__ void __launch_bounds__(kLandThreads) region_to_tiles_masked_kernel(
    const float* __restrict__ region, int C, int H, int W, int ty, int tx, int gx, int sy, int sx, int min_wet,
    const float* __restrict__ off, const float* __restrict__ dv, float* __restrict__ tiles,
    float* __restrict__ off_out, float* __restrict__ div_out, int* __restrict__ bad, int* __restrict__ nwet) {
  extern __shared__ float tile[];  // val[ty * tx], then the stamps
  __shared__ double red[kLandThreads / 64];
  __shared__ float redf[2 * kLandThreads / 64];
  __shared__ int redi[kLandThreads / 64];
  const int c = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
  const int y0 = min((t / gx) * sy, H - ty), x0 = min((t % gx) * sx, W - tx);
  const int n = ty * tx;
  float* val = tile;
  unsigned short* stamp = reinterpret_cast<unsigned short*>(tile + n);
  const size_t p = (size_t)t * C + c;
  const float* src = region + (size_t)c * H * W + (size_t)y0 * W + x0;
  // 1. the plane -> LDS, raw; stamp 0 = wet
  if (kVec) {
    const int tx4 = tx >> 2, n4 = ty * tx4;
    for (int i = tid; i < n4; i += kLandThreads) {
      const int r = i / tx4, q = i - r * tx4;
      const float4 v = *reinterpret_cast<const float4*>(src + (size_t)r * W + 4 * q);
      const int o = r * tx + 4 * q;
      val[o] = v.x; val[o + 1] = v.y; val[o + 2] = v.z; val[o + 3] = v.w;
      stamp[o] = isfinite(v.x) ? 0 : kLandDry;
      stamp[o + 1] = isfinite(v.y) ? 0 : kLandDry;
      stamp[o + 2] = isfinite(v.z) ? 0 : kLandDry;
      stamp[o + 3] = isfinite(v.w) ? 0 : kLandDry;
    }
  } else {
    for (int i = tid; i < n; i += kLandThreads) {
      const float a = src[(size_t)(i / tx) * W + (i % tx)];
      val[i] = a;
      stamp[i] = isfinite(a) ? 0 : kLandDry;
    }
  }
  // 2. is the tile bad?  the wet count of every channel of it
  int isbad = 0;
  for (int cc = 0; cc < C; ++cc) {
    if (cc == c) continue;
    const float* s2 = region + (size_t)cc * H * W + (size_t)y0 * W + x0;
    int k = 0;
    for (int i = tid; i < n; i += kLandThreads) k += isfinite(s2[(size_t)(i / tx) * W + (i % tx)]);
    isbad |= block_sum_i32(k, redi) < min_wet;
  }
  __syncthreads();  // the LDS plane is complete
  // 3. statistics over the wet pixels; from here a thread owns the pixels tid, tid + 1024, ...
  int k = 0;
  double s = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  for (int i = tid; i < n; i += kLandThreads) {
    if (stamp[i] == 0) {
      const float a = val[i];
      ++k;
      if (kMode == SRMI_NORM_LNORM) s += (double)a;
      if (kMode == SRMI_NORM_LSCALE) {
        mn = fminf(mn, a);
        mx = fmaxf(mx, a);
      }
    }
  }
  const int nw = block_sum_i32(k, redi);
  isbad |= nw < min_wet;
  double o, inv, sd = 0.0;
  if (kMode == SRMI_NORM_LNORM) {
    o = block_sum_f64<kLandThreads>(s, red) / (double)nw;
    double q = 0.0;
    for (int i = tid; i < n; i += kLandThreads) {
      if (stamp[i] == 0) {
        const double d = (double)val[i] - o;
        q += d * d;
      }
    }
    sd = sqrt(block_sum_f64<kLandThreads>(q, red) / (double)nw);
    inv = 1.0 / sd;
  } else if (kMode == SRMI_NORM_LSCALE) {
    block_minmax<kLandThreads>(mn, mx, redf);
    o = (double)mn;
    inv = 1.0 / ((double)mx - (double)mn);
  } else {
    o = (double)off[p];
    inv = 1.0 / (double)dv[p];
  }
  if (tid == 0) {
    if (nwet) nwet[p] = nw;
    if (kMode == SRMI_NORM_LNORM) {
      off_out[p] = (float)o;
      div_out[p] = (float)sd;
    } else if (kMode == SRMI_NORM_LSCALE) {
      if (off_out) off_out[p] = mn;
      if (div_out) div_out[p] = mx - mn;
    }
    // every workgroup of the tile has counted all its channels and holds the same flag:
    // channel 0's stores it -- no memset before the launch, no atomic
    if (bad && c == 0) bad[t] = isbad;
  }
  float* dst = tiles + p * n;
  if (isbad) {  // (uniform over the block) finite planes for the forward; the blend never reads them
    for (int i = tid; i < n; i += kLandThreads) dst[i] = 0.f;
    return;
  }
  // 4. normalise the wet pixels in place
  for (int i = tid; i < n; i += kLandThreads)
    if (stamp[i] == 0) val[i] = (float)(((double)val[i] - o) * inv);
  __syncthreads();
  // 5. flood fill; not bad => nwet >= min_wet >= 1, so it ends within max(ty, tx) - 1 passes
  land_fill(val, stamp, ty, tx);
  // 6. the tile, once
  if (kVec) {
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (int i = tid; i < n / 4; i += kLandThreads)
      d4[i] = make_float4(val[4 * i], val[4 * i + 1], val[4 * i + 2], val[4 * i + 3]);
  } else {
    for (int i = tid; i < n; i += kLandThreads) dst[i] = val[i];
  }
}

// ------------------------------------------------------- land in training batches
// No reference counterpart (the reference never trains on a tile with land).
//
// tiles_fill: the fill above, in place on [nplanes][h][w] planes that already are what
// the forward takes (the LR batch of a train step).  One workgroup per plane, planes
// blockIdx.x, + gridDim.x, ... (any number of them, as the resampling kernels); the plane
// and its stamps in LDS as in the cut.  A plane without a non-finite pixel is not
// written at all, one without a finite pixel becomes 0.0f (what the cut gives a bad
// tile); of the others only the filled pixels are stored.  passes (optional): the pass
// count, 0 and -1 for those two.  The trip count stays on the device.
__global__ void __launch_bounds__(kLandThreads) tiles_fill_kernel(float* __restrict__ tiles, long long nplanes, int h,
                                                                  int w, int* __restrict__ passes) {
  extern __shared__ float tile[];  // val[h * w], then the stamps
  __shared__ int redi[kLandThreads / 64];
  const int tid = threadIdx.x, n = h * w;
  float* val = tile;
  unsigned short* stamp = reinterpret_cast<unsigned short*>(tile + n);
  for (long long p = blockIdx.x; p < nplanes; p += gridDim.x) {
    float* pl = tiles + (size_t)p * n;
    int k = 0;
    for (int i = tid; i < n; i += kLandThreads) {
      const float a = pl[i];
      const bool wet = isfinite(a);
      val[i] = a;
      stamp[i] = wet ? 0 : kLandDry;
      k += !wet;
    }
    const int ndry = block_sum_i32(k, redi);  // (also orders the LDS stores)
    int np = 0;
    if (ndry == n) {
      for (int i = tid; i < n; i += kLandThreads) pl[i] = 0.f;
      np = -1;
    } else if (ndry) {  // (uniform over the block)
      np = land_fill(val, stamp, h, w);
      for (int i = tid; i < n; i += kLandThreads)
        if (stamp[i] != 0) pl[i] = val[i];
    }
    if (passes && tid == 0) passes[p] = np;
    __syncthreads();  // the next plane overwrites the LDS
  }
}

// batch_prep_norm_kernel for tiles with land: the statistics over the wet (finite)
// pixels with the arithmetic of the masked cut (LNORM: fp64 mean and 2-pass variance over
// nwet; LSCALE / AFFINE: batch_prep_norm_kernel's, so tiles without a non-finite value
// give its bits), the flipped HR tile with the canonical NaN at the dry pixels, and the
// LR tile by downsample_kernel's arithmetic on it -- an LR pixel is NaN iff one of its
// taps is dry.  The LR planes are then filled by tiles_fill_kernel, a second launch: the
// 192^2 HR plane takes 145 of the 150 KiB of LDS this kernel may use, and the LR plane
// with its stamps does not fit beside it.
template <bool kLds, int kMode>
__global__ void __launch_bounds__(kPrepThreads) batch_prep_masked_kernel(
    const float* __restrict__ raw, int T, int flip, int scale, const float* __restrict__ off,
    const float* __restrict__ dv, float* __restrict__ hr, float* __restrict__ lr, float* __restrict__ off_out,
    float* __restrict__ div_out, int* __restrict__ nwet) {
  extern __shared__ float tile[];  // [T][T + 1] when kLds
  __shared__ double red[kPrepThreads / 64];
  __shared__ float redf[2 * kPrepThreads / 64];
  __shared__ int redi[kPrepThreads / 64];
  const size_t p = blockIdx.x;
  const int tid = threadIdx.x;
  const int n = T * T, P = kLds ? T + 1 : T;
  const float* src = raw + p * n;
  const float* buf = kLds ? tile : src;
  float mn = INFINITY, mx = -INFINITY;
  double s = 0.0;
  int k = 0;
  auto take = [&](float a) __attribute__((always_inline)) {
    if (isfinite(a)) {
      ++k;
      if (kMode == SRMI_NORM_LNORM) s += (double)a;
      if (kMode == SRMI_NORM_LSCALE) {
        mn = fminf(mn, a);
        mx = fmaxf(mx, a);
      }
    }
  };
  for (int i = 4 * tid; i < n; i += 4 * kPrepThreads) {  // T even -> n % 4 == 0
    const float4 v = *reinterpret_cast<const float4*>(src + i);
    take(v.x);
    take(v.y);
    take(v.z);
    take(v.w);
    if (kLds) {
      const int y = i / T, x = i - y * T;
      if (x + 3 < T) {
        float* d = tile + y * P + x;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
      } else {  // T % 4 == 2: the float4 straddles two rows
        const float vv[4] = {v.x, v.y, v.z, v.w};
        for (int e = 0; e < 4; ++e) {
          const int ye = (i + e) / T, xe = (i + e) - ye * T;
          tile[ye * P + xe] = vv[e];
        }
      }
    }
  }
  const int nw = block_sum_i32(k, redi);  // (also orders the LDS stores)
  double o, inv, sd = 0.0;
  if (kMode == SRMI_NORM_LNORM) {
    o = block_sum_f64<kPrepThreads>(s, red) / (double)nw;
    double q = 0.0;
    for (int i = tid; i < n; i += kPrepThreads) {
      const int y = i / T, x = i - y * T;
      const float a = buf[y * P + x];
      if (isfinite(a)) {
        const double d = (double)a - o;
        q += d * d;
      }
    }
    sd = sqrt(block_sum_f64<kPrepThreads>(q, red) / (double)nw);
    inv = 1.0 / sd;
  } else if (kMode == SRMI_NORM_LSCALE) {
    block_minmax<kPrepThreads>(mn, mx, redf);
    o = (double)mn;
    inv = 1.0 / ((double)mx - (double)mn);
  } else {
    o = (double)off[p];
    inv = 1.0 / (double)dv[p];
  }
  // batch_prep_norm_kernel's expression, as it stands there: a NaN stays a NaN through it
  // and an infinity stays non-finite, so the HR tile needs a select and the LR taps none
  auto norm = [&](int y, int x) __attribute__((always_inline)) {
    int sy, sx;
    flip_src(flip, T, y, x, sy, sx);
    return (float)(((double)buf[sy * P + sx] - o) * inv);
  };
  float* dst = hr + p * n;
  for (int i = 4 * tid; i < n; i += 4 * kPrepThreads) {
    float q[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int y = (i + e) / T, x = (i + e) - y * T;
      int sy, sx;
      flip_src(flip, T, y, x, sy, sx);
      q[e] = isfinite(buf[sy * P + sx]) ? norm(y, x) : __int_as_float(0x7fc00000);
    }
    *reinterpret_cast<float4*>(dst + i) = make_float4(q[0], q[1], q[2], q[3]);
  }
  if (lr) {
    // downsample_kernel's arithmetic (small.hip), tap order as in batch_prep_kernel; a dry
    // tap makes the pixel non-finite (NaN, or an infinity's), which is all the fill asks
    const int t = T / scale;
    const float kk[4] = {-3.f / 32.f, 19.f / 32.f, 19.f / 32.f, -3.f / 32.f};
    float* ldst = lr + p * t * t;
    for (int i = tid; i < t * t; i += kPrepThreads) {
      const int y = i / t, x = i - y * t;
      const int y0 = y * scale + scale / 2 - 2, x0 = x * scale + scale / 2 - 2;
      float acc = 0.f;
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const int yy = min(max(y0 + a, 0), T - 1);
        float rsum = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) rsum += kk[j] * norm(yy, min(max(x0 + j, 0), T - 1));
        acc += kk[a] * rsum;
      }
      ldst[i] = acc;
    }
  }
  if (tid == 0) {
    if (nwet) nwet[p] = nw;
    if (kMode == SRMI_NORM_LNORM) {
      if (off_out) off_out[p] = (float)o;
      if (div_out) div_out[p] = (float)sd;
    } else if (kMode == SRMI_NORM_LSCALE) {
      if (off_out) off_out[p] = mn;
      if (div_out) div_out[p] = mx - mn;
    }
  }
}

// ------------------------------------------------------------ LLC4320 source
// The reference expands a '>f4' wet-value file through a '>f4' mask template
// (13 nx^2 cells, 0 = land) on the host, then cuts the east | flipped-west
// image and the ROI.  Device version: the template -> ROI index map is built
// ONCE (the template is static): per-cell wet flags, a 3-kernel exclusive scan
// (block counts, one-block scan of the counts, block-local ranks), then each ROI
// pixel looks up the rank of its LLC cell.  Every time slice is then ONE
// gather: out[p] = bswap(data[idx[p]]) or NaN -- HBM-bound byte work.
constexpr int kScanThreads = 1024, kScanPer = 16, kScanBlk = kScanThreads * kScanPer;

__device__ __forceinline__ bool llc_wet(uint32_t be_word) {
  // file bytes are big-endian float32; "template != 0" (+-0 are land, NaN is wet)
  return (__builtin_bswap32(be_word) & 0x7fffffffu) != 0u;
}

__global__ void __launch_bounds__(kScanThreads) llc_count_kernel(const uint32_t* __restrict__ tmpl, long long n,
                                                                 int* __restrict__ blkcnt) {
  __shared__ int red[kScanThreads / 64];
  const long long base = (long long)blockIdx.x * kScanBlk + (long long)threadIdx.x * kScanPer;
  int c = 0;
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) c += (base + k < n) && llc_wet(tmpl[base + k]);
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int i = 0; i < kScanThreads / 64; ++i) t += red[i];
    blkcnt[blockIdx.x] = t;
  }
}

// one block: blkoff[b] = sum_{i<b} blkcnt[i]; *total = sum
__global__ void __launch_bounds__(kScanThreads) llc_scan_counts_kernel(const int* __restrict__ blkcnt, int nb,
                                                                       long long* __restrict__ blkoff,
                                                                       long long* __restrict__ total) {
  __shared__ long long wsum[kScanThreads / 64];
  const int per = (nb + kScanThreads - 1) / kScanThreads;
  const int b0 = threadIdx.x * per;
  long long s = 0;
  for (int i = 0; i < per; ++i)
    if (b0 + i < nb) s += blkcnt[b0 + i];
  // exclusive scan of s over the block: wave inclusive scan + wave offsets
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  long long inc = s;
  for (int o = 1; o < 64; o <<= 1) {
    const long long t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  long long woff = 0;
  for (int i = 0; i < w; ++i) woff += wsum[i];
  long long run = woff + inc - s;
  for (int i = 0; i < per; ++i)
    if (b0 + i < nb) {
      blkoff[b0 + i] = run;
      run += blkcnt[b0 + i];
    }
  if (threadIdx.x == kScanThreads - 1) *total = run;
}

// rank[i] = number of wet cells before i (wet i), -1 for land
__global__ void __launch_bounds__(kScanThreads) llc_rank_kernel(const uint32_t* __restrict__ tmpl, long long n,
                                                                const long long* __restrict__ blkoff,
                                                                int* __restrict__ rank) {
  __shared__ int wsum[kScanThreads / 64];
  const long long base = (long long)blockIdx.x * kScanBlk + (long long)threadIdx.x * kScanPer;
  uint32_t bits = 0;
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) bits |= (uint32_t)((base + k < n) && llc_wet(tmpl[base + k])) << k;
  const int c = __builtin_popcount(bits);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = c;
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  int woff = 0;
  for (int i = 0; i < w; ++i) woff += wsum[i];
  long long r = blkoff[blockIdx.x] + woff + inc - c;
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) {
    if (base + k < n) {
      const bool wet = (bits >> k) & 1u;
      rank[base + k] = wet ? (int)r : -1;
      r += wet;
    }
  }
}

// ROI pixel (y, x) of the [3nx, 4nx] east | west.T[::-1] image -> LLC cell
__device__ __forceinline__ long long llc_cell(int Y, int X, int nx) {
  const long long n2 = (long long)nx * nx;
  if (X < nx) return (long long)Y * nx + X;
  if (X < 2 * nx) return 3 * n2 + (long long)Y * nx + (X - nx);
  return 7 * n2 + (long long)(X - 2 * nx) * 3 * nx + (3 * nx - 1 - Y);
}

__global__ void __launch_bounds__(256) llc_map_kernel(const int* __restrict__ rank, int nx, int y0, int ys, int x0,
                                                      int xs, int* __restrict__ idx) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long long)ys * xs) return;
  const int y = (int)(p / xs), x = (int)(p - (long long)y * xs);
  idx[p] = rank[llc_cell(y0 + y, x0 + x, nx)];
}

// out[p] = float(bswap(data[idx[p]])), NaN for land (idx < 0) or idx >= nvals
__global__ void __launch_bounds__(256) llc_gather_kernel(const uint32_t* __restrict__ data, long long nvals,
                                                         const int* __restrict__ idx, long long np,
                                                         float* __restrict__ out) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= np) return;
  const int i = idx[p];
  out[p] = (i >= 0 && i < nvals) ? __uint_as_float(__builtin_bswap32(data[i])) : __int_as_float(0x7fc00000);
}

// get_tiles' keep mask: bad[c * gy*gx + t] = 1 when tile t of channel c holds a
// non-finite value (its mean is then not finite).  grid (gy*gx, C)
__global__ void __launch_bounds__(256) tiles_nonfinite_kernel(const float* __restrict__ region, int H, int W, int ty,
                                                              int tx, int gx, int* __restrict__ bad) {
  const int t = blockIdx.x, c = blockIdx.y;
  const int y0 = (t / gx) * ty, x0 = (t % gx) * tx;
  const float* src = region + (size_t)c * H * W + (size_t)y0 * W + x0;
  int nf = 0;
  for (int i = threadIdx.x; i < ty * tx; i += 256) nf |= !isfinite(src[(size_t)(i / tx) * W + (i % tx)]);
  nf = __syncthreads_or(nf);
  if (threadIdx.x == 0) bad[(size_t)c * gridDim.x + t] = nf;
}

// tiles_nonfinite_kernel with a threshold, for training on coastal tiles (no reference
// counterpart: get_tiles drops a tile for one NaN).  nwet[c * ncells + t] = the finite
// pixels of plane (c, t); a tile is bad when SOME channel has fewer than min_wet, and
// that one flag goes into every channel's row, so the keep list that tiles_keep_kernel
// makes of it stays channel-aligned.  One workgroup counts all the channels of a tile
// and stores with plain stores -- for the masked cut's reason, neither a memset nor an
// atomic.  grid (ncells)
__global__ void __launch_bounds__(256) tiles_dry_kernel(const float* __restrict__ region, int C, int H, int W, int ty,
                                                        int tx, int gx, int min_wet, int* __restrict__ bad,
                                                        int* __restrict__ nwet) {
  __shared__ int red[4];
  const int t = blockIdx.x, ncells = gridDim.x;
  const int y0 = (t / gx) * ty, x0 = (t % gx) * tx;
  int isbad = 0;
  for (int c = 0; c < C; ++c) {
    const float* src = region + (size_t)c * H * W + (size_t)y0 * W + x0;
    int k = 0;
    for (int i = threadIdx.x; i < ty * tx; i += 256) k += isfinite(src[(size_t)(i / tx) * W + (i % tx)]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) k += __shfl_xor(k, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = k;
    __syncthreads();
    const int nw = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    if (nwet && threadIdx.x == 0) nwet[(size_t)c * ncells + t] = nw;
    isbad |= nw < min_wet;
  }
  for (int c = threadIdx.x; c < C; c += 256) bad[(size_t)c * ncells + t] = isbad;
}

// out plane m (= [m / C][m % C] of the [n/C][C][ty][tx] result) <- tile plane
// src[m] = c * gy*gx + t of the channel-major flattening.  grid (ceil(ty*tx/1024), nslots)
__global__ void __launch_bounds__(256) tiles_gather_kernel(const float* __restrict__ region, int H, int W, int ty,
                                                           int tx, int gx, int ntile, const int* __restrict__ src,
                                                           float* __restrict__ out) {
  const int m = blockIdx.y, j = src[m];
  const int c = j / ntile, t = j - c * ntile;
  const int y0 = (t / gx) * ty, x0 = (t % gx) * tx;
  const float* s = region + (size_t)c * H * W + (size_t)y0 * W + x0;
  float* d = out + (size_t)m * ty * tx;
  for (int i = blockIdx.x * 1024 + threadIdx.x; i < min(ty * tx, (int)(blockIdx.x + 1) * 1024); i += 256)
    d[i] = s[(size_t)(i / tx) * W + (i % tx)];
}

// ------------------------------------------------- sparse file reads (srmi.feed)
// A ROI touches a small share of a wet-value file.  The file is cut into blocks of
// 2^shift words; block_mask marks the blocks the ROI's index map touches (the host
// then reads only those, back to back, into a compact staging buffer) and
// compact_map rewrites the index map into that buffer.  Both run once per
// template and ROI; every file is then llc_gather_kernel on the compact words.
// err[0] is set when an index lies past the n_blocks blocks (never stored through).
__global__ void __launch_bounds__(256) llc_block_mask_kernel(const int* __restrict__ idx, long long np, int shift,
                                                             int* __restrict__ mask, int n_blocks,
                                                             int* __restrict__ err) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= np) return;
  const int i = idx[p];
  if (i < 0) return;
  const int b = i >> shift;
  if (b < n_blocks) mask[b] = 1;  // every writer stores the same value
  else err[0] = 1;
}

// out[p] = block_base[idx >> shift] + (idx & (2^shift - 1)); -1 for land, for a
// block that is not read (base -1) and for an index past the blocks
__global__ void __launch_bounds__(256) llc_compact_map_kernel(const int* __restrict__ idx, long long np, int shift,
                                                              const int* __restrict__ base, int n_blocks,
                                                              int* __restrict__ out) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= np) return;
  const int i = idx[p];
  int o = -1;
  if (i >= 0 && (i >> shift) < n_blocks) {
    const int b = base[i >> shift];
    if (b >= 0) o = b + (i & ((1 << shift) - 1));
  }
  out[p] = o;
}

// get_tiles' keep list on the device: keep = flatnonzero(bad == 0), n = len(keep) / C,
// src = keep[:n * C] (srmi.llc.get_tiles).  ONE workgroup: a first pass counts the kept
// flags (so nothing past n * C is stored), a second walks them in chunks of
// kKeepThreads with a wave inclusive scan + wave offsets (as llc_rank_kernel) and
// carries the running offset from chunk to chunk.  Fixed order, no atomics.
constexpr int kKeepThreads = 1024;

__global__ void __launch_bounds__(kKeepThreads) tiles_keep_kernel(const int* __restrict__ bad, int C, int total,
                                                                  int* __restrict__ src, int* __restrict__ count) {
  __shared__ int wsum[kKeepThreads / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int c = 0;
  for (int i = threadIdx.x; i < total; i += kKeepThreads) c += bad[i] == 0;
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if (lane == 0) wsum[w] = c;
  __syncthreads();
  int nkeep = 0;
  for (int i = 0; i < kKeepThreads / 64; ++i) nkeep += wsum[i];
  __syncthreads();
  const int n = nkeep / C, nsrc = n * C;
  if (threadIdx.x == 0) {
    count[0] = n;
    count[1] = nkeep;
  }
  int run = 0;
  for (int a = 0; a < total && run < nsrc; a += kKeepThreads) {  // (run is uniform over the block)
    const int i = a + threadIdx.x;
    const int k = i < total && bad[i] == 0;
    int inc = k;
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(inc, o, 64);
      if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int woff = 0, tot = 0;
    for (int j = 0; j < kKeepThreads / 64; ++j) {
      woff += j < w ? wsum[j] : 0;
      tot += wsum[j];
    }
    const int pos = run + woff + inc - k;
    if (k && pos < nsrc) src[pos] = i;
    run += tot;
    __syncthreads();
  }
}

// tiles_gather_kernel with the slot count on the device (count[0] * C, tiles_keep's
// result): launched for max_slots planes, a plane at or past the count returns
// before it reads src or writes out.  grid (max_slots, ceil(ty*tx/1024))
__global__ void __launch_bounds__(256) tiles_gather_dev_kernel(const float* __restrict__ region, int C, int H, int W,
                                                               int ty, int tx, int gx, int ntile,
                                                               const int* __restrict__ src,
                                                               const int* __restrict__ count,
                                                               float* __restrict__ out) {
  const int m = blockIdx.x;
  if (m >= count[0] * C) return;
  const int j = src[m];
  const int c = j / ntile, t = j - c * ntile;
  const int y0 = (t / gx) * ty, x0 = (t % gx) * tx;
  const float* s = region + (size_t)c * H * W + (size_t)y0 * W + x0;
  float* d = out + (size_t)m * ty * tx;
  for (int i = blockIdx.y * 1024 + threadIdx.x; i < min(ty * tx, (int)(blockIdx.y + 1) * 1024); i += 256)
    d[i] = s[(size_t)(i / tx) * W + (i % tx)];
}

}  // namespace srmi

using namespace srmi;

extern "C" {

int srmi_region_to_tiles(const float* region, int C, int H, int W, int ty, int tx, float* tiles, float* mean,
                         float* stdv, int* bad, void* stream) {
  if (!region || !tiles || !mean || !stdv) return SRMI_ERR_ARG;
  if (C < 1 || ty < 1 || tx < 1 || H < ty || W < tx) return SRMI_ERR_SHAPE;
  return region_to_tiles_plan_launch(region, C, H, W, ty, tx, H / ty, W / tx, ty, tx, tiles, mean, stdv, bad,
                                     static_cast<hipStream_t>(stream));
}

int srmi_tiles_to_region(const float* tiles, const float* mean, const float* stdv, const int* inv, int C, int ty,
                         int tx, int gy, int gx, float* out, void* stream) {
  if (!tiles || !out || (mean && !stdv)) return SRMI_ERR_ARG;
  if (C < 1 || ty < 1 || tx < 1 || gy < 1 || gx < 1) return SRMI_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (tx % 4 == 0 && ((uintptr_t)tiles & 15) == 0 && ((uintptr_t)out & 15) == 0) {
    hipLaunchKernelGGL(tiles_to_region_v4_kernel, dim3((gx * tx / 4 + 255) / 256, gy * ty, C), dim3(256), 0, st,
                       tiles, mean, stdv, inv, C, ty, tx, gx, out);
    SRMI_CHECK_LAUNCH();
    return 0;
  }
  hipLaunchKernelGGL(tiles_to_region_kernel, dim3((gx * tx + 255) / 256, gy * ty, C), dim3(256), 0, st, tiles, mean,
                     stdv, inv, C, ty, tx, gx, out);
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_batch_prep(const float* raw, int B, int C, int T, int flip, int scale, float* hr, float* lr, float* mean,
                    float* stdv, void* stream) {
  if (B < 1 || C < 1 || T < 2 || T % 2 || flip < 0 || flip > 7) return SRMI_ERR_SHAPE;
  if (lr && (scale < 2 || T % scale)) return SRMI_ERR_SHAPE;
  if (!raw || !hr) return SRMI_ERR_ARG;
  const size_t lds = (size_t)T * (T + 1) * sizeof(float);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (lds <= 150 * 1024) {
    hipLaunchKernelGGL(batch_prep_kernel<true>, dim3(C, B), dim3(kPrepThreads), lds, st, raw, C, T, flip, scale, hr,
                       lr, mean, stdv);
  } else {
    hipLaunchKernelGGL(batch_prep_kernel<false>, dim3(C, B), dim3(kPrepThreads), 0, st, raw, C, T, flip, scale, hr,
                       lr, mean, stdv);
  }
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_batch_prep_norm(const float* raw, long long B, int C, int T, int flip, int scale, int mode,
                         const float* off, const float* dv, float* hr, float* lr, float* off_out, float* div_out,
                         void* stream) {
  if (mode == SRMI_NORM_LNORM) {
    if (B > 65535) return SRMI_ERR_SHAPE;  // srmi_batch_prep's grid.y
    return srmi_batch_prep(raw, (int)B, C, T, flip, scale, hr, lr, off_out, div_out, stream);
  }
  if (mode != SRMI_NORM_LSCALE && mode != SRMI_NORM_AFFINE) return SRMI_ERR_ARG;
  if (B < 1 || C < 1 || T < 2 || T % 2 || flip < 0 || flip > 7 || B * C > 0x7fffffffLL) return SRMI_ERR_SHAPE;
  if (lr && (scale < 2 || T % scale)) return SRMI_ERR_SHAPE;
  if (!raw || !hr || (mode == SRMI_NORM_AFFINE && (!off || !dv))) return SRMI_ERR_ARG;
  // the kernel's float4 loads and stores: T even makes every plane a multiple of 16 bytes
  if (((uintptr_t)raw | (uintptr_t)hr) & 15) return SRMI_ERR_ARG;
  const size_t lds = (size_t)T * (T + 1) * sizeof(float);
  const dim3 grid((unsigned)(B * C)), block(kPrepThreads);
  hipStream_t st = static_cast<hipStream_t>(stream);
#define SRMI_PREP_NORM(LDS, MODE, BYTES)                                                                          \
  hipLaunchKernelGGL((batch_prep_norm_kernel<LDS, MODE>), grid, block, BYTES, st, raw, T, flip, scale, off, dv, hr, \
                     lr, off_out, div_out)
  if (lds <= 150 * 1024) {
    if (mode == SRMI_NORM_LSCALE) SRMI_PREP_NORM(true, SRMI_NORM_LSCALE, lds);
    else SRMI_PREP_NORM(true, SRMI_NORM_AFFINE, lds);
  } else {
    if (mode == SRMI_NORM_LSCALE) SRMI_PREP_NORM(false, SRMI_NORM_LSCALE, 0);
    else SRMI_PREP_NORM(false, SRMI_NORM_AFFINE, 0);
  }
#undef SRMI_PREP_NORM
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_region_to_tiles_norm(const float* region, int C, int H, int W, int ty, int tx, int mode, const float* off,
                              const float* dv, float* tiles, float* off_out, float* div_out, int* bad,
                              void* stream) {
  if (mode == SRMI_NORM_LNORM) {
    if (!region || !tiles || !off_out || !div_out) return SRMI_ERR_ARG;
    return srmi_region_to_tiles(region, C, H, W, ty, tx, tiles, off_out, div_out, bad, stream);
  }
  if (mode != SRMI_NORM_LSCALE && mode != SRMI_NORM_AFFINE) return SRMI_ERR_ARG;
  if (C < 1 || ty < 1 || tx < 1 || H < ty || W < tx) return SRMI_ERR_SHAPE;
  if (!region || !tiles || (mode == SRMI_NORM_AFFINE && (!off || !dv))) return SRMI_ERR_ARG;
  const int gy = H / ty, gx = W / tx;
  if ((long long)gy * gx > 65535) return SRMI_ERR_SHAPE;  // grid.y, as region_to_tiles
  return region_to_tiles_norm_plan_launch(region, C, H, W, ty, tx, gy, gx, ty, tx, mode, off, dv, tiles, off_out,
                                          div_out, bad, static_cast<hipStream_t>(stream));
}

int srmi_overlap_count(int L, int t, int S) { return overlap_count(L, t, S); }

int srmi_region_to_tiles_overlap(const float* region, int C, int H, int W, int ty, int tx, int sy, int sx, int mode,
                                 const float* off, const float* dv, float* tiles, float* off_out, float* div_out,
                                 int* bad, void* stream) {
  if (mode != SRMI_NORM_LNORM && mode != SRMI_NORM_LSCALE && mode != SRMI_NORM_AFFINE) return SRMI_ERR_ARG;
  if (C < 1 || C > 65535) return SRMI_ERR_ARG;  // grid.x
  const int gy = overlap_count(H, ty, sy), gx = overlap_count(W, tx, sx);
  if (gy < 0 || gx < 0) return SRMI_ERR_ARG;
  if ((long long)gy * gx > 65535) return SRMI_ERR_SHAPE;  // grid.y, as region_to_tiles
  if (!region || !tiles || (mode == SRMI_NORM_AFFINE && (!off || !dv)) ||
      (mode == SRMI_NORM_LNORM && (!off_out || !div_out)))
    return SRMI_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (mode == SRMI_NORM_LNORM)
    return region_to_tiles_plan_launch(region, C, H, W, ty, tx, gy, gx, sy, sx, tiles, off_out, div_out, bad, st);
  return region_to_tiles_norm_plan_launch(region, C, H, W, ty, tx, gy, gx, sy, sx, mode, off, dv, tiles, off_out,
                                          div_out, bad, st);
}

int srmi_tiles_blend(const float* tiles, const float* off, const float* dv, const int* bad, int C, int Ty, int Tx,
                     int Sy, int Sx, int Ho, int Wo, float* out, void* stream) {
  return tiles_blend_any_launch(tiles, off, dv, bad, C, Ty, Tx, Sy, Sx, Ho, Wo, nullptr, 1, out,
                                static_cast<hipStream_t>(stream));
}

int srmi_tiles_blend_masked(const float* tiles, const float* off, const float* dv, const int* bad, int C, int Ty,
                            int Tx, int Sy, int Sx, int Ho, int Wo, const float* mask_src, int scale, float* out,
                            void* stream) {
  if (!mask_src || scale < 1 || Ho < 1 || Wo < 1 || Ho % scale || Wo % scale) return SRMI_ERR_ARG;
  return tiles_blend_any_launch(tiles, off, dv, bad, C, Ty, Tx, Sy, Sx, Ho, Wo, mask_src, scale, out,
                                static_cast<hipStream_t>(stream));
}

int srmi_tiles_dihedral(const float* in, long long nplanes, int h, int w, int variants, float* out, void* stream) {
  if (variants < 1 || variants > 255 || !in || !out || in == out) return SRMI_ERR_ARG;
  if (nplanes < 1 || h < 1 || w < 1) return SRMI_ERR_SHAPE;
  if ((variants & 0xf0) && h != w) return SRMI_ERR_SHAPE;  // a swap of a rectangular plane
  const int nby = (h + kDihB - 1) / kDihB, nbx = (w + kDihB - 1) / kDihB;
  if (nplanes * nby * nbx > 0x7fffffffLL) return SRMI_ERR_SHAPE;  // grid.x
  const size_t slab = (size_t)nplanes * h * w;
  const dim3 grid((unsigned)(nplanes * nby * nbx));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (w % 4 == 0 && ((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 15) == 0)
    hipLaunchKernelGGL(tiles_dihedral_kernel<true>, grid, dim3(256), 0, st, in, h, w, nby, nbx, variants, slab, out);
  else
    hipLaunchKernelGGL(tiles_dihedral_kernel<false>, grid, dim3(256), 0, st, in, h, w, nby, nbx, variants, slab, out);
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_tiles_blend_ensemble(const float* tiles, int variants, const float* off, const float* dv, const int* bad,
                              int C, int Ty, int Tx, int Sy, int Sx, int Ho, int Wo, const float* mask_src,
                              int scale, float* mean, float* spread, void* stream) {
  if (variants < 1 || variants > 255) return SRMI_ERR_ARG;
  if (mask_src && (scale < 1 || Ho < 1 || Wo < 1 || Ho % scale || Wo % scale)) return SRMI_ERR_ARG;
  // from here as tiles_blend_any_launch
  if (C < 1 || C > 65535) return SRMI_ERR_ARG;  // grid.z
  const int ny = overlap_count(Ho, Ty, Sy), nx = overlap_count(Wo, Tx, Sx);
  if (ny < 0 || nx < 0) return SRMI_ERR_ARG;
  const long long wy = (long long)(Ty / Sy + 2) * (Ty - Sy + 1), wx = (long long)(Tx / Sx + 2) * (Tx - Sx + 1);
  if (Ho > 65535 || (long long)ny * nx > 0x7fffffffLL || wy * wx > 0x7fffffffLL) return SRMI_ERR_SHAPE;
  if ((variants & 0xf0) && Ty != Tx) return SRMI_ERR_SHAPE;  // a swap of a rectangular tile
  if (!tiles || !mean || (off && !dv)) return SRMI_ERR_ARG;
  const int K = __builtin_popcount((unsigned)variants);
  const bool vec = Tx % 4 == 0 && Sx % 4 == 0 && Wo % 4 == 0 && ((uintptr_t)tiles & 15) == 0 &&
                   ((uintptr_t)mean & 15) == 0 && ((uintptr_t)spread & 15) == 0 && (!mask_src || scale % 4 == 0);
  hipStream_t st = static_cast<hipStream_t>(stream);
#define SRMI_BLEND_ENS(V, MASK)                                                                                    \
  hipLaunchKernelGGL((tiles_blend_ensemble_kernel<V, MASK>), dim3((Wo / V + 15) / 16, (Ho + 15) / 16, C), dim3(256), \
                     0, st, tiles, variants, K, off, dv, bad, C, Ty, Tx, Sy, Sx, ny, nx, Ho, Wo, mask_src, scale,    \
                     mean, spread)
  if (mask_src) {
    if (vec) SRMI_BLEND_ENS(4, true);
    else SRMI_BLEND_ENS(1, true);
  } else {
    if (vec) SRMI_BLEND_ENS(4, false);
    else SRMI_BLEND_ENS(1, false);
  }
#undef SRMI_BLEND_ENS
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_tile_stats(const float* tiles, long long n, int C, int ty, int tx, double* acc, int first, void* stream) {
  if (n < 1 || C < 1 || ty < 1 || tx < 1 || n * C > 0x7fffffffLL || (long long)ty * tx > 0x7fffffffLL)
    return SRMI_ERR_SHAPE;
  if (!tiles || !acc) return SRMI_ERR_ARG;
  const int ne = ty * tx, n4 = ne / 4;
  const dim3 grid((unsigned)(n * C));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (ne % 4 || ((uintptr_t)tiles & 15) || n4 > 1024 * kNormKR)
    hipLaunchKernelGGL(tile_stats_kernel, grid, dim3(256), 0, st, tiles, ne, acc, first);
  else if (n4 <= 64 * 4)  // up to 32^2: one wave per plane
    hipLaunchKernelGGL((tile_stats_reg_kernel<64, 4>), grid, dim3(64), 0, st, tiles, n4, acc, first);
  else if (n4 <= 256 * 4)  // up to 64^2
    hipLaunchKernelGGL((tile_stats_reg_kernel<256, 4>), grid, dim3(256), 0, st, tiles, n4, acc, first);
  else  // up to 192^2
    hipLaunchKernelGGL((tile_stats_reg_kernel<1024, kNormKR>), grid, dim3(1024), 0, st, tiles, n4, acc, first);
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_tile_stats_finalize(const double* acc, long long n, int C, int ntimes, float* tstats, float* gstats,
                             void* stream) {
  if (n < 1 || C < 1 || ntimes < 1 || n * C > 0x7fffffffLL) return SRMI_ERR_SHAPE;
  if (!acc || ((uintptr_t)tstats & 15) || ((uintptr_t)gstats & 15)) return SRMI_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (tstats)
    hipLaunchKernelGGL(tile_stats_rows_kernel, dim3((unsigned)((n * C + 255) / 256)), dim3(256), 0, st, acc, n * C,
                       (double)ntimes, tstats);
  if (gstats)
    hipLaunchKernelGGL(tile_stats_global_kernel, dim3(C), dim3(1024), 0, st, acc, n, C, (double)ntimes, gstats);
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_region_to_tiles_overlap_masked(const float* region, int C, int H, int W, int ty, int tx, int sy, int sx,
                                        int mode, const float* off, const float* dv, float* tiles, float* off_out,
                                        float* div_out, int* bad, int min_wet, int* nwet, void* stream) {
  if (mode != SRMI_NORM_LNORM && mode != SRMI_NORM_LSCALE && mode != SRMI_NORM_AFFINE) return SRMI_ERR_ARG;
  if (C < 1 || C > 65535 || min_wet < 1) return SRMI_ERR_ARG;  // grid.x
  const int gy = overlap_count(H, ty, sy), gx = overlap_count(W, tx, sx);
  if (gy < 0 || gx < 0) return SRMI_ERR_ARG;
  if ((long long)gy * gx > 65535) return SRMI_ERR_SHAPE;  // grid.y, as region_to_tiles
  if (!region || !tiles || (mode == SRMI_NORM_AFFINE && (!off || !dv)) ||
      (mode == SRMI_NORM_LNORM && (!off_out || !div_out)))
    return SRMI_ERR_ARG;
  if ((long long)ty * tx > kLandMaxPix) return SRMI_ERR_SHAPE;  // values + stamps in LDS
  const bool vec = tx % 4 == 0 && W % 4 == 0 && sx % 4 == 0 && ((uintptr_t)region & 15) == 0 &&
                   ((uintptr_t)tiles & 15) == 0;
  const size_t lds = (size_t)ty * tx * (sizeof(float) + sizeof(unsigned short));
  const dim3 grid(C, gy * gx), block(kLandThreads);
  hipStream_t st = static_cast<hipStream_t>(stream);
#define SRMI_R2T_MASKED(MODE, VEC)                                                                                 \
  hipLaunchKernelGGL((region_to_tiles_masked_kernel<MODE, VEC>), grid, block, lds, st, region, C, H, W, ty, tx, gx, \
                     sy, sx, min_wet, off, dv, tiles, off_out, div_out, bad, nwet)
  if (mode == SRMI_NORM_LNORM) {
    if (vec) SRMI_R2T_MASKED(SRMI_NORM_LNORM, true);
    else SRMI_R2T_MASKED(SRMI_NORM_LNORM, false);
  } else if (mode == SRMI_NORM_LSCALE) {
    if (vec) SRMI_R2T_MASKED(SRMI_NORM_LSCALE, true);
    else SRMI_R2T_MASKED(SRMI_NORM_LSCALE, false);
  } else {
    if (vec) SRMI_R2T_MASKED(SRMI_NORM_AFFINE, true);
    else SRMI_R2T_MASKED(SRMI_NORM_AFFINE, false);
  }
#undef SRMI_R2T_MASKED
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_tiles_fill(float* tiles, long long nplanes, int h, int w, int* passes, void* stream) {
  if (nplanes < 1 || h < 1 || w < 1) return SRMI_ERR_SHAPE;
  if ((long long)h * w > kLandMaxPix) return SRMI_ERR_SHAPE;  // values + stamps in LDS
  if (!tiles) return SRMI_ERR_ARG;
  const size_t lds = (size_t)h * w * (sizeof(float) + sizeof(unsigned short));
  const unsigned grid = (unsigned)(nplanes < 65535 ? nplanes : 65535);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(tiles_fill_kernel, dim3(grid), dim3(kLandThreads), lds, st, tiles, nplanes, h, w, passes);
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_batch_prep_masked(const float* raw, long long B, int C, int T, int flip, int scale, int mode,
                           const float* off, const float* dv, float* hr, float* lr, float* off_out, float* div_out,
                           int* nwet, void* stream) {
  if (mode != SRMI_NORM_LNORM && mode != SRMI_NORM_LSCALE && mode != SRMI_NORM_AFFINE) return SRMI_ERR_ARG;
  if (B < 1 || C < 1 || T < 2 || T % 2 || flip < 0 || flip > 7 || B * C > 0x7fffffffLL) return SRMI_ERR_SHAPE;
  if (lr && (scale < 2 || T % scale)) return SRMI_ERR_SHAPE;
  if (lr && (long long)(T / scale) * (T / scale) > kLandMaxPix) return SRMI_ERR_SHAPE;  // tiles_fill's plane
  if (!raw || !hr || (mode == SRMI_NORM_AFFINE && (!off || !dv))) return SRMI_ERR_ARG;
  // the kernel's float4 loads and stores: T even makes every plane a multiple of 16 bytes
  if (((uintptr_t)raw | (uintptr_t)hr) & 15) return SRMI_ERR_ARG;
  const size_t lds = (size_t)T * (T + 1) * sizeof(float);
  const dim3 grid((unsigned)(B * C)), block(kPrepThreads);
  hipStream_t st = static_cast<hipStream_t>(stream);
#define SRMI_PREP_MASKED(LDS, MODE, BYTES)                                                                          \
  hipLaunchKernelGGL((batch_prep_masked_kernel<LDS, MODE>), grid, block, BYTES, st, raw, T, flip, scale, off, dv, hr, \
                     lr, off_out, div_out, nwet)
  if (lds <= 150 * 1024) {
    if (mode == SRMI_NORM_LNORM) SRMI_PREP_MASKED(true, SRMI_NORM_LNORM, lds);
    else if (mode == SRMI_NORM_LSCALE) SRMI_PREP_MASKED(true, SRMI_NORM_LSCALE, lds);
    else SRMI_PREP_MASKED(true, SRMI_NORM_AFFINE, lds);
  } else {
    if (mode == SRMI_NORM_LNORM) SRMI_PREP_MASKED(false, SRMI_NORM_LNORM, 0);
    else if (mode == SRMI_NORM_LSCALE) SRMI_PREP_MASKED(false, SRMI_NORM_LSCALE, 0);
    else SRMI_PREP_MASKED(false, SRMI_NORM_AFFINE, 0);
  }
#undef SRMI_PREP_MASKED
  SRMI_CHECK_LAUNCH();
  if (lr) return srmi_tiles_fill(lr, B * C, T / scale, T / scale, nullptr, stream);
  return 0;
}

int srmi_llc_index_map_workspace(long long n, size_t* bytes) {
  if (!bytes) return SRMI_ERR_ARG;
  if (n < 1) return SRMI_ERR_SHAPE;
  const long long nb = (n + kScanBlk - 1) / kScanBlk;
  *bytes = (size_t)n * 4 + (size_t)nb * 4 + (size_t)nb * 8 + 64;
  return 0;
}

int srmi_llc_index_map(const void* template_be, long long n, int nx, int y0, int ys, int x0, int xs, int* idx,
                       long long* n_wet, void* ws, size_t ws_bytes, void* stream) {
  const uint32_t* tmpl = static_cast<const uint32_t*>(template_be);
  if (nx < 1 || n != 13LL * nx * nx || ys < 1 || xs < 1 || y0 < 0 || x0 < 0 || y0 + ys > 3 * nx ||
      x0 + xs > 4 * nx)
    return SRMI_ERR_SHAPE;
  size_t need = 0;
  srmi_llc_index_map_workspace(n, &need);
  if (!tmpl || !idx || !n_wet || !ws || ws_bytes < need) return SRMI_ERR_ARG;
  const long long nb = (n + kScanBlk - 1) / kScanBlk;
  char* w = static_cast<char*>(ws);
  int* rank = reinterpret_cast<int*>(w);
  long long* blkoff = reinterpret_cast<long long*>(w + (((size_t)n * 4 + 7) & ~(size_t)7));
  int* blkcnt = reinterpret_cast<int*>(reinterpret_cast<char*>(blkoff) + (size_t)nb * 8);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(llc_count_kernel, dim3((unsigned)nb), dim3(kScanThreads), 0, st, tmpl, n, blkcnt);
  hipLaunchKernelGGL(llc_scan_counts_kernel, dim3(1), dim3(kScanThreads), 0, st, blkcnt, (int)nb, blkoff, n_wet);
  hipLaunchKernelGGL(llc_rank_kernel, dim3((unsigned)nb), dim3(kScanThreads), 0, st, tmpl, n, blkoff, rank);
  const long long np = (long long)ys * xs;
  hipLaunchKernelGGL(llc_map_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, rank, nx, y0, ys, x0, xs,
                     idx);
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_llc_gather(const void* data_be, long long nvals, const int* idx, long long np, float* out, void* stream) {
  const uint32_t* data = static_cast<const uint32_t*>(data_be);
  if (np < 1 || nvals < 0) return SRMI_ERR_SHAPE;
  if (!data || !idx || !out) return SRMI_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(llc_gather_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, data, nvals, idx, np,
                     out);
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_tiles_nonfinite(const float* region, int C, int H, int W, int ty, int tx, int* bad, void* stream) {
  if (C < 1 || ty < 1 || tx < 1 || H < ty || W < tx) return SRMI_ERR_SHAPE;
  if (!region || !bad) return SRMI_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(tiles_nonfinite_kernel, dim3((H / ty) * (W / tx), C), dim3(256), 0, st, region, H, W, ty, tx,
                     W / tx, bad);
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_tiles_dry(const float* region, int C, int H, int W, int ty, int tx, int min_wet, int* bad, int* nwet,
                   void* stream) {
  if (C < 1 || ty < 1 || tx < 1 || H < ty || W < tx) return SRMI_ERR_SHAPE;
  if (!region || !bad || min_wet < 1) return SRMI_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(tiles_dry_kernel, dim3((H / ty) * (W / tx)), dim3(256), 0, st, region, C, H, W, ty, tx, W / tx,
                     min_wet, bad, nwet);
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_tiles_gather(const float* region, int C, int H, int W, int ty, int tx, const int* src, int nslots,
                      float* out, void* stream) {
  if (C < 1 || ty < 1 || tx < 1 || H < ty || W < tx || nslots < 0) return SRMI_ERR_SHAPE;
  if (nslots == 0) return 0;
  if (!region || !src || !out) return SRMI_ERR_ARG;
  const int gx = W / tx, ntile = (H / ty) * gx;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(tiles_gather_kernel, dim3((ty * tx + 1023) / 1024, nslots), dim3(256), 0, st, region, H, W, ty,
                     tx, gx, ntile, src, out);
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_llc_block_mask(const int* idx, long long np, int shift, int* mask, int n_blocks, void* stream) {
  if (np < 1 || shift < 0 || shift > 30 || n_blocks < 1) return SRMI_ERR_SHAPE;
  if (!idx || !mask) return SRMI_ERR_ARG;
  int* err = nullptr;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&err), sizeof(int));
  if (e != hipSuccess) return -(int)e;
  int herr = 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  e = hipMemsetAsync(err, 0, sizeof(int), st);
  if (e == hipSuccess) e = hipMemsetAsync(mask, 0, sizeof(int) * (size_t)n_blocks, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(llc_block_mask_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, idx, np, shift,
                       mask, n_blocks, err);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&herr, err, sizeof(int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(err);
  if (e != hipSuccess) return -(int)e;
  return herr ? SRMI_ERR_SHAPE : 0;
}

int srmi_llc_compact_map(const int* idx, long long np, int shift, const int* base, int n_blocks, int* out,
                         void* stream) {
  if (np < 1 || shift < 0 || shift > 30 || n_blocks < 1) return SRMI_ERR_SHAPE;
  if (!idx || !base || !out) return SRMI_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(llc_compact_map_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, idx, np, shift,
                     base, n_blocks, out);
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_tiles_keep(const int* bad, int C, int ncells, int* src, int* count, void* stream) {
  if (C < 1 || ncells < 1 || (long long)C * ncells > 0x7fffffffLL) return SRMI_ERR_SHAPE;
  if (!bad || !src || !count) return SRMI_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(tiles_keep_kernel, dim3(1), dim3(kKeepThreads), 0, st, bad, C, C * ncells, src, count);
  SRMI_CHECK_LAUNCH();
  return 0;
}

int srmi_tiles_gather_dev(const float* region, int C, int H, int W, int ty, int tx, const int* src,
                          const int* count, int max_slots, float* out, void* stream) {
  if (C < 1 || ty < 1 || tx < 1 || H < ty || W < tx || max_slots < 0) return SRMI_ERR_SHAPE;
  if ((long long)ty * tx > 65535LL * 1024) return SRMI_ERR_SHAPE;  // grid.y
  if (max_slots == 0) return 0;
  if (!region || !src || !count || !out) return SRMI_ERR_ARG;
  const int gx = W / tx, ntile = (H / ty) * gx;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(tiles_gather_dev_kernel, dim3(max_slots, (ty * tx + 1023) / 1024), dim3(256), 0, st, region, C, H,
                     W, ty, tx, gx, ntile, src, count, out);
  SRMI_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
