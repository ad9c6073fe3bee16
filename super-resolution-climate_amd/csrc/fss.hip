// Fractions skill score of a super-resolved field (Roberts & Lean 2008): for a threshold, the
// event fraction of a prediction and of a truth in n x n neighbourhoods, for a ladder of n --
// no reference counterpart.  srmi.h states the definition ("the fractions skill score");
// tests/fss_oracle.py restates it in numpy.  Every sum is an integer.
//
// Launches, no global atomics, no host read:
//   fss_events_kernel   one read of the two fields.  A wave takes 64 pixels of a row; per
//       threshold the wave's __ballot of the event IS the packed word of a bit plane in the
//       workspace (bits past W are zero).  used and events are popcounts, summed per workgroup
//       and stored as uint32 partials.
//   fss_windows_kernel  the grid is (channel, threshold, scale, tile), a tile being kFssTileH
//       rows of one 64-pixel word column; each of the four waves walks kFssBandH rows of it
//       downwards.  The count of a row's bits in columns x - h .. x + h is the popcount of the
//       (at most five) words around the lane's word under per-lane masks that do not change
//       from row to row (the words are the same for every lane: scalar loads; a plane's rows
//       are padded by two words either side so that the five are contiguous, and the mask of a
//       padding word is empty); the window count slides down: it gains the row entering and loses the
//       row leaving.  Nothing loops over the n x n window: the work per output position is four
//       such row counts, whatever n.  num and den are 64-bit per lane, then per workgroup.
//   fss_finish_kernel   one workgroup per (channel, threshold): the partials of both launches
//       and the derived values.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.hpp"
#include "srmi_internal.hpp"

namespace srmi {

namespace {

typedef unsigned long long u64;

constexpr int kFssThreads = 256;
constexpr int kFssWaves = kFssThreads / 64;
constexpr int kFssMaxT = 8, kFssMaxN = 16, kFssMaxScale = 255;
constexpr int kFssEvSlots = 1 + 2 * kFssMaxT;  // used, then {pred, truth} per threshold
constexpr int kFssEvPerWave = 8;               // 64-pixel row segments a wave of the events launch takes
constexpr int kFssEvPerBlock = kFssEvPerWave * kFssWaves;
constexpr int kFssBandH = 128;                 // rows a wave of the windows launch walks
constexpr int kFssTileH = kFssBandH * kFssWaves, kFssTileW = 64;  // srmi.fss.FSS_TILE
constexpr int kFssHalfWords = 2;               // words beside the lane's own that a 255-wide window can reach

struct FssPlan {
  int Ww, pitch;           // 64-bit words of a row of a bit plane, and with its padding
  int items;               // H * Ww, the 64-pixel row segments of a plane (at most H W)
  long long plane_words;   // H * pitch
  int ev_blocks;           // workgroups of the events launch per channel
  int tiles_y, tiles;      // of the windows launch, per plane
  size_t off_ev, off_win;  // byte offsets of the two partial tables behind the bit planes
  size_t bytes;
};

struct FssScales {
  int n[kFssMaxN];
};

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

int fss_plan(int C, int H, int W, int T, int N, FssPlan* p) {
  if (C < 1 || H < 1 || W < 1 || (long long)H * W > 2147483647LL || T < 1 || T > kFssMaxT || N < 1 || N > kFssMaxN)
    return SRMI_ERR_ARG;
  p->Ww = (W + 63) / 64;
  p->pitch = p->Ww + 2 * kFssHalfWords;
  p->items = H * p->Ww;
  p->plane_words = (long long)H * p->pitch;
  const long long evb = ((long long)p->items + kFssEvPerBlock - 1) / kFssEvPerBlock;
  p->tiles_y = (H + kFssTileH - 1) / kFssTileH;
  const long long tiles = (long long)p->tiles_y * p->Ww;
  if (evb * C >= (1LL << 31) || tiles * C * T * N >= (1LL << 31)) return SRMI_ERR_ARG;
  p->ev_blocks = (int)evb;
  p->tiles = (int)tiles;
  p->off_ev = align16((size_t)C * T * 2 * (size_t)p->plane_words * sizeof(u64));
  p->off_win = p->off_ev + align16((size_t)C * kFssEvSlots * (size_t)evb * sizeof(uint32_t));
  p->bytes = p->off_win + (size_t)C * T * N * (size_t)tiles * 2 * sizeof(u64);
  return 0;
}

__device__ __forceinline__ bool fss_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__global__ void __launch_bounds__(kFssThreads) fss_events_kernel(const float* __restrict__ pred,
                                                                 const float* __restrict__ truth,
                                                                 const float* __restrict__ thr, int H, int W, int T,
                                                                 FssPlan plan, char* __restrict__ ws) {
  __shared__ uint32_t red[kFssWaves][kFssEvSlots];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = blockIdx.x / plan.ev_blocks, g = blockIdx.x % plan.ev_blocks;
  const size_t pbase = (size_t)c * (size_t)H * (size_t)W;
  u64* planes = reinterpret_cast<u64*>(ws) + (size_t)c * 2 * T * (size_t)plan.plane_words;
  float th[kFssMaxT];
#pragma unroll
  for (int t = 0; t < kFssMaxT; ++t) th[t] = thr[c * T + min(t, T - 1)];
  uint32_t nused = 0, cnt = 0;  // cnt: lane 2 t counts the prediction's events of threshold t, lane 2 t + 1 the truth's
  // every load first (a segment past the plane's end reads the last one and is not used)
  const unsigned item0 = (unsigned)g * kFssEvPerBlock + wave;  // items <= H W < 2^31: below 2^32 with the round-up
  float pv[kFssEvPerWave], tv[kFssEvPerWave];
#pragma unroll
  for (int i = 0; i < kFssEvPerWave; ++i) {
    const unsigned item = min(item0 + i * kFssWaves, (unsigned)plan.items - 1u);
    const int y = (int)(item / (unsigned)plan.Ww), x = (int)(item % (unsigned)plan.Ww) * kFssTileW + lane;
    const size_t at = pbase + (size_t)y * W + (x < W ? x : 0);
    pv[i] = pred[at];
    tv[i] = truth[at];
  }
#pragma unroll
  for (int i = 0; i < kFssEvPerWave; ++i) {
    const unsigned item = item0 + i * kFssWaves;
    if (item < (unsigned)plan.items) {  // the same for every lane
      const int y = (int)(item / (unsigned)plan.Ww), wx = (int)(item % (unsigned)plan.Ww);
      const bool in = wx * kFssTileW + lane < W;
      const bool used = in && fss_finite(pv[i]) && fss_finite(tv[i]);
      nused += (uint32_t)__popcll(__ballot(used));
      u64 word = 0;
#pragma unroll
      for (int t = 0; t < kFssMaxT; ++t) {
        if (t < T) {
          const u64 bp = __ballot(used && pv[i] >= th[t]);
          const u64 bt = __ballot(used && tv[i] >= th[t]);
          if (lane == 2 * t) word = bp;
          if (lane == 2 * t + 1) word = bt;
        }
      }
      if (lane < 2 * T) {
        planes[(size_t)lane * (size_t)plan.plane_words + (size_t)y * plan.pitch + kFssHalfWords + wx] = word;
        cnt += (uint32_t)__popcll(word);
      }
    }
  }
  if (lane == 63) red[wave][0] = nused;
  if (lane < 2 * T) red[wave][1 + lane] = cnt;
  __syncthreads();
  if (tid < 1 + 2 * T) {
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < kFssWaves; ++w) s += red[w][tid];
    uint32_t* ev = reinterpret_cast<uint32_t*>(ws + plan.off_ev);
    ev[((size_t)c * kFssEvSlots + tid) * (size_t)plan.ev_blocks + g] = s;
  }
}

// bits lo .. hi of a word, clipped to 0 .. 63; empty when the range misses the word
__device__ __forceinline__ u64 fss_bit_range(int lo, int hi) {
  if (hi < 0 || lo > 63 || hi < lo) return 0;
  lo = max(lo, 0);
  hi = min(hi, 63);
  return (~0ULL >> (63 - hi)) & (~0ULL << lo);
}

// the events of one row in columns x - h .. x + h of the lane's pixel: R words each side of
// the lane's own.  row points at the word two to the left of the lane's own and is the same
// for every lane (scalar loads of neighbouring words), m is the lane's
template <int R>
__device__ __forceinline__ int fss_row_count(const u64* __restrict__ row, const u64 (&m)[2 * kFssHalfWords + 1]) {
  int cnt = 0;
#pragma unroll
  for (int j = kFssHalfWords - R; j <= kFssHalfWords + R; ++j) cnt += __popcll(row[j] & m[j]);
  return cnt;
}

// bp, bt: the word two to the left of the lane's own in row 0 of the two bit planes
template <int R>
__device__ __forceinline__ void fss_walk(const u64* __restrict__ bp, const u64* __restrict__ bt, int pitch, int H, int h,
                                         int ys, int ye, const u64 (&m)[2 * kFssHalfWords + 1], bool live, u64& num,
                                         u64& den) {
  int sp = 0, st = 0;
  for (int r = max(ys - h, 0); r <= min(ys + h, H - 1); ++r) {
    sp += fss_row_count<R>(bp + (size_t)r * pitch, m);
    st += fss_row_count<R>(bt + (size_t)r * pitch, m);
  }
  for (int y = ys; y < ye; ++y) {
    if (live) {
      const int d = sp - st;
      num += (u64)((long long)d * d);
      den += (u64)sp * (u64)sp + (u64)st * (u64)st;
    }
    // the row entering and the row leaving, the same for every lane; one outside the plane is
    // read at the plane's edge and counts nothing, so that all loads of a step go out together
    const int in = y + h + 1, out = y - h;
    const int gin = in < H ? -1 : 0, gout = out >= 0 ? -1 : 0;
    const size_t oin = (size_t)min(in, H - 1) * pitch, oout = (size_t)max(out, 0) * pitch;
    const int pin = fss_row_count<R>(bp + oin, m), tin = fss_row_count<R>(bt + oin, m);
    const int pout = fss_row_count<R>(bp + oout, m), tout = fss_row_count<R>(bt + oout, m);
    sp += (pin & gin) - (pout & gout);
    st += (tin & gin) - (tout & gout);
  }
}

__global__ void __launch_bounds__(kFssThreads) fss_windows_kernel(int H, int W, int T, int N, FssScales scales,
                                                                  FssPlan plan, char* __restrict__ ws) {
  __shared__ u64 red[2][kFssThreads];
  const int tid = threadIdx.x, lane = tid & 63;
  const int band = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = blockIdx.x % plan.tiles, rest = blockIdx.x / plan.tiles;
  const int k = rest % N, ct = rest / N;  // ct = c T + t
  const int wx = tile % plan.Ww, ty = tile / plan.Ww;
  const int h = (scales.n[k] - 1) / 2;
  // a row of a bit plane has two words of padding on either side (never written, never
  // counted), so word wx + kFssHalfWords of it is the lane's own
  const u64* bp = reinterpret_cast<const u64*>(ws) + (size_t)ct * 2 * (size_t)plan.plane_words + wx;
  const u64* bt = bp + plan.plane_words;
  // the bits of word j - 2 beside the lane's own that lie inside the lane's window; the mask
  // of a word that is padding is empty, whatever the padding holds
  u64 m[2 * kFssHalfWords + 1];
#pragma unroll
  for (int j = 0; j <= 2 * kFssHalfWords; ++j) {
    const int w = wx + j - kFssHalfWords, rel = 64 * (j - kFssHalfWords);
    m[j] = (w >= 0 && w < plan.Ww) ? fss_bit_range(lane - h - rel, lane + h - rel) : 0;
  }
  const int ys = ty * kFssTileH + band * kFssBandH, ye = min(ys + kFssBandH, H);
  const bool live = wx * kFssTileW + lane < W;
  u64 num = 0, den = 0;
  if (ys < ye) {
    if (h == 0)
      fss_walk<0>(bp, bt, plan.pitch, H, h, ys, ye, m, live, num, den);
    else if (h <= 64)
      fss_walk<1>(bp, bt, plan.pitch, H, h, ys, ye, m, live, num, den);
    else
      fss_walk<2>(bp, bt, plan.pitch, H, h, ys, ye, m, live, num, den);
  }
  red[0][tid] = num;
  red[1][tid] = den;
  __syncthreads();
  for (int w = kFssThreads / 2; w > 0; w >>= 1) {
    if (tid < w) {
      red[0][tid] += red[0][tid + w];
      red[1][tid] += red[1][tid + w];
    }
    __syncthreads();
  }
  if (tid < 2) {
    u64* part = reinterpret_cast<u64*>(ws + plan.off_win);
    part[(size_t)blockIdx.x * 2 + tid] = red[tid][0];
  }
}

__device__ __forceinline__ u64 fss_block_sum(u64 v, u64* sh) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int w = kFssThreads / 2; w > 0; w >>= 1) {
    if (tid < w) sh[tid] += sh[tid + w];
    __syncthreads();
  }
  const u64 r = sh[0];
  __syncthreads();
  return r;
}

__global__ void __launch_bounds__(kFssThreads) fss_finish_kernel(int T, int N, FssScales scales, FssPlan plan,
                                                                 const char* __restrict__ ws,
                                                                 long long* __restrict__ num, long long* __restrict__ den,
                                                                 long long* __restrict__ events,
                                                                 long long* __restrict__ used,
                                                                 double* __restrict__ derived) {
  __shared__ u64 sh[kFssThreads];
  __shared__ u64 tab[2][kFssMaxN];
  const int tid = threadIdx.x;
  const int ct = blockIdx.x, c = ct / T, t = ct % T;
  const uint32_t* ev = reinterpret_cast<const uint32_t*>(ws + plan.off_ev) + (size_t)c * kFssEvSlots * plan.ev_blocks;
  u64 s[3] = {0, 0, 0};
  for (int g = tid; g < plan.ev_blocks; g += kFssThreads) {
    s[0] += ev[g];
    s[1] += ev[(size_t)(1 + 2 * t) * plan.ev_blocks + g];
    s[2] += ev[(size_t)(2 + 2 * t) * plan.ev_blocks + g];
  }
  const u64 nu = fss_block_sum(s[0], sh), ep = fss_block_sum(s[1], sh), et = fss_block_sum(s[2], sh);
  const u64* part = reinterpret_cast<const u64*>(ws + plan.off_win) + (size_t)ct * N * plan.tiles * 2;
  for (int k = 0; k < N; ++k) {
    u64 a = 0, b = 0;
    for (int i = tid; i < plan.tiles; i += kFssThreads) {
      a += part[((size_t)k * plan.tiles + i) * 2];
      b += part[((size_t)k * plan.tiles + i) * 2 + 1];
    }
    a = fss_block_sum(a, sh);
    b = fss_block_sum(b, sh);
    if (tid == 0) {
      tab[0][k] = a;
      tab[1][k] = b;
    }
  }
  if (tid != 0) return;
  if (t == 0) used[c] = (long long)nu;
  events[(size_t)ct * 2] = (long long)ep;
  events[(size_t)ct * 2 + 1] = (long long)et;
  double* d = derived + (size_t)ct * (N + 6);
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  for (int k = 0; k < N; ++k) {
    num[(size_t)ct * N + k] = (long long)tab[0][k];
    den[(size_t)ct * N + k] = (long long)tab[1][k];
  }
  if (nu == 0) {  // no used pixel: NaN in every derived entry (the tables are 0 by themselves)
    for (int k = 0; k < N + 6; ++k) d[k] = nan;
    return;
  }
  const double dep = (double)(long long)ep, det = (double)(long long)et, dn = (double)(long long)nu;
  const double f_truth = det / dn, target = 0.5 + f_truth / 2.0;
  double skilful = nan;
  for (int k = N - 1; k >= 0; --k) {
    const double f = tab[1][k] == 0 ? nan : 1.0 - (double)(long long)tab[0][k] / (double)(long long)tab[1][k];
    d[k] = f;
    if (f >= target) skilful = (double)scales.n[k];
  }
  d[N] = dep / dn;
  d[N + 1] = f_truth;
  d[N + 2] = dep / det;
  d[N + 3] = target;
  d[N + 4] = 2.0 * dep * det / (dep * dep + det * det);
  d[N + 5] = skilful;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace srmi

using namespace srmi;

extern "C" {

int srmi_fss_workspace(int C, int H, int W, int T, int N, size_t* bytes) {
  FssPlan p;
  if (!bytes) return SRMI_ERR_ARG;
  const int rc = fss_plan(C, H, W, T, N, &p);
  if (rc) return rc;
  *bytes = p.bytes;
  return 0;
}

int srmi_fss(const float* pred, const float* truth, int C, int H, int W, const float* thresholds, int T,
             const int* scales, int N, void* workspace, size_t workspace_bytes, long long* num, long long* den,
             long long* events, long long* used, double* derived, int launches, void* stream) {
  FssPlan p;
  if (launches & ~(SRMI_FSS_EVENTS | SRMI_FSS_WINDOWS | SRMI_FSS_FINISH)) return SRMI_ERR_ARG;
  if (!pred || !truth || !thresholds || !scales || !workspace || !aligned16(workspace) || !num || !den || !events ||
      !used || !derived)
    return SRMI_ERR_ARG;
  const int rc = fss_plan(C, H, W, T, N, &p);
  if (rc) return rc;
  if (workspace_bytes < p.bytes) return SRMI_ERR_ARG;
  FssScales sc;
  for (int k = 0; k < kFssMaxN; ++k) sc.n[k] = 1;
  for (int k = 0; k < N; ++k) {
    const int n = scales[k];
    if (n < 1 || n > kFssMaxScale || n % 2 == 0 || (k > 0 && n <= scales[k - 1])) return SRMI_ERR_ARG;
    sc.n[k] = n;
  }
  const u64 nmax = (u64)sc.n[N - 1];
  if ((u64)H * (u64)W * (nmax * nmax * nmax * nmax) > (1ULL << 62)) return SRMI_ERR_ARG;  // below 2^63: no wrap
  char* w = static_cast<char*>(workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 block(kFssThreads);
  if (!launches) launches = SRMI_FSS_EVENTS | SRMI_FSS_WINDOWS | SRMI_FSS_FINISH;
  if (launches & SRMI_FSS_EVENTS) {
    hipLaunchKernelGGL(fss_events_kernel, dim3((unsigned)(C * p.ev_blocks)), block, 0, st, pred, truth, thresholds, H,
                       W, T, p, w);
    SRMI_CHECK_LAUNCH();
  }
  if (launches & SRMI_FSS_WINDOWS) {
    hipLaunchKernelGGL(fss_windows_kernel, dim3((unsigned)(C * T * N * p.tiles)), block, 0, st, H, W, T, N, sc, p, w);
    SRMI_CHECK_LAUNCH();
  }
  if (launches & SRMI_FSS_FINISH) {
    hipLaunchKernelGGL(fss_finish_kernel, dim3((unsigned)(C * T)), block, 0, st, T, N, sc, p, w, num, den, events,
                       used, derived);
    SRMI_CHECK_LAUNCH();
  }
  return 0;
}

}  // extern "C"
