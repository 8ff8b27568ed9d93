// Box evaluation around the boxes-to-video chain (gfx950): what the reference's evaluation tools do on the host in numpy with a
// device-to-host copy of every candidate's frames.
//   ctrlv_best_candidate    per clip, the candidate with the largest mask IoU (tools/eval_overall.py:106-110), ties to the later one
//   ctrlv_gather_clips      dst[i] = src[winner[i]][i], the index read on the device
//   ctrlv_boundary_counts   the four counts of f_measure (src/ctrlv/metrics/FandJ.py:94-156): boundary maps, dilation by a disk
//   ctrlv_boundary_radius   its tolerance in pixels (host)
// The boundary kernel works on bit masks: one workgroup owns a band of rows of one frame, keeps the mask words of the band, its
// halo and the row below in LDS, turns them into boundary words by shift and xor and forms the dilation per row offset as a
// horizontal OR-spread; only eight integers per workgroup leave it.  Wave reductions first, one atomic per workgroup and value.
#include <math.h>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxCandidates = 8;
constexpr int kMaxRadius = 32;
constexpr size_t kLdsBytes = 60 * 1024;      // of the 64 KiB a launch may ask for without an attribute: room for the static arrays
typedef unsigned long long u64;
struct Spans { int8_t v[kMaxRadius + 4]; };      // a kernel argument by value

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---------------------------------------------------------------------------------------------------------------- the candidates
// One thread per clip.  counts [C][n][2][3]; the all-frames triple is the first of a block.
__global__ __launch_bounds__(kThreads) void best_candidate_kernel(const u64* __restrict__ counts, int n, int C,
                                                                   int32_t* __restrict__ winner) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  double best = -1.0;
  int w = 0;
  for (int c = 0; c < C; ++c) {
    const u64* t = counts + ((size_t)c * n + i) * 6;
    const u64 gt = t[0], pred = t[1], inter = t[2];
    const u64 uni = gt + pred - inter;
    const double iou = uni > 0 ? (double)inter / (double)uni : 1.0;      // IEEE division: numpy's quotient
    if (iou >= best) {                                                   // (>=: a later equal score replaces an earlier one)
      best = iou;
      w = c;
    }
  }
  winner[i] = w;
}

// blockIdx.x = clip * groups + group; the threads of a clip's groups stride over its 16-byte units (or its bytes).
__global__ __launch_bounds__(kThreads) void gather_clips_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ winner,
                                                                 int n, int C, size_t bpc, int groups, uint8_t* __restrict__ dst) {
  const int clip = blockIdx.x / groups;
  int w = winner[clip];
  w = w < 0 ? 0 : (w >= C ? C - 1 : w);
  const uint8_t* s = src + ((size_t)w * n + clip) * bpc;
  uint8_t* d = dst + (size_t)clip * bpc;
  const size_t t = (size_t)(blockIdx.x % groups) * kThreads + threadIdx.x, T = (size_t)groups * kThreads;
  if ((((uintptr_t)s ^ (uintptr_t)d) & 15) == 0) {
    size_t head = (size_t)(-(intptr_t)(uintptr_t)d & 15);
    if (head > bpc) head = bpc;
    const size_t units = (bpc - head) / 16, tail = bpc - head - units * 16;
    if (t < head) d[t] = s[t];
    const uint4* s4 = (const uint4*)(s + head);
    uint4* d4 = (uint4*)(d + head);
    for (size_t u = t; u < units; u += T) d4[u] = s4[u];
    if (t < tail) d[head + units * 16 + t] = s[head + units * 16 + t];
  } else {
    for (size_t b = t; b < bpc; b += T) d[b] = s[b];
  }
}

// ---------------------------------------------------------------------------------------------------------------- the boundaries
__device__ __forceinline__ bool in_mask(unsigned r, unsigned g, unsigned b, int mode) {
  return mode == 0 ? (r | g | b) != 0u : ((19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16) != 0u;
}

// the 16 mask bits of 16 consecutive pixels whose three channel planes start at p (16-byte aligned), HW apart
__device__ __forceinline__ unsigned mask16(const uint8_t* __restrict__ p, long HW, int mode) {
  __attribute__((aligned(16))) uint8_t c[3][16];
#pragma unroll
  for (int k = 0; k < 3; ++k) *(uint4*)&c[k][0] = *(const uint4*)(p + k * HW);
  unsigned m = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) m |= (in_mask(c[0][k], c[1][k], c[2][k], mode) ? 1u : 0u) << k;
  return m;
}

// bits of word k whose column is < lim
__device__ __forceinline__ u64 cols_below(int lim, int k) {
  const int left = lim - 64 * k;
  return left >= 64 ? ~0ull : (left <= 0 ? 0ull : (1ull << left) - 1ull);
}

// the word of row[k] after an OR-spread of the row by s columns to either side (0 <= s <= 32); lo / hi: row[k - 1] / row[k + 1]
__device__ __forceinline__ u64 spread(u64 lo, u64 mid, u64 hi, int s) {
  // towards lower columns on the pair (mid, hi), towards higher columns on the pair (lo, mid); the reach doubles per step
  u64 dm = mid, dh = hi;          // bit x = OR of the source over [x, x + reach]
  u64 ul = lo, um = mid;          // bit x = OR of the source over [x - reach, x]
  int reach = 0;
  while (reach < s) {
    const int step = reach + 1 < s - reach ? reach + 1 : s - reach;        // 1 <= step <= 32
    dm |= (dm >> step) | (dh << (64 - step));
    dh |= dh >> step;
    um |= (um << step) | (ul >> (64 - step));
    ul |= ul << step;
    reach += step;
  }
  return dm | um;
}

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// One workgroup: frame = blockIdx.x / bands, the rows [y0, y0 + band) of it.  LDS (dynamic): mask words [2][R + 1][Wd], then
// boundary words [2][R][Wd], R = band + 2 r; row j of either is image row y0 - r + j, a row outside the image holds zeros.
// span.v[dy] = floor(sqrt(r^2 - dy^2)), dy = 0 .. r.  counts [frame][4] = {n_fg, n_gt, fg_match, gt_match}.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void boundary_counts_kernel(const uint8_t* __restrict__ gt, const uint8_t* __restrict__ pred,
                                                                    int H, int W, int Wd, int band, int bands, int r, int mode,
                                                                    Spans span, u64* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) u64 lds[];
  const int R = band + 2 * r;
  u64* mask = lds;                              // [2][R + 1][Wd]
  u64* bnd = lds + (size_t)2 * (R + 1) * Wd;    // [2][R][Wd]
  __shared__ int8_t sp[kMaxRadius + 1];
  __shared__ unsigned part[kThreads / 64][4];
  const long frame = blockIdx.x / bands;
  const int y0 = (int)(blockIdx.x % bands) * band;
  const long HW = (long)H * W;
  const uint8_t* img[2] = {gt + frame * 3 * HW, pred + frame * 3 * HW};
  if (threadIdx.x <= r) sp[threadIdx.x] = span.v[threadIdx.x];

  // ---- 1. the mask words
  if constexpr (VEC) {
    // a task is 16 pixels: four consecutive lanes make one word
    const int upr = Wd * 4, real = W / 16;
    const int tasks = (R + 1) * upr;
    for (int t0 = 0; t0 < tasks; t0 += kThreads) {              // (tasks is a multiple of 4: a word's lanes stay together)
      const int t = t0 + threadIdx.x;
      const int j = t / upr, u = t % upr, y = y0 - r + j;
      const bool live = t < tasks && u < real && y >= 0 && y < H;
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        u64 v = 0;
        if (live) v = (u64)mask16(img[m] + (long)y * W + 16 * u, HW, mode) << (16 * (u & 3));
        v |= __shfl_xor(v, 1, 64);
        v |= __shfl_xor(v, 2, 64);
        if (t < tasks && (u & 3) == 0) mask[((size_t)m * (R + 1) + j) * Wd + (u >> 2)] = v;
      }
    }
  } else {
    // a task is one word: a wave takes it, one pixel per lane
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tasks = (R + 1) * Wd;
    for (int t = wave; t < tasks; t += kThreads / 64) {
      const int j = t / Wd, k = t % Wd, y = y0 - r + j, x = 64 * k + lane;
      const bool live = x < W && y >= 0 && y < H;
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        bool in = false;
        if (live) {
          const uint8_t* p = img[m] + (long)y * W + x;
          in = in_mask(p[0], p[HW], p[2 * HW], mode);
        }
        const u64 v = __ballot(in);
        if (lane == 0) mask[((size_t)m * (R + 1) + j) * Wd + k] = v;
      }
    }
  }
  __syncthreads();

  // ---- 2. the boundary words
  for (int t = threadIdx.x; t < 2 * R * Wd; t += kThreads) {
    const int m = t / (R * Wd), j = (t / Wd) % R, k = t % Wd, y = y0 - r + j;
    u64 b = 0;
    if (y >= 0 && y < H) {
      const u64* row = mask + ((size_t)m * (R + 1) + j) * Wd;
      const u64 a = row[k];
      const u64 right = (a >> 1) | (k + 1 < Wd ? row[k + 1] << 63 : 0ull);                  // S[y, x + 1] at bit x
      const u64 inner = cols_below(W - 1, k);
      b = (a ^ right) & inner;
      if (y < H - 1) {
        const u64 d = row[Wd + k];                                                            // S[y + 1, x]
        const u64 dright = (d >> 1) | (k + 1 < Wd ? row[Wd + k + 1] << 63 : 0ull);
        b |= ((a ^ d) & cols_below(W, k)) | ((a ^ dright) & inner);
      }
    }
    bnd[((size_t)m * R + j) * Wd + k] = b;
  }
  __syncthreads();

  // ---- 3. the counts of the band's own rows
  unsigned cnt[4] = {0u, 0u, 0u, 0u};
  const int rows = H - y0 < band ? H - y0 : band;
  for (int t = threadIdx.x; t < rows * Wd; t += kThreads) {
    const int j = r + t / Wd, k = t % Wd;
    const u64* bg = bnd + (size_t)j * Wd;
    const u64* bp = bnd + ((size_t)R + j) * Wd;
    u64 dg = 0, dp = 0;                     // the dilated boundary words at (j, k)
    for (int dy = 0; dy <= r; ++dy) {
      const int s = sp[dy];
      const long up = -(long)dy * Wd, dn = (long)dy * Wd;
      u64 g[3], p[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const int kk = k + q - 1;
        const bool in = kk >= 0 && kk < Wd;
        g[q] = in ? bg[up + kk] | bg[dn + kk] : 0ull;
        p[q] = in ? bp[up + kk] | bp[dn + kk] : 0ull;
      }
      dg |= spread(g[0], g[1], g[2], s);
      dp |= spread(p[0], p[1], p[2], s);
    }
    const u64 g = bg[k], p = bp[k];
    cnt[0] += __popcll(p);
    cnt[1] += __popcll(g);
    cnt[2] += __popcll(p & dg);
    cnt[3] += __popcll(g & dp);
  }
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const unsigned s = wave_sum(cnt[v]);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][v] = s;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    u64 s = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) s += part[w][threadIdx.x];
    if (s) atomicAdd(&counts[frame * 4 + threadIdx.x], s);
  }
}

// LDS bytes of a band of `band` rows
inline size_t band_bytes(int band, int r, int Wd) { return (size_t)8 * Wd * (4 * ((size_t)band + 2 * r) + 2); }

}  // namespace

extern "C" int ctrlv_best_candidate(const unsigned long long* counts, int n, int C, int32_t* winner, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(counts != nullptr && winner != nullptr, "best_candidate: null pointer");
  CTRLV_CHECK_ARG(((uintptr_t)counts & 7) == 0, "best_candidate: counts must be 8-byte aligned");
  CTRLV_CHECK_ARG(((uintptr_t)winner & 3) == 0, "best_candidate: winner must be 4-byte aligned");
  CTRLV_CHECK_SHAPE(C >= 1 && C <= kMaxCandidates, "best_candidate: C=%d candidates must be in [1, %d]", C, kMaxCandidates);
  CTRLV_CHECK_SHAPE(n > 0, "best_candidate: n=%d clips must be positive", n);
  hipLaunchKernelGGL(best_candidate_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                     counts, n, C, winner);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

extern "C" int ctrlv_gather_clips(const void* src, const int32_t* winner, int n, int C, size_t bytes_per_clip, void* dst,
                                  ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(src != nullptr && winner != nullptr && dst != nullptr, "gather_clips: null pointer");
  CTRLV_CHECK_ARG(((uintptr_t)winner & 3) == 0, "gather_clips: winner must be 4-byte aligned");
  CTRLV_CHECK_SHAPE(C >= 1 && C <= kMaxCandidates, "gather_clips: C=%d candidates must be in [1, %d]", C, kMaxCandidates);
  CTRLV_CHECK_SHAPE(n > 0, "gather_clips: n=%d clips must be positive", n);
  CTRLV_CHECK_SHAPE(bytes_per_clip > 0, "gather_clips: bytes_per_clip is 0");
  // enough groups to give every thread one 16-byte unit, at most 4096 per clip (the threads stride), under 2^31 - 1 in all
  size_t groups = (bytes_per_clip / 16 + kThreads) / kThreads;
  const size_t cap = 0x7fffffffull / (size_t)n;
  CTRLV_CHECK_SHAPE(cap >= 1, "gather_clips: n=%d clips need more than 2^31 - 1 workgroups", n);
  if (groups > 4096) groups = 4096;
  if (groups > cap) groups = cap;
  hipLaunchKernelGGL(gather_clips_kernel, dim3((unsigned)(groups * (size_t)n)), dim3(kThreads), 0, (hipStream_t)stream,
                     (const uint8_t*)src, winner, n, C, bytes_per_clip, (int)groups, (uint8_t*)dst);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

extern "C" int ctrlv_boundary_radius(int H, int W, double bound_th) {
  CTRLV_CHECK_SHAPE(H > 0 && W > 0, "boundary_radius: H=%d, W=%d must be positive", H, W);
  CTRLV_CHECK_ARG(isfinite(bound_th) && bound_th >= 0.0, "boundary_radius: bound_th=%g must be finite and not negative", bound_th);
  if (bound_th >= 1.0) {
    CTRLV_CHECK_ARG(bound_th == floor(bound_th) && bound_th <= 1e9, "boundary_radius: bound_th=%g is >= 1 and must then be an "
                    "integer number of pixels", bound_th);
    return (int)bound_th;
  }
  const double diag = sqrt((double)((long long)H * H + (long long)W * W));
  const double r = ceil(bound_th * diag);
  return r > 1e9 ? 1000000000 : (int)r;
}

extern "C" int ctrlv_boundary_counts(const void* gt_u8, const void* pred_u8, int n, int F, int H, int W, int mask_mode, int radius,
                                     unsigned long long* counts, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(gt_u8 && pred_u8 && counts, "boundary_counts: null pointer");
  CTRLV_CHECK_ARG(((uintptr_t)counts & 7) == 0, "boundary_counts: counts must be 8-byte aligned");
  CTRLV_CHECK_SHAPE(radius >= 1 && radius <= kMaxRadius, "boundary_counts: radius=%d must be in [1, %d]", radius, kMaxRadius);
  CTRLV_CHECK_SHAPE(mask_mode == 0 || mask_mode == 1, "boundary_counts: mask_mode=%d must be 0 (any channel) or 1 (luma)", mask_mode);
  CTRLV_CHECK_SHAPE(n > 0 && F > 0 && H > 0 && W > 0, "boundary_counts: n, F, H, W must be positive (got %d, %d, %d, %d)", n, F, H, W);
  const int Wd = (W + 63) / 64;
  CTRLV_CHECK_SHAPE(band_bytes(1, radius, Wd) <= kLdsBytes, "boundary_counts: a width of %d pixels does not fit the LDS layout at "
                    "radius %d (%zu bytes for one row and its halo, %zu at hand)", W, radius, band_bytes(1, radius, Wd), kLdsBytes);
  // the tallest band that fits, at most 32 rows and no taller than the image; then the bands are evened out.  (Shorter bands
  // read more halo and give more workgroups: 25 x 576 x 1024 at radius 10 took 85 us with 64 rows, 58 with 32, 53 with 16)
  int band = (int)((kLdsBytes / ((size_t)8 * Wd) - 2) / 4) - 2 * radius;
  if (band > 32) band = 32;
  if (band > H) band = H;
  int bands = (H + band - 1) / band;
  band = (H + bands - 1) / bands;
  bands = (H + band - 1) / band;
  CTRLV_CHECK_SHAPE((long)bands * n * F <= 0x7fffffffL, "boundary_counts: %d x %d frames of %d rows need more than 2^31 - 1 "
                    "workgroups", n, F, H);
  const hipStream_t s = (hipStream_t)stream;
  Spans spans;                       // span[dy] = floor(sqrt(radius^2 - dy^2)): the half-width of the disk dy rows away
  for (int dy = 0; dy < (int)sizeof(spans.v); ++dy) {
    int sx = 0;
    while (dy <= radius && (sx + 1) * (sx + 1) + dy * dy <= radius * radius) ++sx;
    spans.v[dy] = (int8_t)sx;
  }
  CTRLV_HIP_TRY(hipMemsetAsync(counts, 0, (size_t)n * F * 4 * sizeof(unsigned long long), s));
  const size_t smem = band_bytes(band, radius, Wd);
  const dim3 grid((unsigned)((long)bands * n * F));
  const bool vec = W % 16 == 0 && aligned16(gt_u8) && aligned16(pred_u8);
  if (vec)
    hipLaunchKernelGGL(boundary_counts_kernel<true>, grid, dim3(kThreads), smem, s, (const uint8_t*)gt_u8, (const uint8_t*)pred_u8, H,
                       W, Wd, band, bands, radius, mask_mode, spans, counts);
  else
    hipLaunchKernelGGL(boundary_counts_kernel<false>, grid, dim3(kThreads), smem, s, (const uint8_t*)gt_u8, (const uint8_t*)pred_u8,
                       H, W, Wd, band, bands, radius, mask_mode, spans, counts);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}
