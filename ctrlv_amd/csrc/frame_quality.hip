// Per-frame quality of a generated clip against its ground truth (gfx950): the ssim_score_image / psnr_score_image numbers of the
// reference's evaluate_vids (src/ctrlv/metrics/fvd.py:251-267), which it forms on the host with scikit-image after a copy of
// every frame.
//   ctrlv_frame_stats   per frame {min byte, max byte, sum of squared byte differences}: the integers PSNR is made of, and the
//                       joint value range R both metrics scale by
//   ctrlv_frame_ssim    structural_similarity(channel_axis=0, data_range=R, gaussian_weights=True, sigma=1.5) per frame
// The SSIM kernel is a separable 11 x 11 stencil over five moment images (x, y, x^2, y^2, xy).  One workgroup owns a tile of
// output pixels of one channel of one frame: the tile and its halo of both frames go into LDS once, a horizontal pass leaves the
// five row-filtered moments in LDS, the vertical pass and the SSIM expression run from there; the filtered images never reach
// HBM.  The moments are taken about the frame's midpoint (min + max) / 2 -- variances are shift-invariant, the means are shifted
// back -- so that every term scales with R^2 as C1 and C2 do: about 127.5, fp32 cancels in u_xx - u_x^2 on low-contrast frames.
// No floating-point atomics: a workgroup adds its S values in a fixed order into its own slot, a second launch adds a frame's
// slots in a fixed order.  A frame's value never depends on n, on its neighbours or on the pointers' alignment.
#include <math.h>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTaps = 11, kHalo = 5;            // the window of sigma = 1.5 truncated at 3.5 sigma
constexpr int kTW = 64, kTH = 16;               // output pixels of a workgroup
constexpr int kBlk = 4;                         // outputs a thread forms per pass from one run of 14 inputs held in registers
constexpr int kIW = kTW + 2 * kHalo + 2, kIH = kTH + 2 * kHalo;         // (76 columns: rows of whole 16-byte units)
static_assert(kTW == 64 && kTH == kBlk * (kThreads / 64) && kIW % 4 == 0 && kIW >= kTW + 3 * kBlk, "the passes' thread maps");
// LDS of the SSIM kernel: 2 x 26 x 76 + 5 x 26 x 64 floats + four doubles = 49120 bytes, under the 64 KiB a workgroup may hold
// statically.  The horizontal pass reads and writes 16-byte units, consecutive lanes at consecutive units; the vertical pass
// reads single floats, consecutive lanes at consecutive columns: no bank conflicts in either.
typedef unsigned long long u64;
struct Window { float g[kTaps]; };              // a kernel argument by value

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---------------------------------------------------------------------------------------------------------------- the integers
__global__ void frame_stats_init_kernel(u64* __restrict__ stats, long frames) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= frames) return;
  stats[3 * i] = 255ull;
  stats[3 * i + 1] = 0ull;
  stats[3 * i + 2] = 0ull;
}

// blockIdx.x = frame * groups + group; the threads of a frame's groups stride over its 16-byte units (or its bytes).
template <bool VEC>
__global__ __launch_bounds__(kThreads) void frame_stats_kernel(const uint8_t* __restrict__ gt, const uint8_t* __restrict__ gen,
                                                                size_t per, int groups, u64* __restrict__ stats) {
  __shared__ unsigned plo[kThreads / 64], phi[kThreads / 64];
  __shared__ u64 pss[kThreads / 64];
  const size_t frame = blockIdx.x / groups;
  const uint8_t* a = gt + frame * per;
  const uint8_t* b = gen + frame * per;
  const size_t t = (size_t)(blockIdx.x % groups) * kThreads + threadIdx.x, T = (size_t)groups * kThreads;
  unsigned lo = 255u, hi = 0u;
  u64 sse = 0;
  if constexpr (VEC) {
    const uint4* a4 = (const uint4*)a;
    const uint4* b4 = (const uint4*)b;
    const size_t units = per / 16;
    for (size_t u = t; u < units; u += T) {
      const uint4 qa = a4[u], qb = b4[u];
      const unsigned wa[4] = {qa.x, qa.y, qa.z, qa.w}, wb[4] = {qb.x, qb.y, qb.z, qb.w};
      unsigned s = 0;                                       // 16 x 255^2 fits easily
#pragma unroll
      for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const unsigned x = (wa[k] >> (8 * j)) & 255u, y = (wb[k] >> (8 * j)) & 255u;
          lo = min(lo, min(x, y));
          hi = max(hi, max(x, y));
          const int d = (int)x - (int)y;
          s += (unsigned)(d * d);
        }
      }
      sse += s;
    }
  } else {
    for (size_t i = t; i < per; i += T) {
      const unsigned x = a[i], y = b[i];
      lo = min(lo, min(x, y));
      hi = max(hi, max(x, y));
      const int d = (int)x - (int)y;
      sse += (unsigned)(d * d);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = min(lo, (unsigned)__shfl_down(lo, off, 64));
    hi = max(hi, (unsigned)__shfl_down(hi, off, 64));
    sse += __shfl_down(sse, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    plo[threadIdx.x >> 6] = lo;
    phi[threadIdx.x >> 6] = hi;
    pss[threadIdx.x >> 6] = sse;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) {
      lo = min(lo, plo[w]);
      hi = max(hi, phi[w]);
      sse += pss[w];
    }
    atomicMin(&stats[frame * 3], (u64)lo);
    atomicMax(&stats[frame * 3 + 1], (u64)hi);
    if (sse) atomicAdd(&stats[frame * 3 + 2], sse);
  }
}

// ---------------------------------------------------------------------------------------------------------------- SSIM
// blockIdx.x = ((frame * 3 + channel) * tiles_y + ty) * tiles_x + tx.  Output pixel (oy, ox) of the cropped image is image pixel
// (oy + 5, ox + 5); its window covers the image rows oy .. oy + 10 and columns ox .. ox + 10, all inside the image.
// Every product that SSIM compares with another is formed by its own rounded operation (__fmul_rn / __fadd_rn / fmaf, never a
// contraction the compiler picks): with gen == gt the five moments pair up bit for bit and S is exactly 1.
__global__ __launch_bounds__(kThreads) void frame_ssim_kernel(const uint8_t* __restrict__ gt, const uint8_t* __restrict__ gen,
                                                               int H, int W, int tiles_x, int tiles_y,
                                                               const long long* __restrict__ stats, const Window win,
                                                               double* __restrict__ slots) {
  __shared__ __attribute__((aligned(16))) float in[2][kIH][kIW];
  __shared__ __attribute__((aligned(16))) float mom[5][kIH][kTW];
  __shared__ double part[kThreads / 64];
  const int tid = threadIdx.x;
  const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y;
  const long plane = blockIdx.x / ((unsigned)tiles_x * tiles_y);             // frame * 3 + channel
  const long frame = plane / 3;
  const float lo = (float)stats[frame * 3], hi = (float)stats[frame * 3 + 1];
  const float m = 0.5f * (lo + hi), R = hi - lo;                             // exact: halves of small integers
  const uint8_t* img[2] = {gt + plane * H * W, gen + plane * H * W};
  const int y0 = ty * kTH, x0 = tx * kTW;

  // ---- 1. the tile and its halo, as b - m (exact in fp32); outside the image: 0, never used by a live output
  for (int i = tid; i < kIH * kIW; i += kThreads) {
    const int r = i / kIW, q = i % kIW;
    const int y = y0 + r, x = x0 + q;
    const bool live = y < H && x < W;
#pragma unroll
    for (int f = 0; f < 2; ++f) in[f][r][q] = live ? (float)img[f][(long)y * W + x] - m : 0.f;
  }
  __syncthreads();

  // ---- 2. the horizontal pass: a thread takes four neighbouring output columns of one row -- 14 inputs of each frame, read as
  // 16-byte units, their three products formed once -- and leaves the five moments of each; tap order 0 .. 10 per output
  for (int i = tid; i < kIH * (kTW / kBlk); i += kThreads) {
    const int r = i / (kTW / kBlk), c = (i % (kTW / kBlk)) * kBlk;
    float x[4 * kBlk], y[4 * kBlk];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float4 vx = *(const float4*)&in[0][r][c + 4 * j], vy = *(const float4*)&in[1][r][c + 4 * j];
      x[4 * j] = vx.x; x[4 * j + 1] = vx.y; x[4 * j + 2] = vx.z; x[4 * j + 3] = vx.w;
      y[4 * j] = vy.x; y[4 * j + 1] = vy.y; y[4 * j + 2] = vy.z; y[4 * j + 3] = vy.w;
    }
    float a[kBlk][5];
#pragma unroll
    for (int o = 0; o < kBlk; ++o)
#pragma unroll
      for (int k = 0; k < 5; ++k) a[o][k] = 0.f;
#pragma unroll
    for (int j = 0; j < kTaps + kBlk - 1; ++j) {
      const float xx = __fmul_rn(x[j], x[j]), yy = __fmul_rn(y[j], y[j]), xy = __fmul_rn(x[j], y[j]);
#pragma unroll
      for (int o = 0; o < kBlk; ++o) {
        const int t = j - o;
        if (t < 0 || t >= kTaps) continue;
        const float g = win.g[t];
        a[o][0] = fmaf(g, x[j], a[o][0]);
        a[o][1] = fmaf(g, y[j], a[o][1]);
        a[o][2] = fmaf(g, xx, a[o][2]);
        a[o][3] = fmaf(g, yy, a[o][3]);
        a[o][4] = fmaf(g, xy, a[o][4]);
      }
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) *(float4*)&mom[k][r][c] = make_float4(a[0][k], a[1][k], a[2][k], a[3][k]);
  }
  __syncthreads();

  // ---- 3. the vertical pass and S: a thread takes four output rows of one column (a wave: four rows of the tile)
  const float C1 = __fmul_rn(__fmul_rn(0.01f, R), __fmul_rn(0.01f, R)), C2 = __fmul_rn(__fmul_rn(0.03f, R), __fmul_rn(0.03f, R));
  const float cov = 121.f / 120.f, shift = m - 127.5f;
  const int q = tid & 63, r0 = (tid >> 6) * kBlk;
  float u[kBlk][5];
#pragma unroll
  for (int o = 0; o < kBlk; ++o)
#pragma unroll
    for (int k = 0; k < 5; ++k) u[o][k] = 0.f;
#pragma unroll
  for (int j = 0; j < kTaps + kBlk - 1; ++j) {
    float v[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] = mom[k][r0 + j][q];
#pragma unroll
    for (int o = 0; o < kBlk; ++o) {
      const int t = j - o;
      if (t < 0 || t >= kTaps) continue;
#pragma unroll
      for (int k = 0; k < 5; ++k) u[o][k] = fmaf(win.g[t], v[k], u[o][k]);
    }
  }
  double acc = 0.0;
#pragma unroll
  for (int o = 0; o < kBlk; ++o) {
    if (y0 + r0 + o >= H - 2 * kHalo || x0 + q >= W - 2 * kHalo) continue;
    const float vx = __fmul_rn(cov, __fsub_rn(u[o][2], __fmul_rn(u[o][0], u[o][0])));
    const float vy = __fmul_rn(cov, __fsub_rn(u[o][3], __fmul_rn(u[o][1], u[o][1])));
    const float vxy = __fmul_rn(cov, __fsub_rn(u[o][4], __fmul_rn(u[o][0], u[o][1])));
    const float ux = __fadd_rn(u[o][0], shift), uy = __fadd_rn(u[o][1], shift);
    const float a1 = __fadd_rn(__fmul_rn(2.f, __fmul_rn(ux, uy)), C1);
    const float a2 = __fadd_rn(__fmul_rn(2.f, vxy), C2);
    const float b1 = __fadd_rn(__fadd_rn(__fmul_rn(ux, ux), __fmul_rn(uy, uy)), C1);
    const float b2 = __fadd_rn(__fadd_rn(vx, vy), C2);
    acc += (double)__fdiv_rn(__fmul_rn(a1, a2), __fmul_rn(b1, b2));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((tid & 63) == 0) part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) slots[blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}

// One wave per frame: lane l adds the frame's slots l, l + 64, ... in index order, the lanes are added by a shuffle tree.
__global__ __launch_bounds__(64) void frame_ssim_mean_kernel(const double* __restrict__ slots, int per_frame, double count,
                                                             double* __restrict__ ssim) {
  const double* s = slots + (size_t)blockIdx.x * per_frame;
  double acc = 0.0;
  for (int i = threadIdx.x; i < per_frame; i += 64) acc += s[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (threadIdx.x == 0) ssim[blockIdx.x] = acc / count;
}

inline long ssim_tiles(int H, int W) {
  return (long)((H - 2 * kHalo + kTH - 1) / kTH) * ((W - 2 * kHalo + kTW - 1) / kTW);
}

int frame_ssim_check(int n, int F, int H, int W) {
  CTRLV_CHECK_SHAPE(n > 0 && F > 0, "frame_ssim: n=%d, F=%d must be positive", n, F);
  CTRLV_CHECK_SHAPE(H >= kTaps && W >= kTaps, "frame_ssim: a %d x %d frame is smaller than the %d x %d window", H, W, kTaps, kTaps);
  CTRLV_CHECK_SHAPE((long)H * W <= 0x7fffffffL / 3, "frame_ssim: a frame of %d x %d pixels is above 2^31 - 1 bytes", H, W);
  CTRLV_CHECK_SHAPE((double)n * F * 3 * (double)ssim_tiles(H, W) <= 2147483647.0, "frame_ssim: %d x %d frames of %d x %d need more "
                    "than 2^31 - 1 workgroups", n, F, H, W);
  return CTRLV_OK;
}

}  // namespace

extern "C" int ctrlv_frame_stats(const void* gt_u8, const void* gen_u8, int n, int F, int H, int W, long long* stats,
                                 ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(gt_u8 && gen_u8 && stats, "frame_stats: null pointer");
  CTRLV_CHECK_ARG(((uintptr_t)stats & 7) == 0, "frame_stats: stats must be 8-byte aligned");
  CTRLV_CHECK_SHAPE(n > 0 && F > 0 && H > 0 && W > 0, "frame_stats: n, F, H, W must be positive (got %d, %d, %d, %d)", n, F, H, W);
  const long frames = (long)n * F;
  const size_t per = (size_t)3 * H * W;
  // a thread takes about four 16-byte units; at most 256 groups per frame (the threads stride)
  size_t groups = (per / 16 + 4 * kThreads - 1) / (4 * kThreads);
  if (groups < 1) groups = 1;
  if (groups > 256) groups = 256;
  const size_t cap = 0x7fffffffull / (size_t)frames;
  CTRLV_CHECK_SHAPE(cap >= 1, "frame_stats: %d x %d frames need more than 2^31 - 1 workgroups", n, F);
  if (groups > cap) groups = cap;
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(frame_stats_init_kernel, dim3((unsigned)((frames + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, (u64*)stats,
                     frames);
  CTRLV_LAUNCH_CHECK();
  const dim3 grid((unsigned)(groups * (size_t)frames));
  if (per % 16 == 0 && aligned16(gt_u8) && aligned16(gen_u8))
    hipLaunchKernelGGL(frame_stats_kernel<true>, grid, dim3(kThreads), 0, s, (const uint8_t*)gt_u8, (const uint8_t*)gen_u8, per,
                       (int)groups, (u64*)stats);
  else
    hipLaunchKernelGGL(frame_stats_kernel<false>, grid, dim3(kThreads), 0, s, (const uint8_t*)gt_u8, (const uint8_t*)gen_u8, per,
                       (int)groups, (u64*)stats);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

extern "C" size_t ctrlv_frame_ssim_ws_bytes(int n, int F, int H, int W) {
  if (frame_ssim_check(n, F, H, W) != CTRLV_OK) return 0;
  return (size_t)n * F * 3 * (size_t)ssim_tiles(H, W) * sizeof(double);
}

extern "C" int ctrlv_frame_ssim(const void* gt_u8, const void* gen_u8, int n, int F, int H, int W, const long long* stats,
                                double* ssim, void* ws, size_t ws_bytes, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(gt_u8 && gen_u8 && stats && ssim && ws, "frame_ssim: null pointer");
  CTRLV_CHECK_ARG(((uintptr_t)stats & 7) == 0, "frame_ssim: stats must be 8-byte aligned");
  CTRLV_CHECK_ARG(((uintptr_t)ssim & 7) == 0, "frame_ssim: ssim must be 8-byte aligned");
  CTRLV_CHECK_ARG(((uintptr_t)ws & 7) == 0, "frame_ssim: the workspace must be 8-byte aligned");
  CTRLV_TRY(frame_ssim_check(n, F, H, W));
  const size_t need = ctrlv_frame_ssim_ws_bytes(n, F, H, W);
  if (ws_bytes < need) {
    ctrlv_set_error("frame_ssim: ws_bytes=%zu is smaller than the %zu bytes these frames need (ctrlv_frame_ssim_ws_bytes)", ws_bytes,
                    need);
    return CTRLV_E_WORKSPACE;
  }
  Window win;                              // g[i] = exp(-i^2 / (2 sigma^2)) / sum, sigma = 1.5, formed in double
  double g[kTaps], sum = 0.0;
  for (int i = 0; i < kTaps; ++i) {
    const double d = (double)(i - kHalo);
    g[i] = exp(-d * d / 4.5);
    sum += g[i];
  }
  for (int i = 0; i < kTaps; ++i) win.g[i] = (float)(g[i] / sum);
  const int tiles_x = (W - 2 * kHalo + kTW - 1) / kTW, tiles_y = (H - 2 * kHalo + kTH - 1) / kTH;
  const long frames = (long)n * F;
  const int per_frame = 3 * tiles_x * tiles_y;
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(frame_ssim_kernel, dim3((unsigned)(frames * per_frame)), dim3(kThreads), 0, s, (const uint8_t*)gt_u8,
                     (const uint8_t*)gen_u8, H, W, tiles_x, tiles_y, stats, win, (double*)ws);
  CTRLV_LAUNCH_CHECK();
  hipLaunchKernelGGL(frame_ssim_mean_kernel, dim3((unsigned)frames), dim3(64), 0, s, (const double*)ws, per_frame,
                     3.0 * (double)(H - 2 * kHalo) * (double)(W - 2 * kHalo), ssim);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}
