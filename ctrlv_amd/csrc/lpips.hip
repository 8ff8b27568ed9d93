// LPIPS (AlexNet, v0.1) of generated frames against their ground truth (gfx950): the lpips_score of the reference's
// evaluate_vids (src/ctrlv/metrics/fvd.py:241-248), which it forms with the `lpips` package per clip.
//   ctrlv_lpips_im2col_split    the A operand of one convolution as element rows [lo | hi | hi]
//   ctrlv_lpips_pack_weight     a convolution's parameter as element rows [whi | wlo | whi] in the matching column order
//   ctrlv_relu_maxpool_rows     max_pool2d(relu(x), 3, 2) on fp32 rows
//   ctrlv_lpips_layer_distance  per frame, fp64 per-block partial sums of sum_c lin[c] (n_gt - n_gen)^2 over its pixels
//   ctrlv_lpips_finish          per frame, sum over the layers of (partials in block order) / pixels
//   ctrlv_lpips_plan_* / ctrlv_lpips_frames   the network as one call on library-owned split weights
// The metric subtracts two normalised feature maps: with activations rounded to 16 bits it is lost where the frames are close
// (DESIGN.md 3.14).  So every convolution contracts SPLIT operands -- x = hi + lo, w = whi + wlo in the element type, y = lo whi +
// hi wlo + hi whi -- as one ctrlv_gemm launch over the concatenated K with fp32 output, and everything between the
// convolutions is fp32 rows holding the output BEFORE ReLU; each consumer applies max(v, 0) when it reads.  These kernels move
// bytes: a thread reads and writes 16-byte units, sums have one fixed order, there are no floating-point atomics, and nothing a
// frame's value is made of depends on the other frames of the launch.
#include <string>
#include <vector>

#include "plan_walk.h"
#include "weight_loader.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPixPerBlock = 64;                 // pixels of one frame a workgroup of the distance kernel owns (16 per wave)
constexpr int kMaxLayers = 8;
constexpr int kK1 = 11, kStride1 = 4, kPad1 = 2; // AlexNet's first convolution
constexpr int kSrcF32 = 0, kSrcU8 = 3;           // src_dtype codes of the first-layer form

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline int kp_of(int C, int k) { return pad_to(k * k * C, 64); }

// the value an element can hold: the fp16 library saturates (a NaN stays a NaN), bf16 has fp32's range
__device__ __forceinline__ float el_sat(float x) {
#ifdef CTRLV_ELEM_F16
  return fabsf(x) > 65504.f ? copysignf(65504.f, x) : x;
#else
  return x;
#endif
}
// hi = rne_el(v), lo = rne_el(v - hi); v - hi is exact in fp32 (hi is v rounded to fewer bits)
__device__ __forceinline__ void split8(const float* v, uint4& hi, uint4& lo) {
#pragma clang fp contract(off)
  float s[8], h[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = el_sat(v[e]);
  hi = pack_elx8(s);
  unpack_elx8(hi, h);
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = el_sat(v[e] - h[e]);
  lo = pack_elx8(s);
}
// The blocks of a row are lo | hi | hi, against whi | wlo | whi of the weight: ctrlv_gemm walks K in order, so the two small
// products are summed first, while the fp32 accumulator is still small, and the chain that carries the full-size sum is one
// block long instead of three.
__device__ __forceinline__ void store_split(el_t* row, int kp, int k0, const uint4& hi, const uint4& lo) {
  *(uint4*)(row + k0) = lo;
  *(uint4*)(row + kp + k0) = hi;
  *(uint4*)(row + 2 * kp + k0) = hi;
}
__device__ __forceinline__ float relu_f(float v) { return v > 0.f ? v : 0.f; }

// ---------------------------------------------------------------------------------------------------------------- im2col
// First layer.  One thread forms 8 consecutive columns of one row: k = (c * 11 + ky) * 11 + kx, 363 live columns of 384.
template <bool U8>
__global__ __launch_bounds__(kThreads) void im2col_first_kernel(const void* __restrict__ src, int H, int W, int Ho, int Wo, long M,
                                                                 el_t* __restrict__ rows) {
  constexpr int K = 3 * kK1 * kK1, Kp = 384, CH = Kp / 8;
  const long idx = (long)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= M * CH) return;
  const long row = idx / CH;
  const int k0 = (int)(idx - row * CH) * 8;
  const int hw = Ho * Wo;
  const long img = row / hw;
  const int rem = (int)(row - img * hw), oy = rem / Wo, ox = rem - oy * Wo;
  const float shift[3] = {-0.030f, -0.088f, -0.188f}, scale[3] = {0.458f, 0.448f, 0.450f};
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = k0 + e;
    const int c = k / (kK1 * kK1), r = k - c * (kK1 * kK1), ky = r / kK1, kx = r - ky * kK1;
    const int y = oy * kStride1 - kPad1 + ky, x = ox * kStride1 - kPad1 + kx;
    v[e] = 0.f;
    if (k < K && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) {
      const long p = ((img * 3 + c) * H + y) * W + x;
      float t;
      if constexpr (U8) t = __fsub_rn(__fdiv_rn((float)((const uint8_t*)src)[p], 127.5f), 1.0f);
      else t = ((const float*)src)[p];
      v[e] = __fdiv_rn(__fsub_rn(t, shift[c]), scale[c]);
    }
  }
  uint4 hi, lo;
  split8(v, hi, lo);
  store_split(rows + row * (3 * Kp), Kp, k0, hi, lo);
}

// Rows form.  One thread takes 8 channels of one tap of one row: k = (ky * kw + kx) * C + c; two 16-byte reads, three writes.
__global__ __launch_bounds__(kThreads) void im2col_rows_kernel(const float* __restrict__ src, int ld, int H, int W, int C, int kw,
                                                                int K, int Kp, long M, el_t* __restrict__ rows) {
  const int CH = Kp >> 3;
  const long idx = (long)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= M * CH) return;
  const long row = idx / CH;
  const int k0 = (int)(idx - row * CH) * 8;
  float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (k0 < K) {                                        // (C is a multiple of 8: a unit is all live or all padding)
    const int tap = k0 / C, c = k0 - tap * C, ky = tap / kw, kx = tap - ky * kw, pad = (kw - 1) >> 1;
    const int hw = H * W;
    const long img = row / hw;
    const int rem = (int)(row - img * hw), y = rem / W, x = rem - y * W;
    const int yy = y + ky - pad, xx = x + kx - pad;
    if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) {
      const float* p = src + (img * hw + (long)yy * W + xx) * ld + c;
      const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
      v[0] = relu_f(a.x); v[1] = relu_f(a.y); v[2] = relu_f(a.z); v[3] = relu_f(a.w);
      v[4] = relu_f(b.x); v[5] = relu_f(b.y); v[6] = relu_f(b.z); v[7] = relu_f(b.w);
    }
  }
  uint4 hi, lo;
  split8(v, hi, lo);
  store_split(rows + row * (3L * Kp), Kp, k0, hi, lo);
}

// ---------------------------------------------------------------------------------------------------------------- weights
__device__ __forceinline__ float ld_param(const void* p, int dtype, long i) {
  if (dtype == 0) return ((const float*)p)[i];
  if (dtype == 1) return (float)((const _Float16*)p)[i];
  return bf16_to_f32(((const bf16_t*)p)[i]);
}
// one thread per (n, column of a Kp block); load-time only
__global__ __launch_bounds__(kThreads) void pack_split_weight_kernel(const void* __restrict__ w, int dtype, int N, int C, int kw,
                                                                      int order, int Kp, el_t* __restrict__ dst) {
#pragma clang fp contract(off)
  const long idx = (long)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= (long)N * Kp) return;
  const int n = (int)(idx / Kp), k = (int)(idx - (long)n * Kp), taps = kw * kw, K = taps * C;
  float v = 0.f;
  if (k < K) {
    long s = (long)n * K + k;                            // order 0: (c, ky, kx), the parameter's own order
    if (order == 1) { const int tap = k / C, c = k - tap * C; s = ((long)n * C + c) * taps + tap; }
    v = ld_param(w, dtype, s);
  }
  const el_t hi = f32_to_el(el_sat(v)), lo = f32_to_el(el_sat(v - el_to_f32(hi)));
  el_t* row = dst + (long)n * 3 * Kp;
  row[k] = hi;
  row[Kp + k] = lo;
  row[2 * Kp + k] = hi;
}

// ---------------------------------------------------------------------------------------------------------------- pool
// one thread per (output pixel, 4 channels): nine 16-byte reads; max(., 0) is the start value, so ReLU is applied on read
__global__ __launch_bounds__(kThreads) void relu_maxpool_kernel(const float* __restrict__ x, int H, int W, int Ho, int Wo, int C,
                                                                 int ldx, long Mo, float* __restrict__ out, int ldo) {
  const int c4 = C >> 2;
  const long idx = (long)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= Mo * c4) return;
  const long row = idx / c4;
  const int c = (int)(idx - row * c4) * 4;
  const int hw = Ho * Wo;
  const long img = row / hw;
  const int rem = (int)(row - img * hw), oy = rem / Wo, ox = rem - oy * Wo;
  const float* base = x + (img * H * W + (long)(2 * oy) * W + 2 * ox) * ldx + c;
  float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const float4 v = *(const float4*)(base + ((long)dy * W + dx) * ldx);
      m.x = v.x > m.x ? v.x : m.x; m.y = v.y > m.y ? v.y : m.y; m.z = v.z > m.z ? v.z : m.z; m.w = v.w > m.w ? v.w : m.w;
    }
  *(float4*)(out + row * ldo + c) = m;
}

// ---------------------------------------------------------------------------------------------------------------- distance
// blockIdx.x = frame * nb + block; wave w takes the pixels block * 64 + w * 16 + (0 .. 15) of the frame, one after the other.
// A lane holds the 16-byte units lane and lane + 64 of a pixel's channels (C <= 512).  Every operation is its own rounded
// instruction: with gen == gt the two normalised vectors agree bit for bit and d is exactly 0.
__global__ __launch_bounds__(kThreads) void layer_distance_kernel(const float* __restrict__ gt, const float* __restrict__ gen, int ld,
                                                                   const float* __restrict__ lin, int pix, int nb, int C,
                                                                   double* __restrict__ partials) {
  __shared__ double part[kThreads / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int frame = blockIdx.x / nb, b = blockIdx.x - frame * nb;
  const int c4 = C >> 2;
  float4 l[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int q = lane + 64 * j;
    l[j] = q < c4 ? ((const float4*)lin)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  double acc = 0.0;
  for (int i = 0; i < kPixPerBlock / 4; ++i) {
    const int p = b * kPixPerBlock + w * (kPixPerBlock / 4) + i;
    if (p >= pix) break;                                 // (the whole wave leaves together)
    const long r = ((long)frame * pix + p) * ld;
    float xa[8], xg[8];
    float sa = 0.f, sg = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int q = lane + 64 * j;
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f), g = a;
      if (q < c4) { a = *(const float4*)(gt + r + 4 * q); g = *(const float4*)(gen + r + 4 * q); }
      xa[4 * j] = relu_f(a.x); xa[4 * j + 1] = relu_f(a.y); xa[4 * j + 2] = relu_f(a.z); xa[4 * j + 3] = relu_f(a.w);
      xg[4 * j] = relu_f(g.x); xg[4 * j + 1] = relu_f(g.y); xg[4 * j + 2] = relu_f(g.z); xg[4 * j + 3] = relu_f(g.w);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      sa = __fmaf_rn(xa[e], xa[e], sa);
      sg = __fmaf_rn(xg[e], xg[e], sg);
    }
    sa = wave_sum(sa);                                   // (xor butterfly: every lane ends with the same bits)
    sg = wave_sum(sg);
    const float da = __fadd_rn(__fsqrt_rn(sa), 1e-10f), dg = __fadd_rn(__fsqrt_rn(sg), 1e-10f);
    float d = 0.f;
    const float lw[8] = {l[0].x, l[0].y, l[0].z, l[0].w, l[1].x, l[1].y, l[1].z, l[1].w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float t = __fsub_rn(__fdiv_rn(xa[e], da), __fdiv_rn(xg[e], dg));
      d = __fmaf_rn(lw[e], __fmul_rn(t, t), d);
    }
    d = wave_sum(d);
    acc += (double)d;
  }
  if (lane == 0) part[w] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}

struct FinishArgs { int n_layers; int nb[kMaxLayers]; int pix[kMaxLayers]; };     // a kernel argument by value
// one thread per frame: the layers in order, a layer's blocks in order
__global__ __launch_bounds__(64) void lpips_finish_kernel(const double* __restrict__ partials, int frames, const FinishArgs a,
                                                          double* __restrict__ out) {
  const int frame = blockIdx.x * 64 + threadIdx.x;
  if (frame >= frames) return;
  double total = 0.0;
  long off = 0;
  for (int l = 0; l < a.n_layers; ++l) {
    const double* s = partials + off + (long)frame * a.nb[l];
    double acc = 0.0;
    for (int i = 0; i < a.nb[l]; ++i) acc += s[i];
    total += acc / (double)a.pix[l];
    off += (long)frames * a.nb[l];
  }
  out[frame] = total;
}

inline unsigned blocks_of(long threads) { return (unsigned)((threads + kThreads - 1) / kThreads); }

// ---------------------------------------------------------------------------------------------------------------- the network
struct ConvSpec { int feat, cin, n, k; };
constexpr ConvSpec kConv[5] = {{0, 3, 64, 11}, {3, 64, 192, 5}, {6, 192, 384, 3}, {8, 384, 256, 3}, {10, 256, 256, 3}};

// sizes of the five taps for H x W frames; ok = false when the second pool has no output
struct Geometry {
  int h[5], w[5], kp[5];
  bool ok;
  long pix(int l) const { return (long)h[l] * w[l]; }
};
Geometry geometry(int H, int W) {
  Geometry g;
  g.ok = H >= 31 && W >= 31;
  g.h[0] = (H + 2 * kPad1 - kK1) / kStride1 + 1; g.w[0] = (W + 2 * kPad1 - kK1) / kStride1 + 1;
  g.h[1] = (g.h[0] - 3) / 2 + 1; g.w[1] = (g.w[0] - 3) / 2 + 1;
  g.h[2] = (g.h[1] - 3) / 2 + 1; g.w[2] = (g.w[1] - 3) / 2 + 1;
  g.h[3] = g.h[4] = g.h[2]; g.w[3] = g.w[4] = g.w[2];
  for (int l = 0; l < 5; ++l) g.kp[l] = kp_of(kConv[l].cin, kConv[l].k);
  return g;
}

}  // namespace

struct ctrlv_lpips_plan {
  int device = 0;
  bool loaded = false;
  std::vector<void*> owned;
  ctrlv_load::PackedLinear conv[5];       // w: [N][3 Kp] = whi | wlo | whi, b: fp32 [N]
  float* lin[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
};

// ================================================================================================================ kernels' entries
extern "C" int ctrlv_lpips_im2col_split(const void* src, int form, int src_dtype, int m, int H, int W, int C, int ld, int k,
                                        void* rows, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(src && rows, "lpips_im2col_split: null pointer");
  CTRLV_CHECK_ARG(form == 0 || form == 1, "lpips_im2col_split: form %d (0 first layer, 1 rows)", form);
  CTRLV_CHECK_ARG(aligned16(rows), "lpips_im2col_split: rows must be 16-byte aligned");
  CTRLV_CHECK_SHAPE(m > 0 && H > 0 && W > 0, "lpips_im2col_split: m=%d, H=%d, W=%d must be positive", m, H, W);
  const hipStream_t s = (hipStream_t)stream;
  if (form == 0) {
    CTRLV_CHECK_DTYPE(src_dtype == kSrcF32 || src_dtype == kSrcU8, "lpips_im2col_split: src_dtype %d (0 fp32, 3 uint8)", src_dtype);
    CTRLV_CHECK_ARG(src_dtype == kSrcU8 || ((uintptr_t)src & 3) == 0, "lpips_im2col_split: fp32 frames must be 4-byte aligned");
    CTRLV_CHECK_SHAPE(C == 3 && k == kK1, "lpips_im2col_split: the first layer is C=3, k=11 (got C=%d, k=%d)", C, k);
    CTRLV_CHECK_SHAPE(H >= kK1 - 2 * kPad1 && W >= kK1 - 2 * kPad1, "lpips_im2col_split: a %d x %d frame is smaller than the window", H, W);
    const int Ho = (H + 2 * kPad1 - kK1) / kStride1 + 1, Wo = (W + 2 * kPad1 - kK1) / kStride1 + 1;
    const long M = (long)m * Ho * Wo;
    CTRLV_CHECK_SHAPE((double)M * 3 * 384 < 2147483648.0 && (double)m * 3 * H * W < 9.0e15,
                      "lpips_im2col_split: %ld rows of %d columns are 2^31 elements or more: split the batch", M, 3 * 384);
    const unsigned grid = blocks_of(M * (384 / 8));
    if (src_dtype == kSrcU8)
      hipLaunchKernelGGL(im2col_first_kernel<true>, dim3(grid), dim3(kThreads), 0, s, src, H, W, Ho, Wo, M, (el_t*)rows);
    else
      hipLaunchKernelGGL(im2col_first_kernel<false>, dim3(grid), dim3(kThreads), 0, s, src, H, W, Ho, Wo, M, (el_t*)rows);
  } else {
    CTRLV_CHECK_SHAPE(k == 3 || k == 5, "lpips_im2col_split: rows form takes k = 3 or 5 (got %d)", k);
    CTRLV_CHECK_SHAPE(C > 0 && C % 8 == 0 && ld % 4 == 0 && ld >= C, "lpips_im2col_split: C=%d must be a multiple of 8, ld=%d a "
                      "multiple of 4 and >= C", C, ld);
    CTRLV_CHECK_ARG(aligned16(src), "lpips_im2col_split: src rows must be 16-byte aligned");
    const int K = k * k * C, Kp = kp_of(C, k);
    const long M = (long)m * H * W;
    CTRLV_CHECK_SHAPE((double)M * 3 * Kp < 2147483648.0, "lpips_im2col_split: %ld rows of %d columns are 2^31 elements or more: "
                      "split the batch", M, 3 * Kp);
    hipLaunchKernelGGL(im2col_rows_kernel, dim3(blocks_of(M * (Kp / 8))), dim3(kThreads), 0, s, (const float*)src, ld, H, W, C, k, K,
                       Kp, M, (el_t*)rows);
  }
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

extern "C" int ctrlv_lpips_pack_weight(const void* w, int dtype_code, int N, int C, int k, int order, void* dst,
                                       ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(w && dst && aligned16(dst), "lpips_pack_weight: null pointer, or dst not 16-byte aligned");
  CTRLV_CHECK_DTYPE(dtype_code >= 0 && dtype_code <= 2, "lpips_pack_weight: dtype code %d (0 fp32, 1 fp16, 2 bf16)", dtype_code);
  CTRLV_CHECK_ARG(order == 0 || order == 1, "lpips_pack_weight: order %d (0 (c, ky, kx), 1 (ky, kx, c))", order);
  CTRLV_CHECK_SHAPE(N > 0 && C > 0 && k > 0 && k <= 15 && N <= 65535 && C <= 65535, "lpips_pack_weight: bad shape N=%d C=%d k=%d", N,
                    C, k);
  const int Kp = kp_of(C, k);
  hipLaunchKernelGGL(pack_split_weight_kernel, dim3(blocks_of((long)N * Kp)), dim3(kThreads), 0, (hipStream_t)stream, w, dtype_code,
                     N, C, k, order, Kp, (el_t*)dst);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

extern "C" int ctrlv_relu_maxpool_rows(const float* x, int m, int H, int W, int C, int ldx, float* out, int ldo,
                                       ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(x && out && aligned16(x) && aligned16(out), "relu_maxpool_rows: null pointer, or rows not 16-byte aligned");
  CTRLV_CHECK_SHAPE(m > 0 && H >= 3 && W >= 3, "relu_maxpool_rows: m=%d must be positive and the %d x %d image hold a 3 x 3 window", m,
                    H, W);
  CTRLV_CHECK_SHAPE(C > 0 && C % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && ldx >= C && ldo >= C,
                    "relu_maxpool_rows: C=%d, ldx=%d, ldo=%d must be multiples of 4 and the pitches >= C", C, ldx, ldo);
  const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
  const long Mo = (long)m * Ho * Wo;
  CTRLV_CHECK_SHAPE((double)Mo * (C / 4) < 2147483647.0 * kThreads, "relu_maxpool_rows: too many workgroups (m=%d)", m);
  hipLaunchKernelGGL(relu_maxpool_kernel, dim3(blocks_of(Mo * (C / 4))), dim3(kThreads), 0, (hipStream_t)stream, x, H, W, Ho, Wo, C,
                     ldx, Mo, out, ldo);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

extern "C" int ctrlv_lpips_distance_blocks(int pix) { return pix > 0 ? (pix + kPixPerBlock - 1) / kPixPerBlock : 0; }

extern "C" int ctrlv_lpips_layer_distance(const float* gt, const float* gen, int ld, const float* lin, int frames, int pix, int C,
                                          double* partials, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(gt && gen && lin && partials, "lpips_layer_distance: null pointer");
  CTRLV_CHECK_ARG(aligned16(gt) && aligned16(gen) && aligned16(lin) && ((uintptr_t)partials & 7) == 0,
                  "lpips_layer_distance: rows and lin must be 16-byte aligned, partials 8-byte aligned");
  CTRLV_CHECK_SHAPE(frames > 0 && pix > 0, "lpips_layer_distance: frames=%d, pix=%d must be positive", frames, pix);
  CTRLV_CHECK_SHAPE(C > 0 && C % 4 == 0 && C <= 512 && ld % 4 == 0 && ld >= C,
                    "lpips_layer_distance: C=%d must be a multiple of 4, at most 512; ld=%d a multiple of 4 and >= C", C, ld);
  const int nb = ctrlv_lpips_distance_blocks(pix);
  CTRLV_CHECK_SHAPE((double)frames * nb <= 2147483647.0, "lpips_layer_distance: %d frames of %d pixels need more than 2^31 - 1 "
                    "workgroups", frames, pix);
  hipLaunchKernelGGL(layer_distance_kernel, dim3((unsigned)((long)frames * nb)), dim3(kThreads), 0, (hipStream_t)stream, gt, gen, ld,
                     lin, pix, nb, C, partials);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

extern "C" int ctrlv_lpips_finish(const double* partials, int frames, int n_layers, const int* pix, double* out,
                                  ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(partials && pix && out, "lpips_finish: null pointer");
  CTRLV_CHECK_ARG(((uintptr_t)partials & 7) == 0 && ((uintptr_t)out & 7) == 0, "lpips_finish: partials and out must be 8-byte aligned");
  CTRLV_CHECK_SHAPE(frames > 0 && n_layers >= 1 && n_layers <= kMaxLayers, "lpips_finish: frames=%d must be positive, n_layers=%d in "
                    "[1, %d]", frames, n_layers, kMaxLayers);
  FinishArgs a;
  memset(&a, 0, sizeof a);
  a.n_layers = n_layers;
  for (int l = 0; l < n_layers; ++l) {
    CTRLV_CHECK_SHAPE(pix[l] > 0, "lpips_finish: pix[%d]=%d must be positive", l, pix[l]);
    a.pix[l] = pix[l];
    a.nb[l] = ctrlv_lpips_distance_blocks(pix[l]);
  }
  hipLaunchKernelGGL(lpips_finish_kernel, dim3((unsigned)((frames + 63) / 64)), dim3(64), 0, (hipStream_t)stream, partials, frames, a,
                     out);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

// ================================================================================================================ the plan
namespace {

using ctrlv_load::WeightLoader;

void free_owned(ctrlv_lpips_plan* p) {
  for (void* d : p->owned) (void)hipFree(d);
  p->owned.clear();
  for (int l = 0; l < 5; ++l) { p->conv[l] = ctrlv_load::PackedLinear(); p->lin[l] = nullptr; }
  p->loaded = false;
}

int load_all(WeightLoader& L, ctrlv_lpips_plan* p) {
  for (int l = 0; l < 5; ++l) {
    const ConvSpec& c = kConv[l];
    const std::string mod = "features." + std::to_string(c.feat);
    const ctrlv_tensor_desc* t;
    CTRLV_TRY(L.find(mod + ".weight", (long)c.n * c.cin * c.k * c.k, &t));
    const void* src;
    CTRLV_TRY(L.dev_ptr(t, &src));
    CTRLV_TRY(L.new_linear(p->conv[l], c.n, 3 * kp_of(c.cin, c.k), true));
    CTRLV_TRY(ctrlv_lpips_pack_weight(src, t->dtype, c.n, c.cin, c.k, l == 0 ? 0 : 1, p->conv[l].w, L.st));
    CTRLV_TRY(L.pack_v(mod + ".bias", c.n, p->conv[l].b, 0, 0, 0));
    CTRLV_TRY(L.vec("lin" + std::to_string(l) + ".model.1.weight", c.n, &p->lin[l]));
  }
  return CTRLV_OK;
}

// a chunk's buffers inside the caller's workspace: the im2col rows every convolution shares, the five pre-ReLU outputs, the two
// pooled maps and the fp64 partials of the five taps
struct Regions {
  el_t* a;
  float* y[5];
  float* q[2];
  double* part;
  size_t total;
};
Regions carve(const Geometry& g, int chunk, char* base) {
  Regions r;
  size_t off = 0;
  auto take = [&](size_t bytes) { char* q = base + off; off += up256(bytes); return q; };
  const size_t imgs = 2 * (size_t)chunk;
  size_t a_el = 0;
  for (int l = 0; l < 5; ++l) {
    const size_t e = imgs * (size_t)g.pix(l) * 3 * g.kp[l];
    if (e > a_el) a_el = e;
  }
  r.a = (el_t*)take(a_el * 2);
  for (int l = 0; l < 5; ++l) r.y[l] = (float*)take(imgs * (size_t)g.pix(l) * kConv[l].n * 4);
  for (int l = 0; l < 2; ++l) r.q[l] = (float*)take(imgs * (size_t)g.pix(l + 1) * kConv[l].n * 4);
  size_t nb = 0;
  for (int l = 0; l < 5; ++l) nb += (size_t)ctrlv_lpips_distance_blocks((int)g.pix(l));
  r.part = (double*)take((size_t)chunk * nb * 8);
  r.total = off;
  return r;
}
// the largest chunk whose every im2col buffer stays below 2^31 elements; 0: one frame pair does not fit
long chunk_cap(const Geometry& g) {
  long cap = 1L << 20;
  for (int l = 0; l < 5; ++l) {
    const long per = 2 * g.pix(l) * 3 * g.kp[l];               // elements of one frame pair
    const long c = 0x7fffffffL / per;
    if (c < cap) cap = c;
  }
  return cap;
}

int conv(const ctrlv_lpips_plan* p, int l, const el_t* A, long M, float* out, hipStream_t st) {
  const ctrlv_load::PackedLinear& w = p->conv[l];
  ctrlv_gemm_desc d = ctrlv_linear_desc(A, w.k, w, out, w.n, M, w.n, w.k, w.n);
  d.out_f32 = 1;
  d.tile = 1;            // the 2-stage 128 x 128 kernel whatever M is: a frame's bits do not depend on the batch
  return ctrlv_gemm(&d, st);
}

int run_chunk(const ctrlv_lpips_plan* p, const Geometry& g, const Regions& r, const void* gt, const void* gen, int src_dtype, int c,
              int H, int W, double* out, hipStream_t st) {
  const int imgs = 2 * c;
  size_t poff = 0;
  int pixs[5];
  auto tap = [&](int l) -> int {       // the distance of layer l: gt rows are the first c images, gen rows the next c
    const long pix = g.pix(l);
    const int N = kConv[l].n;
    pixs[l] = (int)pix;
    double* part = r.part + poff;
    poff += (size_t)c * ctrlv_lpips_distance_blocks((int)pix);
    return ctrlv_lpips_layer_distance(r.y[l], r.y[l] + (size_t)c * pix * N, N, p->lin[l], c, (int)pix, N, part, st);
  };
  // conv1 from the frames: the gt chunk fills the first c images' rows, the gen chunk the rest
  const size_t rows1 = (size_t)c * g.pix(0) * 3 * g.kp[0];
  CTRLV_TRY(ctrlv_lpips_im2col_split(gt, 0, src_dtype, c, H, W, 3, 0, kK1, r.a, st));
  CTRLV_TRY(ctrlv_lpips_im2col_split(gen, 0, src_dtype, c, H, W, 3, 0, kK1, r.a + rows1, st));
  CTRLV_TRY(conv(p, 0, r.a, (long)imgs * g.pix(0), r.y[0], st));
  CTRLV_TRY(tap(0));
  for (int l = 1; l < 5; ++l) {
    const float* x = r.y[l - 1];
    if (l <= 2) {
      CTRLV_TRY(ctrlv_relu_maxpool_rows(r.y[l - 1], imgs, g.h[l - 1], g.w[l - 1], kConv[l - 1].n, kConv[l - 1].n, r.q[l - 1],
                                        kConv[l - 1].n, st));
      x = r.q[l - 1];
    }
    CTRLV_TRY(ctrlv_lpips_im2col_split(x, 1, 0, imgs, g.h[l], g.w[l], kConv[l].cin, kConv[l].cin, kConv[l].k, r.a, st));
    CTRLV_TRY(conv(p, l, r.a, (long)imgs * g.pix(l), r.y[l], st));
    CTRLV_TRY(tap(l));
  }
  return ctrlv_lpips_finish(r.part, c, 5, pixs, out, st);
}

int lpips_check(const char* who, int H, int W, Geometry* g) {
  *g = geometry(H, W);
  CTRLV_CHECK_SHAPE(g->ok, "%s: frames of %d x %d are smaller than 31 x 31 (the second max-pool has no output)", who, H, W);
  CTRLV_CHECK_SHAPE(H <= 16384 && W <= 16384 && chunk_cap(*g) >= 1, "%s: a %d x %d frame pair needs 2^31 im2col elements or more", who,
                    H, W);
  return CTRLV_OK;
}

}  // namespace

extern "C" int ctrlv_lpips_plan_create(int device, ctrlv_lpips_plan** out) {
  CTRLV_CHECK_ARG(out, "lpips_plan_create: null argument");
  CTRLV_CHECK_ARG(device >= 0 && device < CTRLV_MAX_DEVICES, "lpips_plan_create: device %d", device);
  ctrlv_lpips_plan* p = new ctrlv_lpips_plan();
  p->device = device;
  *out = p;
  return CTRLV_OK;
}

extern "C" int ctrlv_lpips_plan_destroy(ctrlv_lpips_plan* p) {
  if (!p) return CTRLV_OK;
  if (!p->owned.empty()) {
    ctrlv_walk::DeviceScope on(p->device);
    free_owned(p);
  }
  delete p;
  return CTRLV_OK;
}

extern "C" int ctrlv_lpips_plan_load_weights(ctrlv_lpips_plan* p, const ctrlv_tensor_desc* tensors, size_t n) {
  CTRLV_CHECK_ARG(p && tensors, "lpips_plan_load_weights: null argument");
  WeightLoader L("lpips_plan_load_weights", &p->owned);
  const int rc = ctrlv_load::run_load(L, p->device, true, [&]() -> int {
    free_owned(p);
    L.add(tensors, n);
    return load_all(L, p);
  });
  if (rc != CTRLV_OK) { free_owned(p); return rc; }
  p->loaded = true;
  return CTRLV_OK;
}

extern "C" size_t ctrlv_lpips_ws_bytes(ctrlv_lpips_plan* p, int H, int W, int frames_per_chunk) {
  if (!p) { ctrlv_set_error("lpips_ws_bytes: null plan"); return 0; }
  Geometry g;
  if (lpips_check("lpips_ws_bytes", H, W, &g) != CTRLV_OK) return 0;
  if (frames_per_chunk < 1 || frames_per_chunk > chunk_cap(g)) {
    ctrlv_set_error("lpips_ws_bytes: frames_per_chunk=%d must be in [1, %ld] for %d x %d frames", frames_per_chunk, chunk_cap(g), H, W);
    return 0;
  }
  return carve(g, frames_per_chunk, nullptr).total;
}

extern "C" int ctrlv_lpips_frames(ctrlv_lpips_plan* p, const void* gt, const void* gen, int src_dtype, int n, int F, int H, int W,
                                  double* out, void* ws, size_t ws_bytes, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(p && p->loaded, "lpips_frames: plan not loaded");
  CTRLV_CHECK_ARG(gt && gen && out && ws, "lpips_frames: null pointer");
  CTRLV_CHECK_DTYPE(src_dtype == kSrcF32 || src_dtype == kSrcU8, "lpips_frames: src_dtype %d (0 fp32, 3 uint8)", src_dtype);
  CTRLV_CHECK_ARG(src_dtype == kSrcU8 || ((((uintptr_t)gt) | ((uintptr_t)gen)) & 3) == 0, "lpips_frames: fp32 frames must be 4-byte "
                  "aligned");
  CTRLV_CHECK_ARG(((uintptr_t)ws & 255) == 0 && ((uintptr_t)out & 7) == 0, "lpips_frames: workspace must be 256-byte aligned, out "
                  "8-byte aligned");
  CTRLV_CHECK_SHAPE(n > 0 && F > 0 && (double)n * F <= 2147483647.0, "lpips_frames: n=%d, F=%d must be positive", n, F);
  Geometry g;
  CTRLV_TRY(lpips_check("lpips_frames", H, W, &g));
  const long total = (long)n * F;
  // the largest chunk the workspace holds (carve grows with the chunk)
  long lo = 0, hi = chunk_cap(g) < total ? chunk_cap(g) : total;
  while (lo < hi) {
    const long mid = (lo + hi + 1) / 2;
    if (carve(g, (int)mid, nullptr).total <= ws_bytes) lo = mid;
    else hi = mid - 1;
  }
  if (lo < 1) {
    ctrlv_set_error("lpips_frames: workspace of %zu bytes, %zu needed for one frame pair of %d x %d (ctrlv_lpips_ws_bytes)", ws_bytes,
                    carve(g, 1, nullptr).total, H, W);
    return CTRLV_E_WORKSPACE;
  }
  const size_t per = (size_t)3 * H * W * (src_dtype == kSrcU8 ? 1 : 4);
  for (long f0 = 0; f0 < total; f0 += lo) {
    const int c = (int)(total - f0 < lo ? total - f0 : lo);
    const Regions r = carve(g, c, (char*)ws);
    CTRLV_TRY(run_chunk(p, g, r, (const char*)gt + f0 * per, (const char*)gen + f0 * per, src_dtype, c, H, W, out + f0,
                        (hipStream_t)stream));
  }
  return CTRLV_OK;
}
