// Image pre- / post-processing and classifier-free-guidance assembly of a whole clip (gfx950): what sits between the plan-level
// calls of StableVideoControlPipeline.__call__ and so far existed only as torch ops in ctrlv_amd/pipelines/pipeline_utils.py.
//   ctrlv_resize_antialias   _resize_with_antialiasing (Gaussian pre-blur + bicubic, align_corners) fused with the affine steps
//                            around it: uint8 -> [-1, 1] in front, the CLIP normalisation behind (_clamped: with the training
//                            prologue's clamp to [0, 1] in it)
//   ctrlv_pixels_prepare     VaeImageProcessor.preprocess + the noise augmentation of prepare_clip
//   ctrlv_frames_to_u8       VaeImageProcessor.postprocess + numpy_to_pil's (x * 255).round()
//   ctrlv_randn              counter-based Gaussian noise: Philox4x32-10, fp32 uniforms, Box-Muller (keyed per clip)
//   ctrlv_euler_schedule     EulerDiscreteScheduler.set_timesteps' tables (host arithmetic)
//   ctrlv_resize_lanczos_u8  PIL's 8-bit Lanczos resize, byte for byte (integer arithmetic on host-built tables)
//   ctrlv_resize_frames_u8   the same two passes on single planes with PIL's LANCZOS, BILINEAR or BICUBIC kernel
//   ctrlv_pio_*              the doubling / repeating / scattering of the loop's inputs (pipeline_io.h; csrc/pipeline.hip)
// All arithmetic is fp32.  Where the Python expression is a multiply followed by an add that a test compares bit for bit the two
// roundings are kept (__fmul_rn / __fadd_rn: never contracted into an fma).  Once per clip, HBM-bound, no atomics.
#include <math.h>

#include <vector>

#include "philox.h"
#include "pipeline_io.h"

namespace {

constexpr int kMaxTaps = 15;     // Gaussian taps per axis: ks = int(max(4 sigma, 3)) made odd, sigma = (factor - 1) / 2, factor <= 8
constexpr int kTileW = 32;       // output columns per workgroup (256 threads: up to 8 output rows)

struct ResizeParams {
  int n, H, W, h, w;
  int ksy, ksx;
  float ky[kMaxTaps], kx[kMaxTaps];
  float sy, sx;                  // align_corners source step per output pixel: (in - 1) / (out - 1), 0 for one output pixel
  int th, span_y, span_x;        // output rows per workgroup; rows / columns of the LDS tile (upper bounds of what a tile needs)
  int src_u8, dst_dtype, normalize, clamp;   // clamp: (y + 1) / 2 limited to [0, 1] in the normalising epilogue
  float mean[3], stdv[3];
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// index of F.pad(mode="reflect") for i in [-(n - 1), 2 (n - 1)]; the clamp only guards the address
__device__ __forceinline__ int reflecti(int i, int n) { return clampi(i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i), 0, n - 1); }

// cubic convolution weights of torch's upsample_bicubic2d (A = -0.75) for the taps at -1, 0, 1, 2 around floor(x), t = frac(x)
__device__ __forceinline__ void cubic_weights(float t, float* w) {
  const float A = -0.75f;
  const float x0 = t + 1.f, x3 = 2.f - t, u = 1.f - t;
  w[0] = ((A * x0 - 5.f * A) * x0 + 8.f * A) * x0 - 4.f * A;
  w[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
  w[2] = ((A + 2.f) * u - (A + 3.f)) * u * u + 1.f;
  w[3] = ((A * x3 - 5.f * A) * x3 + 8.f * A) * x3 - 4.f * A;
}

// One workgroup = one (image, channel) and a th x 32 tile of OUTPUT pixels.  Stage 1 writes the vertically blurred source rows
// the tile's bicubic taps touch (plus the horizontal blur's halo columns) into LDS -- the only pass over the source; stage 2
// forms, per output pixel, the 4 x 4 horizontally blurred values from LDS and interpolates.  The blurred image never reaches
// HBM.  One kernel for every input / output form (runtime branches at the load and the store only): the element-type output is
// the fp32 output's value rounded once, and the normalised output is the plain output's value pushed through the epilogue.
__global__ __launch_bounds__(256) void resize_antialias_kernel(const void* __restrict__ src, void* __restrict__ dst,
                                                               const ResizeParams P) {
  extern __shared__ __attribute__((aligned(16))) float vb[];
  const int tid = threadIdx.x;
  const int c = blockIdx.z % 3, img = blockIdx.z / 3;
  const int H = P.H, W = P.W;
  const int ox0 = blockIdx.x * kTileW, oy0 = blockIdx.y * P.th;
  const int ox1 = min(ox0 + kTileW, P.w) - 1, oy1 = min(oy0 + P.th, P.h) - 1;
  const int ry = P.ksy / 2, rx = P.ksx / 2;
  // source rows / columns the tile's taps touch after the clamp to the image, and the columns the horizontal blur reads
  const int ylo = clampi((int)floorf(P.sy * (float)oy0) - 1, 0, H - 1), yhi = clampi((int)floorf(P.sy * (float)oy1) + 2, 0, H - 1);
  const int xlo = clampi((int)floorf(P.sx * (float)ox0) - 1, 0, W - 1), xhi = clampi((int)floorf(P.sx * (float)ox1) + 2, 0, W - 1);
  const int plo = max(xlo - rx, 0), phi = min(xhi + rx, W - 1);
  const int rows = min(yhi - ylo + 1, P.span_y), cols = min(phi - plo + 1, P.span_x);

  for (int i = tid; i < rows * cols; i += 256) {
    const int r = ylo + i / cols, q = plo + i % cols;
    float acc = 0.f;
    for (int t = 0; t < P.ksy; ++t) {
      const int yy = reflecti(r + t - ry, H);
      float v;
      if (P.src_u8) {
        const float b = (float)((const uint8_t*)src)[(((long)img * H + yy) * W + q) * 3 + c];
        v = __fsub_rn(__fmul_rn(__fdiv_rn(b, 255.0f), 2.0f), 1.0f);
      } else {
        v = ((const float*)src)[(((long)img * 3 + c) * H + yy) * W + q];
      }
      acc += P.ky[t] * v;
    }
    vb[i] = acc;
  }
  __syncthreads();

  for (int o = tid; o < P.th * kTileW; o += 256) {
    const int oy = oy0 + o / kTileW, ox = ox0 + o % kTileW;
    if (oy > oy1 || ox > ox1) continue;
    const float fy = P.sy * (float)oy, fx = P.sx * (float)ox;
    const float gy = floorf(fy), gx = floorf(fx);
    float wy[4], wx[4];
    cubic_weights(fy - gy, wy);
    cubic_weights(fx - gx, wx);
    const int iy = (int)gy, ix = (int)gx;
    float out = 0.f;
    for (int a = 0; a < 4; ++a) {
      const int row = clampi(clampi(iy - 1 + a, 0, H - 1) - ylo, 0, rows - 1);
      const float* line = vb + row * cols;
      float rv = 0.f;
      for (int b = 0; b < 4; ++b) {
        const int col = clampi(ix - 1 + b, 0, W - 1);
        float hb = 0.f;
        for (int j = 0; j < P.ksx; ++j) hb += P.kx[j] * line[clampi(reflecti(col + j - rx, W) - plo, 0, cols - 1)];
        rv += wx[b] * hb;
      }
      out += wy[a] * rv;
    }
    if (P.normalize) {
      float u = __fmul_rn(__fadd_rn(out, 1.0f), 0.5f);
      if (P.clamp) u = u < 0.0f ? 0.0f : (u > 1.0f ? 1.0f : u);          // torch.clamp: a NaN stays
      out = __fdiv_rn(__fsub_rn(u, P.mean[c]), P.stdv[c]);
    }
    const long di = (((long)img * 3 + c) * P.h + oy) * P.w + ox;
    if (P.dst_dtype == 0) ((float*)dst)[di] = out;
    else ((el_t*)dst)[di] = round_to_el(out);
  }
}

// one thread per pixel: three bytes in, one element into each of the three channel planes (coalesced over pixels)
__global__ void pixels_prepare_kernel(const uint8_t* __restrict__ img, const float* __restrict__ noise, float strength, int n,
                                      long HW, el_t* __restrict__ out) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)n * HW) return;
  const long b = idx / HW, p = idx % HW;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const long oi = (b * 3 + c) * HW + p;
    float v = __fsub_rn(__fmul_rn(2.0f, __fdiv_rn((float)img[idx * 3 + c], 255.0f)), 1.0f);
    if (noise) v = __fadd_rn(v, __fmul_rn(strength, noise[oi]));
    out[oi] = round_to_el(v);
  }
}

__device__ __forceinline__ unsigned to_u8(float x) {
  const float v = fminf(fmaxf(__fadd_rn(__fmul_rn(x, 0.5f), 0.5f), 0.0f), 1.0f);
  return (unsigned)rintf(__fmul_rn(v, 255.0f));          // rintf: round half to even, like numpy's round
}

// One thread per FOUR consecutive pixels of the flat (frame, y, x) order: 12 output bytes = three aligned dword stores; the last
// group of the tensor (m H W not a multiple of 4) stores its bytes one by one.  A group may straddle two frames: every pixel
// finds its own frame.
__global__ void frames_to_u8_kernel(const el_t* __restrict__ frames, long total, long HW, uint8_t* __restrict__ out) {
  const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long p0 = g * 4;
  if (p0 >= total) return;
  unsigned bytes[12];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long p = p0 + k < total ? p0 + k : total - 1;
    const long f = p / HW, s = p % HW;
#pragma unroll
    for (int c = 0; c < 3; ++c) bytes[k * 3 + c] = to_u8(el_to_f32(frames[(f * 3 + c) * HW + s]));
  }
  if (p0 + 4 <= total) {
    uint32_t* o = (uint32_t*)(out + p0 * 3);
#pragma unroll
    for (int d = 0; d < 3; ++d)
      o[d] = bytes[4 * d] | (bytes[4 * d + 1] << 8) | (bytes[4 * d + 2] << 16) | (bytes[4 * d + 3] << 24);
  } else {
    const int left = (int)(total - p0) * 3;
    for (int i = 0; i < left; ++i) out[p0 * 3 + i] = (uint8_t)bytes[i];
  }
}

__device__ __forceinline__ float pio_load(const void* p, int dtype, long i) {
  if (dtype == 0) return ((const float*)p)[i];
  if (dtype == 1) return (float)((const _Float16*)p)[i];
  return bf16_to_f32(((const bf16_t*)p)[i]);
}

__global__ void cfg_double_kernel(const void* __restrict__ src, int dtype, el_t* __restrict__ dst, long n_src, int cfg) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_src) return;
  const el_t v = f32_to_el(pio_load(src, dtype, i));
  if (cfg) {
    dst[i] = 0;
    dst[n_src + i] = v;
  } else {
    dst[i] = v;
  }
}

__global__ void lmi_cond_kernel(const el_t* __restrict__ first, el_t* __restrict__ lmi, int B, int F, int c_lat, int hw, int cfg) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;          // over (half, b, f, c, s)
  const long per = (long)c_lat * hw, total = (long)(cfg ? 2 : 1) * B * F * per;
  if (i >= total) return;
  const long cs = i % per, bf = i / per;                               // bf = (half * B + b) * F + f
  const long hb = bf / F;
  const int half = (int)(hb / B), b = (int)(hb % B);
  const bool cond = !cfg || half == 1;
  lmi[bf * 2 * per + per + cs] = cond ? first[(long)b * per + cs] : (el_t)0;
}

// The box predictor's overwrite of the conditioning channels: the `take` frames j of every clip -- frame j for j < K, frame F - 1
// for the one behind them -- come from src (dtype 0 / 1 / 2, src_frames frames per clip, the taken frames packed in front when
// `compact`) and land in the conditional half only: the unconditional half keeps lmi_cond_kernel's zeros.
__global__ void lmi_boxes_kernel(const void* __restrict__ src, int dtype, int src_frames, int compact, el_t* __restrict__ lmi,
                                 int B, int F, int K, int take, int c_lat, int hw, int cfg) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;          // over (b, j, c, s)
  const long per = (long)c_lat * hw, total = (long)B * take * per;
  if (i >= total) return;
  const long cs = i % per, bj = i / per;
  const int j = (int)(bj % take), b = (int)(bj / take);
  const int f = j < K ? j : F - 1;
  const el_t v = f32_to_el(pio_load(src, dtype, ((long)b * src_frames + (compact ? j : f)) * per + cs));
  const long bf = ((long)(cfg ? B : 0) + b) * F + f;
  lmi[bf * 2 * per + per + cs] = v;
}

// x [n] elements clamped to [-1, 1] in place (torch.clamp: a NaN stays); eight elements per thread where the base is 16-byte
// aligned, the last n % 8 -- or everything, from an unaligned base -- one by one
__device__ __forceinline__ el_t clamp_unit(el_t e) {
  const float v = el_to_f32(e);
  return v < -1.0f ? f32_to_el(-1.0f) : (v > 1.0f ? f32_to_el(1.0f) : e);
}

__global__ void clamp_frames_kernel(el_t* __restrict__ x, long n, int vec) {
  const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (vec) {
    const long i0 = g * 8;
    if (i0 + 8 <= n) {
      uint4 q = *(const uint4*)(x + i0);
      uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        w[k] = (uint32_t)clamp_unit((el_t)(w[k] & 0xffffu)) | ((uint32_t)clamp_unit((el_t)(w[k] >> 16)) << 16);
      *(uint4*)(x + i0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
      for (long i = i0; i < n; ++i) x[i] = clamp_unit(x[i]);
    }
  } else if (g < n) {
    x[g] = clamp_unit(x[g]);
  }
}

__global__ void lmi_scatter_kernel(const el_t* __restrict__ scaled, el_t* __restrict__ lmi, long n_half, long per, int cfg) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;          // over (b, f, c, s) of `scaled`
  if (i >= n_half) return;
  const long cs = i % per, bf = i / per;
  const el_t v = scaled[i];
  lmi[bf * 2 * per + cs] = v;
  if (cfg) lmi[(n_half / per + bf) * 2 * per + cs] = v;
}

__global__ void scale_latents_kernel(const float* x, float* out, el_t* __restrict__ scaled, long n,
                                     float inv) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v = x[i];
  if (out != x) out[i] = v;
  scaled[i] = round_to_el(__fmul_rn(v, inv));
}

__global__ void decode_input_kernel(const float* __restrict__ x, el_t* __restrict__ z, long n, float inv) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  z[i] = round_to_el(__fmul_rn(el_to_f32(round_to_el(x[i])), inv));
}

// ---- ctrlv_randn: Philox4x32-10 -> fp32 uniforms -> Box-Muller (the arithmetic is stated in include/ctrlv_hip.h; the device
// functions are csrc/philox.h's)
// One Philox block (four normals) per thread and iteration over (clip, block) pairs.  A block's four elements go out as one
// 16-byte (fp32) / 8-byte (elements) store where their address allows it -- decided per block from the address, so the values
// never depend on the alignment --, one by one elsewhere and in the tail block of a per_clip that is no multiple of 4.
__global__ __launch_bounds__(256) void randn_kernel(uint32_t k0, uint32_t k1, uint32_t clip0, uint32_t call, uint32_t stream_id,
                                                    unsigned long long per_clip, unsigned long long nblk,
                                                    unsigned long long total, float scale, int round_el, void* __restrict__ out,
                                                    int out_el) {
  for (unsigned long long g = (unsigned long long)blockIdx.x * 256 + threadIdx.x; g < total;
       g += (unsigned long long)gridDim.x * 256) {
    const unsigned long long i = g / nblk, j = g % nblk;
    uint32_t x[4];
    philox4x32_10((uint32_t)j, call, stream_id, clip0 + (uint32_t)i, k0, k1, x);
    float z[4];
    box_muller(philox_uniform(x[0]), philox_uniform(x[1]), z);
    box_muller(philox_uniform(x[2]), philox_uniform(x[3]), z + 2);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      z[k] = round_el ? el_to_f32(round_to_el(__fmul_rn(el_to_f32(round_to_el(z[k])), scale))) : __fmul_rn(scale, z[k]);
    const unsigned long long e0 = 4 * j;
    const int left = per_clip - e0 < 4 ? (int)(per_clip - e0) : 4;
    if (out_el) {
      el_t* o = (el_t*)out + i * per_clip + e0;
      el_t e[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) e[k] = round_to_el(z[k]);
      if (left == 4 && ((uintptr_t)o & 7) == 0) {
        *(uint2*)o = make_uint2((uint32_t)e[0] | ((uint32_t)e[1] << 16), (uint32_t)e[2] | ((uint32_t)e[3] << 16));
      } else {
        for (int k = 0; k < left; ++k) o[k] = e[k];
      }
    } else {
      float* o = (float*)out + i * per_clip + e0;
      if (left == 4 && ((uintptr_t)o & 15) == 0) {
        *(float4*)o = make_float4(z[0], z[1], z[2], z[3]);
      } else {
        for (int k = 0; k < left; ++k) o[k] = z[k];
      }
    }
  }
}

// ---- ctrlv_resize_lanczos_u8: one pass of PIL's 8-bit resample along `axis` (0: columns, 1: rows)
constexpr int kLzTx = 64, kLzTy = 4;     // a workgroup's tile of output pixels
constexpr int kLzMaxScale = 16;          // per-axis down-scale: at most 2 * 48 + 1 = 97 taps, 64 rows of them in 24.3 KiB of LDS

// src (n, Hi, Wi, CH) -> dst (n, Ho, Wo, CH); the axis that is not resampled has the same size on both sides.  CH = 3: interleaved
// RGB images; CH = 1: single planes (ctrlv_resize_frames_u8).  bounds[o] = (first tap, taps) and weights[o][ksize] (22-bit fixed
// point) of output index o along the axis.  The workgroup stages the weight rows of its tile -- 64 along x, 4 along y -- in LDS
// (ksize is odd: the 64 rows of the horizontal pass fall on different banks).
template <int CH>
__global__ __launch_bounds__(256) void lanczos_pass_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                           const int2* __restrict__ bounds, const int* __restrict__ weights,
                                                           int ksize, int axis, int Hi, int Wi, int Ho, int Wo) {
  extern __shared__ int kw[];
  const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * kLzTx + tx;
  const int x = blockIdx.x * kLzTx + tx, y = blockIdx.y * kLzTy + ty, img = blockIdx.z;
  const int o0 = axis == 0 ? blockIdx.x * kLzTx : blockIdx.y * kLzTy;
  const int rows = min(axis == 0 ? kLzTx : kLzTy, (axis == 0 ? Wo : Ho) - o0);
  for (int i = tid; i < rows * ksize; i += kLzTx * kLzTy) kw[i] = weights[(long)o0 * ksize + i];
  __syncthreads();
  if (x >= Wo || y >= Ho) return;
  const int lo = axis == 0 ? tx : ty;
  const int2 b = bounds[o0 + lo];
  const int* k = kw + lo * ksize;
  const uint8_t* p = axis == 0 ? src + (((long)img * Hi + y) * Wi + b.x) * CH : src + (((long)img * Hi + b.x) * Wi + x) * CH;
  const long step = axis == 0 ? CH : (long)Wi * CH;
  int s[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) s[c] = 1 << 21;
  for (int t = 0; t < b.y; ++t) {
    const int w = k[t];
#pragma unroll
    for (int c = 0; c < CH; ++c) s[c] += (int)p[c] * w;
    p += step;
  }
  uint8_t* o = dst + (((long)img * Ho + y) * Wo + x) * CH;
#pragma unroll
  for (int c = 0; c < CH; ++c) o[c] = (uint8_t)clampi(s[c] >> 22, 0, 255);
}

// PIL's filter codes (Image.Resampling) and their kernels (libImaging/Resample.c): support and function
constexpr int kFilterLanczos = 1, kFilterBilinear = 2, kFilterBicubic = 3;

double resample_support(int filter) { return filter == kFilterBilinear ? 1.0 : (filter == kFilterBicubic ? 2.0 : 3.0); }

double lanczos_sinc(double v) {
  if (v == 0.0) return 1.0;
  v *= M_PI;
  return sin(v) / v;
}

double resample_filter(int filter, double v) {
  if (filter == kFilterLanczos) return (-3.0 <= v && v < 3.0) ? lanczos_sinc(v) * lanczos_sinc(v / 3.0) : 0.0;
  if (v < 0.0) v = -v;
  if (filter == kFilterBilinear) return v < 1.0 ? 1.0 - v : 0.0;
  const double a = -0.5;                                  // bicubic
  if (v < 1.0) return ((a + 2.0) * v - (a + 3.0)) * v * v + 1;
  if (v < 2.0) return (((v - 5) * v + 8) * v - 4) * a;
  return 0.0;
}

int resample_ksize(int in, int out, int filter) {
  const double scale = (double)in / (double)out, fs = scale < 1.0 ? 1.0 : scale;
  return (int)ceil(resample_support(filter) * fs) * 2 + 1;
}

// bounds [out][2] and weights [out][ksize] of one axis, as PIL's precompute_coeffs + normalize_coeffs_8bpc form them
void resample_tables(int in, int out, int ksize, int filter, int32_t* bounds, int32_t* weights) {
  const double scale = (double)in / (double)out, fs = scale < 1.0 ? 1.0 : scale, support = resample_support(filter) * fs;
  std::vector<double> k((size_t)ksize);
  for (int x = 0; x < out; ++x) {
    const double center = (x + 0.5) * scale;
    int xmin = (int)(center - support + 0.5), xmax = (int)(center + support + 0.5);
    if (xmin < 0) xmin = 0;
    if (xmax > in) xmax = in;
    int cnt = xmax - xmin;
    if (cnt > ksize) cnt = ksize;                     // (cannot happen: 2 support + 1 <= ksize; guards the table)
    double sum = 0.0;
    for (int t = 0; t < cnt; ++t) {
      k[t] = resample_filter(filter, (t + xmin - center + 0.5) / fs);
      sum += k[t];
    }
    int32_t* w = weights + (size_t)x * ksize;
    for (int t = 0; t < ksize; ++t) {
      double q = t < cnt ? k[t] : 0.0;
      if (t < cnt && sum != 0.0) q /= sum;
      w[t] = q < 0.0 ? (int32_t)(-0.5 + q * 4194304.0) : (int32_t)(0.5 + q * 4194304.0);
    }
    bounds[2 * x] = xmin;
    bounds[2 * x + 1] = cnt;
  }
}

// the tables of one call in `ws`, in ints: bounds x [w][2] | bounds y [h][2] | weights x [w][ksx] | weights y [h][ksy]
size_t resample_table_ints(int H, int W, int h, int w, int filter) {
  return (size_t)w * (2 + resample_ksize(W, w, filter)) + (size_t)h * (2 + resample_ksize(H, h, filter));
}

// Both passes of one resize of `imgs` images of CH interleaved channels: the tables of `filter` built on the host, one upload,
// horizontal into `mid` (imgs, H, w, CH), vertical into dst.  ws holds the tables, then (256-byte aligned) mid.  At most 65535
// images per launch: the images go out in runs of that many.
template <int CH>
int resample_two_pass(const uint8_t* src, long imgs, int H, int W, uint8_t* dst, int h, int w, int filter, void* ws, hipStream_t s) {
  const int ksx = resample_ksize(W, w, filter), ksy = resample_ksize(H, h, filter);
  const size_t ints = resample_table_ints(H, W, h, w, filter);
  // the host staging of the one upload: the copy of a pageable source is staged before hipMemcpyAsync returns, as with the
  // driver's constants block (csrc/pipeline.hip)
  static thread_local std::vector<int32_t> tab;
  tab.assign(ints, 0);
  int32_t* bx = tab.data();
  int32_t* by = bx + 2 * (size_t)w;
  int32_t* wx = by + 2 * (size_t)h;
  int32_t* wy = wx + (size_t)w * ksx;
  resample_tables(W, w, ksx, filter, bx, wx);
  resample_tables(H, h, ksy, filter, by, wy);
  int32_t* d = (int32_t*)ws;
  uint8_t* mid = (uint8_t*)ws + up256(ints * sizeof(int32_t));
  CTRLV_HIP_TRY(hipMemcpyAsync(d, tab.data(), ints * sizeof(int32_t), hipMemcpyHostToDevice, s));
  const dim3 block(kLzTx, kLzTy);
  for (long i0 = 0; i0 < imgs; i0 += 65535) {
    const unsigned run = (unsigned)(imgs - i0 < 65535 ? imgs - i0 : 65535);
    const uint8_t* sp = src + (size_t)i0 * H * W * CH;
    uint8_t* mp = mid + (size_t)i0 * H * w * CH;
    uint8_t* dp = dst + (size_t)i0 * h * w * CH;
    hipLaunchKernelGGL(lanczos_pass_kernel<CH>, dim3((unsigned)((w + kLzTx - 1) / kLzTx), (unsigned)((H + kLzTy - 1) / kLzTy), run),
                       block, (size_t)kLzTx * ksx * sizeof(int), s, sp, mp, (const int2*)d,
                       (const int*)(d + 2 * (size_t)w + 2 * (size_t)h), ksx, 0, H, W, H, w);
    CTRLV_LAUNCH_CHECK();
    hipLaunchKernelGGL(lanczos_pass_kernel<CH>, dim3((unsigned)((w + kLzTx - 1) / kLzTx), (unsigned)((h + kLzTy - 1) / kLzTy), run),
                       block, (size_t)kLzTy * ksy * sizeof(int), s, (const uint8_t*)mp, dp, (const int2*)(d + 2 * (size_t)w),
                       (const int*)(d + 2 * (size_t)w + 2 * (size_t)h + (size_t)w * ksx), ksy, 1, H, w, h, w);
    CTRLV_LAUNCH_CHECK();
  }
  return CTRLV_OK;
}

inline unsigned blocks_for(long n) { return (unsigned)((n + 255) / 256); }
constexpr long kMaxThreads = 0x7fffffffL * 256;      // one-dimensional grids: 2^31 - 1 workgroups of 256

// ks and the normalised weights of _gaussian_kernel1d for one axis (fp32 like the torch restatement)
int gaussian_taps(int in, int out, float* k) {
  const double factor = (double)in / (double)out;
  const double sigma = fmax((factor - 1.0) / 2.0, 0.001);
  int ks = (int)fmax(2.0 * 2 * sigma, 3.0);
  if (ks % 2 == 0) ks += 1;
  if (ks > kMaxTaps) return ks;
  const float den = (float)(2 * sigma * sigma);
  float sum = 0.f;
  for (int i = 0; i < ks; ++i) {
    const float x = (float)(i - ks / 2);
    k[i] = expf(-(x * x) / den);
    sum += k[i];
  }
  for (int i = 0; i < ks; ++i) k[i] /= sum;
  return ks;
}

}  // namespace

// Host-side validation of one resize (shared with the clip driver, which must refuse a request before its first launch).
int ctrlv_resize_check(int n, int H, int W, int h, int w) {
  CTRLV_CHECK_SHAPE(n > 0 && H > 0 && W > 0 && h > 0 && w > 0 && (long)n * 3 <= 65535, "resize_antialias: n, H, W, h, w must be "
                    "positive and n <= 21845 (got n=%d, %dx%d -> %dx%d)", n, H, W, h, w);
  CTRLV_CHECK_SHAPE((long)H <= 8L * h && (long)W <= 8L * w, "resize_antialias: a down-scale factor above 8 (%dx%d -> %dx%d) needs "
                    "more than %d blur taps", H, W, h, w, kMaxTaps);
  float k[kMaxTaps];
  const int ksy = gaussian_taps(H, h, k), ksx = gaussian_taps(W, w, k);
  CTRLV_CHECK_SHAPE(ksy <= kMaxTaps && ksx <= kMaxTaps, "resize_antialias: %d / %d blur taps, at most %d", ksy, ksx, kMaxTaps);
  CTRLV_CHECK_SHAPE(ksy / 2 < H && ksx / 2 < W, "resize_antialias: the blur's reflect padding (%d rows, %d columns) is undefined "
                    "for a %dx%d image", ksy / 2, ksx / 2, H, W);
  return CTRLV_OK;
}

// the one launch behind ctrlv_resize_antialias (clamp = 0) and ctrlv_resize_antialias_clamped (clamp = 1)
static int resize_antialias_launch(const void* src, int src_u8, int n, int H, int W, void* dst, int dst_dtype, int h, int w,
                                   const float* mean, const float* std, int clamp, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(src && dst, "resize_antialias: null pointer");
  CTRLV_CHECK_ARG((mean == nullptr) == (std == nullptr), "resize_antialias: mean and std come together");
  if (dst_dtype != 0 && dst_dtype != CTRLV_ELEM_DTYPE) {
    ctrlv_set_error("resize_antialias: dst dtype code %d (0 fp32 or %d, this library's element type)", dst_dtype, CTRLV_ELEM_DTYPE);
    return CTRLV_E_BAD_DTYPE;
  }
  const int rc = ctrlv_resize_check(n, H, W, h, w);
  if (rc != CTRLV_OK) return rc;
  ResizeParams P;
  memset(&P, 0, sizeof(P));
  P.n = n; P.H = H; P.W = W; P.h = h; P.w = w;
  P.ksy = gaussian_taps(H, h, P.ky);
  P.ksx = gaussian_taps(W, w, P.kx);
  P.sy = h > 1 ? (float)(H - 1) / (float)(h - 1) : 0.f;
  P.sx = w > 1 ? (float)(W - 1) / (float)(w - 1) : 0.f;
  P.src_u8 = src_u8 ? 1 : 0;
  P.dst_dtype = dst_dtype;
  P.normalize = mean ? 1 : 0;
  P.clamp = clamp;
  for (int c = 0; c < 3; ++c) {
    P.mean[c] = mean ? mean[c] : 0.f;
    P.stdv[c] = std ? std[c] : 1.f;
    CTRLV_CHECK_ARG(P.stdv[c] != 0.f, "resize_antialias: std[%d] is zero", c);
  }
  // the LDS tile: an upper bound of the source rows / columns a th x 32 output tile touches (the kernel clamps to it)
  P.span_x = (int)fmin((double)W, floor((kTileW - 1) * (double)P.sx) + 6 + 2 * (P.ksx / 2));
  size_t lds = 0;
  for (P.th = 8; P.th >= 1; P.th >>= 1) {
    P.span_y = (int)fmin((double)H, floor((P.th - 1) * (double)P.sy) + 6);
    lds = (size_t)P.span_y * P.span_x * sizeof(float);
    if (lds <= 64 * 1024) break;
  }
  CTRLV_CHECK_SHAPE(P.th >= 1, "resize_antialias: a one-row tile needs %zu bytes of LDS", lds);
  const dim3 grid((unsigned)((w + kTileW - 1) / kTileW), (unsigned)((h + P.th - 1) / P.th), (unsigned)(n * 3));
  CTRLV_CHECK_SHAPE(grid.y <= 65535, "resize_antialias: %d output rows in tiles of %d", h, P.th);
  hipLaunchKernelGGL(resize_antialias_kernel, grid, dim3(256), lds, (hipStream_t)stream, src, dst, P);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

extern "C" int ctrlv_resize_antialias(const void* src, int src_u8, int n, int H, int W, void* dst, int dst_dtype, int h, int w,
                                      const float* mean, const float* std, ctrlv_stream_t stream) {
  return resize_antialias_launch(src, src_u8, n, H, W, dst, dst_dtype, h, w, mean, std, 0, stream);
}

extern "C" int ctrlv_resize_antialias_clamped(const void* src, int src_u8, int n, int H, int W, void* dst, int dst_dtype, int h,
                                              int w, const float* mean, const float* std, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(mean != nullptr && std != nullptr, "resize_antialias_clamped: mean and std are required (the clamp belongs to "
                  "the normalising epilogue)");
  return resize_antialias_launch(src, src_u8, n, H, W, dst, dst_dtype, h, w, mean, std, 1, stream);
}

extern "C" int ctrlv_pixels_prepare(const void* image_u8, const float* noise, float strength, int n, int H, int W, void* out,
                                    ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(image_u8 && out, "pixels_prepare: null pointer");
  CTRLV_CHECK_SHAPE(n > 0 && H > 0 && W > 0 && (long)n * H * W <= kMaxThreads, "pixels_prepare: n, H, W must be positive");
  const long HW = (long)H * W;
  hipLaunchKernelGGL(pixels_prepare_kernel, dim3(blocks_for(n * HW)), dim3(256), 0, (hipStream_t)stream,
                     (const uint8_t*)image_u8, noise, strength, n, HW, (el_t*)out);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

extern "C" int ctrlv_frames_to_u8(const void* frames, int m, int H, int W, void* out_u8, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(frames && out_u8, "frames_to_u8: null pointer");
  CTRLV_CHECK_SHAPE(m > 0 && H > 0 && W > 0, "frames_to_u8: m, H, W must be positive");
  CTRLV_CHECK_ARG(((uintptr_t)out_u8 & 3) == 0, "frames_to_u8: the output must be 4-byte aligned");
  const long HW = (long)H * W, total = (long)m * HW;
  hipLaunchKernelGGL(frames_to_u8_kernel, dim3(blocks_for((total + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                     (const el_t*)frames, total, HW, (uint8_t*)out_u8);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

int ctrlv_pio_cfg_double(const void* src, int src_dtype, void* dst, int B, long per, int cfg, hipStream_t s) {
  const long n = (long)B * per;
  hipLaunchKernelGGL(cfg_double_kernel, dim3(blocks_for(n)), dim3(256), 0, s, src, src_dtype, (el_t*)dst, n, cfg);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

int ctrlv_pio_lmi_cond(const void* first, void* lmi, int B, int F, int c_lat, int hw, int cfg, hipStream_t s) {
  const long total = (long)(cfg ? 2 : 1) * B * F * c_lat * hw;
  hipLaunchKernelGGL(lmi_cond_kernel, dim3(blocks_for(total)), dim3(256), 0, s, (const el_t*)first, (el_t*)lmi, B, F, c_lat, hw,
                     cfg);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

int ctrlv_pio_lmi_boxes(const void* src, int src_dtype, int src_frames, int compact, void* lmi, int B, int F, int K, int c_lat,
                        int hw, int cfg, hipStream_t s) {
  const int take = K + 1 < F ? K + 1 : F;
  const long total = (long)B * take * c_lat * hw;
  hipLaunchKernelGGL(lmi_boxes_kernel, dim3(blocks_for(total)), dim3(256), 0, s, src, src_dtype, src_frames, compact, (el_t*)lmi,
                     B, F, K, take, c_lat, hw, cfg);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

int ctrlv_pio_clamp_frames(void* x, long n, hipStream_t s) {
  const int vec = ((uintptr_t)x & 15) == 0 ? 1 : 0;
  hipLaunchKernelGGL(clamp_frames_kernel, dim3(blocks_for(vec ? (n + 7) / 8 : n)), dim3(256), 0, s, (el_t*)x, n, vec);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

int ctrlv_pio_lmi_scatter(const void* scaled, void* lmi, int B, int F, int c_lat, int hw, int cfg, hipStream_t s) {
  const long per = (long)c_lat * hw, n_half = (long)B * F * per;
  hipLaunchKernelGGL(lmi_scatter_kernel, dim3(blocks_for(n_half)), dim3(256), 0, s, (const el_t*)scaled, (el_t*)lmi, n_half, per,
                     cfg);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

int ctrlv_pio_scale_latents(const float* x, float* out, void* scaled, long n, float inv, hipStream_t s) {
  hipLaunchKernelGGL(scale_latents_kernel, dim3(blocks_for(n)), dim3(256), 0, s, x, out, (el_t*)scaled, n, inv);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

int ctrlv_pio_decode_input(const float* x, void* z, long n, float inv, hipStream_t s) {
  hipLaunchKernelGGL(decode_input_kernel, dim3(blocks_for(n)), dim3(256), 0, s, x, (el_t*)z, n, inv);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

extern "C" int ctrlv_randn(uint64_t seed, uint32_t clip0, uint32_t call, uint32_t stream_id, int n_clips, size_t per_clip,
                           float scale, int round_dtype, void* out, int out_dtype, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(out != nullptr, "randn: null output");
  CTRLV_CHECK_ARG(round_dtype == 0 || round_dtype == 1, "randn: round_dtype=%d must be 0 (fp32) or 1 (the element type)", round_dtype);
  CTRLV_CHECK_ARG(isfinite(scale), "randn: scale=%g", (double)scale);
  if (out_dtype != 0 && out_dtype != CTRLV_ELEM_DTYPE) {
    ctrlv_set_error("randn: out dtype code %d (0 fp32 or %d, this library's element type)", out_dtype, CTRLV_ELEM_DTYPE);
    return CTRLV_E_BAD_DTYPE;
  }
  CTRLV_CHECK_SHAPE(n_clips >= 1 && n_clips <= 65536 && per_clip >= 1, "randn: n_clips=%d must be in [1, 65536] and per_clip=%zu "
                    "positive", n_clips, per_clip);
  CTRLV_CHECK_SHAPE(per_clip <= ((size_t)1 << 34), "randn: per_clip=%zu is above the counter's range (2^32 blocks of 4 elements "
                    "per clip)", per_clip);
  CTRLV_CHECK_ARG(((uintptr_t)out & (out_dtype == 0 ? 3 : 1)) == 0, "randn: the output is not aligned to its element size");
  const unsigned long long nblk = ((unsigned long long)per_clip + 3) / 4, total = nblk * (unsigned long long)n_clips;
  const unsigned long long want = (total + 255) / 256;
  const unsigned grid = (unsigned)(want < 16384 ? want : 16384);       // grid-stride: 64 workgroups per CU at the most
  hipLaunchKernelGGL(randn_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (uint32_t)(seed & 0xffffffffu),
                     (uint32_t)(seed >> 32), clip0, call, stream_id, (unsigned long long)per_clip, nblk, total, scale, round_dtype,
                     out, out_dtype != 0 ? 1 : 0);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

extern "C" int ctrlv_euler_schedule(int num_steps, float sigma_min, float sigma_max, float* sigmas, float* timesteps,
                                    double* init_noise_sigma) {
  CTRLV_CHECK_SHAPE(num_steps >= 1 && num_steps <= 1024, "euler_schedule: num_steps=%d must be in [1, 1024]", num_steps);
  CTRLV_CHECK_ARG(sigmas != nullptr && timesteps != nullptr, "euler_schedule: sigmas / timesteps are null (host arrays of "
                  "num_steps + 1 and num_steps floats)");
  const bool svd = sigma_min == 0.f && sigma_max == 0.f;          // SVD's bounds as the doubles the Python scheduler holds
  const double lo = svd ? 0.002 : (double)sigma_min, hi = svd ? 700.0 : (double)sigma_max;
  CTRLV_CHECK_ARG(isfinite(lo) && isfinite(hi) && lo > 0.0 && lo < hi,
                  "euler_schedule: sigma_min=%g / sigma_max=%g must be finite, positive and ordered (both 0: 0.002 and 700)", lo, hi);
  const double a = pow(hi, 1.0 / 7.0), b = pow(lo, 1.0 / 7.0);
  const double step = num_steps > 1 ? 1.0 / (double)(num_steps - 1) : 0.0;
  for (int i = 0; i < num_steps; ++i) {
    const double ramp = i == num_steps - 1 && num_steps > 1 ? 1.0 : (double)i * step;
    sigmas[i] = (float)pow(a + ramp * (b - a), 7.0);
    timesteps[i] = 0.25f * (float)log((double)sigmas[i]);
  }
  sigmas[num_steps] = 0.f;
  if (init_noise_sigma) *init_noise_sigma = sqrt((double)sigmas[0] * (double)sigmas[0] + 1.0);
  return CTRLV_OK;
}

// Host-side validation of one Lanczos resize (shared with ctrlv_pipeline_prepare, which refuses before its first launch).
int ctrlv_resize_lanczos_check(int n, int H, int W, int h, int w) {
  CTRLV_CHECK_SHAPE(n > 0 && H > 0 && W > 0 && h > 0 && w > 0, "resize_lanczos: an image with a zero dimension (n=%d, %dx%d -> "
                    "%dx%d)", n, H, W, h, w);
  CTRLV_CHECK_SHAPE(n <= 65535 && (h + kLzTy - 1) / kLzTy <= 65535 && (H + kLzTy - 1) / kLzTy <= 65535,
                    "resize_lanczos: n=%d images of %d -> %d rows: at most 65535 images and 262140 rows", n, H, h);
  CTRLV_CHECK_SHAPE((long)H <= (long)kLzMaxScale * h && (long)W <= (long)kLzMaxScale * w, "resize_lanczos: a down-scale above %d "
                    "(%dx%d -> %dx%d)", kLzMaxScale, H, W, h, w);
  return CTRLV_OK;
}

extern "C" size_t ctrlv_resize_lanczos_ws_bytes(int n, int H, int W, int h, int w) {
  if (ctrlv_resize_lanczos_check(n, H, W, h, w) != CTRLV_OK) return 0;
  return up256(resample_table_ints(H, W, h, w, kFilterLanczos) * sizeof(int32_t)) + up256((size_t)n * H * w * 3);
}

extern "C" int ctrlv_resize_lanczos_u8(const void* src_u8, int n, int H, int W, void* dst_u8, int h, int w, void* ws,
                                       size_t ws_bytes, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(src_u8 != nullptr && dst_u8 != nullptr, "resize_lanczos: null pointer");
  CTRLV_TRY(ctrlv_resize_lanczos_check(n, H, W, h, w));
  CTRLV_CHECK_ARG(ws != nullptr && ((uintptr_t)ws & 15) == 0, "resize_lanczos: the workspace must be non-null and 16-byte aligned");
  const size_t need = ctrlv_resize_lanczos_ws_bytes(n, H, W, h, w);
  if (ws_bytes < need) {
    ctrlv_set_error("resize_lanczos: ws_bytes=%zu is smaller than the %zu bytes this resize needs (ctrlv_resize_lanczos_ws_bytes)",
                    ws_bytes, need);
    return CTRLV_E_WORKSPACE;
  }
  return resample_two_pass<3>((const uint8_t*)src_u8, n, H, W, (uint8_t*)dst_u8, h, w, kFilterLanczos, ws, (hipStream_t)stream);
}

// Host-side validation of one resize of planes.
static int resize_frames_check(int planes, int H, int W, int h, int w, int filter) {
  CTRLV_CHECK_ARG(filter == kFilterLanczos || filter == kFilterBilinear || filter == kFilterBicubic, "resize_frames: filter=%d "
                  "must be one of PIL's codes 1 (LANCZOS), 2 (BILINEAR), 3 (BICUBIC)", filter);
  CTRLV_CHECK_SHAPE(planes > 0 && H > 0 && W > 0 && h > 0 && w > 0, "resize_frames: a zero dimension (planes=%d, %dx%d -> %dx%d)",
                    planes, H, W, h, w);
  CTRLV_CHECK_SHAPE((h + kLzTy - 1) / kLzTy <= 65535 && (H + kLzTy - 1) / kLzTy <= 65535, "resize_frames: %d -> %d rows: at most "
                    "262140 rows", H, h);
  CTRLV_CHECK_SHAPE((long)H <= (long)kLzMaxScale * h && (long)W <= (long)kLzMaxScale * w, "resize_frames: a down-scale above %d "
                    "(%dx%d -> %dx%d)", kLzMaxScale, H, W, h, w);
  return CTRLV_OK;
}

extern "C" size_t ctrlv_resize_frames_ws_bytes(int planes, int H, int W, int h, int w, int filter) {
  if (resize_frames_check(planes, H, W, h, w, filter) != CTRLV_OK) return 0;
  return up256(resample_table_ints(H, W, h, w, filter) * sizeof(int32_t)) + up256((size_t)planes * H * w);
}

extern "C" int ctrlv_resize_frames_u8(const void* src_u8, int planes, int H, int W, void* dst_u8, int h, int w, int filter, void* ws,
                                      size_t ws_bytes, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(src_u8 != nullptr && dst_u8 != nullptr, "resize_frames: null pointer");
  CTRLV_TRY(resize_frames_check(planes, H, W, h, w, filter));
  CTRLV_CHECK_ARG(ws != nullptr && ((uintptr_t)ws & 15) == 0, "resize_frames: the workspace must be non-null and 16-byte aligned");
  const size_t need = ctrlv_resize_frames_ws_bytes(planes, H, W, h, w, filter);
  if (ws_bytes < need) {
    ctrlv_set_error("resize_frames: ws_bytes=%zu is smaller than the %zu bytes this resize needs (ctrlv_resize_frames_ws_bytes)",
                    ws_bytes, need);
    return CTRLV_E_WORKSPACE;
  }
  return resample_two_pass<1>((const uint8_t*)src_u8, planes, H, W, (uint8_t*)dst_u8, h, w, filter, ws, (hipStream_t)stream);
}
