// Layout / element-wise kernels of the denoising path (gfx950).  All HBM-bound; 16-byte vectors where the layout
// allows it.  See include/ctrlv_hip.h for the reference call sites each one replaces.
#include "common.h"

namespace {

__device__ __forceinline__ float load_any(const void* p, int dtype, long i) {
  if (dtype == 0) return ((const float*)p)[i];
  if (dtype == 1) return (float)((const _Float16*)p)[i];
  return bf16_to_f32(((const bf16_t*)p)[i]);
}
__device__ __forceinline__ void store_any(void* p, int dtype, long i, float v) {
  if (dtype == 0) ((float*)p)[i] = v;
  else if (dtype == 1) ((_Float16*)p)[i] = (_Float16)v;
  else ((bf16_t*)p)[i] = f32_to_bf16(v);
}

// one thread per (image, pixel): reads are coalesced over pixels for every channel plane
__global__ void nchw_to_rows_kernel(const void* __restrict__ src, int dtype, int n_img, int C, int HW,
                                    el_t* __restrict__ dst, int ldc, int c_off) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)n_img * HW) return;
  const long n = idx / HW, p = idx % HW;
  el_t* d = dst + idx * ldc + c_off;
  for (int c = 0; c < C; ++c) d[c] = f32_to_el(load_any(src, dtype, (n * C + c) * HW + p));
}

__global__ void rows_to_nchw_kernel(const el_t* __restrict__ src, int ldc, int n_img, int C, int HW,
                                    void* __restrict__ dst, int dtype) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)n_img * HW) return;
  const long n = idx / HW, p = idx % HW;
  const el_t* s = src + idx * ldc;
  for (int c = 0; c < C; ++c) store_any(dst, dtype, (n * C + c) * HW + p, el_to_f32(s[c]));
}

// Conv3d(C, C, (3, 1, 1), padding (1, 0, 0)) over the frames of ONE clip on channels-last rows with C <= 4 channels, written
// as NCHW: the `time_conv_out` that ends AutoencoderKLTemporalDecoder.decode (3 -> 3 channels).  One thread per
// (frame, pixel): 3 taps x C inputs, C outputs, fp32 (the reference runs this conv in the VAE's dtype on NCHW tensors).
__global__ void time_conv_rows_to_nchw_kernel(const el_t* __restrict__ src, int ldc, int n_frames, int C, int HW,
                                              const float* __restrict__ w, const float* __restrict__ bias,
                                              void* __restrict__ dst, int dtype) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)n_frames * HW) return;
  const int f = (int)(idx / HW);
  const long p = idx % HW;
  float acc[4];
#pragma unroll
  for (int o = 0; o < 4; ++o) acc[o] = o < C ? bias[o] : 0.f;
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int ff = f + t - 1;
    if (ff < 0 || ff >= n_frames) continue;
    const el_t* s = src + ((long)ff * HW + p) * ldc;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c >= C) break;
      const float x = el_to_f32(s[c]);
#pragma unroll
      for (int o = 0; o < 4; ++o)
        if (o < C) acc[o] = __builtin_fmaf(w[(o * C + c) * 3 + t], x, acc[o]);
    }
  }
  for (int o = 0; o < C; ++o) store_any(dst, dtype, ((long)f * C + o) * HW + p, acc[o]);
}

// quant_conv (1x1, 2L -> 2L) + DiagonalGaussianDistribution of AutoencoderKL.encode on the rows the encoder's conv_out GEMM
// wrote: one thread per (image, pixel), L <= 8 latent channels.  fp32 throughout: q[o] = b[o] + sum_c w[o][c] x[c] with c
// ascending (fmaf), mean = q[:L], logvar = clamp(q[L:], -30, 20), latent = scale * (mean + exp(0.5 logvar) * noise).  No
// atomics, fixed channel order: the same bits in every run.  Either output may be absent; each value is rounded once.
__global__ void vae_posterior_kernel(const el_t* __restrict__ rows, int ld, int n_img, int L, int HW, const float* __restrict__ qw,
                                     const float* __restrict__ qb, const float* __restrict__ noise, float scale,
                                     void* __restrict__ moments, void* __restrict__ latents, int dtype) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)n_img * HW) return;
  const long n = idx / HW, p = idx % HW;
  const int C = 2 * L;
  const el_t* s = rows + idx * ld;
  float x[16], q[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) x[c] = c < C ? el_to_f32(s[c]) : 0.f;
#pragma unroll
  for (int o = 0; o < 16; ++o) {
    float a = 0.f;
    if (o < C) {
      a = qb[o];
#pragma unroll
      for (int c = 0; c < 16; ++c)
        if (c < C) a = __builtin_fmaf(qw[o * C + c], x[c], a);
    }
    q[o] = a;
  }
  if (moments != nullptr) {
#pragma unroll
    for (int o = 0; o < 16; ++o)
      if (o < C) store_any(moments, dtype, (n * C + o) * HW + p, q[o]);
  }
  if (latents != nullptr) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (c >= L) break;
      float v = q[c];
      if (noise != nullptr) {
        // (q[] is indexed by unrolled constants only: L + c is a runtime index, so the log-variance is picked by a select chain)
        float lv = 0.f;
#pragma unroll
        for (int o = 0; o < 16; ++o)
          if (o == L + c) lv = q[o];
        lv = fminf(fmaxf(lv, -30.f), 20.f);
        v = __builtin_fmaf(expf(0.5f * lv), noise[(n * L + c) * HW + p], v);
      }
      store_any(latents, dtype, (n * L + c) * HW + p, scale * v);
    }
  }
}

// Backward of time_conv_rows_to_nchw_kernel.  One thread per (frame, pixel), grid-stride over at most kTcbBlocks blocks:
//   drows[f, p, c]  = sum_{t, o} w[o, c, t] * dout[f - t + 1, o, p]      (frames of the SAME clip only: the forward's zero padding)
//   dw[o, c, t]    += dout[f, o, p] * src[f + t - 1, p, c],   db[o] += dout[f, o, p]
// The parameter sums stay in registers over the thread's pixels, are reduced over the block (wave shuffles, then a fixed
// 4-term sum) and written as ONE row of `partials` per block; time_conv_bwd_finish_kernel adds the rows in block order.
// Grid and order are functions of the shape only: the same bits in every run.  Slots: (o * 4 + c) * 3 + t, 48 + o = db[o].
constexpr int kTcbBlocks = 256, kTcbSlots = 52, kTcbPitch = 64;
__global__ __launch_bounds__(256) void time_conv_bwd_kernel(const float* __restrict__ dout, const el_t* __restrict__ src, int lds,
                                                            int n_frames, int clip, int C, int HW, const float* __restrict__ w,
                                                            el_t* __restrict__ drows, int ldd, float* __restrict__ partials) {
  __shared__ float red[4][kTcbSlots];
  float acc[kTcbSlots];
#pragma unroll
  for (int j = 0; j < kTcbSlots; ++j) acc[j] = 0.f;
  float wr[48];
#pragma unroll
  for (int o = 0; o < 4; ++o)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int t = 0; t < 3; ++t) wr[(o * 4 + c) * 3 + t] = (o < C && c < C) ? w[(o * C + c) * 3 + t] : 0.f;
  const long total = (long)n_frames * HW;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int f = (int)(idx / HW);
    const long p = idx % HW;
    const int f0 = f - f % clip, f1 = f0 + clip;             // this frame's clip: [f0, f1)
    float g[3][4];                                           // dout of frames f + 1, f, f - 1 (tap t reads frame f - t + 1)
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int fo = f - t + 1;
      const bool in = fo >= f0 && fo < f1;
#pragma unroll
      for (int o = 0; o < 4; ++o) g[t][o] = (in && o < C) ? dout[((long)fo * C + o) * HW + p] : 0.f;
    }
    float dr[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int c = 0; c < 4; ++c) dr[c] = __builtin_fmaf(wr[(o * 4 + c) * 3 + t], g[t][o], dr[c]);
    el_t* d = drows + idx * ldd;
    if (ldd == 4) {
      *(uint2*)d = make_uint2(pack_elx2(dr[0], dr[1]), pack_elx2(dr[2], dr[3]));      // (channels >= C: wr is zero there)
    } else {
      for (int c = 0; c < ldd; ++c) d[c] = f32_to_el(c < 4 ? dr[c] : 0.f);
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) acc[48 + o] += g[1][o];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int ff = f + t - 1;
      if (ff < f0 || ff >= f1) continue;
      const el_t* s = src + ((long)ff * HW + p) * lds;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (c >= C) break;
        const float x = el_to_f32(s[c]);
#pragma unroll
        for (int o = 0; o < 4; ++o) acc[(o * 4 + c) * 3 + t] = __builtin_fmaf(g[1][o], x, acc[(o * 4 + c) * 3 + t]);
      }
    }
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < kTcbSlots; ++j) {
    const float v = wave_sum(acc[j]);
    if (lane == 0) red[wid][j] = v;
  }
  __syncthreads();
  if (threadIdx.x < kTcbSlots)
    partials[(long)blockIdx.x * kTcbPitch + threadIdx.x] =
        (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

__global__ void time_conv_bwd_finish_kernel(const float* __restrict__ partials, int nblocks, int C, float* __restrict__ dw,
                                            float* __restrict__ db) {
  const int j = threadIdx.x;
  if (j >= kTcbSlots) return;
  float s = 0.f;
  for (int b = 0; b < nblocks; ++b) s += partials[(long)b * kTcbPitch + j];
  if (j >= 48) {
    if (j - 48 < C) db[j - 48] = s;
    return;
  }
  const int o = j / 12, c = (j / 3) % 4, t = j % 3;
  if (o < C && c < C) dw[(o * C + c) * 3 + t] = s;
}

// tiled transpose for wide tensors (foreign NCHW ControlNet residuals): 64 pixels x 64 channels per block
__global__ __launch_bounds__(256) void nchw_to_rows_tiled_kernel(const void* __restrict__ src, int dtype, int C,
                                                                 int HW, el_t* __restrict__ dst, int ldc,
                                                                 int c_off) {
  __shared__ float tile[64][65];
  const long n = blockIdx.z;
  const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int c = ty; c < 64; c += 4)
    tile[c][tx] = (c0 + c < C && p0 + tx < HW) ? load_any(src, dtype, (n * C + c0 + c) * HW + p0 + tx) : 0.f;
  __syncthreads();
  for (int p = ty; p < 64; p += 4)
    if (p0 + p < HW && c0 + tx < C) dst[(n * HW + p0 + p) * ldc + c_off + c0 + tx] = f32_to_el(tile[tx][p]);
}
__global__ __launch_bounds__(256) void rows_to_nchw_tiled_kernel(const el_t* __restrict__ src, int ldc, int C,
                                                                 int HW, void* __restrict__ dst, int dtype) {
  __shared__ float tile[64][65];
  const long n = blockIdx.z;
  const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int p = ty; p < 64; p += 4)
    tile[p][tx] = (p0 + p < HW && c0 + tx < C) ? el_to_f32(src[(n * HW + p0 + p) * ldc + c0 + tx]) : 0.f;
  __syncthreads();
  for (int c = ty; c < 64; c += 4)
    if (c0 + c < C && p0 + tx < HW) store_any(dst, dtype, (n * C + c0 + c) * HW + p0 + tx, tile[tx][c]);
}

__global__ void im2col3x3_kernel(const el_t* __restrict__ x, int n_img, int H, int W, int Cp, el_t* __restrict__ col,
                                 int Kp) {
  const int cpr = Kp >> 3;  // 16-B chunks per output row
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)n_img * H * W * cpr;
  if (idx >= total) return;
  const long m = idx / cpr;
  const int j = (int)(idx % cpr);
  const int k0 = j * 8, tap = k0 / Cp, c0 = k0 % Cp;
  uint4 v = make_uint4(0, 0, 0, 0);
  if (tap < 9) {
    const int hw = H * W;
    const long n = m / hw;
    const int rem = (int)(m % hw), y = rem / W, xx = rem % W;
    const int yi = y + tap / 3 - 1, xi = xx + tap % 3 - 1;
    if (yi >= 0 && yi < H && xi >= 0 && xi < W) v = *(const uint4*)(x + ((n * H + yi) * W + xi) * Cp + c0);
  }
  *(uint4*)(col + m * Kp + k0) = v;
}

// (x / y carry no __restrict__: in place -- y == x -- is part of the contract, ctrlv_hip.h; plan.hip add_res uses it)
__global__ void axpby_kernel(const el_t* x, const el_t* __restrict__ r, float a, float b, el_t* y, size_t n) {
  const size_t nv = n >> 3;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (size_t)gridDim.x * blockDim.x) {
    float fx[8], fr[8];
    unpack_elx8(((const uint4*)x)[i], fx);
    unpack_elx8(((const uint4*)r)[i], fr);
#pragma unroll
    for (int e = 0; e < 8; ++e) fx[e] = a * fx[e] + b * fr[e];
    ((uint4*)y)[i] = pack_elx8(fx);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 7)) {
    const size_t i = (nv << 3) + threadIdx.x;
    y[i] = f32_to_el(a * el_to_f32(x[i]) + b * el_to_f32(r[i]));
  }
}

// (y, y_lo) = split(a * (x + x_lo) + b * r) on a SPLIT skip tensor (common.h split_lo8); n a multiple of 8
// (in place allowed: y == x and ylo == xlo, so none of the four carries __restrict__)
__global__ void axpby_split_kernel(const el_t* x, const lo_t* xlo, const el_t* __restrict__ r, float a, float b, el_t* y,
                                   lo_t* ylo, size_t n) {
  const size_t nv = n >> 3;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (size_t)gridDim.x * blockDim.x) {
    float fx[8], fr[8];
    unpack_elx8(((const uint4*)x)[i], fx);
    if (xlo) add_lo8(fx, ((const uint2*)xlo)[i]);
    unpack_elx8(((const uint4*)r)[i], fr);
#pragma unroll
    for (int e = 0; e < 8; ++e) fx[e] = a * fx[e] + b * fr[e];
    const uint4 hi = pack_elx8(fx);
    ((uint4*)y)[i] = hi;
    ((uint2*)ylo)[i] = split_lo8(fx, hi);
  }
}

__global__ void silu_kernel(const el_t* __restrict__ x, el_t* __restrict__ y, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    y[i] = f32_to_el(silu_f(el_to_f32(x[i])));
}

__global__ void timestep_embedding_kernel(const float* __restrict__ t, int n, int dim, el_t* __restrict__ out) {
  const int half = dim >> 1;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * half) return;
  const int r = idx / half, i = idx % half;
  const float freq = expf(-9.210340371976184f * (float)i / (float)half);  // ln(10000)
  const float arg = t[r] * freq;
  float s, c;
  sincosf(arg, &s, &c);
  out[(long)r * dim + i] = f32_to_el(c);          // flip_sin_to_cos: [cos | sin]
  out[(long)r * dim + half + i] = f32_to_el(s);
}

__global__ void cfg_euler_kernel(float* __restrict__ lat, const void* __restrict__ pred, int pred_dtype, int cfg,
                                 const float* __restrict__ guidance, int B, int F, int CHW, float sigma,
                                 float sigma_next, el_t* __restrict__ scaled_next) {
  const long total = (long)B * F * CHW;
  const float c_out = -sigma / sqrtf(sigma * sigma + 1.0f);
  const float c_skip = 1.0f / (sigma * sigma + 1.0f);
  const float dt = sigma_next - sigma;
  const float inv_next = 1.0f / sqrtf(sigma_next * sigma_next + 1.0f);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int f = (int)((i / CHW) % F);
    float v = load_any(pred, pred_dtype, cfg ? total + i : i);
    if (cfg) {
      const float u = load_any(pred, pred_dtype, i);
      // the reference combines in the model dtype: round the guided prediction like `noise_pred` would be
      v = u + guidance[f] * (v - u);
      if (pred_dtype == 2) v = bf16_to_f32(f32_to_bf16(v));
      else if (pred_dtype == 1) v = (float)(_Float16)v;
    }
    const float x = lat[i];
    const float x0 = v * c_out + x * c_skip;
    const float deriv = (x - x0) / sigma;
    const float xn = x + deriv * dt;
    lat[i] = xn;
    if (scaled_next) scaled_next[i] = f32_to_el(xn * inv_next);
  }
}

}  // namespace

static inline unsigned grid_for(size_t n, int bs, unsigned cap = 256 * 16) {
  size_t g = (n + bs - 1) / bs;
  if (g < 1) g = 1;
  return (unsigned)(g > cap ? cap : g);
}

extern "C" int ctrlv_nchw_to_rows(const void* src, int src_dtype, int n_img, int C, int HW, void* dst, int ldc,
                                  int c_off, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(src && dst && src_dtype >= 0 && src_dtype <= 2, "nchw_to_rows: bad arguments");
  CTRLV_CHECK_SHAPE(n_img > 0 && C > 0 && HW > 0 && c_off >= 0 && c_off + C <= ldc, "nchw_to_rows: bad shape");
  if (C >= 32) {
    dim3 grid((HW + 63) / 64, (C + 63) / 64, n_img);
    hipLaunchKernelGGL(nchw_to_rows_tiled_kernel, grid, dim3(256), 0, (hipStream_t)stream, src, src_dtype, C, HW,
                       (el_t*)dst, ldc, c_off);
  } else {
    const long total = (long)n_img * HW;
    hipLaunchKernelGGL(nchw_to_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       src, src_dtype, n_img, C, HW, (el_t*)dst, ldc, c_off);
  }
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

extern "C" int ctrlv_rows_to_nchw(const void* src, int ldc, int n_img, int C, int HW, void* dst, int dst_dtype,
                                  ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(src && dst && dst_dtype >= 0 && dst_dtype <= 2, "rows_to_nchw: bad arguments");
  CTRLV_CHECK_SHAPE(n_img > 0 && C > 0 && HW > 0 && C <= ldc, "rows_to_nchw: bad shape");
  if (C >= 32) {
    dim3 grid((HW + 63) / 64, (C + 63) / 64, n_img);
    hipLaunchKernelGGL(rows_to_nchw_tiled_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const el_t*)src, ldc, C,
                       HW, dst, dst_dtype);
  } else {
    const long total = (long)n_img * HW;
    hipLaunchKernelGGL(rows_to_nchw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const el_t*)src, ldc, n_img, C, HW, dst, dst_dtype);
  }
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

extern "C" int ctrlv_time_conv_rows_to_nchw(const void* src, int ldc, int n_frames, int C, int HW, const float* weight,
                                            const float* bias, void* dst, int dst_dtype, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(src && dst && weight && bias && dst_dtype >= 0 && dst_dtype <= 2, "time_conv_rows_to_nchw: bad arguments");
  CTRLV_CHECK_SHAPE(n_frames > 0 && HW > 0 && C > 0 && C <= 4 && C <= ldc, "time_conv_rows_to_nchw: 1 <= C <= 4 channels");
  const long total = (long)n_frames * HW;
  hipLaunchKernelGGL(time_conv_rows_to_nchw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const el_t*)src, ldc, n_frames, C, HW, weight, bias, dst, dst_dtype);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

extern "C" int ctrlv_vae_posterior(const void* rows, int ld, int n_img, int L, int HW, const float* quant_weight,
                                   const float* quant_bias, const float* noise, float scale, void* moments_out,
                                   void* latents_out, int out_dtype, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(rows && quant_weight && quant_bias, "vae_posterior: null pointer");
  CTRLV_CHECK_ARG(moments_out || latents_out, "vae_posterior: moments_out and latents_out are both NULL");
  CTRLV_CHECK_ARG(out_dtype >= 0 && out_dtype <= 2, "vae_posterior: out_dtype=%d (0 fp32, 1 fp16, 2 bf16)", out_dtype);
  CTRLV_CHECK_SHAPE(L > 0 && L <= 8, "vae_posterior: latent_channels=%d must be in [1, 8]", L);
  CTRLV_CHECK_SHAPE(n_img > 0 && HW > 0 && ld >= 2 * L, "vae_posterior: bad shape (n=%d, pixels=%d, ld=%d < 2 L=%d)", n_img, HW, ld,
                    2 * L);
  const long total = (long)n_img * HW;
  hipLaunchKernelGGL(vae_posterior_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const el_t*)rows, ld, n_img, L, HW, quant_weight, quant_bias, noise, scale, moments_out, latents_out,
                     out_dtype);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

extern "C" int ctrlv_time_conv_rows_to_nchw_bwd(const float* dout, const void* src, int ldc_src, int n_frames, int clip_frames,
                                                int C, int HW, const float* weight, void* drows, int ldc, float* dweight,
                                                float* dbias, float* scratch, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(dout && src && weight && drows && dweight && dbias && scratch, "time_conv_rows_to_nchw_bwd: null pointer");
  CTRLV_CHECK_SHAPE(n_frames > 0 && HW > 0 && C > 0 && C <= 4 && C <= ldc_src && C <= ldc && ldc <= 64,
                    "time_conv_rows_to_nchw_bwd: 1 <= C <= 4 channels, C <= ldc <= 64");
  CTRLV_CHECK_SHAPE(clip_frames > 0 && n_frames % clip_frames == 0,
                    "time_conv_rows_to_nchw_bwd: n_frames=%d must be whole clips of clip_frames=%d", n_frames, clip_frames);
  static_assert(kTcbBlocks * kTcbPitch == CTRLV_TIME_CONV_BWD_SCRATCH_FLOATS, "scratch size of the header");
  const long total = (long)n_frames * HW;
  const long want = (total + 255) / 256;
  const int blocks = (int)(want < kTcbBlocks ? want : kTcbBlocks);
  hipLaunchKernelGGL(time_conv_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dout, (const el_t*)src, ldc_src,
                     n_frames, clip_frames, C, HW, weight, (el_t*)drows, ldc, scratch);
  CTRLV_LAUNCH_CHECK();
  hipLaunchKernelGGL(time_conv_bwd_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, scratch, blocks, C, dweight, dbias);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

extern "C" int ctrlv_im2col3x3(const void* x, int n_img, int H, int W, int Cp, void* col, int Kp,
                               ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(x && col, "im2col3x3: null pointer");
  CTRLV_CHECK_SHAPE(n_img > 0 && H > 0 && W > 0 && Cp > 0 && Cp % 8 == 0 && Kp % 64 == 0 && Kp >= 9 * Cp,
                    "im2col3x3: Cp must be a multiple of 8 and Kp a multiple of 64 >= 9*Cp");
  const long total = (long)n_img * H * W * (Kp / 8);
  hipLaunchKernelGGL(im2col3x3_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const el_t*)x, n_img, H, W, Cp, (el_t*)col, Kp);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

extern "C" int ctrlv_axpby(const void* x, const void* r, float a, float b, void* y, size_t n, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(x && r && y && n > 0, "axpby: bad arguments");
  hipLaunchKernelGGL(axpby_kernel, dim3(grid_for(n / 8 + 1, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const el_t*)x, (const el_t*)r, a, b, (el_t*)y, n);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

extern "C" int ctrlv_axpby_split(const void* x, const void* x_lo, const void* r, float a, float b, void* y, void* y_lo,
                                 size_t n, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(x && r && y && y_lo && n > 0 && n % 8 == 0, "axpby_split: bad arguments (n must be a multiple of 8)");
  hipLaunchKernelGGL(axpby_split_kernel, dim3(grid_for(n / 8 + 1, 256)), dim3(256), 0, (hipStream_t)stream, (const el_t*)x,
                     (const lo_t*)x_lo, (const el_t*)r, a, b, (el_t*)y, (lo_t*)y_lo, n);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

extern "C" int ctrlv_silu(const void* x, void* y, size_t n, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(x && y && n > 0, "silu: bad arguments");
  hipLaunchKernelGGL(silu_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, (const el_t*)x,
                     (el_t*)y, n);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

extern "C" int ctrlv_timestep_embedding(const float* t, int n, int dim, void* out, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(t && out, "timestep_embedding: null pointer");
  CTRLV_CHECK_SHAPE(n > 0 && dim > 0 && dim % 2 == 0, "timestep_embedding: dim must be even");
  const int total = n * (dim / 2);
  hipLaunchKernelGGL(timestep_embedding_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, t, n,
                     dim, (el_t*)out);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

extern "C" int ctrlv_cfg_euler_step(float* latents, const void* noise_pred, int pred_dtype, int cfg,
                                    const float* guidance, int B, int F, int CHW, float sigma, float sigma_next,
                                    void* scaled_next, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(latents && noise_pred && pred_dtype >= 0 && pred_dtype <= 2, "cfg_euler_step: bad arguments");
  CTRLV_CHECK_ARG(!cfg || guidance, "cfg_euler_step: guidance table required with cfg");
  CTRLV_CHECK_SHAPE(B > 0 && F > 0 && CHW > 0 && sigma > 0.f, "cfg_euler_step: bad shape / sigma");
  const size_t total = (size_t)B * F * CHW;
  hipLaunchKernelGGL(cfg_euler_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, latents,
                     noise_pred, pred_dtype, cfg, guidance, B, F, CHW, sigma, sigma_next, (el_t*)scaled_next);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}
