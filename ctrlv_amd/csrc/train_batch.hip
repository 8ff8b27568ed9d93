// A training batch's arithmetic between the VAE / CLIP calls and the model call (gfx950): what tools/train_video_controlnet.py:
// 399-446 and tools/train_video_diffusion.py:440-514 do as eager torch ops, keyed on (seed, step, clip index).
//   ctrlv_train_draws     per clip: the index into the scheduler's tables, sigma, timestep, random_p and the two dropout masks
//   ctrlv_train_assemble  one pass over the latents: noisy = target + noise * sigma, the scaled model input, the masked
//                         conditioning channels in either frame layout, the channel concat; the noise given or drawn in place
//   ctrlv_tb_*            the driver's glue (train_batch.h; csrc/train_batch_plan.hip)
// The arithmetic is stated in include/ctrlv_hip.h; the generator is ctrlv_randn's (philox.h).  All fp32, every operation
// rounded on its own, HBM-bound, no atomics.  The roundings are kept by writing the operations as plain operators under `#pragma
// clang fp contract(off)`: the header's __fmul_rn / __fadd_rn are inline `x * y` / `x + y` compiled with the header's own
// contraction setting, and a product feeding a sum through them does become one fma.
#include <math.h>

#include "philox.h"
#include "train_batch.h"

namespace {

constexpr uint32_t kStreamDraws = 2, kStreamNoise = 3;      // the Philox stream ids of the header
constexpr unsigned kMaxGrid = 16384;                        // grid-stride launches: 64 workgroups per CU at the most

inline unsigned grid_for(unsigned long long threads) {
  const unsigned long long want = (threads + 255) / 256;
  return (unsigned)(want < kMaxGrid ? (want > 0 ? want : 1) : kMaxGrid);
}

__global__ __launch_bounds__(256) void train_draws_kernel(uint32_t k0, uint32_t k1, uint32_t clip0, uint32_t call, int n,
                                                          const float* __restrict__ sigma_table,
                                                          const float* __restrict__ timestep_table, uint32_t T, int dropout,
                                                          float t1, float t2, float t3, int32_t* __restrict__ indices,
                                                          float* __restrict__ sigmas, float* __restrict__ timesteps,
                                                          float* __restrict__ random_p, float* __restrict__ prompt_keep,
                                                          float* __restrict__ image_mask) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint32_t x[4];
  philox4x32_10(0u, call, kStreamDraws, clip0 + (uint32_t)i, k0, k1, x);
  const uint32_t idx = (uint32_t)(((uint64_t)x[0] * (uint64_t)T) >> 32);      // < T
  const float p = philox_uniform(x[1]);
  if (indices) indices[i] = (int32_t)idx;
  if (sigmas) sigmas[i] = sigma_table[idx];
  if (timesteps) timesteps[i] = timestep_table[idx];
  if (random_p) random_p[i] = p;
  if (prompt_keep) prompt_keep[i] = dropout && p < t2 ? 0.0f : 1.0f;
  if (image_mask) image_mask[i] = dropout && p >= t1 && p < t3 ? 0.0f : 1.0f;
}

struct AssembleParams {
  const float* target;
  const float* noise;
  const float* sigmas;
  const float* mask;
  const float* cond_frames;
  const float* cond_image;
  float* noisy;
  void* sample;
  float* noise_out;
  unsigned long long per_clip, nblk, total;     // elements and Philox blocks per clip; blocks of the batch
  unsigned long long plane;                     // L h w
  int F, K, layout, sample_el, vec;
  uint32_t k0, k1, clip0, call;
};

// One thread per Philox block of a clip -- four consecutive elements e0 .. e0 + 3 of its (F, L, h, w) order -- and iteration,
// grid-stride over (clip, block).  vec (decided on the host: plane % 4 == 0 and every pointer 16-byte aligned): the four share a
// frame and every access is one 16-byte load / store (8 bytes for a 16-bit sample).  Otherwise every element is read, placed
// and written on its own: a block may straddle two frames, and the last block of a clip may be short.  The values are formed by
// the same statements either way.
__global__ __launch_bounds__(256) void train_assemble_kernel(const AssembleParams P) {
#pragma clang fp contract(off)
  for (unsigned long long g = (unsigned long long)blockIdx.x * 256 + threadIdx.x; g < P.total;
       g += (unsigned long long)gridDim.x * 256) {
    const unsigned long long i = g / P.nblk, j = g % P.nblk;
    const unsigned long long e0 = 4 * j;
    const int left = P.per_clip - e0 < 4 ? (int)(P.per_clip - e0) : 4;
    const unsigned long long at = i * P.per_clip + e0;
    const float sigma = P.sigmas[i];
    const float mask = P.mask ? P.mask[i] : 1.0f;
    const float s2 = sigma * sigma;
    const float den = sqrtf(s2 + 1.0f);
    const bool vec = P.vec && left == 4;

    float t[4] = {0.f, 0.f, 0.f, 0.f}, z[4] = {0.f, 0.f, 0.f, 0.f}, c[4] = {0.f, 0.f, 0.f, 0.f};
    unsigned long long so[4];                   // offset of each element's noisy channel in `sample`
    if (vec) {
      const float4 v = *(const float4*)(P.target + at);
      t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
    } else {
      for (int k = 0; k < left; ++k) t[k] = P.target[at + k];
    }
    if (P.noise) {
      if (vec) {
        const float4 v = *(const float4*)(P.noise + at);
        z[0] = v.x; z[1] = v.y; z[2] = v.z; z[3] = v.w;
      } else {
        for (int k = 0; k < left; ++k) z[k] = P.noise[at + k];
      }
    } else {
      philox_normals4((uint32_t)j, P.call, kStreamNoise, P.clip0 + (uint32_t)i, P.k0, P.k1, z);
    }
    if (vec) {
      const unsigned long long f = e0 / P.plane, q = e0 % P.plane;
      const bool frames = P.layout == 1 && ((long long)f < P.K || (long long)f == P.F - 1);
      const float4 v = frames ? *(const float4*)(P.cond_frames + at) : *(const float4*)(P.cond_image + i * P.plane + q);
      c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
      const unsigned long long s0 = (i * P.F + f) * 2 * P.plane + q;
      so[0] = s0; so[1] = s0 + 1; so[2] = s0 + 2; so[3] = s0 + 3;
    } else {
      for (int k = 0; k < left; ++k) {
        const unsigned long long e = e0 + k, f = e / P.plane, q = e % P.plane;
        const bool frames = P.layout == 1 && ((long long)f < P.K || (long long)f == P.F - 1);
        c[k] = frames ? P.cond_frames[at + k] : P.cond_image[i * P.plane + q];
        so[k] = (i * P.F + f) * 2 * P.plane + q;
      }
    }

    float noisy[4], inp[4], cm[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float zs = z[k] * sigma;
      noisy[k] = t[k] + zs;
      inp[k] = noisy[k] / den;
      cm[k] = mask * c[k];
    }

    if (vec) {
      *(float4*)(P.noisy + at) = make_float4(noisy[0], noisy[1], noisy[2], noisy[3]);
      if (P.noise_out) *(float4*)(P.noise_out + at) = make_float4(z[0], z[1], z[2], z[3]);
      if (P.sample_el) {
        el_t* s = (el_t*)P.sample;
        el_t a[4], b[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { a[k] = round_to_el(inp[k]); b[k] = round_to_el(cm[k]); }
        *(uint2*)(s + so[0]) = make_uint2((uint32_t)a[0] | ((uint32_t)a[1] << 16), (uint32_t)a[2] | ((uint32_t)a[3] << 16));
        *(uint2*)(s + so[0] + P.plane) = make_uint2((uint32_t)b[0] | ((uint32_t)b[1] << 16), (uint32_t)b[2] | ((uint32_t)b[3] << 16));
      } else {
        float* s = (float*)P.sample;
        *(float4*)(s + so[0]) = make_float4(inp[0], inp[1], inp[2], inp[3]);
        *(float4*)(s + so[0] + P.plane) = make_float4(cm[0], cm[1], cm[2], cm[3]);
      }
    } else {
      for (int k = 0; k < left; ++k) {
        P.noisy[at + k] = noisy[k];
        if (P.noise_out) P.noise_out[at + k] = z[k];
        if (P.sample_el) {
          el_t* s = (el_t*)P.sample;
          s[so[k]] = round_to_el(inp[k]);
          s[so[k] + P.plane] = round_to_el(cm[k]);
        } else {
          float* s = (float*)P.sample;
          s[so[k]] = inp[k];
          s[so[k] + P.plane] = cm[k];
        }
      }
    }
  }
}

__device__ __forceinline__ float tb_load(const void* p, int dtype, unsigned long long i) {
  if (dtype == 0) return ((const float*)p)[i];
  if (dtype == 1) return (float)((const _Float16*)p)[i];
  return bf16_to_f32(((const bf16_t*)p)[i]);
}

__global__ __launch_bounds__(256) void first_frames_kernel(const void* __restrict__ src, int dtype, unsigned long long total,
                                                           unsigned long long per, unsigned long long F,
                                                           float* __restrict__ dst) {
  for (unsigned long long g = (unsigned long long)blockIdx.x * 256 + threadIdx.x; g < total;
       g += (unsigned long long)gridDim.x * 256) {
    const unsigned long long b = g / per, p = g % per;
    dst[g] = tb_load(src, dtype, b * F * per + p);
  }
}

__global__ __launch_bounds__(256) void keep_rows_kernel(const el_t* __restrict__ emb, const float* __restrict__ keep, long total,
                                                        int D, el_t* __restrict__ out) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  out[g] = round_to_el(keep[g / D] * el_to_f32(emb[g]));
}

__global__ __launch_bounds__(256) void scale_kernel(const float* __restrict__ x, float scale, unsigned long long total,
                                                    float* __restrict__ out) {
  for (unsigned long long g = (unsigned long long)blockIdx.x * 256 + threadIdx.x; g < total;
       g += (unsigned long long)gridDim.x * 256)
    out[g] = x[g] * scale;
}

}  // namespace

extern "C" int ctrlv_train_draws(uint64_t seed, uint32_t clip0, uint32_t call, int n_clips, const float* sigma_table,
                                 const float* timestep_table, int T, double dropout_prob, int32_t* indices, float* sigmas,
                                 float* timesteps, float* random_p, float* prompt_keep, float* image_mask, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(sigma_table != nullptr && timestep_table != nullptr, "train_draws: sigma_table / timestep_table are null (device "
                  "arrays of T floats)");
  CTRLV_CHECK_SHAPE(T >= 1 && T <= 65536, "train_draws: T=%d must be in [1, 65536]", T);
  CTRLV_CHECK_SHAPE(n_clips >= 1 && n_clips <= 65536, "train_draws: n_clips=%d must be in [1, 65536]", n_clips);
  CTRLV_CHECK_ARG(isfinite(dropout_prob), "train_draws: dropout_prob=%g is not finite (negative: no dropout)", dropout_prob);
  CTRLV_CHECK_ARG(indices || sigmas || timesteps || random_p || prompt_keep || image_mask, "train_draws: every output is null");
  const int dropout = dropout_prob >= 0.0 ? 1 : 0;
  // the products in double, rounded once: torch compares an fp32 tensor with the Python scalar cast to fp32
  const float t1 = (float)dropout_prob, t2 = (float)(2.0 * dropout_prob), t3 = (float)(3.0 * dropout_prob);
  hipLaunchKernelGGL(train_draws_kernel, dim3((unsigned)((n_clips + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), clip0, call, n_clips, sigma_table, timestep_table,
                     (uint32_t)T, dropout, t1, t2, t3, indices, sigmas, timesteps, random_p, prompt_keep, image_mask);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

int ctrlv_train_assemble_check(int layout, int K, int n, int F, int L, int h, int w) {
  CTRLV_CHECK_ARG(layout == 0 || layout == 1, "train_assemble: layout=%d must be 0 (the image latent for every frame) or 1 (the box "
                  "predictor's)", layout);
  CTRLV_CHECK_SHAPE(n >= 1 && n <= 65536, "train_assemble: n=%d must be in [1, 65536]", n);
  CTRLV_CHECK_SHAPE(F >= 1 && F <= 32, "train_assemble: F=%d must be in [1, 32]", F);
  CTRLV_CHECK_SHAPE(L >= 1 && L <= 8, "train_assemble: L=%d must be in [1, 8]", L);
  CTRLV_CHECK_SHAPE(h >= 1 && w >= 1 && (long long)h * w <= (1ll << 26), "train_assemble: h=%d, w=%d must be positive, h w <= 2^26",
                    h, w);
  if (layout == 1) CTRLV_CHECK_SHAPE(K >= 0 && K <= F, "train_assemble: K=%d must be in [0, %d] (F)", K, F);
  return CTRLV_OK;
}

extern "C" int ctrlv_train_assemble(const float* target, const float* noise, const float* sigmas, const float* image_mask,
                                    const float* cond_frames, const float* cond_image, int layout, int K, int n, int F, int L,
                                    int h, int w, uint64_t seed, uint32_t clip0, uint32_t call, float* noisy, void* sample,
                                    int sample_dtype, float* noise_out, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(target && sigmas && cond_image && noisy && sample, "train_assemble: null pointer (target, sigmas, cond_image, "
                  "noisy and sample are required)");
  CTRLV_TRY(ctrlv_train_assemble_check(layout, K, n, F, L, h, w));
  CTRLV_CHECK_ARG(layout == 0 || cond_frames != nullptr, "train_assemble: layout 1 needs cond_frames");
  if (sample_dtype != 0 && sample_dtype != CTRLV_ELEM_DTYPE) {
    ctrlv_set_error("train_assemble: sample dtype code %d (0 fp32 or %d, this library's element type)", sample_dtype,
                    CTRLV_ELEM_DTYPE);
    return CTRLV_E_BAD_DTYPE;
  }
  const uintptr_t f32s = (uintptr_t)target | (uintptr_t)noise | (uintptr_t)sigmas | (uintptr_t)image_mask | (uintptr_t)cond_frames |
                         (uintptr_t)cond_image | (uintptr_t)noisy | (uintptr_t)noise_out;
  CTRLV_CHECK_ARG((f32s & 3) == 0 && ((uintptr_t)sample & (sample_dtype == 0 ? 3 : 1)) == 0,
                  "train_assemble: a tensor is not aligned to its element size");
  AssembleParams P;
  memset(&P, 0, sizeof(P));
  P.target = target; P.noise = noise; P.sigmas = sigmas; P.mask = image_mask;
  P.cond_frames = layout == 1 ? cond_frames : nullptr; P.cond_image = cond_image;
  P.noisy = noisy; P.sample = sample; P.noise_out = noise_out;
  P.plane = (unsigned long long)L * h * w;
  P.per_clip = P.plane * F;                                  // <= 32 * 8 * 2^26 = 2^34: the counter's range
  P.nblk = (P.per_clip + 3) / 4;
  P.total = P.nblk * (unsigned long long)n;
  P.F = F; P.K = K; P.layout = layout;
  P.sample_el = sample_dtype != 0 ? 1 : 0;
  // the per-tensor bases only: with plane % 4 == 0 every block's offsets are multiples of four elements
  const uintptr_t wide = (uintptr_t)target | (uintptr_t)noise | (uintptr_t)P.cond_frames | (uintptr_t)cond_image | (uintptr_t)noisy |
                         (uintptr_t)noise_out | (uintptr_t)sample;
  P.vec = P.plane % 4 == 0 && (wide & 15) == 0 ? 1 : 0;
  P.k0 = (uint32_t)(seed & 0xffffffffu); P.k1 = (uint32_t)(seed >> 32); P.clip0 = clip0; P.call = call;
  hipLaunchKernelGGL(train_assemble_kernel, dim3(grid_for(P.total)), dim3(256), 0, (hipStream_t)stream, P);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

int ctrlv_tb_first_frames(const void* src, int dtype, int n, int F, long per, float* dst, hipStream_t s) {
  const unsigned long long total = (unsigned long long)n * (unsigned long long)per;
  hipLaunchKernelGGL(first_frames_kernel, dim3(grid_for(total)), dim3(256), 0, s, src, dtype, total, (unsigned long long)per,
                     (unsigned long long)F, dst);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

int ctrlv_tb_keep_rows(const void* emb, const float* keep, int n, int D, void* out, hipStream_t s) {
  const long total = (long)n * D;
  hipLaunchKernelGGL(keep_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const el_t*)emb, keep, total, D,
                     (el_t*)out);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

int ctrlv_tb_scale(const float* x, float scale, long count, float* out, hipStream_t s) {
  hipLaunchKernelGGL(scale_kernel, dim3(grid_for((unsigned long long)count)), dim3(256), 0, s, x, scale,
                     (unsigned long long)count, out);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}
