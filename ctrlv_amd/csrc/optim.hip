// Optimiser pass of the training steps (gfx950): AdamW over one flat fp32 buffer with the EMA shadow update fused in, and
// the EMA update alone.  One pass, 16-byte loads and stores per lane, a scalar tail for n % 4; no pointer tables, no atomics,
// no barrier.  HBM-bound: 28 bytes per element (p, m, v read and written, g read), 36 with the shadow.  All arithmetic is
// fp32 and does not depend on the library's element type.
//
// Global gradient-norm clipping in front of it: one more read of g (4 bytes per element) sums its squares in fp64 into one
// partial per 4096 elements (a partition that depends on n alone), one workgroup turns the partials into a device record
// (norm, clip coefficient, skip flag), and a variant of the AdamW kernel reads coefficient and flag from that record.  No
// atomics, no host read, no second pass over the gradients.
//
// Every fused multiply-add is EXPLICIT and the unit is compiled with contraction off (EXTRA_FLAGS of the build): the fused
// kernel and the two-launch form (AdamW, then ctrlv_ema_step) must give the same bits, so the rounding of each operation may
// not depend on which kernel inlines it.
#include <math.h>

#include "common.h"

namespace {

struct adamw_consts {
  float decay_mul;     // 1 - lr * weight_decay
  float w1, omw1;      // 1 - beta1 (the lerp weight) and 1 - w1 in fp32
  int w1_small;        // |w1| < 0.5: which of lerp's two forms applies
  float beta2, omb2;   // beta2, 1 - beta2
  float neg_step;      // -lr / bias1
  float inv_bias2_sqrt;  // 1 / sqrt(bias2), the reciprocal taken in fp32
  float eps;
  float grad_scale;
  float ema_omd;       // 1 - ema_decay
};

// torch.optim.AdamW (amsgrad=False, maximize=False):
//   p *= 1 - lr*wd;  m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g*g;  p -= (lr/bias1) * m / (sqrt(v)/sqrt(bias2) + eps)
// evaluated in the rounding order of torch's own single-tensor path on the device (optim/adam.py _single_tensor_adam and the
// ATen kernels behind it), so that a run continued from a torch checkpoint follows torch's trajectory as closely as fp32 allows:
//   mul_(1 - lr*wd);  lerp_(g, 1 - b1): m + w (g - m) as one fma for w < 0.5, g - (g - m)(1 - w) otherwise;
//   mul_(b2) then addcmul_: fma(1 - b2, g*g, b2*v);  sqrt, times the fp32 reciprocal of sqrt(bias2), plus eps;
//   addcdiv_: fma(-lr/bias1, m / denom, p).
// sqrtf and '/' are the correctly rounded ones (hipcc's default for fp32).
__device__ __forceinline__ void adamw_core(float& p, float g, float& m, float& v, const adamw_consts& c) {
  const float pd = p * c.decay_mul;
  const float d = g - m;
  m = c.w1_small ? __builtin_fmaf(c.w1, d, m) : __builtin_fmaf(-d, c.omw1, g);
  v = __builtin_fmaf(c.omb2, g * g, v * c.beta2);
  const float denom = sqrtf(v) * c.inv_bias2_sqrt + c.eps;
  p = __builtin_fmaf(c.neg_step, m / denom, pd);
}
__device__ __forceinline__ void adamw_one(float& p, float g, float& m, float& v, const adamw_consts& c) {
  adamw_core(p, g * c.grad_scale, m, v, c);
}
// ... behind a clip: (g * grad_scale) * coef, two roundings in that order (an unscale, then torch's mul_(clip_coef))
__device__ __forceinline__ void adamw_one_clipped(float& p, float g, float& m, float& v, const adamw_consts& c, float coef) {
  adamw_core(p, (g * c.grad_scale) * coef, m, v, c);
}

// diffusers' EMAModel.step: ema -= (1 - decay) * (ema - p)
__device__ __forceinline__ float ema_one(float e, float p, float omd) { return __builtin_fmaf(-omd, e - p, e); }

constexpr int kThreads = 256, kVecPerThread = 4;            // one workgroup: 256 lanes x 4 vectors x 4 floats = 4096 elements
constexpr size_t kBlockElems = (size_t)kThreads * kVecPerThread * 4;

template <bool EMA>
__global__ __launch_bounds__(kThreads) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, float* __restrict__ ema, size_t n, adamw_consts c) {
  const size_t nvec = n / 4;
  const size_t v0 = (size_t)blockIdx.x * (kThreads * kVecPerThread) + threadIdx.x;
  f32x4 pp[kVecPerThread], gg[kVecPerThread], mm[kVecPerThread], vv[kVecPerThread], ee[kVecPerThread];
#pragma unroll
  for (int j = 0; j < kVecPerThread; ++j) {                 // all loads of the thread in flight before the first use
    const size_t i = v0 + (size_t)j * kThreads;
    if (i < nvec) {
      pp[j] = ((const f32x4*)p)[i];
      gg[j] = ((const f32x4*)g)[i];
      mm[j] = ((const f32x4*)m)[i];
      vv[j] = ((const f32x4*)v)[i];
      if (EMA) ee[j] = ((const f32x4*)ema)[i];
    }
  }
#pragma unroll
  for (int j = 0; j < kVecPerThread; ++j) {
    const size_t i = v0 + (size_t)j * kThreads;
    if (i < nvec) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float pk = pp[j][k], mk = mm[j][k], vk = vv[j][k];
        adamw_one(pk, gg[j][k], mk, vk, c);
        pp[j][k] = pk, mm[j][k] = mk, vv[j][k] = vk;
        if (EMA) ee[j][k] = ema_one(ee[j][k], pk, c.ema_omd);
      }
      ((f32x4*)p)[i] = pp[j];
      ((f32x4*)m)[i] = mm[j];
      ((f32x4*)v)[i] = vv[j];
      if (EMA) ((f32x4*)ema)[i] = ee[j];
    }
  }
  // scalar tail: elements [4 * nvec, n), at most three, by the first lanes of the first workgroup
  const size_t t = nvec * 4 + threadIdx.x;
  if (blockIdx.x == 0 && t < n) {
    float pk = p[t], mk = m[t], vk = v[t];
    adamw_one(pk, g[t], mk, vk, c);
    p[t] = pk, m[t] = mk, v[t] = vk;
    if (EMA) ema[t] = ema_one(ema[t], pk, c.ema_omd);
  }
}

// the EMA update of one workgroup's 4096 elements (ema_kernel; the skipped step of adamw_dev_kernel)
__device__ __forceinline__ void ema_block(float* __restrict__ ema, const float* __restrict__ p, size_t n, float omd) {
  const size_t nvec = n / 4;
  const size_t v0 = (size_t)blockIdx.x * (kThreads * kVecPerThread) + threadIdx.x;
  f32x4 pp[kVecPerThread], ee[kVecPerThread];
#pragma unroll
  for (int j = 0; j < kVecPerThread; ++j) {
    const size_t i = v0 + (size_t)j * kThreads;
    if (i < nvec) {
      pp[j] = ((const f32x4*)p)[i];
      ee[j] = ((const f32x4*)ema)[i];
    }
  }
#pragma unroll
  for (int j = 0; j < kVecPerThread; ++j) {
    const size_t i = v0 + (size_t)j * kThreads;
    if (i < nvec) {
#pragma unroll
      for (int k = 0; k < 4; ++k) ee[j][k] = ema_one(ee[j][k], pp[j][k], omd);
      ((f32x4*)ema)[i] = ee[j];
    }
  }
  const size_t t = nvec * 4 + threadIdx.x;
  if (blockIdx.x == 0 && t < n) ema[t] = ema_one(ema[t], p[t], omd);
}

__global__ __launch_bounds__(kThreads) void ema_kernel(float* __restrict__ ema, const float* __restrict__ p, size_t n, float omd) {
  ema_block(ema, p, n, omd);
}

// ctrlv_adamw_step_dev: adamw_kernel with the clip coefficient and the skip flag read from the device record (one uniform load:
// the record was written by an earlier launch and nobody writes it during this one).  A skipped step leaves p, m and v alone and
// reads neither g, m nor v; the shadow still moves towards the unchanged p, as ema_kernel would move it.
template <bool EMA>
__device__ __forceinline__ void adamw_dev_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                               float* __restrict__ v, float* __restrict__ ema, size_t n, const adamw_consts& c,
                                               float coef, int skip) {
  if (skip) {
    if (EMA) ema_block(ema, p, n, c.ema_omd);
    return;
  }
  const size_t nvec = n / 4;
  const size_t v0 = (size_t)blockIdx.x * (kThreads * kVecPerThread) + threadIdx.x;
  f32x4 pp[kVecPerThread], gg[kVecPerThread], mm[kVecPerThread], vv[kVecPerThread], ee[kVecPerThread];
#pragma unroll
  for (int j = 0; j < kVecPerThread; ++j) {                 // all loads of the thread in flight before the first use
    const size_t i = v0 + (size_t)j * kThreads;
    if (i < nvec) {
      pp[j] = ((const f32x4*)p)[i];
      gg[j] = ((const f32x4*)g)[i];
      mm[j] = ((const f32x4*)m)[i];
      vv[j] = ((const f32x4*)v)[i];
      if (EMA) ee[j] = ((const f32x4*)ema)[i];
    }
  }
#pragma unroll
  for (int j = 0; j < kVecPerThread; ++j) {
    const size_t i = v0 + (size_t)j * kThreads;
    if (i < nvec) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float pk = pp[j][k], mk = mm[j][k], vk = vv[j][k];
        adamw_one_clipped(pk, gg[j][k], mk, vk, c, coef);
        pp[j][k] = pk, mm[j][k] = mk, vv[j][k] = vk;
        if (EMA) ee[j][k] = ema_one(ee[j][k], pk, c.ema_omd);
      }
      ((f32x4*)p)[i] = pp[j];
      ((f32x4*)m)[i] = mm[j];
      ((f32x4*)v)[i] = vv[j];
      if (EMA) ((f32x4*)ema)[i] = ee[j];
    }
  }
  const size_t t = nvec * 4 + threadIdx.x;                  // scalar tail, as in adamw_kernel
  if (blockIdx.x == 0 && t < n) {
    float pk = p[t], mk = m[t], vk = v[t];
    adamw_one_clipped(pk, g[t], mk, vk, c, coef);
    p[t] = pk, m[t] = mk, v[t] = vk;
    if (EMA) ema[t] = ema_one(ema[t], pk, c.ema_omd);
  }
}

template <bool EMA>
__global__ __launch_bounds__(kThreads) void adamw_dev_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                             float* __restrict__ v, float* __restrict__ ema, size_t n, adamw_consts c,
                                                             const ctrlv_grad_state* __restrict__ state) {
  adamw_dev_body<EMA>(p, g, m, v, ema, n, c, state->coef, state->skip);
}

// ctrlv_adamw_step_scaled: the same with the unscale multiplier read from the loss-scale record (written by grad_finish_scaled_kernel in
// an earlier launch) in the place of the host's grad_scale: (g * ls->unscale) * state->coef.  g is only read.
template <bool EMA>
__global__ __launch_bounds__(kThreads) void adamw_scaled_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                float* __restrict__ v, float* __restrict__ ema, size_t n, adamw_consts c,
                                                                const ctrlv_loss_scale_state* __restrict__ ls,
                                                                const ctrlv_grad_state* __restrict__ state) {
  c.grad_scale = ls->unscale;
  adamw_dev_body<EMA>(p, g, m, v, ema, n, c, state->coef, state->skip);
}

// ---- global gradient norm: stage 1, one fp64 partial per block of kBlockElems elements
// Sum over a workgroup in a fixed order: down the 64 lanes of each wave (a fixed tree of shuffles), then the waves in index order
// by lane 0.  The result is valid in thread 0 only.
template <int THREADS>
__device__ __forceinline__ double block_sum_f64(double s) {
  __shared__ double wave_sums[THREADS / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = s;
  __syncthreads();
  double total = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) total += wave_sums[w];
  }
  return total;
}

// Block b of the grid sums the squares of elements [b * kBlockElems, min(n, (b + 1) * kBlockElems)) into partials[b]; the n % 4
// tail (always inside the last block) goes through scalar loads of the last workgroup's first lanes.  (double)g * (double)g is
// exact (24 x 24 bits); lanes past the end add +0.  g is only read.
__global__ __launch_bounds__(kThreads) void grad_sumsq_kernel(const float* __restrict__ g, size_t n, double* __restrict__ partials) {
  const size_t nvec = n / 4;
  const size_t v0 = (size_t)blockIdx.x * (kThreads * kVecPerThread) + threadIdx.x;
  f32x4 gg[kVecPerThread];
#pragma unroll
  for (int j = 0; j < kVecPerThread; ++j) {                 // all loads of the thread in flight before the first use
    const size_t i = v0 + (size_t)j * kThreads;
    gg[j] = i < nvec ? ((const f32x4*)g)[i] : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < kVecPerThread; ++j)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double x = (double)gg[j][k];
      s += x * x;
    }
  const size_t t = nvec * 4 + threadIdx.x;
  if (blockIdx.x == gridDim.x - 1 && t < n) {
    const double x = (double)g[t];
    s += x * x;
  }
  s = block_sum_f64<kThreads>(s);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// ---- stage 2, ONE workgroup: S, then the record.  Lane l adds slots l, l + 1024, ... in index order.
constexpr int kFinishThreads = 1024;
// the record from S and the multiplier of the gradients (thread 0 only); returns the skip flag
__device__ __forceinline__ int finish_record(double s, float grad_scale, float max_norm, int force_skip,
                                             ctrlv_grad_state* __restrict__ state) {
  const float norm = (float)(fabs((double)grad_scale) * sqrt(s));          // rounded once
  float coef = 1.0f;
  if (max_norm < INFINITY) {
    coef = max_norm / (norm + 1e-6f);                                       // torch: max_norm / (total_norm + 1e-6) ...
    coef = coef > 1.0f ? 1.0f : coef;                                       // ... clamp(max=1.0): a NaN stays a NaN
  }
  const int skip = (isfinite(norm) && !force_skip) ? 0 : 1;
  state->norm = norm;
  state->coef = coef;
  state->skip = skip;
  state->skipped_total = state->skipped_total + skip;
  return skip;
}

__global__ __launch_bounds__(kFinishThreads) void grad_finish_kernel(const double* __restrict__ partials, size_t count, float grad_scale,
                                                                     float max_norm, ctrlv_grad_state* __restrict__ state) {
  double s = 0.0;
#pragma unroll 8
  for (size_t i = threadIdx.x; i < count; i += kFinishThreads) s += partials[i];
  s = block_sum_f64<kFinishThreads>(s);
  if (threadIdx.x == 0) finish_record(s, grad_scale, max_norm, 0, state);
}

// ctrlv_grad_finish_scaled: the same sum in the same order; the multiplier is formed from the loss-scale record, and the thread that
// wrote the grad record then updates the scale as torch's _amp_update_scale_ does (amp_update_scale_cuda_kernel: the products
// are taken in double there, from factors that are doubles; a product of two fp32 numbers rounded once is the fp32 product).
__global__ __launch_bounds__(kFinishThreads) void grad_finish_scaled_kernel(const double* __restrict__ partials, size_t count,
                                                                            float grad_scale, float max_norm,
                                                                            ctrlv_loss_scale_state* __restrict__ ls,
                                                                            ctrlv_grad_state* __restrict__ state) {
  double s = 0.0;
#pragma unroll 8
  for (size_t i = threadIdx.x; i < count; i += kFinishThreads) s += partials[i];
  s = block_sum_f64<kFinishThreads>(s);
  if (threadIdx.x == 0) {
    const float scale = ls->scale;
    const bool valid = scale > 0.f && isfinite(scale);                      // false for NaN
    // torch: _scale.double().reciprocal().float(), then the host's multiplier in fp32.  An unusable scale: NaN, and a skip
    const float unscale = valid ? grad_scale * (float)(1.0 / (double)scale) : NAN;
    ls->unscale = unscale;
    const int skip = finish_record(s, unscale, max_norm, valid ? 0 : 1, state);
    if (valid) {
      if (skip) {
        ls->scale = scale * ls->backoff_factor;
        ls->growth_tracker = 0;
      } else {
        const int32_t successful = ls->growth_tracker + 1;
        if (successful == ls->growth_interval) {
          const float grown = scale * ls->growth_factor;
          if (isfinite(grown)) ls->scale = grown;
          ls->growth_tracker = 0;
        } else {
          ls->growth_tracker = successful;
        }
      }
    }
  }
}

inline bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }
inline bool unit_open(float x) { return x >= 0.f && x < 1.f; }          // [0, 1); false for NaN

// bias = 1 - beta^t reaches the entry point rounded to fp32.  The step count t it encodes is recovered and the correction is
// recomputed in double, so that lr / bias1 and sqrt(bias2) are rounded ONCE, as where the host derives them from (beta, t) in
// double.  A value that is not of this form (or beta = 0, where every t gives 1) is taken as given.
inline double exact_bias(float beta, float bias) {
  if (!(beta > 0.f) || !(bias < 1.f)) return (double)bias;
  const double t = round(log1p(-(double)bias) / log((double)beta));
  if (!(t >= 1.0 && t <= 1e9)) return (double)bias;
  const double b = 1.0 - pow((double)beta, t);
  return fabs(b - (double)bias) <= 1e-6 * b ? b : (double)bias;
}

// workgroups of kBlockElems elements that cover n; the launches below pass at most 2^30 elements each
inline unsigned blocks_for(size_t n) { return (unsigned)((n + kBlockElems - 1) / kBlockElems); }
constexpr size_t kMaxLaunchElems = (size_t)1 << 30;                      // a multiple of kBlockElems: chunk bases stay aligned

// refusals and kernel constants of ctrlv_adamw_step and ctrlv_adamw_step_dev
int adamw_host(const float* p, const float* g, const float* m, const float* v, const float* ema, size_t n, float lr, float beta1,
               float beta2, float eps, float weight_decay, float bias1, float bias2, float grad_scale, float ema_decay,
               adamw_consts& c) {
  CTRLV_CHECK_ARG(p && g && m && v, "adamw_step: p, g, m and v must be non-null");
  CTRLV_CHECK_SHAPE(n > 0, "adamw_step: n must be positive");
  CTRLV_CHECK_ARG(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && aligned16(ema),
                  "adamw_step: every buffer must be 16-byte aligned");
  CTRLV_CHECK_ARG(isfinite(lr), "adamw_step: lr must be finite");
  CTRLV_CHECK_ARG(unit_open(beta1) && unit_open(beta2), "adamw_step: beta1 and beta2 must lie in [0, 1)");
  CTRLV_CHECK_ARG(eps > 0.f && isfinite(eps), "adamw_step: eps must be positive");
  CTRLV_CHECK_ARG(isfinite(weight_decay), "adamw_step: weight_decay must be finite");
  CTRLV_CHECK_ARG(bias1 > 0.f && bias1 <= 1.f && bias2 > 0.f && bias2 <= 1.f,
                  "adamw_step: bias1 and bias2 (1 - beta^t) must lie in (0, 1]");
  CTRLV_CHECK_ARG(isfinite(grad_scale), "adamw_step: grad_scale must be finite");
  CTRLV_CHECK_ARG(ema == nullptr || (ema_decay >= 0.f && ema_decay <= 1.f), "adamw_step: ema decay must lie in [0, 1]");
  c.decay_mul = (float)(1.0 - (double)lr * (double)weight_decay);
  c.w1 = (float)(1.0 - (double)beta1);
  c.omw1 = 1.0f - c.w1;
  c.w1_small = fabsf(c.w1) < 0.5f;
  c.beta2 = beta2, c.omb2 = (float)(1.0 - (double)beta2);
  c.neg_step = (float)(-(double)lr / exact_bias(beta1, bias1));
  c.inv_bias2_sqrt = 1.0f / (float)sqrt(exact_bias(beta2, bias2));
  c.eps = eps;
  c.grad_scale = grad_scale;
  c.ema_omd = ema ? (float)(1.0 - (double)ema_decay) : 0.f;
  return CTRLV_OK;
}

}  // namespace

extern "C" int ctrlv_adamw_step(float* p, const float* g, float* m, float* v, float* ema, size_t n, float lr, float beta1,
                                float beta2, float eps, float weight_decay, float bias1, float bias2, float grad_scale,
                                float ema_decay, ctrlv_stream_t stream) {
  adamw_consts c;
  CTRLV_TRY(adamw_host(p, g, m, v, ema, n, lr, beta1, beta2, eps, weight_decay, bias1, bias2, grad_scale, ema_decay, c));
  for (size_t off = 0; off < n; off += kMaxLaunchElems) {
    const size_t cnt = n - off < kMaxLaunchElems ? n - off : kMaxLaunchElems;
    if (ema)
      hipLaunchKernelGGL(adamw_kernel<true>, dim3(blocks_for(cnt)), dim3(kThreads), 0, (hipStream_t)stream, p + off, g + off,
                         m + off, v + off, ema + off, cnt, c);
    else
      hipLaunchKernelGGL(adamw_kernel<false>, dim3(blocks_for(cnt)), dim3(kThreads), 0, (hipStream_t)stream, p + off, g + off,
                         m + off, v + off, (float*)nullptr, cnt, c);
    CTRLV_LAUNCH_CHECK();
  }
  return CTRLV_OK;
}

extern "C" int ctrlv_ema_step(float* ema, const float* p, size_t n, float decay, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(ema && p, "ema_step: ema and p must be non-null");
  CTRLV_CHECK_SHAPE(n > 0, "ema_step: n must be positive");
  CTRLV_CHECK_ARG(aligned16(ema) && aligned16(p), "ema_step: every buffer must be 16-byte aligned");
  CTRLV_CHECK_ARG(decay >= 0.f && decay <= 1.f, "ema_step: decay must lie in [0, 1]");
  const float omd = (float)(1.0 - (double)decay);
  for (size_t off = 0; off < n; off += kMaxLaunchElems) {
    const size_t cnt = n - off < kMaxLaunchElems ? n - off : kMaxLaunchElems;
    hipLaunchKernelGGL(ema_kernel, dim3(blocks_for(cnt)), dim3(kThreads), 0, (hipStream_t)stream, ema + off, p + off, cnt, omd);
    CTRLV_LAUNCH_CHECK();
  }
  return CTRLV_OK;
}

// ---- global gradient-norm clipping in front of the AdamW pass: sum of squares, finish, the step that reads the record
extern "C" size_t ctrlv_grad_sumsq_partials(size_t n) { return n / kBlockElems + (n % kBlockElems != 0); }

extern "C" int ctrlv_grad_sumsq(const float* g, size_t n, double* partials, size_t partials_len, size_t slot0,
                                ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(g && partials, "grad_sumsq: g and partials must be non-null");
  CTRLV_CHECK_SHAPE(n > 0, "grad_sumsq: n must be positive");
  CTRLV_CHECK_ARG(aligned16(g), "grad_sumsq: g must be 16-byte aligned");
  CTRLV_CHECK_ARG(((uintptr_t)partials & 7) == 0, "grad_sumsq: partials must be 8-byte aligned");
  const size_t slots = ctrlv_grad_sumsq_partials(n);
  CTRLV_CHECK_ARG(slot0 <= partials_len && slots <= partials_len - slot0,
                  "grad_sumsq: %zu slots from slot %zu on lie beyond the %zu partials of the array", slots, slot0, partials_len);
  for (size_t off = 0; off < n; off += kMaxLaunchElems) {           // (kMaxLaunchElems is a whole number of blocks)
    const size_t cnt = n - off < kMaxLaunchElems ? n - off : kMaxLaunchElems;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(blocks_for(cnt)), dim3(kThreads), 0, (hipStream_t)stream, g + off, cnt,
                       partials + slot0 + off / kBlockElems);
    CTRLV_LAUNCH_CHECK();
  }
  return CTRLV_OK;
}

extern "C" int ctrlv_grad_finish(const double* partials, size_t count, float grad_scale, float max_norm, ctrlv_grad_state* state,
                                 ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(partials && state, "grad_finish: partials and state must be non-null");
  CTRLV_CHECK_SHAPE(count > 0, "grad_finish: count must be positive");
  CTRLV_CHECK_ARG(((uintptr_t)partials & 7) == 0, "grad_finish: partials must be 8-byte aligned");
  CTRLV_CHECK_ARG(aligned16(state), "grad_finish: state must be 16-byte aligned");
  CTRLV_CHECK_ARG(isfinite(grad_scale), "grad_finish: grad_scale must be finite");
  CTRLV_CHECK_ARG(max_norm > 0.f, "grad_finish: max_norm must be positive (+inf: the norm without clipping)");   // false for NaN
  hipLaunchKernelGGL(grad_finish_kernel, dim3(1), dim3(kFinishThreads), 0, (hipStream_t)stream, partials, count, grad_scale,
                     max_norm, state);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

extern "C" int ctrlv_adamw_step_dev(float* p, const float* g, float* m, float* v, float* ema, size_t n, float lr, float beta1,
                                    float beta2, float eps, float weight_decay, float bias1, float bias2, float grad_scale,
                                    float ema_decay, const ctrlv_grad_state* state, ctrlv_stream_t stream) {
  adamw_consts c;
  CTRLV_TRY(adamw_host(p, g, m, v, ema, n, lr, beta1, beta2, eps, weight_decay, bias1, bias2, grad_scale, ema_decay, c));
  CTRLV_CHECK_ARG(state && aligned16(state), "adamw_step_dev: state must be non-null and 16-byte aligned");
  for (size_t off = 0; off < n; off += kMaxLaunchElems) {
    const size_t cnt = n - off < kMaxLaunchElems ? n - off : kMaxLaunchElems;
    if (ema)
      hipLaunchKernelGGL(adamw_dev_kernel<true>, dim3(blocks_for(cnt)), dim3(kThreads), 0, (hipStream_t)stream, p + off, g + off,
                         m + off, v + off, ema + off, cnt, c, state);
    else
      hipLaunchKernelGGL(adamw_dev_kernel<false>, dim3(blocks_for(cnt)), dim3(kThreads), 0, (hipStream_t)stream, p + off, g + off,
                         m + off, v + off, (float*)nullptr, cnt, c, state);
    CTRLV_LAUNCH_CHECK();
  }
  return CTRLV_OK;
}

// ---- dynamic loss scaling on the device: the finish that unscales by the record's scale and updates it, the step that reads both records
extern "C" int ctrlv_grad_finish_scaled(const double* partials, size_t count, float grad_scale, float max_norm,
                                        ctrlv_loss_scale_state* ls, ctrlv_grad_state* state, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(partials && state, "grad_finish_scaled: partials and state must be non-null");
  CTRLV_CHECK_SHAPE(count > 0, "grad_finish_scaled: count must be positive");
  CTRLV_CHECK_ARG(((uintptr_t)partials & 7) == 0, "grad_finish_scaled: partials must be 8-byte aligned");
  CTRLV_CHECK_ARG(aligned16(state), "grad_finish_scaled: state must be 16-byte aligned");
  CTRLV_CHECK_ARG(ls && aligned16(ls), "grad_finish_scaled: ls (the loss-scale record) must be non-null and 16-byte aligned");
  CTRLV_CHECK_ARG(isfinite(grad_scale), "grad_finish_scaled: grad_scale must be finite");
  CTRLV_CHECK_ARG(max_norm > 0.f, "grad_finish_scaled: max_norm must be positive (+inf: the norm without clipping)");
  hipLaunchKernelGGL(grad_finish_scaled_kernel, dim3(1), dim3(kFinishThreads), 0, (hipStream_t)stream, partials, count, grad_scale,
                     max_norm, ls, state);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

extern "C" int ctrlv_adamw_step_scaled(float* p, const float* g, float* m, float* v, float* ema, size_t n, float lr, float beta1,
                                       float beta2, float eps, float weight_decay, float bias1, float bias2, float ema_decay,
                                       const ctrlv_loss_scale_state* ls, const ctrlv_grad_state* state, ctrlv_stream_t stream) {
  adamw_consts c;
  CTRLV_TRY(adamw_host(p, g, m, v, ema, n, lr, beta1, beta2, eps, weight_decay, bias1, bias2, 1.0f, ema_decay, c));
  CTRLV_CHECK_ARG(ls && aligned16(ls), "adamw_step_scaled: ls (the loss-scale record) must be non-null and 16-byte aligned");
  CTRLV_CHECK_ARG(state && aligned16(state), "adamw_step_scaled: state must be non-null and 16-byte aligned");
  for (size_t off = 0; off < n; off += kMaxLaunchElems) {
    const size_t cnt = n - off < kMaxLaunchElems ? n - off : kMaxLaunchElems;
    if (ema)
      hipLaunchKernelGGL(adamw_scaled_kernel<true>, dim3(blocks_for(cnt)), dim3(kThreads), 0, (hipStream_t)stream, p + off, g + off,
                         m + off, v + off, ema + off, cnt, c, ls, state);
    else
      hipLaunchKernelGGL(adamw_scaled_kernel<false>, dim3(blocks_for(cnt)), dim3(kThreads), 0, (hipStream_t)stream, p + off, g + off,
                         m + off, v + off, (float*)nullptr, cnt, c, ls, state);
    CTRLV_LAUNCH_CHECK();
  }
  return CTRLV_OK;
}
