// Row quantisation to OCP e4m3 ("e4m3fn": largest finite value 448, no infinities) for the FP8 feed-forward GEMMs
// (gemm_f8.hip):
//
//   y[m, :] = x[m, :]                                              (gamma == NULL)
//   y[m, :] = LayerNorm(x[m, :] + V[(m / vdiv) % vmod, :])         (gamma != NULL: ctrlv_layernorm's arithmetic, in fp32)
//   a = max |y[m, :]|,  s[m] = a / 448  (a == 0: s[m] = 1),  q[m, k] = e4m3(y[m, k] / s[m])
//
// One wave per row, the row in registers between the passes (mean, centred squares, maximum, conversion) -- one read of the
// 16-bit row and one write of its bytes: the kernel is bound by HBM like the LayerNorm it replaces (norm.hip ln_kernel, whose
// launch geometry this is).  The normalised value is never rounded to 16 bits.  Conversion: v_cvt_pk_fp8_f32 (round to
// nearest even) of a value clamped to [-448, 448], so neither NaN code (0x7f, 0xff) is ever written for finite input.
// A scale below the smallest normal fp32 (a row whose maximum is < 5.3e-36) is raised to it: y / s stays finite.
#include "common.h"

namespace {

constexpr float kF8Max = 448.0f;
constexpr float kF8MinScale = 1.17549435e-38f;

template <int NV, bool LN>
__global__ __launch_bounds__(256) void quant_rows_f8_kernel(const el_t* __restrict__ x, int M, int K, long ldx,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            float eps, const float* __restrict__ V, int vdiv, int vmod, int ldv,
                                                            uint8_t* __restrict__ q, long ldq, float* __restrict__ scale) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int KV = K >> 3;
  const float inv_k = 1.0f / (float)K;
  const long step = (long)gridDim.x * 4;
  for (long m = (long)blockIdx.x * 4 + wid; m < M; m += step) {
    float f[NV][8];
    uint4 raw[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int cv = lane + k * 64;
      raw[k] = cv < KV ? *(const uint4*)(x + m * ldx + cv * 8) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) unpack_elx8(raw[k], f[k]);     // (lanes past the row hold zeros: neutral for every pass)
    if (LN) {
      const float* vrow = V ? V + (long)((m / vdiv) % vmod) * ldv : nullptr;
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int cv = lane + k * 64;
        if (cv < KV) {
          if (vrow) {
#pragma unroll
            for (int e = 0; e < 8; ++e) f[k][e] += vrow[cv * 8 + e];
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) s += f[k][e];
        }
      }
      const float mean = wave_sum(s) * inv_k;
      float sq = 0.f;
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int cv = lane + k * 64;
        if (cv < KV) {
#pragma unroll
          for (int e = 0; e < 8; ++e) { const float dlt = f[k][e] - mean; sq += dlt * dlt; }
        }
      }
      const float rstd = rsqrtf(wave_sum(sq) * inv_k + eps);
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int cv = lane + k * 64;
        if (cv < KV) {
#pragma unroll
          for (int e = 0; e < 8; ++e) f[k][e] = (f[k][e] - mean) * rstd * gamma[cv * 8 + e] + beta[cv * 8 + e];
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) f[k][e] = 0.f;
        }
      }
    }
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) a = fmaxf(a, fabsf(f[k][e]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a = fmaxf(a, __shfl_xor(a, o));
    float s = 1.0f;
    if (a > 0.f) s = fmaxf(a / kF8Max, kF8MinScale);
    if (lane == 0) scale[m] = s;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int cv = lane + k * 64;
      if (cv < KV) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = __builtin_amdgcn_fmed3f(f[k][e] / s, -kF8Max, kF8Max);
        int w0 = 0, w1 = 0;
        w0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], w0, false);
        w0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], w0, true);
        w1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[4], v[5], w1, false);
        w1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[6], v[7], w1, true);
        *(uint2*)(q + m * ldq + cv * 8) = make_uint2((unsigned)w0, (unsigned)w1);
      }
    }
  }
}

template <int NV>
void quant_launch(bool ln, long blocks, hipStream_t st, const el_t* x, int M, int K, long ldx, const float* gamma,
                  const float* beta, float eps, const float* V, int vdiv, int vmod, int ldv, uint8_t* q, long ldq, float* scale) {
  if (ln)
    hipLaunchKernelGGL((quant_rows_f8_kernel<NV, true>), dim3((unsigned)blocks), dim3(256), 0, st, x, M, K, ldx, gamma, beta, eps,
                       V, vdiv, vmod, ldv, q, ldq, scale);
  else
    hipLaunchKernelGGL((quant_rows_f8_kernel<NV, false>), dim3((unsigned)blocks), dim3(256), 0, st, x, M, K, ldx, gamma, beta, eps,
                       V, vdiv, vmod, ldv, q, ldq, scale);
}

}  // namespace

extern "C" int ctrlv_quant_rows_f8(const void* x, int M, int K, int ldx, const float* gamma, const float* beta, float eps,
                                   const float* V, int vdiv, int vmod, int ldv, void* q, int ldq, float* scale,
                                   ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(x && q && scale, "quant_rows_f8: null pointer");
  CTRLV_CHECK_ARG((gamma == nullptr) == (beta == nullptr), "quant_rows_f8: gamma and beta come together");
  CTRLV_CHECK_ARG(gamma != nullptr || V == nullptr, "quant_rows_f8: the row-vector add belongs to the LayerNorm form (gamma != NULL)");
  CTRLV_CHECK_SHAPE(M > 0 && K > 0 && K % 8 == 0 && K <= 5120, "quant_rows_f8: K=%d must be a multiple of 8, <= 5120 (M=%d)", K, M);
  CTRLV_CHECK_SHAPE(ldx >= K && ldx % 8 == 0 && ldq >= K && ldq % 8 == 0,
                    "quant_rows_f8: ldx=%d / ldq=%d must be multiples of 8 and >= K=%d", ldx, ldq, K);
  CTRLV_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)q & 7) == 0, "quant_rows_f8: x must be 16-byte, q 8-byte aligned");
  if (V) CTRLV_CHECK_ARG(vdiv > 0 && vmod > 0 && ldv >= K, "quant_rows_f8: bad row-vector table");
  const int nv = (K / 8 + 63) / 64;
  long blocks = ((long)M + 3) / 4;
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipStream_t st = (hipStream_t)stream;
  const bool ln = gamma != nullptr;
#define QL(NV) quant_launch<NV>(ln, blocks, st, (const el_t*)x, M, K, ldx, gamma, beta, eps, V, vdiv, vmod, ldv, (uint8_t*)q, ldq, scale)
  if (nv <= 1) QL(1);
  else if (nv <= 2) QL(2);
  else if (nv <= 3) QL(3);
  else if (nv <= 4) QL(4);
  else if (nv <= 5) QL(5);
  else if (nv <= 8) QL(8);
  else QL(10);
#undef QL
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}
