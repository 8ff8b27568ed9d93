// The counter-based generator of ctrlv_randn (include/ctrlv_hip.h states the arithmetic) as device functions: shared by
// csrc/pipeline_io.hip (ctrlv_randn) and csrc/train_batch.hip (the per-clip draws, the in-kernel noise of ctrlv_train_assemble),
// which must give the same bits.  Device code only, header only.
#pragma once
#include <math.h>

#include "common.h"

// fp32 -> element as its OWN rounding: the empty asm keeps the compiler from folding the fp32 operation in front of it into a
// mixed-precision instruction (v_fma_mixlo_f16 rounds the exact product once; torch rounds to fp32 first, then to fp16)
__device__ __forceinline__ el_t round_to_el(float v) {
  asm volatile("" : "+v"(v));
  return f32_to_el(v);
}

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t* x) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {           // the key is bumped between rounds (the bump behind the last one is dead)
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  x[0] = c0; x[1] = c1; x[2] = c2; x[3] = c3;
}

// (x + 0.5) / 2^32 rounded ONCE: the 33-bit odd integer 2 x + 1 converted to fp32 (nearest even), times 2^-33 (exact)
__device__ __forceinline__ float philox_uniform(uint32_t x) { return (float)(2ull * x + 1ull) * 0x1p-33f; }

__device__ __forceinline__ void box_muller(float ua, float ub, float* z) {
  const float r = sqrtf(-2.0f * logf(ua));
  float s, c;
  sincospif(2.0f * ub, &s, &c);
  z[0] = __fmul_rn(r, c);
  z[1] = __fmul_rn(r, s);
}

// the four normals of block j of a clip: Philox of the counter (j, call, stream_id, clip) -> Box-Muller of (u0, u1) and (u2, u3)
__device__ __forceinline__ void philox_normals4(uint32_t j, uint32_t call, uint32_t stream_id, uint32_t clip, uint32_t k0,
                                                uint32_t k1, float* z) {
  uint32_t x[4];
  philox4x32_10(j, call, stream_id, clip, k0, k1, x);
  box_muller(philox_uniform(x[0]), philox_uniform(x[1]), z);
  box_muller(philox_uniform(x[2]), philox_uniform(x[3]), z + 2);
}
