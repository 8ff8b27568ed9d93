// FP8 (OCP e4m3) linear GEMM for gfx950 on the K = 64 block-scaled MFMA:
//
//   out[m, n] = epilogue( a_scale[m] * w_scale[n] * sum_k A[m, k] * W[n, k]  +  bias[n] )
//
// A [M][lda] and W [N][Cin] hold e4m3 BYTES (ctrlv_quant_rows_f8), one fp32 scale per row of each; everything after the
// accumulator is gemm_epilogue.h, i.e. what ctrlv_gemm does for mode 0.
//   * v_mfma_scale_f32_32x32x64_f8f6f4 with cbsz = blgp = 0 (both operands e4m3) and every block scale the constant 1.0
//     (E8M0 byte 127): twice the FLOPs per clock of the 16-bit MFMAs.  The row and column scales are applied exactly, in
//     fp32, behind the accumulator.  A lane's 32 operand bytes are 32 consecutive k: lane l holds row (l & 31),
//     k = 32 (l >> 5) + j.  The weight tile is the A operand, so the C/D layout is the one gemm_epilogue.h expects.
//   * 128 x 128 tile with four waves (2 x 2, wave tile 64 x 64; 72 KiB of LDS, two workgroups per CU) or -- launches that
//     fill the chip with them -- 256 x 256 with eight waves (2 x 4, wave tile 128 x 64; 136 KiB, one workgroup per CU); K
//     step of 128 bytes per row: the staging image of gemm.hip's 2-stage kernel byte for byte (8 rows x 128 B per 16-byte
//     LDS-DMA wave-instruction, chunk swizzle on the source address), at half the staging bytes per FLOP.  Two stages: the
//     DMA of step t + 1 is in flight under the MFMAs of step t.
//   * both tiles sum a row's K steps in order with the same instruction, so a row's bits do not depend on the batch it is
//     computed in.
// Served (ctrlv_gemm_f8_serves, pure host code; the launcher applies exactly these): mode 0, taps 1, no A2, no lo planes,
// no raw_out / gn_partials / n_scale2 / SiLU, tile 0 (by size) or 1 / 2 (testing: 128 / 256 wide), Cin a multiple of 128, N a multiple of 32, lda a multiple of 16
// and >= Cin, ldo / n_store / ldr / ldv multiples of 4, out_f32 0 or 1; GEGLU with a bias-only epilogue.  Addresses are
// 64-bit: no pitch or offset limit beyond int32 M, N, Cin.  (Cin = 320 is not a multiple of 128: the C = 320 feed-forward
// stays on ff_fused.hip, whose intermediate never reaches HBM.)
#include "common.h"
#include "gemm_epilogue.h"

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x16 mfma_f8_32x32x64(const i32x8& a, const i32x8& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
}

__device__ __forceinline__ i32x8 frag32(const char* p0, const char* p1) {
  const i32x4 lo = *(const i32x4*)p0, hi = *(const i32x4*)p1;
  return i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(WM* WN * 64) void gemm_f8_kernel(const ctrlv_gemm_desc d, const float* __restrict__ a_scale,
                                                              const float* __restrict__ w_scale) {
  constexpr int NW = WM * WN;
  constexpr int WTM = BM / WM, WTN = BN / WN, TM = WTM / 32, TN = WTN / 32;
  constexpr int A_INSTR = BM / 8 / NW, B_INSTR = BN / 8 / NW;
  constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, STAGE = A_BYTES + B_BYTES;
  static_assert(A_INSTR >= 1 && B_INSTR >= 1, "tile too small for the wave count");
  extern __shared__ __attribute__((aligned(1024))) char smem[];

  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wid / WN, wc = wid % WN;
  if (d.geglu) gelu_table_fill(smem + 2 * STAGE, threadIdx.x, NW * 64);   // (the K loop's barriers order it before its use)

  const int tiles_n = (d.N + BN - 1) / BN;
  const int tiles_m = (d.M + BM - 1) / BM;
  const int t_id = xcd_remap(blockIdx.x, tiles_m * tiles_n);
  const int bm = (t_id / tiles_n) * BM, bn = (t_id % tiles_n) * BN;
  const int nk = d.Cin >> 7;              // K steps of 128 bytes

  // ---- LDS-DMA staging: a wave-instruction moves 8 rows x 128 B; physical 16-B chunk p of tile row r holds logical chunk
  // p ^ ((r >> 1) & 7) (the swizzle sits on the per-lane SOURCE address, the LDS image is lane-linear)
  const int prow = lane >> 3, pslot = lane & 7;
  const char* zsrc = (const char*)g_ctrlv_zeros + pslot * 16;
  const char* a_src[A_INSTR];
  const char* b_src[B_INSTR];
#pragma unroll
  for (int q = 0; q < A_INSTR; ++q) {
    const int rt = (q * NW + wid) * 8 + prow;
    const int m = bm + rt;
    a_src[q] = m < d.M ? (const char*)d.A + (long)m * d.lda + (pslot ^ ((rt >> 1) & 7)) * 16 : nullptr;
  }
#pragma unroll
  for (int q = 0; q < B_INSTR; ++q) {
    const int rt = (q * NW + wid) * 8 + prow;
    const int n = bn + rt;
    b_src[q] = n < d.N ? (const char*)d.W + (long)n * d.Cin + (pslot ^ ((rt >> 1) & 7)) * 16 : nullptr;
  }
  auto issue = [&](int kt, int stage) {
    char* sa = smem + stage * STAGE;
    char* sb = sa + A_BYTES;
    const long koff = (long)kt * 128;
#pragma unroll
    for (int q = 0; q < A_INSTR; ++q) {
      const char* p = a_src[q] ? a_src[q] + koff : zsrc;
      __builtin_amdgcn_global_load_lds(GLB_PTR(p), LDS_PTR(sa + (q * NW + wid) * 1024), 16, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < B_INSTR; ++q) {
      const char* p = b_src[q] ? b_src[q] + koff : zsrc;
      __builtin_amdgcn_global_load_lds(GLB_PTR(p), LDS_PTR(sb + (q * NW + wid) * 1024), 16, 0, 0);
    }
  };

  // fragment reads: row (lane & 31) of a 32-row sub-tile, the 32 bytes k = 64 ks + 32 (lane >> 5) ... + 31 = logical chunks
  // 4 ks + 2 hsel and the next one
  const int r32 = lane & 31, hsel = lane >> 5, sw = (lane >> 1) & 7;
  const int a_frag_base = (wr * WTM + r32) * 128;
  const int b_frag_base = A_BYTES + (wc * WTN + r32) * 128;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  issue(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < nk) issue(kt + 1, (kt + 1) & 1);
    const char* st = smem + (kt & 1) * STAGE;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int c0 = ((ks * 4 + hsel * 2) ^ sw) * 16, c1 = ((ks * 4 + hsel * 2 + 1) ^ sw) * 16;
      i32x8 af[TM], wf[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = frag32(st + a_frag_base + i * 32 * 128 + c0, st + a_frag_base + i * 32 * 128 + c1);
#pragma unroll
      for (int j = 0; j < TN; ++j) wf[j] = frag32(st + b_frag_base + j * 32 * 128 + c0, st + b_frag_base + j * 32 * 128 + c1);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = mfma_f8_32x32x64(wf[j], af[i], acc[i][j]);
    }
  }

  // ---- the row / column scales and the bias, in fp32: acc <- (acc * s_a[m]) * s_w[n] + bias[n]; then the shared epilogue
  // (accumulator e of a 32-column sub-tile is column 8 (e >> 2) + 4 hsel + (e & 3); N is a multiple of 32)
  float sa[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int m = bm + wr * WTM + i * 32 + r32;
    sa[i] = m < d.M ? a_scale[m] : 0.f;
  }
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col0 = bn + wc * WTN + j * 32 + 4 * hsel;
    if (col0 >= d.N) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 ws = *(const float4*)(w_scale + col0 + 8 * q);
      float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (d.bias) bv = *(const float4*)(d.bias + col0 + 8 * q);
      const float wsv[4] = {ws.x, ws.y, ws.z, ws.w}, bvv[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
      for (int i = 0; i < TM; ++i) {
#pragma clang fp contract(off)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float t = acc[i][j][4 * q + e] * sa[i];
          acc[i][j][4 * q + e] = __builtin_fmaf(t, wsv[e], bvv[e]);
        }
      }
    }
  }
  gemm_epilogue<TM, TN>(d, acc, bm, bn, wr, wc, WTM, WTN, r32, hsel, smem + 2 * STAGE);
}

const char* f8_unserved(const ctrlv_gemm_desc& d) {
  if (d.M <= 0 || d.N <= 0 || d.Cin <= 0) return "M, N, Cin must be positive";
  if (d.mode != 0 || d.taps != 1) return "mode 0 with taps == 1 only";
  if (d.A2) return "no second A source";
  if (d.R1_lo || d.R2_lo || d.out_lo) return "the split trunk (lo planes) is not served";
  if (d.raw_out || d.gn_partials || d.n_scale2 || d.act || d.pad_br || d.ksplit) return "no raw_out / gn_partials / n_scale2 / SiLU / pad_br";
  if (d.tile < 0 || d.tile > 2) return "tile is 0 (by size), 1 (128 x 128) or 2 (256 x 256)";
  if (d.Cin % 128) return "Cin must be a multiple of 128";
  if (d.N % 32) return "N must be a multiple of 32";
  if (d.lda < d.Cin || d.lda % 16) return "lda must be a multiple of 16 and >= Cin";
  if (d.ldo % 4 || d.n_store % 4 || d.n_store <= 0) return "ldo and n_store must be multiples of 4";
  if (d.out_f32 != 0 && d.out_f32 != 1) return "out_f32 is 0 or 1";
  if ((d.R1 && d.ldr1 % 4) || (d.R2 && d.ldr2 % 4)) return "ldr1 / ldr2 must be multiples of 4";
  if (d.vmode < 0 || d.vmode > 2) return "bad vmode";
  if (d.vmode && !(d.V && d.vdiv > 0 && d.vmod > 0 && d.ldv % 4 == 0 && (d.vmode == 1 || d.vS > 0))) return "bad row-vector table";
  if (d.geglu && (d.R1 || d.R2 || d.vmode || d.out_f32)) return "GEGLU takes a bias-only epilogue";
  {   // a row pitch covers its row (include/ctrlv_hip.h)
    const int n_st = d.geglu ? (d.n_store < d.N / 2 ? d.n_store : d.N / 2) : d.n_store;
    if (d.ldo < n_st) return "row pitch ldo is smaller than the stored columns";
    if ((d.R1 && d.ldr1 < n_st) || (d.R2 && d.ldr2 < n_st)) return "row pitch ldr1 / ldr2 is smaller than the stored columns";
    if (d.vmode && d.ldv < n_st) return "row pitch ldv is smaller than the stored columns";
  }
  if (((uintptr_t)d.A & 15) || ((uintptr_t)d.W & 15) || ((uintptr_t)d.out & (d.out_f32 ? 15 : 7)) || ((uintptr_t)d.bias & 15) ||
      ((uintptr_t)d.R1 & 7) || ((uintptr_t)d.R2 & 7) || ((uintptr_t)d.V & 15))
    return "operands must be aligned (A, W, bias, V 16 bytes; R1, R2, out 8 bytes; out 16 with out_f32)";
  if ((long)((d.M + 127) / 128) * ((d.N + 127) / 128) > 0x7fffffffL) return "too many tiles";
  return nullptr;
}

template <int BM, int BN, int WM, int WN>
int launch_f8(const ctrlv_gemm_desc& d, const float* a_scale, const float* w_scale, hipStream_t stream) {
  constexpr int smem = 2 * (BM + BN) * 128 + kGeluTabBytes;       // staging ring | Phi table (GEGLU launches)
  static_assert(smem <= 160 * 1024, "f8 tile does not fit the LDS");
  static bool attr_set[CTRLV_MAX_DEVICES] = {};      // per device: the attribute belongs to the device's code object
  auto kfn = gemm_f8_kernel<BM, BN, WM, WN>;
  const int dev = ctrlv_current_device();
  if (!attr_set[dev]) {
    CTRLV_HIP_TRY(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    attr_set[dev] = true;
  }
  const long tiles = (long)((d.M + BM - 1) / BM) * ((d.N + BN - 1) / BN);
  hipLaunchKernelGGL(kfn, dim3((unsigned)tiles), dim3(WM * WN * 64), smem, stream, d, a_scale, w_scale);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

}  // namespace

extern "C" int ctrlv_gemm_f8_serves(const ctrlv_gemm_desc* d) { return d != nullptr && f8_unserved(*d) == nullptr; }

extern "C" int ctrlv_gemm_f8(const ctrlv_gemm_desc* dp, const float* a_scale, const float* w_scale, ctrlv_stream_t stream_) {
  CTRLV_CHECK_ARG(dp != nullptr, "ctrlv_gemm_f8: null descriptor");
  const ctrlv_gemm_desc& d = *dp;
  CTRLV_CHECK_ARG(d.A && d.W && d.out && a_scale && w_scale, "ctrlv_gemm_f8: A, W, out and the two scale vectors must be non-null");
  CTRLV_CHECK_ARG((((uintptr_t)a_scale | (uintptr_t)w_scale) & 15) == 0, "ctrlv_gemm_f8: scale vectors must be 16-byte aligned");
  const char* why = f8_unserved(d);
  CTRLV_CHECK_SHAPE(why == nullptr, "ctrlv_gemm_f8: not served (M=%d N=%d Cin=%d): %s", d.M, d.N, d.Cin, why ? why : "");
  // Tile by the launch's size: 256 x 256 (eight waves, one workgroup per CU, half the staging bytes per FLOP) for the wide
  // launches that fill the chip with such tiles -- the GEGLU projections, N = 5120 / 10240: 771 -> 595 and 595 -> 465 us at C =
  // 640 / 1280 --, else 128 x 128 (the output projections, N = 640 / 1280 with long K: 320 against 342 us on the wide tile;
  // profiles/ff_f8_bench.jsonl).  Both sum a row's K steps in the same order with the same instruction, so the choice changes
  // no bit (tests/test_gemm_f8_gpu.py: a row block alone and in a large batch, either tile forced).
  const long tiles256 = (long)((d.M + 255) / 256) * ((d.N + 255) / 256);
  if (d.tile == 2 || (d.tile == 0 && d.M >= 1024 && d.N >= 2048 && tiles256 >= ctrlv_num_cu(ctrlv_current_device())))
    return launch_f8<256, 256, 2, 4>(d, a_scale, w_scale, (hipStream_t)stream_);
  return launch_f8<128, 128, 2, 2>(d, a_scale, w_scale, (hipStream_t)stream_);
}
