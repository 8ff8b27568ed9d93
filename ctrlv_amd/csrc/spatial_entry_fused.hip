// Fused entry of the spatial transformer block at C = 320 (the opening of TransformerSpatioTemporalModel at the 72 x 128 level:
// GroupNorm apply -> proj_in -> LayerNorm (norm1 of the spatial BasicTransformerBlock) -> q|k|v projection), gfx950:
//
//     h0 = el( el(GN(x)) W_in^T + b_in ),      (q | k | v) = el( el(LN(h0)) W_qkv^T [+ b_qkv] ),   q scaled by (1 / 8) log2(e)
//
// per ROW.  The four launches it replaces (gn_apply, proj_in GEMM, ln_rows, q|k|v GEMM; csrc/plan.hip run_tr) move 2.65 GB per
// block at M = 460 800: the normalised rows are written and read back twice only to connect launches.  Here x is read once and
// only h0 (a trunk tensor: the block's later residual) and q|k|v are written: 1.475 GB.
//
// Structure: temporal_fused.hip's.  ONE WAVE = 32 ROWS, the 32 columns of every MFMA; the rows sit in registers as B-operand
// fragments (80 registers) and nothing between them and the output accumulators goes through LDS:
//   * x rows -> GroupNorm with gn_apply_kernel's arithmetic (a = rstd gamma, b = beta - mean a, y = x a + b; per-channel
//     coefficients of the wave's image in an LDS strip of its own, built from the finalized (mean, rstd) array), rounded: the
//     B fragments of the proj_in chains, K steps in natural order (ctrlv_gemm's K order).
//   * proj_in: acc = W_in . y on start values b_in, 10 blocks of 32 output channels.  The ROW order of every packed weight block
//     gives a lane 16 CONSECUTIVE output channels (A row 8 q + 4 hs + r holds channel 32 nb + 16 hs + 4 q + r): h0 goes out as
//     2 x 16 B per lane and block straight from the accumulators, and the rounded values ARE the B fragments of the next chains
//     (K step 2 nb + k2, slot (hs, e) <-> channel 32 nb + 16 hs + 8 k2 + e: baked into the K order of the packed W_qkv).
//   * LayerNorm on the rounded h0 fragments with ln_rows_kernel's two-pass arithmetic (a row lives in one lane pair: one
//     half-wave exchange per sum), rounded.
//   * q|k|v: 30 blocks of 32 output channels on start values b_qkv (or zero), the q blocks scaled in fp32 before the one
//     rounding (ctrlv_gemm's n_scale2 / s_acc2), each block stored as it retires.
// Weights: 40 chunks of 20 KiB (fragment-major, one KiB per MFMA) stream in PAIRS through the 3-slot LDS-DMA ring, two pairs
// ahead; the 8 waves of a workgroup (256 consecutive rows) walk the pairs in two groups half a slot apart (ping-pong).  The
// next row group's x rows and statistics are requested under the q|k|v chains.  A 32-row group lies inside one image
// (S % 32 == 0), so its GroupNorm coefficients are per channel only.
#include "common.h"
#include "gemm_pp_kernel.h"      // wait_vmcnt / raw_barrier / lds_done_barrier / pp_store_out (store-data hazard guard)

namespace {

constexpr int kC = 320, kKS = kC / 16;                           // 20 K steps of 16
constexpr int kChunk = kKS * 1024;                               // 20 KiB: 32 weight rows x 320, one KiB per K step
constexpr int kInChunks = kC / 32, kQkvChunks = 3 * kC / 32, kChunks = kInChunks + kQkvChunks;   // 10 + 30
constexpr int kPair = 2 * kChunk, kPairs = kChunks / 2;          // the ring moves PAIRS of chunks: one barrier per 40 MFMAs
constexpr int kInPairs = kInChunks / 2, kQkvPairs = kQkvChunks / 2;
constexpr int kSlots = 3;
constexpr int kBiasOff = kSlots * kPair;                         // start values: b_in | b_qkv, 1280 floats
constexpr int kLnOff = kBiasOff + 4 * kC * 4;                     // LayerNorm gamma | beta
constexpr int kGnOff = kLnOff + 2 * kC * 4;                       // GroupNorm gamma | beta
constexpr int kCoefOff = kGnOff + 2 * kC * 4;                     // per wave: GroupNorm a | b of its image (fp32)
constexpr int kStatOff = kCoefOff + 8 * 2 * kC * 4;               // per wave: (mean, rstd) of the 32 groups of its image
constexpr int kSmem = kStatOff + 8 * 256;                        // 120 KiB ring + 5 + 2.5 + 2.5 + 20 + 2 KiB
constexpr int kNQ = 6;                                           // fragment reads in flight ahead of the MFMAs
constexpr int kDmaPerWave = 2 * kKS / 8;                         // 5 one-KiB pieces per wave and pair
constexpr int kCoefLoads = kC / 64;                              // 5 channels per lane

struct SeArgs {
  const el_t* x; int ldx;                 // raw trunk rows [M][ldx]
  const el_t* wf;                         // kChunks x 20 KiB (ctrlv_spatial_entry_fused_pack)
  const float* bias_in; const float* bias_qkv;       // [320] / [960] or null
  const float* stats;                     // [n_img][32][2] finalized (mean, rstd)
  const float* gn_g; const float* gn_b;
  const float* ln_g; const float* ln_b; float ln_eps;
  el_t* h0; int ldh;
  el_t* qkv; int ldq;
  int M, S, n_img;
  float q_scale;
};

__device__ __forceinline__ void pin(elx8& v) { asm volatile("" : "+v"(v)); }
// The norms' results exist as fp32 values before they are rounded to the element type, as in gn_apply_kernel / ln_rows_kernel
// (v_fma_f32 + v_cvt_pk_f16_f32): left alone, the fp16 build contracts the last fma and the conversion into v_fma_mix{lo,hi}_f16,
// which rounds ONCE and differs from the launches in rare elements.
__device__ __forceinline__ void fp32_value(float& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ float swap_sum(float v) {
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

__global__ __launch_bounds__(512) void spatial_entry_fused_kernel(const SeArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  CTRLV_CLOCK_BEGIN();
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int f32_ = lane & 31, hsel = lane >> 5;
  const int M = a.M;                                             // (every byte offset fits 31 bits: se_check)
  const int S = a.S;
  const int ngroups = (M + 255) / 256;
  const int G = gridDim.x;
  constexpr unsigned kOOB = 0xFFFFFFFFu;
  constexpr int kFlags = 0x00020000;

  const __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc((void*)a.wf, 0, kChunks * kChunk, kFlags);
  const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, M * a.ldx * 2, kFlags);
  const __amdgpu_buffer_rsrc_t rsH = __builtin_amdgcn_make_buffer_rsrc((void*)a.h0, 0, M * a.ldh * 2, kFlags);
  const __amdgpu_buffer_rsrc_t rsQ = __builtin_amdgcn_make_buffer_rsrc((void*)a.qkv, 0, M * a.ldq * 2, kFlags);
  const __amdgpu_buffer_rsrc_t rsS = __builtin_amdgcn_make_buffer_rsrc((void*)a.stats, 0, a.n_img * 64 * 4, kFlags);

  // LDS-DMA of chunk pair `c` (0 .. kPairs - 1, cyclic) into ring slot `g % 3` (g = the workgroup's running pair count): wave w
  // takes pieces w, w + 8, .., w + 32 of the pair's 40
  auto dma = [&](int c, int g) {
    char* slot = smem + (g % kSlots) * kPair;
#pragma unroll
    for (int k = 0; k < kDmaPerWave; ++k) {
      const int pi = k * 8 + wid;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, LDS_PTR(slot + pi * 1024), 16, (unsigned)(lane * 16), c * kPair + pi * 1024, 0, 0);
    }
  };
  int g = 0;                                                     // finished slots of this workgroup (ring phase)
  // PING-PONG and ring discipline: temporal_fused.hip's, unchanged.  A slot is  [barrier] X: the pair's 40 MFMAs  [barrier] Y:
  // roundings / stores / norms / loads / the DMA issue; group 1 (waves 4..7) runs half a slot behind group 0.  Pair t is read
  // in X(t); DMA(t + 2) refills the slot of pair t - 1 and is the last thing of Y(t); a wave waits for everything it has in
  // flight (vmcnt(0)) at the end of X(t + 1), two barriers in front of the first read of pair t + 2.
  elx8 wq[kNQ];
  auto chain_prefetch = [&]() {
    const char* s1 = smem + (g % kSlots) * kPair + lane * 16;
#pragma unroll
    for (int i = 0; i < kNQ; ++i) wq[i] = *(const elx8*)(s1 + i * 1024);
  };
  // (group 1 may read the chain's first fragments in front of the slot's barrier, group 0 only behind it: temporal_fused.hip)
  const bool early_frags = wid >= 4;
  auto x_begin = [&]() {
    if (early_frags) chain_prefetch();
    lds_done_barrier();
    if (!early_frags) chain_prefetch();
  };
  auto y_begin = [&]() {
    wait_vmcnt<0>();
    lds_done_barrier();
  };
  auto y_end = [&]() {                                           // the slot's DMA issue; g counts finished slots
    dma((g + 2) % kPairs, g + 2);
    ++g;
  };
  // One pair = 2 x 20 MFMAs over K = 320 against the wave's fragments `xb`: acc = W . x (lane = row), accA takes the pair's
  // first chunk, accB its second.  Fragment reads run kNQ MFMAs ahead through rotating registers.
  auto chain2 = [&](const elx8 (&xb)[kKS], f32x16& accA, f32x16& accB) {
    const char* s1 = smem + (g % kSlots) * kPair + lane * 16;
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < 2 * kKS; ++ks) {
      if (ks < kKS) accA = mfma_32x32x16(wq[ks % kNQ], xb[ks], accA);
      else accB = mfma_32x32x16(wq[ks % kNQ], xb[ks - kKS], accB);
      if (ks + kNQ < 2 * kKS) wq[ks % kNQ] = *(const elx8*)(s1 + (ks + kNQ) * 1024);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  // x rows as B fragments: K step ks = channels 16 ks + 8 hsel .. + 7 of the lane's row (rows past the end: zeros)
  auto x_offset = [&](int grp) {
    const int row = (grp * 8 + wid) * 32 + f32_;
    return row < M ? (unsigned)row * (unsigned)(a.ldx * 2) + 16u * hsel : kOOB;
  };
  auto x_loads = [&](elx8 (&xr)[kKS], unsigned xoff, int k0, int k1) {
#pragma unroll
    for (int ks = k0; ks < k1; ++ks)
      xr[ks] = __builtin_bit_cast(elx8, __builtin_amdgcn_raw_buffer_load_b128(rsX, xoff, ks * 32, 0));
  };

  // ---- constants of the launch -> LDS (before any LDS-DMA is in flight)
  for (int i = threadIdx.x; i < 4 * kC; i += 512)
    *(float*)(smem + kBiasOff + i * 4) = i < kC ? (a.bias_in ? a.bias_in[i] : 0.f) : (a.bias_qkv ? a.bias_qkv[i - kC] : 0.f);
  for (int i = threadIdx.x; i < kC; i += 512) {
    *(float*)(smem + kLnOff + i * 4) = a.ln_g[i];
    *(float*)(smem + kLnOff + (kC + i) * 4) = a.ln_b[i];
    *(float*)(smem + kGnOff + i * 4) = a.gn_g[i];
    *(float*)(smem + kGnOff + (kC + i) * 4) = a.gn_b[i];
  }
  __syncthreads();
  const unsigned bias_lds = (unsigned)(unsigned long)LDS_PTR(smem + kBiasOff);
  const unsigned ln_lds = (unsigned)(unsigned long)LDS_PTR(smem + kLnOff);
  const unsigned gn_lds = (unsigned)(unsigned long)LDS_PTR(smem + kGnOff);
  const unsigned coef_lds = (unsigned)(unsigned long)LDS_PTR(smem + kCoefOff + wid * (2 * kC * 4));
  const unsigned stat_lds = (unsigned)(unsigned long)LDS_PTR(smem + kStatOff + wid * 256);

  // GroupNorm coefficients of a row group's image: lanes 0 .. 31 fetch (mean, rstd) of their group from the finalized array
  // (requested a few slots before use) and park them in the wave's strip; lane l then turns channels l, l + 64, .. (group
  // c / 10) into a | b in the wave's coefficient strip.
  auto coef_request = [&](int grp, u32x2_t& st) {
    const int row0 = (grp * 8 + wid) * 32;
    const bool live = row0 < M;
    const int n = live ? row0 / S : 0;
    st = __builtin_amdgcn_raw_buffer_load_b64(rsS, live ? (unsigned)((n * 32 + f32_) * 8) : kOOB, 0, 0);     // lane's group = lane & 31
  };
  // (asm LDS accesses with their own wait: the compiler puts a vmcnt(0) in front of an LDS access it knows of while LDS-DMA of
  //  this wave is in flight, gemm_pp_kernel.h.  The strips' readers are this wave's own: LDS operations of a wave run in order)
  auto coef_write = [&](const u32x2_t& st) {
    if (lane < 32) asm volatile("ds_write_b64 %0, %1" ::"v"(stat_lds + 8u * lane), "v"(st) : "memory");
#pragma unroll
    for (int t = 0; t < kCoefLoads; ++t) {
      float gam, bet;
      u32x2_t mr;
      const unsigned gq = (unsigned)(t * 64 + lane) / (kC / 32);
      asm volatile("ds_read_b64 %0, %1" : "=v"(mr) : "v"(stat_lds + 8u * gq) : "memory");
      asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(gam) : "v"(gn_lds + 4u * lane), "n"(t * 256) : "memory");
      asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(bet) : "v"(gn_lds + 4u * lane), "n"(kC * 4 + t * 256) : "memory");
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(gam), "+v"(bet), "+v"(mr));
      const float mean = __uint_as_float(mr[0]), rstd = __uint_as_float(mr[1]);
      const float ca = rstd * gam;
      const float cb = bet - mean * ca;
      asm volatile("ds_write_b32 %0, %1 offset:%2" ::"v"(coef_lds + 4u * lane), "v"(ca), "n"(t * 256) : "memory");
      asm volatile("ds_write_b32 %0, %1 offset:%2" ::"v"(coef_lds + 4u * lane), "v"(cb), "n"(kC * 4 + t * 256) : "memory");
    }
  };
  // y = x a + b on the raw fragments (gn_apply_kernel's expression), rounded to the element type
  auto gn_apply = [&](elx8 (&xr)[kKS], bool keep) {
    const unsigned ca = coef_lds + 32u * hsel;                   // a of channels 16 ks + 8 hsel .. + 7 at ca + 64 ks
#pragma unroll
    for (int ks = 0; ks < kKS; ++ks) {
      f32x4 a0, a1, b0, b1;
      asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(a0) : "v"(ca), "n"(ks * 64) : "memory");
      asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(a1) : "v"(ca), "n"(ks * 64 + 16) : "memory");
      asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(b0) : "v"(ca), "n"(kC * 4 + ks * 64) : "memory");
      asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(b1) : "v"(ca), "n"(kC * 4 + ks * 64 + 16) : "memory");
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a0), "+v"(a1), "+v"(b0), "+v"(b1));
      const float aa[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
      const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
      float f[8];
      unpack_elx8(__builtin_bit_cast(uint4, xr[ks]), f);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        f[e] = f[e] * aa[e] + bb[e];
        fp32_value(f[e]);
      }
      uint4 pk = pack_elx8(f);
      if (!keep) pk = make_uint4(0, 0, 0, 0);                    // rows past the end stay zero rows
      xr[ks] = __builtin_bit_cast(elx8, pk);
      pin(xr[ks]);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  // LayerNorm on the rounded h0 fragments (hb[2 nb + k2] = channels 32 nb + 16 hsel + 8 k2 .. + 7 of the lane's row): the
  // two-pass arithmetic of ln_rows_kernel, a row's two halves in lanes l and l + 32
  auto layer_norm = [&](elx8 (&hb)[kKS], bool keep) {
    float sm = 0.f;
#pragma unroll
    for (int ks = 0; ks < kKS; ++ks) {
      float f[8];
      unpack_elx8(__builtin_bit_cast(uint4, hb[ks]), f);
#pragma unroll
      for (int e = 0; e < 8; ++e) sm += f[e];
      __builtin_amdgcn_sched_barrier(0);                         // (one K step's eight values alive at a time)
    }
    float mean = swap_sum(sm) * (1.0f / kC);
    asm volatile("" : "+v"(mean));
    float sq = 0.f;
#pragma unroll
    for (int ks = 0; ks < kKS; ++ks) {
      pin(hb[ks]);                                               // (opaque between the passes: unpack again, do not keep 160 floats)
      float f[8];
      unpack_elx8(__builtin_bit_cast(uint4, hb[ks]), f);
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float dl = f[e] - mean; sq += dl * dl; }
      __builtin_amdgcn_sched_barrier(0);
    }
    float rstd = rsqrtf(swap_sum(sq) * (1.0f / kC) + a.ln_eps);
    asm volatile("" : "+v"(rstd));
    const unsigned ga = ln_lds + 64u * hsel;                     // gamma of the K step's channels at ga + 128 (ks >> 1) + 32 (ks & 1)
#pragma unroll
    for (int ks = 0; ks < kKS; ++ks) {
      f32x4 g0, g1, b0, b1;
      asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(g0) : "v"(ga), "n"((ks >> 1) * 128 + (ks & 1) * 32) : "memory");
      asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(g1) : "v"(ga), "n"((ks >> 1) * 128 + (ks & 1) * 32 + 16) : "memory");
      asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(b0) : "v"(ga), "n"(kC * 4 + (ks >> 1) * 128 + (ks & 1) * 32) : "memory");
      asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(b1) : "v"(ga), "n"(kC * 4 + (ks >> 1) * 128 + (ks & 1) * 32 + 16) : "memory");
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(g0), "+v"(g1), "+v"(b0), "+v"(b1));
      const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
      const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
      pin(hb[ks]);
      float f[8], o[8];
      unpack_elx8(__builtin_bit_cast(uint4, hb[ks]), f);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        o[e] = (f[e] - mean) * rstd * gg[e] + bb[e];
        fp32_value(o[e]);
      }
      uint4 pk = pack_elx8(o);
      if (!keep) pk = make_uint4(0, 0, 0, 0);
      hb[ks] = __builtin_bit_cast(elx8, pk);
      pin(hb[ks]);                                               // (computed HERE, not sunk to the chain that uses it)
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  // start values of a pair of output blocks (global blocks gb, gb + 1 of the 40): the lane's 2 x 16 channels from the table
  auto start_values = [&](int gb, f32x16 (&acc)[2]) {
    f32x4 iq[2][4];
    const unsigned ia = bias_lds + (unsigned)((gb * 32 + 16 * hsel) * 4);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(iq[t][q]) : "v"(ia), "n"(t * 128 + q * 16) : "memory");
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(iq[0][0]), "+v"(iq[0][1]), "+v"(iq[0][2]), "+v"(iq[0][3]), "+v"(iq[1][0]), "+v"(iq[1][1]), "+v"(iq[1][2]),
                   "+v"(iq[1][3]));
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        acc[t][4 * q] = iq[t][q].x; acc[t][4 * q + 1] = iq[t][q].y; acc[t][4 * q + 2] = iq[t][q].z; acc[t][4 * q + 3] = iq[t][q].w;
      }
  };

  // ---- prologue: pairs 0 and 1 in flight, the first row group's rows and statistics requested
  dma(0, 0);
  dma(1, 1);
  elx8 xr[kKS];
  u32x2_t st;
  x_loads(xr, x_offset(blockIdx.x), 0, kKS);
  coef_request(blockIdx.x, st);
  wait_vmcnt<0>();
  coef_write(st);
  if (wid >= 4) raw_barrier();                                   // group 1 starts half a slot behind

  for (int grp = blockIdx.x; grp < ngroups; grp += G) {
    const int row = (grp * 8 + wid) * 32 + f32_;                // this lane's row
    const bool ok = row < M;
    elx8 hb[kKS];                                                // h0, rounded: the q|k|v chains' B fragments
    gn_apply(xr, ok);
    // ---- proj_in, 10 blocks of 32 channels in pairs; lane (row, hsel) ends with channels 32 nb + 16 hsel .. + 15
    const unsigned hbase = ok ? (unsigned)row * (unsigned)(a.ldh * 2) + 32u * hsel : kOOB;
#pragma unroll
    for (int np = 0; np < kInPairs; ++np) {
      f32x16 acc[2];
      start_values(2 * np, acc);
      x_begin();
      chain2(xr, acc[0], acc[1]);
      y_begin();
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int hq = 0; hq < 2; ++hq) {
          float o[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = acc[t][8 * hq + e];
          const uint4 pk = pack_elx8(o);
          hb[4 * np + 2 * t + hq] = __builtin_bit_cast(elx8, pk);
          pin(hb[4 * np + 2 * t + hq]);
          const u32x4_t pv = {pk.x, pk.y, pk.z, pk.w};
          pp_store_out(pv, rsH, hbase, (2 * np + t) * 64 + hq * 16);
        }
      y_end();
    }
    layer_norm(hb, ok);
    // ---- q|k|v, 30 blocks of 32 channels in pairs, stored as they retire
    const unsigned qbase = ok ? (unsigned)row * (unsigned)(a.ldq * 2) + 32u * hsel : kOOB;
    const unsigned xoff_next = x_offset(grp + G);
#pragma unroll
    for (int np = 0; np < kQkvPairs; ++np) {
      f32x16 acc[2];
      start_values(kInChunks + 2 * np, acc);
      x_begin();
      chain2(hb, acc[0], acc[1]);
      y_begin();
      const float sc = 2 * np < kInChunks ? a.q_scale : 1.0f;    // (blocks 0 .. 9 are q; a pair never straddles the boundary)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int hq = 0; hq < 2; ++hq) {
          float o[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = acc[t][8 * hq + e] * sc;              // (the bias is already in the accumulator)
          const uint4 pk = pack_elx8(o);
          const u32x4_t pv = {pk.x, pk.y, pk.z, pk.w};
          pp_store_out(pv, rsQ, qbase, (2 * np + t) * 64 + hq * 16);
        }
      // the NEXT row group's rows, four K steps per slot (the x registers are free behind proj_in), and its statistics; the
      // coefficients go to the strip a slot later (its last readers were this group's gn_apply)
      if (np < 5) x_loads(xr, xoff_next, np * 4, np * 4 + 4);
      if (np == 5) coef_request(grp + G, st);
      if (np == 7) coef_write(st);                               // (behind the vmcnt(0) of slots 6 and 7)
      y_end();
    }
  }
  if (wid < 4) raw_barrier();                                    // group 0's closing barrier (pairs with group 1's last one)
  wait_vmcnt<0>();                                               // the look-ahead DMA: nothing may be in flight at exit
  CTRLV_CLOCK_END();
#endif
}

// fragment-major copy of the packed weights.  Chunk c < 10: block c of W_in, K steps in natural order.  Chunk 10 + nb: block nb
// of the fused [3C][C] projection with its K steps in the order h0 arrives: step ks, slot (hs', e) <-> input channel
// 32 (ks >> 1) + 16 hs' + 8 (ks & 1) + e.  Every block's rows permuted: A row 8 q + 4 hs + r holds output channel
// 32 nb + 16 hs + 4 q + r.
__global__ void spatial_entry_pack_kernel(const el_t* __restrict__ win, int ld_in, const el_t* __restrict__ wqkv, int ld_qkv,
                                          el_t* __restrict__ wf) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)kChunks * kKS * 512) return;
  const int e = i & 7, lane = (i >> 3) & 63, ks = (int)((i >> 9) % kKS), c = (int)(i / (kKS * 512));
  const int i32 = lane & 31, hs = lane >> 5;
  const int q = i32 >> 3, hs_r = (i32 >> 2) & 1, r = i32 & 3;              // A row i32 = 8 q + 4 hs_r + r
  el_t v;
  if (c < kInChunks) {
    const int n = c * 32 + 16 * hs_r + 4 * q + r;
    v = win[(long)n * ld_in + ks * 16 + 8 * hs + e];
  } else {
    const int n = (c - kInChunks) * 32 + 16 * hs_r + 4 * q + r;
    v = wqkv[(long)n * ld_qkv + 32 * (ks >> 1) + 16 * hs + 8 * (ks & 1) + e];
  }
  wf[i] = v;
}

}  // namespace

CTRLV_CLOCK_READER(spatial_entry_fused)

extern "C" size_t ctrlv_spatial_entry_fused_weight_bytes(void) { return (size_t)kChunks * kChunk; }

extern "C" int ctrlv_spatial_entry_fused_pack(const void* win_packed, int ld_in, const void* wqkv_packed, int ld_qkv, void* wf,
                                              ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(win_packed && wqkv_packed && wf, "ctrlv_spatial_entry_fused_pack: null pointer");
  CTRLV_CHECK_SHAPE(ld_in >= kC && ld_qkv >= kC, "ctrlv_spatial_entry_fused_pack: the packed weights must have K >= 320");
  const long n = (long)kChunks * kKS * 512;
  hipLaunchKernelGGL(spatial_entry_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const el_t*)win_packed, ld_in, (const el_t*)wqkv_packed, ld_qkv, (el_t*)wf);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

// the launcher's conditions (one function for it and for the callers' switch, ctrlv_spatial_entry_fused_serves): shape and
// operands only
static int se_check(const ctrlv_spatial_entry_desc& d, bool report) {
#define SE_REQ(cond, code, ...)                        \
  do {                                                 \
    if (!(cond)) {                                     \
      if (report) ctrlv_set_error(__VA_ARGS__);        \
      return code;                                     \
    }                                                  \
  } while (0)
  SE_REQ(d.C == kC && d.head_dim == 64, CTRLV_E_BAD_SHAPE, "ctrlv_spatial_entry_fused: serves C = 320 with head_dim 64 only (C=%d, head_dim=%d)",
         d.C, d.head_dim);
  SE_REQ(d.n_img > 0 && d.S > 0 && d.S % 32 == 0, CTRLV_E_BAD_SHAPE,
         "ctrlv_spatial_entry_fused: S=%d must be a positive multiple of 32 (a 32-row group lies in one image)", d.S);
  SE_REQ(!d.x_lo && !d.h0_lo, CTRLV_E_BAD_ARG, "ctrlv_spatial_entry_fused: split trunk planes are not served");
  SE_REQ(d.ldx >= kC && d.ldx % 8 == 0 && d.ldh >= kC && d.ldh % 8 == 0 && d.ldq >= 3 * kC && d.ldq % 8 == 0, CTRLV_E_BAD_SHAPE,
         "ctrlv_spatial_entry_fused: row pitches must be >= 320 (q|k|v: 960) and multiples of 8");
  const long M = (long)d.n_img * d.S, lim = 0x7FFFFFF0L;
  SE_REQ(M * d.ldx * 2 <= lim && M * d.ldh * 2 <= lim && M * d.ldq * 2 <= lim, CTRLV_E_BAD_SHAPE,
         "ctrlv_spatial_entry_fused: operands beyond 31-bit byte offsets");
  return CTRLV_OK;
#undef SE_REQ
}

extern "C" int ctrlv_spatial_entry_fused_serves(const ctrlv_spatial_entry_desc* d) {
  return (d && se_check(*d, false) == CTRLV_OK) ? 1 : 0;
}

extern "C" int ctrlv_spatial_entry_fused(const ctrlv_spatial_entry_desc* dp, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(dp && dp->x && dp->wf && dp->stats && dp->gn_gamma && dp->gn_beta && dp->ln_gamma && dp->ln_beta && dp->h0 && dp->qkv,
                  "ctrlv_spatial_entry_fused: null pointer");
  const ctrlv_spatial_entry_desc& d = *dp;
  const int rc = se_check(d, true);
  if (rc != CTRLV_OK) return rc;
  SeArgs a;
  a.x = (const el_t*)d.x; a.ldx = d.ldx; a.wf = (const el_t*)d.wf; a.bias_in = d.bias_in; a.bias_qkv = d.bias_qkv;
  a.stats = d.stats; a.gn_g = d.gn_gamma; a.gn_b = d.gn_beta; a.ln_g = d.ln_gamma; a.ln_b = d.ln_beta; a.ln_eps = d.ln_eps;
  a.h0 = (el_t*)d.h0; a.ldh = d.ldh; a.qkv = (el_t*)d.qkv; a.ldq = d.ldq;
  a.M = d.n_img * d.S; a.S = d.S; a.n_img = d.n_img; a.q_scale = d.q_scale;
  const int dev = ctrlv_current_device();
  const long groups = ((long)a.M + 255) / 256;
  const int num_cu = ctrlv_num_cu(dev);
  long grid = groups;
  if (groups > num_cu) {                    // persistent, every workgroup (nearly) the same number of row groups
    const long rounds = (groups + num_cu - 1) / num_cu;
    grid = (groups + rounds - 1) / rounds;
  }
  static bool attr_set[CTRLV_MAX_DEVICES] = {};
  if (!attr_set[dev]) {
    CTRLV_HIP_TRY(hipFuncSetAttribute((const void*)spatial_entry_fused_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kSmem));
    attr_set[dev] = true;
  }
  hipLaunchKernelGGL(spatial_entry_fused_kernel, dim3((unsigned)grid), dim3(512), kSmem, (hipStream_t)stream, a);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}
