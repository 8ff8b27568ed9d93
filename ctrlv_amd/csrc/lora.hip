// LoRA adapters of the stage-1 UNet fine-tuning step (the reference's --enable_lora: tools/train_video_diffusion.py:126-136,
// 205-216; rank-r factors on every to_q / to_k / to_v / to_out.0, the UNet itself frozen).
//
// One adapted linear, s = lora_alpha / r:   Y = X . W'^T,  W' = W + s . B . A,  A [r, Cin], B [N, r].
// The factor gradients are formed WITHOUT the [N, Cin] weight gradient:
//   H = X . A^T, G = dY . B   ([M, r] each)       dA = s . G^T . X   [r, Cin]        dB = s . dY^T . H   [N, r]
// Precision: X and dY are the layer's element rows; every other operand of the matrix pipe -- A, B, H, G -- is carried as an
// element PAIR hi + lo (hi = rne(v), lo = rne(v - hi): ~16 significant bits in bf16) and multiplied twice, so the factor
// gradients come out as fp32 products of the element rows (rel-L2 ~1e-5 against fp32; one rounding to bf16 would leave
// ~1.5e-3).  The extra MFMAs are free: both passes are bound by the HBM stream of X and dY.
// Groups: g adapters side by side along N (the fused q|k|v projection: g = 3, one shared X, dY = the [M, 3C] dqkv).  The
// g factor pairs are handled as ONE concatenated rank R = g.r: H_cat = X . A_cat^T, G_cat = dY . Bbd with Bbd the block
// diagonal [N, R] (column block i holds B_i on group i's rows), dA_cat = s . G_cat^T . X is exactly [A_0; A_1; ...]'s
// gradient, and dB is the block diagonal of s . dY^T . H_cat (the off-diagonal blocks are computed and dropped: the MFMA
// work is ~M.N.32.2 FLOP, microseconds).  R is padded to RP = a multiple of 32 (the MFMA width) in registers and LDS only.
//
// Four launches, all deterministic (no atomics; the partition is a function of M, Cin, N, g, r only):
//   lora_fac_kernel    the factors once, as (hi, lo) element planes of A_cat and Bbd^T (a few hundred KB);
//   lora_hg_kernel     128 rows per workgroup (a 32-row MFMA tile per wave): H_cat and G_cat over the whole row,
//                      written TRANSPOSED ([RP][Mp] element rows, Mp = slabs x rows per slab, zero rows beyond M) so that
//                      the second pass reads them m-contiguous;
//   lora_part_kernel   (row slab, 64-column chunk of [X | dY]): out[j][q] = sum over the slab's rows of L[m][j] . T[m][q]
//                      with (L, T) = (G, X) for the dA columns and (H, dY) for the dB columns; T staged row-major in LDS
//                      and read down the columns, the four waves' row quarters summed in LDS in wave order;
//                      one fp32 [RP][Cin + N] partial per slab;
//   lora_reduce_kernel the slab partials added in slab order, times s, written to dA / dB (assigned, not accumulated).
// X and dY cross HBM twice (once per pass: the H / G of a row are needed before its dA / dB terms).
#include "common.h"

namespace {

constexpr int kLdsPitch = 72;          // element pitch of the [64 rows][64] LDS tile: 144 B, 16-B aligned, row + 8 on other banks
constexpr int kHgRows = 128;           // rows per lora_hg_kernel workgroup
constexpr int kSub = 64;               // rows per sub-block of lora_part_kernel

struct LoraArgs {
  const el_t* X; const el_t* dY; const float* A; const float* B; float* dA; float* dB;
  el_t* HT; el_t* GT; el_t* FP; float* part;   // HT / GT: [2 (hi, lo)][RP][Mp] each; FP: [2][RP][Cin + N]
  int M, Cin, N, Ng, g, r, R, RP, Mp, slabs, rows_per_slab, ldx, ldy;
  float scale;
};

__device__ __forceinline__ elx8 ld8(const el_t* p) { return *(const elx8*)p; }
__device__ __forceinline__ elx8 zero8() {
  elx8 z;
#pragma unroll
  for (int i = 0; i < 8; ++i) z[i] = (el_native_t)0.0f;
  return z;
}

// ---- the factors, once per launch: FP[2 (hi, lo)][RP][Cin + N] element planes -- columns q < Cin hold A_cat[j][q], columns
// Cin + n hold the block-diagonal Bbd[n][j] (B_i[n][j - i r] on group i's rows, else 0); rows j >= R are zeros.
__global__ void __launch_bounds__(256) lora_fac_kernel(LoraArgs a) {
  const int Q = a.Cin + a.N;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)a.RP * Q) return;
  const int j = (int)(idx / Q), q = (int)(idx % Q);
  float v = 0.0f;
  if (q < a.Cin) {
    if (j < a.R) v = a.A[(size_t)j * a.Cin + q];
  } else {
    const int n = q - a.Cin, jj = j - (n / a.Ng) * a.r;
    if (jj >= 0 && jj < a.r) v = a.B[(size_t)n * a.r + jj];
  }
  const el_t hi = f32_to_el(v);
  a.FP[idx] = hi;
  a.FP[idx + (size_t)a.RP * Q] = f32_to_el(v - el_to_f32(hi));
}

// ---- pass 1: H_cat = X . A_cat^T and G_cat = dY . Bbd for 128 rows (a 32-row tile per wave), stored transposed as (hi,
// lo) element planes.  Both operands straight from memory into registers (16 B per lane and k step: a row of X / dY, a
// row of FP, which every workgroup shares from L2): no LDS, no barrier.
template <int NJB>
__global__ void __launch_bounds__(256) lora_hg_kernel(LoraArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * kHgRows + wave * 32;
  const int mrow = m0 + (lane & 31);
  const int kofs = (lane >> 5) * 8;
  const bool live = mrow < a.M;
  const int Q = a.Cin + a.N;
  const size_t flo = (size_t)a.RP * Q;
  for (int which = 0; which < 2; ++which) {             // 0: H from X and A_cat; 1: G from dY and the block-diagonal B
    const int K = which == 0 ? a.Cin : a.N;
    const el_t* src = which == 0 ? a.X + (size_t)(live ? mrow : 0) * a.ldx : a.dY + (size_t)(live ? mrow : 0) * a.ldy;
    const el_t* fac = a.FP + (size_t)(lane & 31) * Q + (which == 0 ? 0 : a.Cin) + kofs;
    f32x16 acc[NJB];
#pragma unroll
    for (int jb = 0; jb < NJB; ++jb)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[jb][v] = 0.0f;
    for (int k0 = 0; k0 < K; k0 += 64) {
      elx8 x[4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) x[ks] = live ? ld8(src + k0 + ks * 16 + kofs) : zero8();
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int jb = 0; jb < NJB; ++jb) {
          const el_t* f = fac + (size_t)jb * 32 * Q + k0 + ks * 16;
          acc[jb] = mfma_32x32x16(x[ks], ld8(f), acc[jb]);
          acc[jb] = mfma_32x32x16(x[ks], ld8(f + flo), acc[jb]);
        }
    }
    // acc[jb][v] = row m0 + 8 (v / 4) + 4 (lane / 32) + v % 4, column jb * 32 + lane % 32: four consecutive rows per store
    el_t* dst = which == 0 ? a.HT : a.GT;
#pragma unroll
    for (int jb = 0; jb < NJB; ++jb) {
      el_t* col = dst + (size_t)(jb * 32 + (lane & 31)) * a.Mp + m0 + (lane >> 5) * 4;
      const size_t lo_off = (size_t)a.RP * a.Mp;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        el_t h[4], l[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          h[i] = f32_to_el(acc[jb][q * 4 + i]);
          l[i] = f32_to_el(acc[jb][q * 4 + i] - el_to_f32(h[i]));
        }
        *(uint2*)(col + q * 8) = make_uint2((uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16));
        *(uint2*)(col + lo_off + q * 8) =
            make_uint2((uint32_t)l[0] | ((uint32_t)l[1] << 16), (uint32_t)l[2] | ((uint32_t)l[3] << 16));
      }
    }
  }
}

// ---- pass 2: per (row slab, 64-column chunk of [X | dY]) the fp32 partial [RP][64] of L^T . T over the slab's rows.
template <int NJB>
__global__ void __launch_bounds__(256) lora_part_kernel(LoraArgs a) {
  __shared__ __attribute__((aligned(16))) el_t tile[kSub * kLdsPitch];
  __shared__ float red[NJB * 32 * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int slab = blockIdx.y, q0 = blockIdx.x * 64;     // (the chunks of one slab are dispatched together: its L rows
                                                        //  are read from cache after the first chunk)
  const bool isA = q0 < a.Cin;
  const el_t* T = isA ? a.X + q0 : a.dY + (q0 - a.Cin);
  const int ldt = isA ? a.ldx : a.ldy;
  const el_t* L = isA ? a.GT : a.HT;
  const int r0 = slab * a.rows_per_slab;
  const int r1 = r0 + a.rows_per_slab;                  // (<= Mp: L rows beyond M are zeros, T rows beyond M read as zeros)
  f32x16 acc[NJB][2];
#pragma unroll
  for (int jb = 0; jb < NJB; ++jb)
#pragma unroll
    for (int qb = 0; qb < 2; ++qb)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[jb][qb][v] = 0.0f;
  const int kofs = (lane >> 5) * 8;
  for (int ms = r0; ms < r1; ms += kSub) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {                       // T[64 rows][64 columns] -> LDS, 16 B per thread and step
      const int row = (tid >> 3) + i * 32, seg = (tid & 7) * 8;
      const int m = ms + row;
      elx8 v = m < a.M ? ld8(T + (size_t)m * ldt + seg) : zero8();
      *(elx8*)&tile[row * kLdsPitch + seg] = v;
    }
    __syncthreads();
    const int mw = wave * 16;                           // this wave's 16 rows of the sub-block: one MFMA k step
    elx8 tb[2];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb)
#pragma unroll
      for (int t = 0; t < 8; ++t)
        tb[qb][t] = __builtin_bit_cast(el_native_t, tile[(mw + kofs + t) * kLdsPitch + qb * 32 + (lane & 31)]);
#pragma unroll
    for (int jb = 0; jb < NJB; ++jb) {
      const el_t* lp = L + (size_t)(jb * 32 + (lane & 31)) * a.Mp + ms + mw + kofs;
      const elx8 lh = ld8(lp), ll = ld8(lp + (size_t)a.RP * a.Mp);
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) {
        acc[jb][qb] = mfma_32x32x16(lh, tb[qb], acc[jb][qb]);
        acc[jb][qb] = mfma_32x32x16(ll, tb[qb], acc[jb][qb]);
      }
    }
  }
  // the four waves' partials, added in wave order
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int jb = 0; jb < NJB; ++jb)
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
#pragma unroll
          for (int v = 0; v < 16; ++v) {
            const int j = jb * 32 + (v >> 2) * 8 + (lane >> 5) * 4 + (v & 3), q = qb * 32 + (lane & 31);
            float& dst = red[j * 64 + q];
            dst = w == 0 ? acc[jb][qb][v] : dst + acc[jb][qb][v];
          }
    }
    __syncthreads();
  }
  const int Q = a.Cin + a.N;
  float* out = a.part + (size_t)slab * a.RP * Q + q0;
  for (int e = tid; e < NJB * 32 * 64; e += 256) out[(size_t)(e >> 6) * Q + (e & 63)] = red[e];
}

// ---- pass 3: dA / dB = s . (sum of the slab partials in slab order); only the R valid rows, dB's diagonal blocks.
__global__ void __launch_bounds__(256) lora_reduce_kernel(LoraArgs a) {
  const int Q = a.Cin + a.N;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)a.R * Q) return;
  const int j = (int)(idx / Q), q = (int)(idx % Q);
  int n = -1, jj = 0;
  if (q >= a.Cin) {
    n = q - a.Cin;
    jj = j - (n / a.Ng) * a.r;
    if (jj < 0 || jj >= a.r) return;                    // off the block diagonal
  }
  const float* p = a.part + (size_t)j * Q + q;
  float s = 0.0f;
  for (int k = 0; k < a.slabs; ++k) s += p[(size_t)k * a.RP * Q];
  s *= a.scale;
  if (n < 0) a.dA[(size_t)j * a.Cin + q] = s;
  else a.dB[(size_t)n * a.r + jj] = s;
}

// W' = W + s . B . A in fp32 (torch layout [N][Cin]); one thread per element, the r products in index order.
__global__ void __launch_bounds__(256) lora_merge_kernel(const void* W, int w_dtype, const float* A, const float* B, int N,
                                                         int Cin, int r, float scale, float* out) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)N * Cin) return;
  const int n = (int)(idx / Cin), c = (int)(idx % Cin);
  float acc = 0.0f;
  for (int j = 0; j < r; ++j) acc = __builtin_fmaf(B[(size_t)n * r + j], A[(size_t)j * Cin + c], acc);
  float w;
  if (w_dtype == 0) w = ((const float*)W)[idx];
  else if (w_dtype == 2) w = bf16_to_f32(((const bf16_t*)W)[idx]);
  else w = (float)__builtin_bit_cast(_Float16, ((const uint16_t*)W)[idx]);
  out[idx] = __builtin_fmaf(scale, acc, w);
}

// The launch plan: a pure function of (M, Cin, N, g, r).  Row slabs are multiples of 128 rows (lora_hg_kernel's workgroup),
// at least 1024 rows each, and few enough that the fp32 slab partials stay within 16 MiB.
struct LoraPlan {
  int R, RP, slabs, rows_per_slab, Mp;
};

LoraPlan lora_plan(int M, int Cin, int N, int g, int r) {
  LoraPlan p;
  p.R = g * r;
  p.RP = (p.R + 31) / 32 * 32;
  const long per_slab = (long)p.RP * (Cin + N) * 4;
  long cap = (16L << 20) / per_slab;
  if (cap < 1) cap = 1;
  long by_rows = (M + 1023) / 1024;
  long n = by_rows < cap ? by_rows : cap;
  if (n < 1) n = 1;
  p.rows_per_slab = (int)(((M + n - 1) / n + kHgRows - 1) / kHgRows * kHgRows);
  p.slabs = (M + p.rows_per_slab - 1) / p.rows_per_slab;
  p.Mp = p.slabs * p.rows_per_slab;
  return p;
}

size_t lora_scratch_parts(const LoraPlan& p, int Cin, int N, size_t* off_gt, size_t* off_fp, size_t* off_part) {
  const size_t ht = ((size_t)2 * p.RP * p.Mp * 2 + 255) / 256 * 256;      // hi and lo planes
  const size_t fp = ((size_t)2 * p.RP * (Cin + N) * 2 + 255) / 256 * 256;
  *off_gt = ht;
  *off_fp = 2 * ht;
  *off_part = 2 * ht + fp;
  return 2 * ht + fp + (size_t)p.slabs * p.RP * (Cin + N) * 4;
}

int lora_check(const ctrlv_lora_desc* d) {
  CTRLV_CHECK_ARG(d != nullptr, "lora_grad: null descriptor");
  CTRLV_CHECK_SHAPE(d->M > 0 && d->g >= 1 && d->r >= 4 && d->r <= 64 && d->r % 4 == 0 && d->g * d->r <= 192,
                    "lora_grad: need M > 0, rank r a multiple of 4 in [4, 64] and g * r <= 192 (M %d, g %d, r %d)", d->M,
                    d->g, d->r);
  CTRLV_CHECK_SHAPE(d->Cin > 0 && d->Cin % 64 == 0 && d->N > 0 && d->N % d->g == 0 && (d->N / d->g) % 64 == 0,
                    "lora_grad: Cin %d and the group width N / g (N %d, g %d) must be multiples of 64", d->Cin, d->N, d->g);
  CTRLV_CHECK_SHAPE(d->ldx >= d->Cin && d->ldx % 8 == 0 && d->ldy >= d->N && d->ldy % 8 == 0,
                    "lora_grad: row pitches ldx %d / ldy %d must cover the rows and be multiples of 8", d->ldx, d->ldy);
  return CTRLV_OK;
}

template <int NJB>
void lora_launch(const LoraArgs& a, hipStream_t s) {
  const long nf = (long)a.RP * (a.Cin + a.N);
  hipLaunchKernelGGL(lora_fac_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(lora_hg_kernel<NJB>, dim3(a.Mp / kHgRows), dim3(256), 0, s, a);
  hipLaunchKernelGGL(lora_part_kernel<NJB>, dim3((a.Cin + a.N) / 64, a.slabs), dim3(256), 0, s, a);
}

}  // namespace

extern "C" size_t ctrlv_lora_grad_scratch_bytes(const ctrlv_lora_desc* d) {
  if (lora_check(d) != CTRLV_OK) return 0;
  const LoraPlan p = lora_plan(d->M, d->Cin, d->N, d->g, d->r);
  size_t og, of, op;
  return lora_scratch_parts(p, d->Cin, d->N, &og, &of, &op);
}

extern "C" int ctrlv_lora_grad(const ctrlv_lora_desc* d, void* scratch, size_t scratch_bytes, ctrlv_stream_t stream) {
  const int rc = lora_check(d);
  if (rc != CTRLV_OK) return rc;
  CTRLV_CHECK_ARG(d->X && d->dY && d->A && d->B && d->dA && d->dB && scratch, "lora_grad: null pointer");
  CTRLV_CHECK_ARG(((uintptr_t)d->X | (uintptr_t)d->dY | (uintptr_t)scratch) % 16 == 0,
                  "lora_grad: X, dY and scratch must be 16-byte aligned");
  const LoraPlan p = lora_plan(d->M, d->Cin, d->N, d->g, d->r);
  size_t og, of, op;
  const size_t need = lora_scratch_parts(p, d->Cin, d->N, &og, &of, &op);
  CTRLV_CHECK_ARG(scratch_bytes >= need, "lora_grad: scratch of %zu bytes, needs %zu (ctrlv_lora_grad_scratch_bytes)",
                  scratch_bytes, need);
  LoraArgs a;
  a.X = (const el_t*)d->X; a.dY = (const el_t*)d->dY; a.A = d->A; a.B = d->B; a.dA = d->dA; a.dB = d->dB;
  a.HT = (el_t*)scratch; a.GT = (el_t*)((char*)scratch + og);
  a.FP = (el_t*)((char*)scratch + of); a.part = (float*)((char*)scratch + op);
  a.M = d->M; a.Cin = d->Cin; a.N = d->N; a.Ng = d->N / d->g; a.g = d->g; a.r = d->r; a.R = p.R; a.RP = p.RP; a.Mp = p.Mp;
  a.slabs = p.slabs; a.rows_per_slab = p.rows_per_slab; a.ldx = d->ldx; a.ldy = d->ldy; a.scale = d->scale;
  hipStream_t s = (hipStream_t)stream;
  switch (p.RP / 32) {
    case 1: lora_launch<1>(a, s); break;
    case 2: lora_launch<2>(a, s); break;
    case 3: lora_launch<3>(a, s); break;
    case 4: lora_launch<4>(a, s); break;
    case 5: lora_launch<5>(a, s); break;
    default: lora_launch<6>(a, s); break;
  }
  CTRLV_LAUNCH_CHECK();
  const long tot = (long)p.R * (d->Cin + d->N);
  hipLaunchKernelGGL(lora_reduce_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, a);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

extern "C" int ctrlv_lora_merge(const void* W, int w_dtype, const float* A, const float* B, int N, int Cin, int r, float scale,
                                float* out, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(W && A && B && out, "lora_merge: null pointer");
  CTRLV_CHECK_ARG(w_dtype >= 0 && w_dtype <= 2, "lora_merge: W dtype code %d (0 fp32, 1 fp16, 2 bf16)", w_dtype);
  CTRLV_CHECK_SHAPE(N > 0 && Cin > 0 && r > 0, "lora_merge: bad shape N %d Cin %d r %d", N, Cin, r);
  const long tot = (long)N * Cin;
  hipLaunchKernelGGL(lora_merge_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, W, w_dtype,
                     A, B, N, Cin, r, scale, out);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}
