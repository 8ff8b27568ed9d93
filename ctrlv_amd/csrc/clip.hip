// The CLIP vision tower's own kernels (transformers CLIPVisionModelWithProjection: ViT-H/14 of SVD's image_encoder/, called
// by pipeline_video_control.py:220 and src/ctrlv/utils/util.py:97-125).  Everything dense runs on ctrlv_gemm and the norms on
// ctrlv_layernorm; this unit adds what they cannot express:
//
//   ctrlv_attention_tokens  self-attention over the S tokens of an image at ANY 1 <= S <= 4096 and head_dim 16..128 (ViT-H:
//                           257 tokens, 16 heads of 80)
//   ctrlv_clip_patch_rows   NCHW pixels -> one GEMM row per patch (the stride-`patch` convolution as a plain GEMM)
//   ctrlv_clip_tokens       class token + patch rows + position table -> token rows
//   ctrlv_act_rows          erf-GELU / quick-GELU in place
//
// ATTENTION.  One wave per (image, head, block of 32 queries); key tiles of 32.  Both products use v_mfma_f32_32x32x16:
//   scores  S^T = K . Q^T   A = K rows (keys), B = Q rows: head_dim / 16 K-steps -- d = 80 is 5 steps, nothing padded; each
//                           lane owns ONE query (the accumulator's column) and holds 16 of the tile's 32 keys, the other
//                           half-wave the other 16: softmax statistics are 16 registers + one cross-half exchange
//   output  O^T += V^T . P  the exponentiated tile, packed to elements, IS the B operand (guide: "accumulator tile as the
//                           next MFMA's operand"); O^T has ceil(head_dim / 32) blocks of 32 rows -- d = 80 computes 96 rows,
//                           16 of them on zero padding.
// Why 32x32x16 and not 16x16x32 (5 exact output blocks at d = 80): with 32x32x16 the score accumulator feeds P.V with no lane
// movement and no LDS round trip, and one shape means one fragment layout to get right; the price is 1/6 more MFMA work in
// P.V at d = 80 (11 instead of 10 MFMAs per tile) on a workload of 16 x 257^2 scores per image that is bound by launch
// latency, not by the matrix pipe.  16x16x32 scores would put a query's 32 keys on 4 lane groups (two more exchanges per
// statistic) and need P transposed through LDS.
// K fragments are 16-byte global loads (a fragment is 8 consecutive channels of one key row); V needs its KEY index contiguous
// per lane, so a V tile is written transposed into LDS ([channel][key slot], the slots in the permuted k order of the
// accumulator-as-operand idiom) and read back as one ds_read_b128 per fragment.  Keys >= S: K rows are clamped to row S - 1 for
// the load (never out of the image) and their scores set to -inf before the statistics; V rows are written as zeros (P is 0
// there and 0 x NaN must not happen).  Queries >= S are loaded as zeros and never stored.  A workgroup touches one image only,
// sums in a fixed order and uses no atomics: results do not depend on n_img and repeat bit for bit.
#include <math.h>

#include "common.h"

namespace {

constexpr int kVtPitch = 40;   // elements per [channel] row of the transposed V tile: 32 key slots + 8 (80 B: 16-B aligned,
                               // consecutive channels start 20 banks apart)

// slot of key `k` (0..31) of a tile in the B-operand k order: element j of lane half h in K-step s is key
// 16 s + 8 (j >> 2) + 4 h + (j & 3) and sits at slot 16 s + 8 h + j
__device__ __forceinline__ int key_slot(int k) {
  const int r = k & 15;
  return (k & 16) + 8 * ((r >> 2) & 1) + 4 * (r >> 3) + (r & 3);
}

template <int KS>   // head_dim / 16
__global__ __launch_bounds__(64) void attn_tokens_kernel(const el_t* __restrict__ qkv, el_t* __restrict__ out, int S, int C,
                                                         float scale_log2) {
  constexpr int D = KS * 16, NDB = (KS + 1) / 2, DP = NDB * 32;
  __shared__ __attribute__((aligned(16))) el_t vt[DP * kVtPitch];
  const int lane = threadIdx.x, r32 = lane & 31, h = lane >> 5;
  const int head = blockIdx.y, img = blockIdx.z;
  const size_t ld = 3 * (size_t)C;
  const el_t* qp = qkv + (size_t)img * S * ld + head * D;
  const el_t* kp = qp + C;
  const el_t* vp = qp + 2 * C;

  // the padding channels [D, DP) stay zero for the whole kernel; the rest is overwritten by every tile
  for (int i = lane; i < DP * kVtPitch / 8; i += 64) ((uint4*)vt)[i] = make_uint4(0, 0, 0, 0);

  const int qrow = blockIdx.x * 32 + r32;
  elx8 qf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (qrow < S) v = *(const uint4*)(qp + qrow * ld + 16 * ks + 8 * h);
    qf[ks] = __builtin_bit_cast(elx8, v);
  }

  // V tile: 32 keys x (D / 8) 16-byte chunks = KS chunks per lane, consecutive lanes on consecutive chunks of a row
  uint4 vreg[KS];
  auto load_v = [&](int t) {
#pragma unroll
    for (int i = 0; i < KS; ++i) {
      const int c = i * 64 + lane, key = c / (2 * KS), dc = c % (2 * KS);
      const int krow = t * 32 + key;
      vreg[i] = make_uint4(0, 0, 0, 0);
      if (krow < S) vreg[i] = *(const uint4*)(vp + krow * ld + dc * 8);
    }
  };
  auto store_v = [&]() {
#pragma unroll
    for (int i = 0; i < KS; ++i) {
      const int c = i * 64 + lane, key = c / (2 * KS), dc = c % (2 * KS);
      const int slot = key_slot(key);
      const uint32_t w[4] = {vreg[i].x, vreg[i].y, vreg[i].z, vreg[i].w};
#pragma unroll
      for (int e = 0; e < 8; ++e) vt[(dc * 8 + e) * kVtPitch + slot] = (el_t)(w[e >> 1] >> (16 * (e & 1)));
    }
  };

  f32x16 oacc[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db)
#pragma unroll
    for (int e = 0; e < 16; ++e) oacc[db][e] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;   // l_run: this half-wave's part of the row sum (both halves share m_run)

  const int nt = (S + 31) / 32;
  load_v(0);
  __syncthreads();                        // the zero fill is complete
  store_v();
  for (int t = 0; t < nt; ++t) {
    __syncthreads();                      // tile t of V^T is in LDS
    const int krow = min(t * 32 + r32, S - 1);
    elx8 kf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) kf[ks] = __builtin_bit_cast(elx8, *(const uint4*)(kp + krow * ld + 16 * ks + 8 * h));
    if (t + 1 < nt) load_v(t + 1);

    f32x16 s;
#pragma unroll
    for (int e = 0; e < 16; ++e) s[e] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) s = mfma_32x32x16(kf[ks], qf[ks], s);

    // register e of the tile is key t * 32 + 8 (e >> 2) + 4 h + (e & 3) of query r32
    const int key0 = t * 32 + 4 * h;
    float mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int key = key0 + 8 * (e >> 2) + (e & 3);
      s[e] = key < S ? s[e] * scale_log2 : -INFINITY;
      mx = fmaxf(mx, s[e]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m_run, mx);
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);     // first tile: exp2(-inf) = 0
    float lsum = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      s[e] = __builtin_amdgcn_exp2f(s[e] - m_new);
      lsum += s[e];
    }
    l_run = l_run * alpha + lsum;
    m_run = m_new;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int e = 0; e < 16; ++e) oacc[db][e] *= alpha;

#pragma unroll
    for (int st = 0; st < 2; ++st) {
      elx8 pf;
#pragma unroll
      for (int j = 0; j < 8; ++j) pf[j] = (el_native_t)s[8 * st + j];
#pragma unroll
      for (int db = 0; db < NDB; ++db) {
        const elx8 vf = __builtin_bit_cast(elx8, *(const uint4*)(vt + (db * 32 + r32) * kVtPitch + 16 * st + 8 * h));
        oacc[db] = mfma_32x32x16(vf, pf, oacc[db]);
      }
    }
    __syncthreads();                      // every read of tile t is done
    if (t + 1 < nt) store_v();
  }

  const float l = l_run + __shfl_xor(l_run, 32);
  const float inv = 1.0f / l;
  if (qrow < S) {
    el_t* op = out + ((size_t)img * S + qrow) * C + head * D;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d0 = db * 32 + 8 * g + 4 * h;        // registers 4 g .. 4 g + 3 are channels d0 .. d0 + 3
        if (d0 < D) {
          uint2 w;
          w.x = pack_elx2(oacc[db][4 * g] * inv, oacc[db][4 * g + 1] * inv);
          w.y = pack_elx2(oacc[db][4 * g + 2] * inv, oacc[db][4 * g + 3] * inv);
          *(uint2*)(op + d0) = w;
        }
      }
  }
}

template <int KS>
int launch_attn_tokens(const void* qkv, void* out, int n_img, int S, int C, hipStream_t st) {
  const float scale_log2 = 1.44269504088896340736f / sqrtf((float)(KS * 16));
  attn_tokens_kernel<KS><<<dim3((S + 31) / 32, C / (KS * 16), n_img), 64, 0, st>>>((const el_t*)qkv, (el_t*)out, S, C, scale_log2);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

// ---------------------------------------------------------------------------------------------- patch rows
__device__ __forceinline__ float load_px(const void* p, int dtype, size_t i) {
  if (dtype == 0) return ((const float*)p)[i];
  if (dtype == 1) return (float)__builtin_bit_cast(_Float16, ((const uint16_t*)p)[i]);
  return bf16_to_f32(((const bf16_t*)p)[i]);
}

// one thread = 8 consecutive columns of one patch row (one 16-byte store); column = (c, dy, dx)
__global__ __launch_bounds__(256) void clip_patch_rows_kernel(const void* __restrict__ px, int dtype, int Hpx, int Wpx, int patch,
                                                              int P, el_t* __restrict__ rows, int ld, size_t n_chunks) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_chunks) return;
  const int cpr = ld / 8;
  const size_t row = idx / cpr;
  const int col0 = (int)(idx % cpr) * 8;
  const int img = (int)(row / P), p = (int)(row % P);
  const int wp = Wpx / patch, py = p / wp, pxx = p % wp, pp = patch * patch;
  float f[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int col = col0 + e;
    f[e] = 0.f;
    if (col < 3 * pp) {
      const int c = col / pp, rem = col % pp, dy = rem / patch, dx = rem % patch;
      f[e] = load_px(px, dtype, (((size_t)img * 3 + c) * Hpx + py * patch + dy) * Wpx + pxx * patch + dx);
    }
  }
  *(uint4*)(rows + row * ld + col0) = pack_elx8(f);
}

// ---------------------------------------------------------------------------------------------- token rows
__global__ __launch_bounds__(256) void clip_tokens_kernel(const el_t* __restrict__ patch_out, const float* __restrict__ cls,
                                                          const float* __restrict__ pos, int P, int C, el_t* __restrict__ out,
                                                          size_t n_chunks) {
#pragma clang fp contract(off)
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_chunks) return;
  const int cpr = C / 8;
  const size_t row = idx / cpr;
  const int c0 = (int)(idx % cpr) * 8;
  const size_t img = row / (P + 1);
  const int tok = (int)(row % (P + 1));
  float f[8];
  if (tok == 0) {
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = cls[c0 + e];
  } else {
    unpack_elx8(*(const uint4*)(patch_out + (img * P + tok - 1) * C + c0), f);
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = f[e] + pos[(size_t)tok * C + c0 + e];
  *(uint4*)(out + row * C + c0) = pack_elx8(f);
}

// ---------------------------------------------------------------------------------------------- activations
template <int KIND>
__global__ __launch_bounds__(256) void act_rows_kernel(el_t* __restrict__ x, int N, int ld, size_t n_chunks) {
#pragma clang fp contract(off)
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_chunks) return;
  const int cpr = N / 8;
  el_t* p = x + (idx / cpr) * ld + (idx % cpr) * 8;
  float f[8];
  unpack_elx8(*(const uint4*)p, f);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float v = f[e];
    if (KIND == 0) {
      f[e] = (v * 0.5f) * (1.0f + erff(v * 0.70710678118654752440f));      // x Phi(x), the erf form of nn.GELU()
    } else {
      f[e] = v * (1.0f / (1.0f + expf(-(1.702f * v))));                    // quick-GELU  x sigmoid(1.702 x)
    }
  }
  *(uint4*)p = pack_elx8(f);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int ctrlv_attention_tokens(const void* qkv, void* out, int n_img, int S, int C, int head_dim, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(qkv && out, "attention_tokens: null pointer");
  CTRLV_CHECK_ARG(aligned16(qkv) && aligned16(out), "attention_tokens: qkv and out must be 16-byte aligned");
  CTRLV_CHECK_SHAPE(head_dim >= 16 && head_dim <= 128 && head_dim % 16 == 0,
                    "attention_tokens: head_dim=%d must be a multiple of 16 in [16, 128]", head_dim);
  CTRLV_CHECK_SHAPE(C > 0 && C % head_dim == 0 && C / head_dim <= 65535, "attention_tokens: C=%d must be a multiple of head_dim=%d",
                    C, head_dim);
  CTRLV_CHECK_SHAPE(S >= 1 && S <= 4096, "attention_tokens: S=%d must be in [1, 4096] tokens", S);
  CTRLV_CHECK_SHAPE(n_img >= 1 && n_img <= 65535, "attention_tokens: n_img=%d must be in [1, 65535]", n_img);
  hipStream_t st = (hipStream_t)stream;
  switch (head_dim / 16) {
    case 1: return launch_attn_tokens<1>(qkv, out, n_img, S, C, st);
    case 2: return launch_attn_tokens<2>(qkv, out, n_img, S, C, st);
    case 3: return launch_attn_tokens<3>(qkv, out, n_img, S, C, st);
    case 4: return launch_attn_tokens<4>(qkv, out, n_img, S, C, st);
    case 5: return launch_attn_tokens<5>(qkv, out, n_img, S, C, st);
    case 6: return launch_attn_tokens<6>(qkv, out, n_img, S, C, st);
    case 7: return launch_attn_tokens<7>(qkv, out, n_img, S, C, st);
    default: return launch_attn_tokens<8>(qkv, out, n_img, S, C, st);
  }
}

extern "C" int ctrlv_clip_patch_rows(const void* pixels, int dtype_code, int n, int Hpx, int Wpx, int patch, void* rows, int ld,
                                     ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(pixels && rows, "clip_patch_rows: null pointer");
  if (dtype_code < 0 || dtype_code > 2) {
    ctrlv_set_error("clip_patch_rows: dtype code %d (0 fp32, 1 fp16, 2 bf16)", dtype_code);
    return CTRLV_E_BAD_DTYPE;
  }
  CTRLV_CHECK_ARG(aligned16(rows), "clip_patch_rows: rows must be 16-byte aligned");
  CTRLV_CHECK_SHAPE(n > 0 && patch > 0 && patch <= 64 && Hpx > 0 && Wpx > 0 && Hpx % patch == 0 && Wpx % patch == 0,
                    "clip_patch_rows: image %dx%d must be whole patches of %d", Hpx, Wpx, patch);
  CTRLV_CHECK_SHAPE(ld % 8 == 0 && ld >= 3 * patch * patch, "clip_patch_rows: ld=%d must be a multiple of 8, >= 3 * patch^2 = %d", ld,
                    3 * patch * patch);
  const int P = (Hpx / patch) * (Wpx / patch);
  const size_t n_chunks = (size_t)n * P * (ld / 8);
  CTRLV_CHECK_SHAPE((n_chunks + 255) / 256 < (1u << 31), "clip_patch_rows: too many rows");
  clip_patch_rows_kernel<<<(unsigned)((n_chunks + 255) / 256), 256, 0, (hipStream_t)stream>>>(pixels, dtype_code, Hpx, Wpx, patch, P,
                                                                                            (el_t*)rows, ld, n_chunks);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

extern "C" int ctrlv_clip_tokens(const void* patch_out, const float* class_emb, const float* pos_emb, int n, int P, int C, void* out,
                                 ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(patch_out && class_emb && pos_emb && out, "clip_tokens: null pointer");
  CTRLV_CHECK_ARG(aligned16(patch_out) && aligned16(out), "clip_tokens: patch_out and out must be 16-byte aligned");
  CTRLV_CHECK_SHAPE(n > 0 && P > 0 && C > 0 && C % 8 == 0, "clip_tokens: C=%d must be a multiple of 8 (n=%d, P=%d)", C, n, P);
  const size_t n_chunks = (size_t)n * (P + 1) * (C / 8);
  CTRLV_CHECK_SHAPE((n_chunks + 255) / 256 < (1u << 31), "clip_tokens: too many rows");
  clip_tokens_kernel<<<(unsigned)((n_chunks + 255) / 256), 256, 0, (hipStream_t)stream>>>((const el_t*)patch_out, class_emb, pos_emb, P,
                                                                                        C, (el_t*)out, n_chunks);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

extern "C" int ctrlv_act_rows(void* x, int M, int N, int ld, int kind, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(x != nullptr, "act_rows: null pointer");
  CTRLV_CHECK_ARG(kind == 0 || kind == 1, "act_rows: kind %d (0 erf-GELU, 1 quick-GELU)", kind);
  CTRLV_CHECK_ARG(aligned16(x), "act_rows: x must be 16-byte aligned");
  CTRLV_CHECK_SHAPE(M > 0 && N > 0 && N % 8 == 0 && ld % 8 == 0 && ld >= N, "act_rows: N=%d and ld=%d must be multiples of 8, ld >= N",
                    N, ld);
  const size_t n_chunks = (size_t)M * (N / 8);
  CTRLV_CHECK_SHAPE((n_chunks + 255) / 256 < (1u << 31), "act_rows: too many rows");
  const unsigned grid = (unsigned)((n_chunks + 255) / 256);
  if (kind == 0)
    act_rows_kernel<0><<<grid, 256, 0, (hipStream_t)stream>>>((el_t*)x, N, ld, n_chunks);
  else
    act_rows_kernel<1><<<grid, 256, 0, (hipStream_t)stream>>>((el_t*)x, N, ld, n_chunks);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}
