// The SVD VAE (AutoencoderKLTemporalDecoder) as ONE C call per half (include/ctrlv_hip.h "VAE as ONE call each"): what
// clip_plan.hip is for the CLIP tower.  The walks are those of the per-op Python executors (models/vae_encoder_hip.py encode
// with native_down, models/vae_decoder_hip.py decode), launch for launch and operand for operand, over packed, library-owned
// weights -- so a host in any language can run the encode of the conditioning image / the bbox frames and the decode of the
// generated frames.  Nothing here is a torch op: the encoder's down-samplers are one pad_br launch each, quant_conv and the
// posterior are ctrlv_vae_posterior.
//
// Workspace: the walk is static, so the buffers are laid out by running the SAME walk function dry (no launches) over a
// first-fit free list with the Python executors' allocation / release order; ctrlv_vae_plan_workspace_bytes is that dry
// run's peak and the forward repeats it on the caller's pointer.  One stream, one chain; the only non-kernel nodes are the
// memsets of the zero-padded input channels.
#include <math.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"

#define TRY(expr)                      \
  do {                                 \
    const int rc__ = (expr);           \
    if (rc__ != CTRLV_OK) return rc__; \
  } while (0)

namespace {

struct VConv { el_t* w = nullptr; float* b = nullptr; int n = 0, k = 0; };      // packed [n (rows, x32), k] + fp32 bias [n]
struct VNorm { float* g = nullptr; float* b = nullptr; };
struct VRes {
  int cin = 0, cout = 0;
  bool temporal = false, shortcut = false;
  VNorm n1, n2, tn1, tn2;
  VConv c1, c2, sc, tc1, tc2;
  float mix = 0.f;                         // sigmoid(time_mixer.mix_factor)
};
struct VAttn { VNorm gn; VConv q, k, v_rows, o; };   // v_rows: to_v.weight as the A operand of V^T (no bias: folded into o.b)
struct VLevel { std::vector<VRes> res; VConv resample; bool has_resample = false; };

constexpr long kLimit32 = (1L << 32) - (1L << 24);   // the kernels address a tensor with 32-bit byte offsets

}  // namespace

struct ctrlv_vae_plan {
  ctrlv_vae_config cfg;
  int device = 0;
  bool loaded = false;
  long limit = kLimit32;
  std::vector<void*> owned;
  // encoder
  VConv e_cin; int e_cp = 0, e_kp = 0;
  std::vector<VLevel> e_down;
  VRes e_mid[2];
  VAttn e_attn;
  VNorm e_gno;
  VConv e_cout;
  float* qw = nullptr;                     // quant_conv [2L, 2L] / [2L] fp32
  float* qb = nullptr;
  // decoder
  VConv d_cin; int d_cp = 0, d_kp = 0;
  std::vector<VRes> d_mid;
  VAttn d_attn;
  std::vector<VLevel> d_up;
  VNorm d_gno;
  VConv d_cout;
  float* tco_w = nullptr;                  // time_conv_out [o, c, t] / [o] fp32
  float* tco_b = nullptr;
};

const ctrlv_vae_config* ctrlv_vae_plan_info(const ctrlv_vae_plan* p, int* device, int* loaded) {
  if (device) *device = p->device;
  if (loaded) *loaded = p->loaded ? 1 : 0;
  return &p->cfg;
}

namespace {

__device__ __forceinline__ float vld_any(const void* p, int dtype, long i) {
  if (dtype == 0) return ((const float*)p)[i];
  if (dtype == 1) return (float)((const _Float16*)p)[i];
  return bf16_to_f32(((const bf16_t*)p)[i]);
}
// PyTorch conv / linear parameter [N, C, taps] -> dst[n * ldk + t * cslot + c] (dst pre-zeroed: row, slot and K padding):
// packing.pack_linear (taps 1), pack_conv3x3 (9), pack_conv_temporal (3), pack_conv_in (9, cslot = padded channel slot)
__global__ void vae_pack_kernel(const void* __restrict__ src, int dtype, long total, int C, int taps, el_t* __restrict__ dst,
                                int ldk, int cslot) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long nc = i / taps;
    const int t = (int)(i - nc * taps), c = (int)(nc % C);
    dst[(nc / C) * ldk + (long)t * cslot + c] = f32_to_el(vld_any(src, dtype, i));
  }
}
__global__ void vae_pack_f32_kernel(const void* __restrict__ src, int dtype, long total, float* __restrict__ dst) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x)
    dst[i] = vld_any(src, dtype, i);
}
inline unsigned vblocks(long total) { return (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096); }

float host_to_f32(const void* p, int dtype, long i) {
  if (dtype == 0) return ((const float*)p)[i];
  const uint16_t h = ((const uint16_t*)p)[i];
  uint32_t u;
  if (dtype == 2) {
    u = (uint32_t)h << 16;
  } else {                                 // IEEE half -> float
    const uint32_t s = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    if (e == 0) {
      if (m == 0) u = s;
      else { int sh = 0; uint32_t mm = m; while (!(mm & 0x400u)) { mm <<= 1; ++sh; } u = s | ((uint32_t)(113 - sh) << 23) | ((mm & 0x3ffu) << 13); }
    } else if (e == 31) u = s | 0x7f800000u | (m << 13);
    else u = s | ((e + 112u) << 23) | (m << 13);
  }
  float f;
  memcpy(&f, &u, 4);
  return f;
}

struct VLoader {
  ctrlv_vae_plan* p;
  std::unordered_map<std::string, const ctrlv_tensor_desc*> map;
  std::vector<void*> staged;

  int desc(const std::string& name, long numel, const ctrlv_tensor_desc** out) {
    auto it = map.find(name);
    if (it == map.end()) { ctrlv_set_error("vae_plan_load_weights: missing tensor '%s'", name.c_str()); return CTRLV_E_BAD_ARG; }
    const ctrlv_tensor_desc* t = it->second;
    if (t->numel != numel) {
      ctrlv_set_error("vae_plan_load_weights: '%s' has %ld elements, expected %ld", name.c_str(), (long)t->numel, numel);
      return CTRLV_E_BAD_SHAPE;
    }
    if (t->dtype < 0 || t->dtype > 2 || !t->data) {
      ctrlv_set_error("vae_plan_load_weights: '%s': dtype code %d / null data", name.c_str(), t->dtype);
      return CTRLV_E_BAD_DTYPE;
    }
    *out = t;
    return CTRLV_OK;
  }
  int find(const std::string& name, long numel, const void** src, int* dtype) {       // device pointer of the tensor
    const ctrlv_tensor_desc* t;
    TRY(desc(name, numel, &t));
    *dtype = t->dtype;
    if (t->on_device) { *src = t->data; return CTRLV_OK; }
    const size_t bytes = (size_t)t->numel * (t->dtype == 0 ? 4 : 2);
    void* d = nullptr;
    CTRLV_HIP_TRY(hipMalloc(&d, bytes));
    staged.push_back(d);
    CTRLV_HIP_TRY(hipMemcpy(d, t->data, bytes, hipMemcpyHostToDevice));
    *src = d;
    return CTRLV_OK;
  }
  int host(const std::string& name, long numel, std::vector<float>& out) {            // fp32 host copy of the tensor
    const ctrlv_tensor_desc* t;
    TRY(desc(name, numel, &t));
    const size_t bytes = (size_t)numel * (t->dtype == 0 ? 4 : 2);
    std::vector<char> raw(bytes);
    if (t->on_device) CTRLV_HIP_TRY(hipMemcpy(raw.data(), t->data, bytes, hipMemcpyDeviceToHost));
    else memcpy(raw.data(), t->data, bytes);
    out.resize(numel);
    for (long i = 0; i < numel; ++i) out[i] = host_to_f32(raw.data(), t->dtype, i);
    return CTRLV_OK;
  }
  int alloc(size_t bytes, void** out, bool zero) {
    void* d = nullptr;
    CTRLV_HIP_TRY(hipMalloc(&d, bytes ? bytes : 256));
    p->owned.push_back(d);
    if (zero) CTRLV_HIP_TRY(hipMemsetAsync(d, 0, bytes ? bytes : 256, nullptr));
    *out = d;
    return CTRLV_OK;
  }
  int vec(const std::string& name, long n, float** dst, long n_pad = 0) {
    TRY(alloc((size_t)(n_pad > n ? n_pad : n) * 4, (void**)dst, n_pad > n));
    const void* src;
    int dt;
    TRY(find(name, n, &src, &dt));
    vae_pack_f32_kernel<<<vblocks(n), 256, 0, nullptr>>>(src, dt, n, *dst);
    CTRLV_LAUNCH_CHECK();
    return CTRLV_OK;
  }
  int upload(const std::vector<float>& v, float** dst) {
    TRY(alloc(v.size() * 4, (void**)dst, false));
    CTRLV_HIP_TRY(hipMemcpy(*dst, v.data(), v.size() * 4, hipMemcpyHostToDevice));
    return CTRLV_OK;
  }
  // weight [N, C, taps] -> rows padded to 32, K = taps * cslot padded to kp (0: no K padding beyond the slots)
  int weight(const std::string& name, int N, int C, int taps, int cslot, int kp, VConv& cv) {
    cv.n = (N + 31) / 32 * 32;
    cv.k = kp ? kp : taps * cslot;
    TRY(alloc((size_t)cv.n * cv.k * 2, (void**)&cv.w, true));
    const void* src;
    int dt;
    const long total = (long)N * C * taps;
    TRY(find(name, total, &src, &dt));
    vae_pack_kernel<<<vblocks(total), 256, 0, nullptr>>>(src, dt, total, C, taps, cv.w, cv.k, cslot);
    CTRLV_LAUNCH_CHECK();
    return CTRLV_OK;
  }
  int conv(const std::string& mod, int N, int C, int taps, VConv& cv, bool pad_b = false) {
    TRY(weight(mod + ".weight", N, C, taps, C, taps == 1 ? (C + 63) / 64 * 64 : 0, cv));
    return vec(mod + ".bias", N, &cv.b, pad_b ? cv.n : 0);
  }
  int conv_in(const std::string& mod, int N, int C, VConv& cv, int* cp, int* kp) {       // packing.pack_conv_in + pad_bias
    *cp = (C + 7) / 8 * 8;
    *kp = (9 * *cp + 63) / 64 * 64;
    TRY(weight(mod + ".weight", N, C, 9, *cp, *kp, cv));
    return vec(mod + ".bias", N, &cv.b, cv.n);
  }
  int norm(const std::string& mod, int C, VNorm& nm) {
    TRY(vec(mod + ".weight", C, &nm.g));
    return vec(mod + ".bias", C, &nm.b);
  }
  int res2d(const std::string& mod, int cin, int cout, VRes& r) {
    r.cin = cin; r.cout = cout;
    TRY(norm(mod + ".norm1", cin, r.n1));
    TRY(conv(mod + ".conv1", cout, cin, 9, r.c1));
    TRY(norm(mod + ".norm2", cout, r.n2));
    TRY(conv(mod + ".conv2", cout, cout, 9, r.c2));
    r.shortcut = cin != cout;
    if (r.shortcut) TRY(conv(mod + ".conv_shortcut", cout, cin, 1, r.sc));
    return CTRLV_OK;
  }
  int res_st(const std::string& mod, int cin, int cout, VRes& r) {
    TRY(res2d(mod + ".spatial_res_block", cin, cout, r));
    r.temporal = true;
    const std::string t = mod + ".temporal_res_block";
    TRY(norm(t + ".norm1", cout, r.tn1));
    TRY(conv(t + ".conv1", cout, cout, 3, r.tc1));
    TRY(norm(t + ".norm2", cout, r.tn2));
    TRY(conv(t + ".conv2", cout, cout, 3, r.tc2));
    std::vector<float> m;
    TRY(host(mod + ".time_mixer.mix_factor", 1, m));
    r.mix = (float)(1.0 / (1.0 + exp(-(double)m[0])));
    return CTRLV_OK;
  }
  int attn(const std::string& mod, int C, VAttn& a) {
    TRY(norm(mod + ".group_norm", C, a.gn));
    TRY(conv(mod + ".to_q", C, C, 1, a.q));
    TRY(conv(mod + ".to_k", C, C, 1, a.k));
    TRY(weight(mod + ".to_v.weight", C, C, 1, C, 0, a.v_rows));
    TRY(weight(mod + ".to_out.0.weight", C, C, 1, C, 0, a.o));
    // folded output bias b_o + W_o . b_v (rows of P sum to one): fp64 on the host from the fp32 values, rounded once
    std::vector<float> wo, bo, bv;
    TRY(host(mod + ".to_out.0.weight", (long)C * C, wo));
    TRY(host(mod + ".to_out.0.bias", C, bo));
    TRY(host(mod + ".to_v.bias", C, bv));
    std::vector<float> fold(C);
    for (int o = 0; o < C; ++o) {
      double s = (double)bo[o];
      for (int c = 0; c < C; ++c) s += (double)wo[(size_t)o * C + c] * (double)bv[c];
      fold[o] = (float)s;
    }
    return upload(fold, &a.o.b);
  }
};

void free_owned(ctrlv_vae_plan* p) {
  for (void* d : p->owned) (void)hipFree(d);
  p->owned.clear();
  p->e_down.clear(); p->d_mid.clear(); p->d_up.clear();
  p->loaded = false;
}

int load_all(VLoader& L) {
  ctrlv_vae_plan* p = L.p;
  const ctrlv_vae_config& c = p->cfg;
  const int nb = c.n_blocks, top = c.block_out_channels[nb - 1], L2 = 2 * c.latent_channels;
  auto S = [](int i) { return std::to_string(i); };
  // ---- encoder
  TRY(L.conv_in("encoder.conv_in", c.block_out_channels[0], c.in_channels, p->e_cin, &p->e_cp, &p->e_kp));
  p->e_down.resize(nb);
  int prev = c.block_out_channels[0];
  for (int i = 0; i < nb; ++i) {
    const int ch = c.block_out_channels[i];
    VLevel& lv = p->e_down[i];
    lv.res.resize(c.layers_per_block);
    for (int j = 0; j < c.layers_per_block; ++j)
      TRY(L.res2d("encoder.down_blocks." + S(i) + ".resnets." + S(j), j == 0 ? prev : ch, ch, lv.res[j]));
    lv.has_resample = i != nb - 1;
    if (lv.has_resample) TRY(L.conv("encoder.down_blocks." + S(i) + ".downsamplers.0.conv", ch, ch, 9, lv.resample));
    prev = ch;
  }
  for (int j = 0; j < 2; ++j) TRY(L.res2d("encoder.mid_block.resnets." + S(j), top, top, p->e_mid[j]));
  TRY(L.attn("encoder.mid_block.attentions.0", top, p->e_attn));
  TRY(L.norm("encoder.conv_norm_out", top, p->e_gno));
  TRY(L.conv("encoder.conv_out", L2, top, 9, p->e_cout, true));
  TRY(L.vec("quant_conv.weight", (long)L2 * L2, &p->qw));
  TRY(L.vec("quant_conv.bias", L2, &p->qb));
  // ---- decoder
  TRY(L.conv_in("decoder.conv_in", top, c.latent_channels, p->d_cin, &p->d_cp, &p->d_kp));
  p->d_mid.resize(c.layers_per_block);
  for (int j = 0; j < c.layers_per_block; ++j) TRY(L.res_st("decoder.mid_block.resnets." + S(j), top, top, p->d_mid[j]));
  TRY(L.attn("decoder.mid_block.attentions.0", top, p->d_attn));
  p->d_up.resize(nb);
  prev = top;
  for (int i = 0; i < nb; ++i) {
    const int ch = c.block_out_channels[nb - 1 - i];
    VLevel& lv = p->d_up[i];
    lv.res.resize(c.layers_per_block + 1);
    for (int j = 0; j <= c.layers_per_block; ++j)
      TRY(L.res_st("decoder.up_blocks." + S(i) + ".resnets." + S(j), j == 0 ? prev : ch, ch, lv.res[j]));
    lv.has_resample = i != nb - 1;
    if (lv.has_resample) TRY(L.conv("decoder.up_blocks." + S(i) + ".upsamplers.0.conv", ch, ch, 9, lv.resample));
    prev = ch;
  }
  TRY(L.norm("decoder.conv_norm_out", c.block_out_channels[0], p->d_gno));
  TRY(L.conv("decoder.conv_out", c.out_channels, c.block_out_channels[0], 9, p->d_cout, true));
  TRY(L.vec("decoder.time_conv_out.weight", (long)c.out_channels * c.out_channels * 3, &p->tco_w));
  return L.vec("decoder.time_conv_out.bias", c.out_channels, &p->tco_b);
}

// ---- the walk: one function for the dry run (layout, peak) and the forward
inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

struct Arena {                             // first-fit free list over workspace offsets
  struct Blk { size_t off, size; bool free; };
  std::vector<Blk> blks;
  size_t peak = 0;
  size_t take(size_t bytes) {
    const size_t sz = up256(bytes ? bytes : 1);
    for (size_t i = 0; i < blks.size(); ++i) {
      if (!blks[i].free || blks[i].size < sz) continue;
      if (blks[i].size > sz) {
        const Blk rest{blks[i].off + sz, blks[i].size - sz, true};
        blks[i].size = sz;
        blks.insert(blks.begin() + i + 1, rest);
      }
      blks[i].free = false;
      return blks[i].off;
    }
    size_t off = blks.empty() ? 0 : blks.back().off + blks.back().size;
    if (!blks.empty() && blks.back().free) {       // grow the free tail
      off = blks.back().off;
      blks.pop_back();
    }
    blks.push_back(Blk{off, sz, false});
    if (off + sz > peak) peak = off + sz;
    return off;
  }
  void give(size_t off) {
    for (size_t i = 0; i < blks.size(); ++i) {
      if (blks[i].off != off) continue;
      blks[i].free = true;
      if (i + 1 < blks.size() && blks[i + 1].free) { blks[i].size += blks[i + 1].size; blks.erase(blks.begin() + i + 1); }
      if (i > 0 && blks[i - 1].free) { blks[i - 1].size += blks[i].size; blks.erase(blks.begin() + i); }
      return;
    }
  }
};

struct Ctx {
  const ctrlv_vae_plan* p;
  bool dry;                                // true: lay out only (base is a fake, never dereferenced address)
  char* base;
  hipStream_t st;
  Arena a;
  el_t* rows(long M, long C) { return (el_t*)(base + a.take((size_t)M * C * 2)); }
  void* bytes(size_t n) { return base + a.take(n); }
  void drop(const void* q) { a.give((size_t)((const char*)q - base)); }
};

ctrlv_gemm_desc gd(const void* A, int lda, const VConv& w, void* out, int ldo, long M, int N, int cin, int n_store) {
  ctrlv_gemm_desc d;
  memset(&d, 0, sizeof d);
  d.A = A; d.W = w.w; d.out = out; d.bias = w.b;
  d.M = (int)M; d.N = N; d.Cin = cin; d.taps = 1;
  d.lda = lda; d.ldo = ldo; d.n_store = n_store;
  d.s_acc = 1.0f; d.s1 = 1.0f; d.s2 = 1.0f;
  d.vdiv = 1; d.vmod = 1 << 30; d.vS = 1;
  return d;
}
void conv2d(ctrlv_gemm_desc& d, int H, int W, int Ho, int Wo, int stride, int up) {
  d.taps = 9; d.mode = 1; d.H = H; d.Wd = W; d.Ho = Ho; d.Wo = Wo; d.stride = stride; d.up = up;
}
void conv_t(ctrlv_gemm_desc& d, int F, int S) { d.taps = 3; d.mode = 2; d.F = F; d.S = S; }
void resid(ctrlv_gemm_desc& d, const void* R1, int ld) { d.R1 = R1; d.ldr1 = ld; }

// ops.gemm: the K-split scratch is offered to every launch whose layer shape asks for it (a function of the shape only)
int gemm(Ctx& c, ctrlv_gemm_desc d) {
  const size_t need = ctrlv_gemm_splitk_ws_bytes(&d);
  void* ws = need ? c.bytes(need) : nullptr;
  int rc = CTRLV_OK;
  if (!c.dry) {
    d.splitk_ws = ws;
    rc = ctrlv_gemm(&d, c.st);
  }
  if (ws) c.drop(ws);                      // (stream order: the next launch that reuses it runs behind this one)
  return rc;
}

int groupnorm(Ctx& c, const el_t* x, int n_img, int S, int C, int ips, const VNorm& nm, float eps, int silu, el_t* y) {
  const size_t fl = ((size_t)n_img * ctrlv_groupnorm_chunks(n_img, S, C, ips) + n_img / ips) * 64;
  float* part = (float*)c.bytes(fl * 4);
  int rc = CTRLV_OK;
  if (!c.dry) {
    rc = ctrlv_groupnorm_stats_split(x, nullptr, nullptr, nullptr, 0, n_img, S, C, ips, eps, part, c.st);
    if (rc == CTRLV_OK)
      rc = ctrlv_groupnorm_apply_split(x, nullptr, nullptr, nullptr, 0, n_img, S, C, ips, part, nm.g, nm.b, silu, y, c.st);
  }
  c.drop(part);
  return rc;
}

// vae_decoder_hip._frame_batches: frames per range of a per-frame op on [frames * S, C] rows
inline int frames_per(long limit, int n, long S, int C) {
  long per = limit / (S * C * 2);
  if (per > n) per = n;
  return per < 1 ? 1 : (int)per;
}

// conv_in: NCHW -> zero-padded rows -> im2col -> GEMM (both executors)
int conv_in(Ctx& c, const void* src, int dtype, int n, int C, int H, int W, const VConv& cv, int cp, int kp, el_t** out) {
  const long M = (long)n * H * W;
  el_t* x16 = c.rows(M, cp);
  if (!c.dry) {
    CTRLV_HIP_TRY(hipMemsetAsync(x16, 0, (size_t)M * cp * 2, c.st));
    TRY(ctrlv_nchw_to_rows(src, dtype, n, C, H * W, x16, cp, 0, c.st));
  }
  el_t* col = c.rows(M, kp);
  if (!c.dry) TRY(ctrlv_im2col3x3(x16, n, H, W, cp, col, kp, c.st));
  el_t* x = c.rows(M, cv.n);
  TRY(gemm(c, gd(col, kp, cv, x, cv.n, M, cv.n, kp, cv.n)));
  c.drop(col);
  c.drop(x16);
  *out = x;
  return CTRLV_OK;
}

// vae_encoder_hip._res (ResnetBlock2D); consumes nothing: the caller releases x
int enc_res(Ctx& c, const VRes& r, const el_t* x, int n, int H, int W, el_t** out) {
  const int S = H * W, cin = r.cin, cout = r.cout;
  const long M = (long)n * S;
  const float eps = 1e-6f;
  el_t* xn = c.rows(M, cin);
  TRY(groupnorm(c, x, n, S, cin, 1, r.n1, eps, 1, xn));
  el_t* h = c.rows(M, cout);
  { ctrlv_gemm_desc d = gd(xn, cin, r.c1, h, cout, M, cout, cin, cout); conv2d(d, H, W, H, W, 1, 0); TRY(gemm(c, d)); }
  c.drop(xn);
  el_t* hn = c.rows(M, cout);
  TRY(groupnorm(c, h, n, S, cout, 1, r.n2, eps, 1, hn));
  const el_t* res = x;
  el_t* rs = nullptr;
  if (r.shortcut) {
    rs = c.rows(M, cout);
    TRY(gemm(c, gd(x, cin, r.sc, rs, cout, M, cout, cin, cout)));
    res = rs;
  }
  { ctrlv_gemm_desc d = gd(hn, cout, r.c2, h, cout, M, cout, cout, cout); conv2d(d, H, W, H, W, 1, 0); resid(d, res, cout); TRY(gemm(c, d)); }
  c.drop(hn);
  if (rs) c.drop(rs);
  *out = h;
  return CTRLV_OK;
}

// vae_decoder_hip._res (SpatioTemporalResBlock, n frames = one clip)
int dec_res(Ctx& c, const VRes& r, const el_t* x, int n, int H, int W, el_t** out) {
  const int S = H * W, cin = r.cin, cout = r.cout;
  const long M = (long)n * S;
  el_t* xn = c.rows(M, cin);
  el_t* h = c.rows(M, cout);
  el_t* hn = c.rows(M, cout);
  el_t* rs = r.shortcut ? c.rows(M, cout) : nullptr;
  const el_t* res = r.shortcut ? rs : x;
  el_t* xs = c.rows(M, cout);
  const int per = frames_per(c.p->limit, n, S, cin > cout ? cin : cout);
  for (int f0 = 0; f0 < n; f0 += per) {
    const int k = (f0 + per < n ? f0 + per : n) - f0;
    const long r0 = (long)f0 * S, Mk = (long)k * S;
    TRY(groupnorm(c, x + r0 * cin, k, S, cin, 1, r.n1, 1e-6f, 1, xn + r0 * cin));
    { ctrlv_gemm_desc d = gd(xn + r0 * cin, cin, r.c1, h + r0 * cout, cout, Mk, cout, cin, cout); conv2d(d, H, W, H, W, 1, 0); TRY(gemm(c, d)); }
    TRY(groupnorm(c, h + r0 * cout, k, S, cout, 1, r.n2, 1e-6f, 1, hn + r0 * cout));
    if (r.shortcut) TRY(gemm(c, gd(x + r0 * cin, cin, r.sc, rs + r0 * cout, cout, Mk, cout, cin, cout)));
    { ctrlv_gemm_desc d = gd(hn + r0 * cout, cout, r.c2, xs + r0 * cout, cout, Mk, cout, cout, cout); conv2d(d, H, W, H, W, 1, 0);
      resid(d, res + r0 * cout, cout); TRY(gemm(c, d)); }
  }
  c.drop(xn);
  if (rs) c.drop(rs);
  // temporal res block on (1, C, n, H, W): statistics over the whole clip, conv along the frames, blend in the epilogue
  TRY(groupnorm(c, xs, n, S, cout, n, r.tn1, 1e-5f, 1, hn));
  { ctrlv_gemm_desc d = gd(hn, cout, r.tc1, h, cout, M, cout, cout, cout); conv_t(d, n, S); TRY(gemm(c, d)); }
  TRY(groupnorm(c, h, n, S, cout, n, r.tn2, 1e-5f, 1, hn));
  { ctrlv_gemm_desc d = gd(hn, cout, r.tc2, h, cout, M, cout, cout, cout); conv_t(d, n, S); d.s_acc = r.mix; resid(d, xs, cout); TRY(gemm(c, d)); }
  c.drop(hn);
  c.drop(xs);
  *out = h;
  return CTRLV_OK;
}

// vae_decoder_hip._attn: GroupNorm -> q, k -> per frame: scores GEMM (fp32) -> row softmax -> V^T GEMM -> P.V GEMM -> to_out + x
int attn(Ctx& c, const VAttn& a, const el_t* x, int n, int H, int W, int C, el_t** out) {
  const int S = H * W;
  const long M = (long)n * S;
  el_t* t = c.rows(M, C);
  TRY(groupnorm(c, x, n, S, C, 1, a.gn, 1e-6f, 0, t));
  el_t* q = c.rows(M, C);
  el_t* k = c.rows(M, C);
  TRY(gemm(c, gd(t, C, a.q, q, C, M, C, C, C)));
  TRY(gemm(c, gd(t, C, a.k, k, C, M, C, C, C)));
  el_t* o = c.rows(M, C);
  float* scores = (float*)c.bytes((size_t)S * S * 4);
  el_t* probs = c.rows(S, S);
  el_t* vt = c.rows(C, S);
  const float scale = (float)pow((double)C, -0.5);
  for (int f = 0; f < n; ++f) {
    const long r0 = (long)f * S * C;
    VConv kw; kw.w = k + r0; kw.b = nullptr;
    { ctrlv_gemm_desc d = gd(q + r0, C, kw, scores, S, S, S, C, S); d.s_acc = scale; d.out_f32 = 1; TRY(gemm(c, d)); }
    if (!c.dry) TRY(ctrlv_softmax_rows(scores, S, S, S, probs, S, c.st));
    VConv tw; tw.w = t + r0; tw.b = nullptr;
    TRY(gemm(c, gd(a.v_rows.w, C, tw, vt, S, C, S, C, S)));
    VConv vw; vw.w = vt; vw.b = nullptr;
    TRY(gemm(c, gd(probs, S, vw, o + r0, C, S, C, S, C)));
  }
  c.drop(scores); c.drop(probs); c.drop(vt); c.drop(q); c.drop(k);
  el_t* y = c.rows(M, C);
  { ctrlv_gemm_desc d = gd(o, C, a.o, y, C, M, C, C, C); resid(d, x, C); TRY(gemm(c, d)); }
  c.drop(t);
  c.drop(o);
  *out = y;
  return CTRLV_OK;
}

int encode_walk(Ctx& c, const void* px, int dtype, int n, int H, int W, const float* noise, float scale, void* latents,
                void* moments, int out_dtype) {
  const ctrlv_vae_plan* p = c.p;
  const ctrlv_vae_config& cf = p->cfg;
  el_t* h;
  TRY(conv_in(c, px, dtype, n, cf.in_channels, H, W, p->e_cin, p->e_cp, p->e_kp, &h));
  for (const VLevel& lv : p->e_down) {
    for (const VRes& r : lv.res) {
      el_t* y;
      TRY(enc_res(c, r, h, n, H, W, &y));
      c.drop(h);
      h = y;
    }
    if (lv.has_resample) {               // F.pad(x, (0, 1, 0, 1)) + stride 2: ONE launch (pad_br)
      const int C = lv.res.back().cout;
      el_t* half = c.rows((long)n * (H / 2) * (W / 2), C);
      ctrlv_gemm_desc d = gd(h, C, lv.resample, half, C, (long)n * (H / 2) * (W / 2), C, C, C);
      conv2d(d, H, W, H / 2, W / 2, 2, 0);
      d.pad_br = 1;
      TRY(gemm(c, d));
      c.drop(h);
      h = half;
      H /= 2; W /= 2;
    }
  }
  const int C = cf.block_out_channels[cf.n_blocks - 1];
  el_t* y;
  TRY(enc_res(c, p->e_mid[0], h, n, H, W, &y)); c.drop(h); h = y;
  TRY(attn(c, p->e_attn, h, n, H, W, C, &y)); c.drop(h); h = y;
  TRY(enc_res(c, p->e_mid[1], h, n, H, W, &y)); c.drop(h); h = y;
  const long M = (long)n * H * W;
  el_t* hn = c.rows(M, C);
  TRY(groupnorm(c, h, n, H * W, C, 1, p->e_gno, 1e-6f, 1, hn));
  const int co = 2 * cf.latent_channels, co_p = (co + 3) / 4 * 4;
  el_t* rows = c.rows(M, co_p);
  { ctrlv_gemm_desc d = gd(hn, C, p->e_cout, rows, co_p, M, p->e_cout.n, C, co_p); conv2d(d, H, W, H, W, 1, 0); TRY(gemm(c, d)); }
  if (!c.dry)
    TRY(ctrlv_vae_posterior(rows, co_p, n, cf.latent_channels, H * W, p->qw, p->qb, noise, scale, moments, latents, out_dtype, c.st));
  c.drop(rows); c.drop(hn); c.drop(h);
  return CTRLV_OK;
}

int decode_clip(Ctx& c, const void* z, int dtype, int n, int H, int W, void* frames, int out_dtype) {
  const ctrlv_vae_plan* p = c.p;
  const ctrlv_vae_config& cf = p->cfg;
  el_t* x;
  el_t* y;
  TRY(conv_in(c, z, dtype, n, cf.latent_channels, H, W, p->d_cin, p->d_cp, p->d_kp, &x));
  const int top = cf.block_out_channels[cf.n_blocks - 1];
  TRY(dec_res(c, p->d_mid[0], x, n, H, W, &y)); c.drop(x); x = y;
  for (size_t j = 1; j < p->d_mid.size(); ++j) {
    TRY(attn(c, p->d_attn, x, n, H, W, top, &y)); c.drop(x); x = y;
    TRY(dec_res(c, p->d_mid[j], x, n, H, W, &y)); c.drop(x); x = y;
  }
  for (const VLevel& lv : p->d_up) {
    for (const VRes& r : lv.res) { TRY(dec_res(c, r, x, n, H, W, &y)); c.drop(x); x = y; }
    if (lv.has_resample) {               // nearest x2 fused into the conv's gather; per-frame op: frame ranges
      const int C = lv.res.back().cout;
      const long S = (long)H * W;
      el_t* up = c.rows((long)n * 4 * S, C);
      const int per = frames_per(p->limit, n, 4 * S, C);
      for (int f0 = 0; f0 < n; f0 += per) {
        const int k = (f0 + per < n ? f0 + per : n) - f0;
        ctrlv_gemm_desc d = gd(x + (long)f0 * S * C, C, lv.resample, up + (long)f0 * 4 * S * C, C, (long)k * 4 * S, C, C, C);
        conv2d(d, H, W, 2 * H, 2 * W, 1, 1);
        TRY(gemm(c, d));
      }
      c.drop(x);
      x = up;
      H *= 2; W *= 2;
    }
  }
  const int C = cf.block_out_channels[0], co = cf.out_channels, co_p = (co + 3) / 4 * 4;
  const long M = (long)n * H * W;
  el_t* xn = c.rows(M, C);
  TRY(groupnorm(c, x, n, H * W, C, 1, p->d_gno, 1e-6f, 1, xn));
  c.drop(x);
  el_t* rows = c.rows(M, co_p);
  { ctrlv_gemm_desc d = gd(xn, C, p->d_cout, rows, co_p, M, p->d_cout.n, C, co_p); conv2d(d, H, W, H, W, 1, 0); TRY(gemm(c, d)); }
  c.drop(xn);
  if (!c.dry) TRY(ctrlv_time_conv_rows_to_nchw(rows, co_p, n, co, H * W, p->tco_w, p->tco_b, frames, out_dtype, c.st));
  c.drop(rows);
  return CTRLV_OK;
}

// vae_encoder_hip.supports / vae_decoder_hip.supports
int check_encode_shape(const ctrlv_vae_plan* p, int n, int H, int W) {
  CTRLV_CHECK_SHAPE(n >= 1 && H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0, "vae_encode: n=%d images of %dx%d: H and W must be "
                    "multiples of 8", n, H, W);
  const long s = (long)(H / 8) * (W / 8);
  CTRLV_CHECK_SHAPE(s % 64 == 0 && s <= 16384, "vae_encode: %ld latent pixels per image must be a multiple of 64, at most 16384 "
                    "(the mid block's attention)", s);
  CTRLV_CHECK_SHAPE((long)n * H * W * p->cfg.block_out_channels[0] * 2 < p->limit, "vae_encode: %d images of %dx%d exceed the "
                    "offset limit of %ld bytes per tensor", n, H, W, p->limit);
  return CTRLV_OK;
}
int check_decode_shape(const ctrlv_vae_plan* p, int n, int nf, int h, int w) {
  CTRLV_CHECK_SHAPE(n >= 1 && nf >= 1 && n % nf == 0, "vae_decode: %d latent frames are not whole clips of num_frames=%d", n, nf);
  CTRLV_CHECK_SHAPE(h > 0 && w > 0 && ((long)h * w) % 64 == 0 && (long)h * w <= 16384, "vae_decode: %dx%d latent pixels per frame "
                    "must be a multiple of 64, at most 16384 (the mid block's attention)", h, w);
  const int nb = p->cfg.n_blocks;
  for (int i = 0; i < nb; ++i) {           // whole-clip tensors of the temporal halves, per resolution level
    const long f = 1L << i;
    CTRLV_CHECK_SHAPE((long)nf * h * w * f * f * p->cfg.block_out_channels[nb - 1 - i] * 2 < p->limit,
                      "vae_decode: a clip of %d frames at %dx%d exceeds the offset limit of %ld bytes per whole-clip tensor", nf,
                      8 * h, 8 * w, p->limit);
  }
  return CTRLV_OK;
}

char* const kFakeBase = (char*)(uintptr_t)0x10000000;       // dry runs: pointers are compared with NULL, never dereferenced

size_t dry_bytes(ctrlv_vae_plan* p, int what, int n, int nf, int H, int W) {
  Ctx c{p, true, kFakeBase, nullptr, {}};
  const int rc = what == 0 ? encode_walk(c, kFakeBase, 0, n, H, W, nullptr, 1.f, kFakeBase, kFakeBase, 0)
                           : decode_clip(c, kFakeBase, 0, nf, H, W, kFakeBase, 0);
  return rc == CTRLV_OK ? c.a.peak : 0;
}

}  // namespace

extern "C" int ctrlv_vae_plan_create(const ctrlv_vae_config* cfg, int device, ctrlv_vae_plan** out) {
  CTRLV_CHECK_ARG(cfg && out, "vae_plan_create: null argument");
  const ctrlv_vae_config& c = *cfg;
  CTRLV_CHECK_SHAPE(c.n_blocks == 4, "vae_plan_create: n_blocks=%d: the HIP VAE walks four down / up blocks", c.n_blocks);
  for (int i = 0; i < c.n_blocks; ++i)
    CTRLV_CHECK_SHAPE(c.block_out_channels[i] > 0 && c.block_out_channels[i] % 64 == 0 && c.block_out_channels[i] <= 1024,
                      "vae_plan_create: block_out_channels[%d]=%d must be a multiple of 64, at most 1024 (GEMM K granularity)", i,
                      c.block_out_channels[i]);
  CTRLV_CHECK_SHAPE(c.latent_channels >= 1 && c.latent_channels <= 8, "vae_plan_create: latent_channels=%d must be in [1, 8]",
                    c.latent_channels);
  CTRLV_CHECK_SHAPE(c.in_channels >= 1 && c.in_channels <= 8, "vae_plan_create: in_channels=%d must be in [1, 8]", c.in_channels);
  CTRLV_CHECK_SHAPE(c.out_channels >= 1 && c.out_channels <= 4, "vae_plan_create: out_channels=%d must be in [1, 4] (time_conv_out)",
                    c.out_channels);
  CTRLV_CHECK_SHAPE(c.layers_per_block >= 1 && c.layers_per_block <= 8, "vae_plan_create: layers_per_block=%d must be in [1, 8]",
                    c.layers_per_block);
  CTRLV_CHECK_ARG(c.offset_limit_bytes >= 0 && c.offset_limit_bytes <= kLimit32, "vae_plan_create: offset_limit_bytes=%ld must be "
                  "0 (the kernels' limit) or at most %ld", (long)c.offset_limit_bytes, kLimit32);
  ctrlv_vae_plan* p = new ctrlv_vae_plan();
  p->cfg = c;
  p->device = device;
  p->limit = c.offset_limit_bytes ? (long)c.offset_limit_bytes : kLimit32;
  *out = p;
  return CTRLV_OK;
}

extern "C" int ctrlv_vae_plan_destroy(ctrlv_vae_plan* p) {
  if (!p) return CTRLV_OK;
  if (!p->owned.empty()) {
    int dev = 0;
    const bool sw = hipGetDevice(&dev) == hipSuccess && dev != p->device;
    if (sw) (void)hipSetDevice(p->device);
    free_owned(p);
    if (sw) (void)hipSetDevice(dev);
  }
  delete p;
  return CTRLV_OK;
}

extern "C" int ctrlv_vae_plan_load_weights(ctrlv_vae_plan* p, const ctrlv_tensor_desc* tensors, size_t n) {
  CTRLV_CHECK_ARG(p && tensors, "vae_plan_load_weights: null argument");
  int prev = 0;
  const bool sw = hipGetDevice(&prev) == hipSuccess && prev != p->device;
  CTRLV_HIP_TRY(hipSetDevice(p->device));
  free_owned(p);
  VLoader L;
  L.p = p;
  for (size_t i = 0; i < n; ++i)
    if (tensors[i].name) L.map[tensors[i].name] = &tensors[i];
  const int rc = load_all(L);
  const hipError_t e = hipDeviceSynchronize();
  for (void* d : L.staged) (void)hipFree(d);
  if (sw) (void)hipSetDevice(prev);
  if (rc != CTRLV_OK) { free_owned(p); return rc; }
  if (e != hipSuccess) {
    free_owned(p);
    ctrlv_set_error("vae_plan_load_weights: %s", hipGetErrorString(e));
    return CTRLV_E_HIP;
  }
  p->loaded = true;
  return CTRLV_OK;
}

extern "C" size_t ctrlv_vae_plan_workspace_bytes(ctrlv_vae_plan* p, int what, int n, int num_frames, int H, int W) {
  if (!p || !p->loaded) { ctrlv_set_error("vae_plan_workspace_bytes: plan not loaded"); return 0; }
  if (what != 0 && what != 1) { ctrlv_set_error("vae_plan_workspace_bytes: what=%d (0 encode, 1 decode)", what); return 0; }
  if ((what == 0 ? check_encode_shape(p, n, H, W) : check_decode_shape(p, n, num_frames, H, W)) != CTRLV_OK) return 0;
  return dry_bytes(p, what, n, num_frames, H, W);
}

extern "C" int ctrlv_vae_encode(ctrlv_vae_plan* p, const void* pixels, int dtype, int n, int Hpx, int Wpx, const float* noise,
                                float scale, void* latents, void* moments, int out_dtype, void* workspace, size_t workspace_bytes,
                                ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(p && p->loaded, "vae_encode: plan not loaded");
  CTRLV_CHECK_ARG(pixels && workspace && (latents || moments), "vae_encode: null pointer (pixels, workspace, and at least one of "
                  "latents / moments)");
  if (dtype < 0 || dtype > 2 || out_dtype < 0 || out_dtype > 2) {
    ctrlv_set_error("vae_encode: dtype codes %d / %d (0 fp32, 1 fp16, 2 bf16)", dtype, out_dtype);
    return CTRLV_E_BAD_DTYPE;
  }
  TRY(check_encode_shape(p, n, Hpx, Wpx));
  CTRLV_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "vae_encode: workspace must be 256-byte aligned");
  const size_t need = dry_bytes(p, 0, n, 0, Hpx, Wpx);
  if (workspace_bytes < need) {
    ctrlv_set_error("vae_encode: workspace of %zu bytes, %zu needed (ctrlv_vae_plan_workspace_bytes)", workspace_bytes, need);
    return CTRLV_E_WORKSPACE;
  }
  Ctx c{p, false, (char*)workspace, (hipStream_t)stream, {}};
  return encode_walk(c, pixels, dtype, n, Hpx, Wpx, noise, scale, latents, moments, out_dtype);
}

extern "C" int ctrlv_vae_decode(ctrlv_vae_plan* p, const void* z, int dtype, int n, int num_frames, int h, int w, void* frames,
                                int out_dtype, void* workspace, size_t workspace_bytes, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(p && p->loaded, "vae_decode: plan not loaded");
  CTRLV_CHECK_ARG(z && frames && workspace, "vae_decode: null pointer");
  if (dtype < 0 || dtype > 2 || out_dtype < 0 || out_dtype > 2) {
    ctrlv_set_error("vae_decode: dtype codes %d / %d (0 fp32, 1 fp16, 2 bf16)", dtype, out_dtype);
    return CTRLV_E_BAD_DTYPE;
  }
  TRY(check_decode_shape(p, n, num_frames, h, w));
  CTRLV_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "vae_decode: workspace must be 256-byte aligned");
  const size_t need = dry_bytes(p, 1, n, num_frames, h, w);
  if (workspace_bytes < need) {
    ctrlv_set_error("vae_decode: workspace of %zu bytes, %zu needed (ctrlv_vae_plan_workspace_bytes)", workspace_bytes, need);
    return CTRLV_E_WORKSPACE;
  }
  const ctrlv_vae_config& cf = p->cfg;
  const size_t in_el = dtype == 0 ? 4 : 2, out_el = out_dtype == 0 ? 4 : 2;
  for (int c0 = 0; c0 < n; c0 += num_frames) {       // independent clips, one after the other in the same workspace
    Ctx c{p, false, (char*)workspace, (hipStream_t)stream, {}};
    TRY(decode_clip(c, (const char*)z + (size_t)c0 * cf.latent_channels * h * w * in_el, dtype, num_frames, h, w,
                    (char*)frames + (size_t)c0 * cf.out_channels * 64 * h * w * out_el, out_dtype));
  }
  return CTRLV_OK;
}
