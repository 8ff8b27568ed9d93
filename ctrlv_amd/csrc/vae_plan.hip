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
#include <vector>

#include "plan_walk.h"
#include "weight_loader.h"

namespace {

using ctrlv_load::WeightLoader;
using ctrlv_walk::conv2d;
using ctrlv_walk::conv_t;
using ctrlv_walk::resid;
using VConv = ctrlv_load::PackedLinear;        // packed [n (rows, x32), k] + fp32 bias [n]
using VNorm = ctrlv_load::NormParams;
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

int res2d(WeightLoader& L, const std::string& mod, int cin, int cout, VRes& r) {
  r.cin = cin; r.cout = cout;
  CTRLV_TRY(L.norm(mod + ".norm1", cin, r.n1));
  CTRLV_TRY(L.conv3x3(mod + ".conv1", cout, cin, r.c1));
  CTRLV_TRY(L.norm(mod + ".norm2", cout, r.n2));
  CTRLV_TRY(L.conv3x3(mod + ".conv2", cout, cout, r.c2));
  r.shortcut = cin != cout;
  if (r.shortcut) CTRLV_TRY(L.linear(mod + ".conv_shortcut", cout, cin, r.sc));
  return CTRLV_OK;
}
int res_st(WeightLoader& L, const std::string& mod, int cin, int cout, VRes& r) {
  CTRLV_TRY(res2d(L, mod + ".spatial_res_block", cin, cout, r));
  r.temporal = true;
  const std::string t = mod + ".temporal_res_block";
  CTRLV_TRY(L.norm(t + ".norm1", cout, r.tn1));
  CTRLV_TRY(L.conv_t(t + ".conv1", cout, cout, r.tc1));
  CTRLV_TRY(L.norm(t + ".norm2", cout, r.tn2));
  CTRLV_TRY(L.conv_t(t + ".conv2", cout, cout, r.tc2));
  double alpha;
  CTRLV_TRY(L.mix_alpha(mod + ".time_mixer.mix_factor", &alpha));
  r.mix = (float)alpha;
  return CTRLV_OK;
}
int attn(WeightLoader& L, const std::string& mod, int C, VAttn& a) {
  CTRLV_TRY(L.norm(mod + ".group_norm", C, a.gn));
  CTRLV_TRY(L.linear(mod + ".to_q", C, C, a.q));
  CTRLV_TRY(L.linear(mod + ".to_k", C, C, a.k));
  CTRLV_TRY(L.linear(mod + ".to_v", C, C, a.v_rows, false));
  CTRLV_TRY(L.linear(mod + ".to_out.0", C, C, a.o, false));
  // folded output bias b_o + W_o . b_v (rows of P sum to one): fp64 on the host from the fp32 values, rounded once
  std::vector<float> wo, bo, bv;
  CTRLV_TRY(L.host_f32(mod + ".to_out.0.weight", (long)C * C, wo));
  CTRLV_TRY(L.host_f32(mod + ".to_out.0.bias", C, bo));
  CTRLV_TRY(L.host_f32(mod + ".to_v.bias", C, bv));
  std::vector<float> fold(C);
  for (int o = 0; o < C; ++o) {
    double s = (double)bo[o];
    for (int c = 0; c < C; ++c) s += (double)wo[(size_t)o * C + c] * (double)bv[c];
    fold[o] = (float)s;
  }
  return L.upload(fold, &a.o.b);
}

void free_owned(ctrlv_vae_plan* p) {
  for (void* d : p->owned) (void)hipFree(d);
  p->owned.clear();
  p->e_down.clear(); p->d_mid.clear(); p->d_up.clear();
  p->loaded = false;
}

int load_all(WeightLoader& L, ctrlv_vae_plan* p) {
  const ctrlv_vae_config& c = p->cfg;
  const int nb = c.n_blocks, top = c.block_out_channels[nb - 1], L2 = 2 * c.latent_channels;
  auto S = [](int i) { return std::to_string(i); };
  // ---- encoder
  CTRLV_TRY(L.conv_in("encoder.conv_in", c.block_out_channels[0], c.in_channels, c.in_channels, p->e_cin, &p->e_cp, &p->e_kp));
  p->e_down.resize(nb);
  int prev = c.block_out_channels[0];
  for (int i = 0; i < nb; ++i) {
    const int ch = c.block_out_channels[i];
    VLevel& lv = p->e_down[i];
    lv.res.resize(c.layers_per_block);
    for (int j = 0; j < c.layers_per_block; ++j)
      CTRLV_TRY(res2d(L, "encoder.down_blocks." + S(i) + ".resnets." + S(j), j == 0 ? prev : ch, ch, lv.res[j]));
    lv.has_resample = i != nb - 1;
    if (lv.has_resample) CTRLV_TRY(L.conv3x3("encoder.down_blocks." + S(i) + ".downsamplers.0.conv", ch, ch, lv.resample));
    prev = ch;
  }
  for (int j = 0; j < 2; ++j) CTRLV_TRY(res2d(L, "encoder.mid_block.resnets." + S(j), top, top, p->e_mid[j]));
  CTRLV_TRY(attn(L, "encoder.mid_block.attentions.0", top, p->e_attn));
  CTRLV_TRY(L.norm("encoder.conv_norm_out", top, p->e_gno));
  CTRLV_TRY(L.conv3x3("encoder.conv_out", L2, top, p->e_cout));
  CTRLV_TRY(L.vec("quant_conv.weight", (long)L2 * L2, &p->qw));
  CTRLV_TRY(L.vec("quant_conv.bias", L2, &p->qb));
  // ---- decoder
  CTRLV_TRY(L.conv_in("decoder.conv_in", top, c.latent_channels, c.latent_channels, p->d_cin, &p->d_cp, &p->d_kp));
  p->d_mid.resize(c.layers_per_block);
  for (int j = 0; j < c.layers_per_block; ++j) CTRLV_TRY(res_st(L, "decoder.mid_block.resnets." + S(j), top, top, p->d_mid[j]));
  CTRLV_TRY(attn(L, "decoder.mid_block.attentions.0", top, p->d_attn));
  p->d_up.resize(nb);
  prev = top;
  for (int i = 0; i < nb; ++i) {
    const int ch = c.block_out_channels[nb - 1 - i];
    VLevel& lv = p->d_up[i];
    lv.res.resize(c.layers_per_block + 1);
    for (int j = 0; j <= c.layers_per_block; ++j)
      CTRLV_TRY(res_st(L, "decoder.up_blocks." + S(i) + ".resnets." + S(j), j == 0 ? prev : ch, ch, lv.res[j]));
    lv.has_resample = i != nb - 1;
    if (lv.has_resample) CTRLV_TRY(L.conv3x3("decoder.up_blocks." + S(i) + ".upsamplers.0.conv", ch, ch, lv.resample));
    prev = ch;
  }
  CTRLV_TRY(L.norm("decoder.conv_norm_out", c.block_out_channels[0], p->d_gno));
  CTRLV_TRY(L.conv3x3("decoder.conv_out", c.out_channels, c.block_out_channels[0], p->d_cout));
  CTRLV_TRY(L.vec("decoder.time_conv_out.weight", (long)c.out_channels * c.out_channels * 3, &p->tco_w));
  return L.vec("decoder.time_conv_out.bias", c.out_channels, &p->tco_b);
}

// ---- the walk: one function for the dry run (layout, peak) and the forward
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

struct Ctx : ctrlv_walk::LaunchGate {      // dry: lay out only (base is a fake, never dereferenced address)
  const ctrlv_vae_plan* p;
  char* base;
  Arena a;
  el_t* rows(long M, long C) { return (el_t*)(base + a.take((size_t)M * C * 2)); }
  void* bytes(size_t n) { return base + a.take(n); }
  void drop(const void* q) { a.give((size_t)((const char*)q - base)); }
};

// ops.gemm: the K-split scratch is offered to every launch whose layer shape asks for it (a function of the shape only)
int gemm(Ctx& c, ctrlv_gemm_desc d) {
  const size_t need = ctrlv_gemm_splitk_ws_bytes(&d);
  void* ws = need ? c.bytes(need) : nullptr;
  d.splitk_ws = ws;
  const int rc = c.run([&] { return ctrlv_gemm(&d, c.st); });
  if (ws) c.drop(ws);                      // (stream order: the next launch that reuses it runs behind this one)
  return rc;
}

int groupnorm(Ctx& c, const el_t* x, int n_img, int S, int C, int ips, const VNorm& nm, float eps, int silu, el_t* y) {
  const size_t fl = ((size_t)n_img * ctrlv_groupnorm_chunks(n_img, S, C, ips) + n_img / ips) * 64;
  float* part = (float*)c.bytes(fl * 4);
  const int rc = c.run([&]() -> int {
    CTRLV_TRY(ctrlv_groupnorm_stats_split(x, nullptr, nullptr, nullptr, 0, n_img, S, C, ips, eps, part, c.st));
    return ctrlv_groupnorm_apply_split(x, nullptr, nullptr, nullptr, 0, n_img, S, C, ips, part, nm.g, nm.b, silu, y, c.st);
  });
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
  CTRLV_TRY(c.run([&]() -> int {
    CTRLV_HIP_TRY(hipMemsetAsync(x16, 0, (size_t)M * cp * 2, c.st));
    return ctrlv_nchw_to_rows(src, dtype, n, C, H * W, x16, cp, 0, c.st);
  }));
  el_t* col = c.rows(M, kp);
  CTRLV_TRY(c.run([&] { return ctrlv_im2col3x3(x16, n, H, W, cp, col, kp, c.st); }));
  el_t* x = c.rows(M, cv.n);
  CTRLV_TRY(gemm(c, ctrlv_linear_desc(col, kp, cv, x, cv.n, M, cv.n, kp, cv.n)));
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
  CTRLV_TRY(groupnorm(c, x, n, S, cin, 1, r.n1, eps, 1, xn));
  el_t* h = c.rows(M, cout);
  { ctrlv_gemm_desc d = ctrlv_linear_desc(xn, cin, r.c1, h, cout, M, cout, cin, cout); conv2d(d, H, W, H, W); CTRLV_TRY(gemm(c, d)); }
  c.drop(xn);
  el_t* hn = c.rows(M, cout);
  CTRLV_TRY(groupnorm(c, h, n, S, cout, 1, r.n2, eps, 1, hn));
  const el_t* res = x;
  el_t* rs = nullptr;
  if (r.shortcut) {
    rs = c.rows(M, cout);
    CTRLV_TRY(gemm(c, ctrlv_linear_desc(x, cin, r.sc, rs, cout, M, cout, cin, cout)));
    res = rs;
  }
  { ctrlv_gemm_desc d = ctrlv_linear_desc(hn, cout, r.c2, h, cout, M, cout, cout, cout); conv2d(d, H, W, H, W); resid(d, res, cout); CTRLV_TRY(gemm(c, d)); }
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
    CTRLV_TRY(groupnorm(c, x + r0 * cin, k, S, cin, 1, r.n1, 1e-6f, 1, xn + r0 * cin));
    { ctrlv_gemm_desc d = ctrlv_linear_desc(xn + r0 * cin, cin, r.c1, h + r0 * cout, cout, Mk, cout, cin, cout); conv2d(d, H, W, H, W); CTRLV_TRY(gemm(c, d)); }
    CTRLV_TRY(groupnorm(c, h + r0 * cout, k, S, cout, 1, r.n2, 1e-6f, 1, hn + r0 * cout));
    if (r.shortcut) CTRLV_TRY(gemm(c, ctrlv_linear_desc(x + r0 * cin, cin, r.sc, rs + r0 * cout, cout, Mk, cout, cin, cout)));
    { ctrlv_gemm_desc d = ctrlv_linear_desc(hn + r0 * cout, cout, r.c2, xs + r0 * cout, cout, Mk, cout, cout, cout); conv2d(d, H, W, H, W);
      resid(d, res + r0 * cout, cout); CTRLV_TRY(gemm(c, d)); }
  }
  c.drop(xn);
  if (rs) c.drop(rs);
  // temporal res block on (1, C, n, H, W): statistics over the whole clip, conv along the frames, blend in the epilogue
  CTRLV_TRY(groupnorm(c, xs, n, S, cout, n, r.tn1, 1e-5f, 1, hn));
  { ctrlv_gemm_desc d = ctrlv_linear_desc(hn, cout, r.tc1, h, cout, M, cout, cout, cout); conv_t(d, n, S); CTRLV_TRY(gemm(c, d)); }
  CTRLV_TRY(groupnorm(c, h, n, S, cout, n, r.tn2, 1e-5f, 1, hn));
  { ctrlv_gemm_desc d = ctrlv_linear_desc(hn, cout, r.tc2, h, cout, M, cout, cout, cout); conv_t(d, n, S); d.s_acc = r.mix; resid(d, xs, cout); CTRLV_TRY(gemm(c, d)); }
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
  CTRLV_TRY(groupnorm(c, x, n, S, C, 1, a.gn, 1e-6f, 0, t));
  el_t* q = c.rows(M, C);
  el_t* k = c.rows(M, C);
  CTRLV_TRY(gemm(c, ctrlv_linear_desc(t, C, a.q, q, C, M, C, C, C)));
  CTRLV_TRY(gemm(c, ctrlv_linear_desc(t, C, a.k, k, C, M, C, C, C)));
  el_t* o = c.rows(M, C);
  float* scores = (float*)c.bytes((size_t)S * S * 4);
  el_t* probs = c.rows(S, S);
  el_t* vt = c.rows(C, S);
  const float scale = (float)pow((double)C, -0.5);
  for (int f = 0; f < n; ++f) {
    const long r0 = (long)f * S * C;
    VConv kw; kw.w = k + r0; kw.b = nullptr;
    { ctrlv_gemm_desc d = ctrlv_linear_desc(q + r0, C, kw, scores, S, S, S, C, S); d.s_acc = scale; d.out_f32 = 1; CTRLV_TRY(gemm(c, d)); }
    CTRLV_TRY(c.run([&] { return ctrlv_softmax_rows(scores, S, S, S, probs, S, c.st); }));
    VConv tw; tw.w = t + r0; tw.b = nullptr;
    CTRLV_TRY(gemm(c, ctrlv_linear_desc(a.v_rows.w, C, tw, vt, S, C, S, C, S)));
    VConv vw; vw.w = vt; vw.b = nullptr;
    CTRLV_TRY(gemm(c, ctrlv_linear_desc(probs, S, vw, o + r0, C, S, C, S, C)));
  }
  c.drop(scores); c.drop(probs); c.drop(vt); c.drop(q); c.drop(k);
  el_t* y = c.rows(M, C);
  { ctrlv_gemm_desc d = ctrlv_linear_desc(o, C, a.o, y, C, M, C, C, C); resid(d, x, C); CTRLV_TRY(gemm(c, d)); }
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
  CTRLV_TRY(conv_in(c, px, dtype, n, cf.in_channels, H, W, p->e_cin, p->e_cp, p->e_kp, &h));
  for (const VLevel& lv : p->e_down) {
    for (const VRes& r : lv.res) {
      el_t* y;
      CTRLV_TRY(enc_res(c, r, h, n, H, W, &y));
      c.drop(h);
      h = y;
    }
    if (lv.has_resample) {               // F.pad(x, (0, 1, 0, 1)) + stride 2: ONE launch (pad_br)
      const int C = lv.res.back().cout;
      el_t* half = c.rows((long)n * (H / 2) * (W / 2), C);
      ctrlv_gemm_desc d = ctrlv_linear_desc(h, C, lv.resample, half, C, (long)n * (H / 2) * (W / 2), C, C, C);
      conv2d(d, H, W, H / 2, W / 2, 2, 0);
      d.pad_br = 1;
      CTRLV_TRY(gemm(c, d));
      c.drop(h);
      h = half;
      H /= 2; W /= 2;
    }
  }
  const int C = cf.block_out_channels[cf.n_blocks - 1];
  el_t* y;
  CTRLV_TRY(enc_res(c, p->e_mid[0], h, n, H, W, &y)); c.drop(h); h = y;
  CTRLV_TRY(attn(c, p->e_attn, h, n, H, W, C, &y)); c.drop(h); h = y;
  CTRLV_TRY(enc_res(c, p->e_mid[1], h, n, H, W, &y)); c.drop(h); h = y;
  const long M = (long)n * H * W;
  el_t* hn = c.rows(M, C);
  CTRLV_TRY(groupnorm(c, h, n, H * W, C, 1, p->e_gno, 1e-6f, 1, hn));
  const int co = 2 * cf.latent_channels, co_p = (co + 3) / 4 * 4;
  el_t* rows = c.rows(M, co_p);
  { ctrlv_gemm_desc d = ctrlv_linear_desc(hn, C, p->e_cout, rows, co_p, M, p->e_cout.n, C, co_p); conv2d(d, H, W, H, W); CTRLV_TRY(gemm(c, d)); }
  CTRLV_TRY(c.run([&] {
    return ctrlv_vae_posterior(rows, co_p, n, cf.latent_channels, H * W, p->qw, p->qb, noise, scale, moments, latents, out_dtype, c.st);
  }));
  c.drop(rows); c.drop(hn); c.drop(h);
  return CTRLV_OK;
}

int decode_clip(Ctx& c, const void* z, int dtype, int n, int H, int W, void* frames, int out_dtype) {
  const ctrlv_vae_plan* p = c.p;
  const ctrlv_vae_config& cf = p->cfg;
  el_t* x;
  el_t* y;
  CTRLV_TRY(conv_in(c, z, dtype, n, cf.latent_channels, H, W, p->d_cin, p->d_cp, p->d_kp, &x));
  const int top = cf.block_out_channels[cf.n_blocks - 1];
  CTRLV_TRY(dec_res(c, p->d_mid[0], x, n, H, W, &y)); c.drop(x); x = y;
  for (size_t j = 1; j < p->d_mid.size(); ++j) {
    CTRLV_TRY(attn(c, p->d_attn, x, n, H, W, top, &y)); c.drop(x); x = y;
    CTRLV_TRY(dec_res(c, p->d_mid[j], x, n, H, W, &y)); c.drop(x); x = y;
  }
  for (const VLevel& lv : p->d_up) {
    for (const VRes& r : lv.res) { CTRLV_TRY(dec_res(c, r, x, n, H, W, &y)); c.drop(x); x = y; }
    if (lv.has_resample) {               // nearest x2 fused into the conv's gather; per-frame op: frame ranges
      const int C = lv.res.back().cout;
      const long S = (long)H * W;
      el_t* up = c.rows((long)n * 4 * S, C);
      const int per = frames_per(p->limit, n, 4 * S, C);
      for (int f0 = 0; f0 < n; f0 += per) {
        const int k = (f0 + per < n ? f0 + per : n) - f0;
        ctrlv_gemm_desc d = ctrlv_linear_desc(x + (long)f0 * S * C, C, lv.resample, up + (long)f0 * 4 * S * C, C, (long)k * 4 * S, C, C, C);
        conv2d(d, H, W, 2 * H, 2 * W, 1, 1);
        CTRLV_TRY(gemm(c, d));
      }
      c.drop(x);
      x = up;
      H *= 2; W *= 2;
    }
  }
  const int C = cf.block_out_channels[0], co = cf.out_channels, co_p = (co + 3) / 4 * 4;
  const long M = (long)n * H * W;
  el_t* xn = c.rows(M, C);
  CTRLV_TRY(groupnorm(c, x, n, H * W, C, 1, p->d_gno, 1e-6f, 1, xn));
  c.drop(x);
  el_t* rows = c.rows(M, co_p);
  { ctrlv_gemm_desc d = ctrlv_linear_desc(xn, C, p->d_cout, rows, co_p, M, p->d_cout.n, C, co_p); conv2d(d, H, W, H, W); CTRLV_TRY(gemm(c, d)); }
  c.drop(xn);
  CTRLV_TRY(c.run([&] { return ctrlv_time_conv_rows_to_nchw(rows, co_p, n, co, H * W, p->tco_w, p->tco_b, frames, out_dtype, c.st); }));
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
  Ctx c{{nullptr, true}, p, kFakeBase};
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
    ctrlv_walk::DeviceScope on(p->device);
    free_owned(p);
  }
  delete p;
  return CTRLV_OK;
}

extern "C" int ctrlv_vae_plan_load_weights(ctrlv_vae_plan* p, const ctrlv_tensor_desc* tensors, size_t n) {
  CTRLV_CHECK_ARG(p && tensors, "vae_plan_load_weights: null argument");
  WeightLoader L("vae_plan_load_weights", &p->owned);
  const int rc = ctrlv_load::run_load(L, p->device, true, [&]() -> int {
    free_owned(p);
    L.add(tensors, n);
    return load_all(L, p);
  });
  if (rc != CTRLV_OK) { free_owned(p); return rc; }
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
  CTRLV_CHECK_DTYPE(dtype >= 0 && dtype <= 2 && out_dtype >= 0 && out_dtype <= 2, "vae_encode: dtype codes %d / %d (0 fp32, 1 fp16, 2 bf16)",
                    dtype, out_dtype);
  CTRLV_TRY(check_encode_shape(p, n, Hpx, Wpx));
  CTRLV_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "vae_encode: workspace must be 256-byte aligned");
  const size_t need = dry_bytes(p, 0, n, 0, Hpx, Wpx);
  if (workspace_bytes < need) {
    ctrlv_set_error("vae_encode: workspace of %zu bytes, %zu needed (ctrlv_vae_plan_workspace_bytes)", workspace_bytes, need);
    return CTRLV_E_WORKSPACE;
  }
  Ctx c{{(hipStream_t)stream, false}, p, (char*)workspace};
  return encode_walk(c, pixels, dtype, n, Hpx, Wpx, noise, scale, latents, moments, out_dtype);
}

extern "C" int ctrlv_vae_decode(ctrlv_vae_plan* p, const void* z, int dtype, int n, int num_frames, int h, int w, void* frames,
                                int out_dtype, void* workspace, size_t workspace_bytes, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(p && p->loaded, "vae_decode: plan not loaded");
  CTRLV_CHECK_ARG(z && frames && workspace, "vae_decode: null pointer");
  CTRLV_CHECK_DTYPE(dtype >= 0 && dtype <= 2 && out_dtype >= 0 && out_dtype <= 2, "vae_decode: dtype codes %d / %d (0 fp32, 1 fp16, 2 bf16)",
                    dtype, out_dtype);
  CTRLV_TRY(check_decode_shape(p, n, num_frames, h, w));
  CTRLV_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "vae_decode: workspace must be 256-byte aligned");
  const size_t need = dry_bytes(p, 1, n, num_frames, h, w);
  if (workspace_bytes < need) {
    ctrlv_set_error("vae_decode: workspace of %zu bytes, %zu needed (ctrlv_vae_plan_workspace_bytes)", workspace_bytes, need);
    return CTRLV_E_WORKSPACE;
  }
  const ctrlv_vae_config& cf = p->cfg;
  const size_t in_el = dtype == 0 ? 4 : 2, out_el = out_dtype == 0 ? 4 : 2;
  for (int c0 = 0; c0 < n; c0 += num_frames) {       // independent clips, one after the other in the same workspace
    Ctx c{{(hipStream_t)stream, false}, p, (char*)workspace};
    CTRLV_TRY(decode_clip(c, (const char*)z + (size_t)c0 * cf.latent_channels * h * w * in_el, dtype, num_frames, h, w,
                    (char*)frames + (size_t)c0 * cf.out_channels * 64 * h * w * out_el, out_dtype));
  }
  return CTRLV_OK;
}
