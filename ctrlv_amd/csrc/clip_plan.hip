// The CLIP vision tower as ONE C call (include/ctrlv_hip.h "CLIP vision tower as ONE call"): what csrc/plan.hip is for the UNet
// and the ControlNet.  The per-op Python executor (models/clip_vision_hip.py encode) pays a ctypes call, a descriptor build and a
// split-plan query per launch, 262 times per ViT-H encode; here the walk is a C++ loop over packed, library-owned weights, fc1
// and its activation are one launch (ctrlv_gemm_tokens), and a host in any language can run it.
//
// Launches of one forward: 4 + 7 L + 2 kernels, one memset node per sliced weight shape (the K-slice counters of
// ctrlv_gemm_tokens, cleared once per forward: every sliced launch leaves them zero for the next; two shapes for ViT-H) and
// one strided copy node (the class rows).  One stream, one chain.
#include <string>
#include <vector>

#include "plan_walk.h"
#include "weight_loader.h"

namespace {

using ctrlv_load::WeightLoader;
using ClipLinear = ctrlv_load::PackedLinear;
using ClipNorm = ctrlv_load::NormParams;
struct ClipLayer { ClipNorm ln1, ln2; ClipLinear qkv, out, fc1, fc2; };

}  // namespace

struct ctrlv_clip_plan {
  ctrlv_clip_config cfg;
  int device = 0;
  bool loaded = false;
  int tokens = 0, kp = 0;                 // tokens per image (patches + 1); patch row width 3 patch^2 rounded up to 64
  std::vector<void*> owned;
  ClipLinear patch, proj;
  float* cls = nullptr;
  float* pos = nullptr;
  ClipNorm pre, post;
  std::vector<ClipLayer> layers;
};

const ctrlv_clip_config* ctrlv_clip_plan_info(const ctrlv_clip_plan* p, int* device, int* loaded) {
  if (device) *device = p->device;
  if (loaded) *loaded = p->loaded ? 1 : 0;
  return &p->cfg;
}

namespace {

// Which GEMM serves a layer's (N, K): true = ctrlv_gemm_tokens, false = ctrlv_gemm.  Keyed on the weight's shape only, never
// on the batch.  fc1 is not in the table: it always takes ctrlv_gemm_tokens, the only GEMM with the activation epilogue.
// Read off profiles/gemm_tokens_bench.jsonl (tools/gemm_tokens_bench.py, one MI355X, device time per launch from HIP-graph
// replays, us, tokens / gemm, bf16; fp16 within 1 %):
//                                      M = 257 (256)      M = 2056 (2048)
//   patch     640 -> 1280              10.0 / 15.1        40.0 / 16.2
//   q|k|v    1280 -> 3840              21.7 / 24.5       119.9 / 32.3
//   out_proj 1280 -> 1280              13.0 / 27.1        75.0 / 31.2
//   fc1      1280 -> 5120 (+ GELU)     24.2 / 28.6       126.4 / 47.4     (gemm arm: + act_rows)
//   fc2      5120 -> 1280              28.6 / 79.8       116.4 / 92.2
// The sliced kernel wins every shape at one image and loses every shape at eight (its fp32 slabs grow with M; the slice count
// may not).  A shape is routed to it where what it gains at one image exceeds what it loses at eight: fc2 only (- 51 / + 24
// us; out_proj - 14 / + 44, patch - 5 / + 24, q|k|v - 3 / + 88) -- the long-K, narrow-N case, where ctrlv_gemm walks K = 5120
// on 10 workgroups.
inline bool use_tokens(int N, int K) { return K >= 4096 && K >= 4 * N; }

void free_owned(ctrlv_clip_plan* p) {
  for (void* d : p->owned) (void)hipFree(d);
  p->owned.clear();
  p->layers.clear();
  p->loaded = false;
}

int load_all(WeightLoader& L, ctrlv_clip_plan* p) {
  const ctrlv_clip_config& c = p->cfg;
  const int C = c.hidden_size, I = c.intermediate_size, pp3 = 3 * c.patch_size * c.patch_size;
  const std::string vm = "vision_model.";
  CTRLV_TRY(L.linear(vm + "embeddings.patch_embedding", C, pp3, p->patch, false));
  CTRLV_TRY(L.vec(vm + "embeddings.class_embedding", C, &p->cls));
  CTRLV_TRY(L.vec(vm + "embeddings.position_embedding.weight", (long)p->tokens * C, &p->pos));
  CTRLV_TRY(L.norm(vm + "pre_layrnorm", C, p->pre));
  p->layers.resize(c.num_hidden_layers);
  for (int i = 0; i < c.num_hidden_layers; ++i) {
    ClipLayer& l = p->layers[i];
    const std::string b = vm + "encoder.layers." + std::to_string(i) + ".";
    CTRLV_TRY(L.norm(b + "layer_norm1", C, l.ln1));
    CTRLV_TRY(L.norm(b + "layer_norm2", C, l.ln2));
    CTRLV_TRY(L.new_linear(l.qkv, 3 * C, pad_to(C, 64), true));
    const char* names[3] = {"q_proj", "k_proj", "v_proj"};
    for (int j = 0; j < 3; ++j) {
      CTRLV_TRY(L.pack_w(b + "self_attn." + names[j] + ".weight", C, C, 1, l.qkv, 0, 0, j * C, 0));
      CTRLV_TRY(L.pack_v(b + "self_attn." + names[j] + ".bias", C, l.qkv.b, j * C, 0, 0));
    }
    CTRLV_TRY(L.linear(b + "self_attn.out_proj", C, C, l.out));
    CTRLV_TRY(L.linear(b + "mlp.fc1", I, C, l.fc1));
    CTRLV_TRY(L.linear(b + "mlp.fc2", C, I, l.fc2));
  }
  CTRLV_TRY(L.norm(vm + "post_layernorm", C, p->post));
  return L.linear("visual_projection", c.projection_dim, C, p->proj, false);
}

// One ctrlv_gemm_tokens workspace per sliced weight shape: the counter block at its head is sized by the shape, so two shapes
// must not share one (the slabs of the smaller block would overwrite the counters of the larger).
struct TokWs { int N = 0, K = 0; char* p = nullptr; size_t bytes = 0, cnt = 0; };

// the forward's buffers inside the caller's workspace
struct Regions {
  el_t *pr, *pe, *tok, *x, *x2, *hn, *qkv, *att, *u, *cls, *pn;
  TokWs tws[5];
  int n_tws;
  size_t total;
};

Regions carve(const ctrlv_clip_plan* p, int n, char* base) {
  const ctrlv_clip_config& c = p->cfg;
  const size_t C = c.hidden_size, I = c.intermediate_size, S = p->tokens, P = S - 1, M = (size_t)n * S;
  Regions r;
  size_t off = 0;
  auto take = [&](size_t elems) { el_t* q = (el_t*)(base + off); off += up256(elems * 2); return q; };
  r.pr = take((size_t)n * P * p->kp);
  r.pe = take((size_t)n * P * C);
  r.tok = take(M * C);
  r.x = take(M * C);
  r.x2 = take(M * C);
  r.hn = take(M * C);
  r.qkv = take(M * 3 * C);
  r.att = take(M * C);
  r.u = take(M * I);
  r.cls = take((size_t)n * C);
  r.pn = take((size_t)n * C);
  r.n_tws = 0;
  auto add = [&](int Mi, int N, int K) {
    for (int i = 0; i < r.n_tws; ++i)
      if (r.tws[i].N == N && r.tws[i].K == K) return;
    const size_t cnt = ctrlv_gemm_tokens_counter_bytes(Mi, N, K);
    if (!cnt) return;                                          // not sliced: no workspace
    TokWs& t = r.tws[r.n_tws++];
    t.N = N; t.K = K;
    t.p = base + off;
    t.bytes = ctrlv_gemm_tokens_ws_bytes(Mi, N, K);
    t.cnt = cnt;
    off += up256(t.bytes);
  };
  const int Mi = (int)M, Ci = (int)C, Ii = (int)I;
  add(Mi, Ii, Ci);                                              // fc1: always
  if (use_tokens(Ci, p->kp)) add(n * (int)P, Ci, p->kp);
  if (use_tokens(3 * Ci, Ci)) add(Mi, 3 * Ci, Ci);
  if (use_tokens(Ci, Ci)) add(Mi, Ci, Ci);
  if (use_tokens(Ci, Ii)) add(Mi, Ci, Ii);
  r.total = off;
  return r;
}

struct Fwd {
  const Regions* r;
  hipStream_t st;
};

// out[M, N] = act(A . l.w^T + l.b) + R1 on the GEMM the table names for (N, K)
int gemm_any(const Fwd& f, const el_t* A, const ClipLinear& l, int M, int N, el_t* out, const el_t* R1, int act) {
  if (act || use_tokens(N, l.k)) {
    ctrlv_gemm_tokens_desc d;
    memset(&d, 0, sizeof d);
    d.A = A; d.W = l.w; d.bias = l.b; d.R1 = R1; d.out = out;
    for (int i = 0; i < f.r->n_tws; ++i)
      if (f.r->tws[i].N == N && f.r->tws[i].K == l.k) { d.workspace = f.r->tws[i].p; d.workspace_bytes = f.r->tws[i].bytes; }
    d.M = M; d.N = N; d.K = l.k;
    d.lda = l.k; d.ldr1 = N; d.ldo = N;
    d.act = act;
    d.ws_zeroed = 1;            // forward() cleared this shape's counters once; every sliced launch leaves them zero
    return ctrlv_gemm_tokens(&d, f.st);
  }
  ctrlv_gemm_desc d = ctrlv_linear_desc(A, l.k, l, out, N, M, N, l.k, N);
  d.R1 = R1; d.ldr1 = R1 ? N : 0;
  return ctrlv_gemm(&d, f.st);
}

int forward(ctrlv_clip_plan* p, const Regions& r, const void* px, int dtype, int n, el_t* embeds, el_t* lhs, hipStream_t st) {
  const ctrlv_clip_config& c = p->cfg;
  const int C = c.hidden_size, I = c.intermediate_size, S = p->tokens, P = S - 1, M = n * S;
  const float eps = c.layer_norm_eps;
  const Fwd f{&r, st};
  for (int i = 0; i < r.n_tws; ++i) CTRLV_HIP_TRY(hipMemsetAsync(r.tws[i].p, 0, r.tws[i].cnt, st));
  CTRLV_TRY(ctrlv_clip_patch_rows(px, dtype, n, c.image_size, c.image_size, c.patch_size, r.pr, p->kp, st));
  CTRLV_TRY(gemm_any(f, r.pr, p->patch, n * P, C, r.pe, nullptr, 0));
  CTRLV_TRY(ctrlv_clip_tokens(r.pe, p->cls, p->pos, n, P, C, r.tok, st));
  el_t* x = r.x;
  el_t* x2 = r.x2;
  CTRLV_TRY(ctrlv_layernorm(r.tok, M, C, p->pre.g, p->pre.b, eps, nullptr, 1, 1 << 30, 0, x, st));
  const int L = (int)p->layers.size();
  for (int i = 0; i < L; ++i) {
    const ClipLayer& l = p->layers[i];
    CTRLV_TRY(ctrlv_layernorm(x, M, C, l.ln1.g, l.ln1.b, eps, nullptr, 1, 1 << 30, 0, r.hn, st));
    CTRLV_TRY(gemm_any(f, r.hn, l.qkv, M, 3 * C, r.qkv, nullptr, 0));
    CTRLV_TRY(ctrlv_attention_tokens(r.qkv, r.att, n, S, C, C / c.num_attention_heads, st));
    CTRLV_TRY(gemm_any(f, r.att, l.out, M, C, x2, x, 0));
    std::swap(x, x2);
    CTRLV_TRY(ctrlv_layernorm(x, M, C, l.ln2.g, l.ln2.b, eps, nullptr, 1, 1 << 30, 0, r.hn, st));
    CTRLV_TRY(gemm_any(f, r.hn, l.fc1, M, I, r.u, nullptr, 1 + c.hidden_act));
    el_t* dst = (i == L - 1 && lhs) ? lhs : x2;        // the last layer writes last_hidden_state in place
    CTRLV_TRY(gemm_any(f, r.u, l.fc2, M, C, dst, x, 0));
    x2 = x;
    x = dst;
  }
  // class rows: row 0 of every image (a strided copy node), then post_layernorm and the projection at M = n
  CTRLV_HIP_TRY(hipMemcpy2DAsync(r.cls, (size_t)C * 2, x, (size_t)S * C * 2, (size_t)C * 2, n, hipMemcpyDeviceToDevice, st));
  CTRLV_TRY(ctrlv_layernorm(r.cls, n, C, p->post.g, p->post.b, eps, nullptr, 1, 1 << 30, 0, r.pn, st));
  return gemm_any(f, r.pn, p->proj, n, c.projection_dim, embeds, nullptr, 0);
}

}  // namespace

extern "C" int ctrlv_clip_plan_create(const ctrlv_clip_config* cfg, int device, ctrlv_clip_plan** out) {
  CTRLV_CHECK_ARG(cfg && out, "clip_plan_create: null argument");
  const ctrlv_clip_config& c = *cfg;
  CTRLV_CHECK_SHAPE(c.hidden_size > 0 && c.hidden_size % 64 == 0 && c.hidden_size <= 2048,
                    "clip_plan_create: hidden_size=%d must be a multiple of 64, at most 2048", c.hidden_size);
  CTRLV_CHECK_SHAPE(c.intermediate_size > 0 && c.intermediate_size % 64 == 0,
                    "clip_plan_create: intermediate_size=%d must be a multiple of 64", c.intermediate_size);
  CTRLV_CHECK_SHAPE(c.projection_dim > 0 && c.projection_dim % 32 == 0, "clip_plan_create: projection_dim=%d must be a multiple of 32",
                    c.projection_dim);
  CTRLV_CHECK_SHAPE(c.num_hidden_layers >= 1, "clip_plan_create: num_hidden_layers=%d", c.num_hidden_layers);
  CTRLV_CHECK_SHAPE(c.num_attention_heads >= 1 && c.hidden_size % c.num_attention_heads == 0,
                    "clip_plan_create: hidden_size=%d is not a multiple of num_attention_heads=%d", c.hidden_size, c.num_attention_heads);
  const int hd = c.hidden_size / c.num_attention_heads;
  CTRLV_CHECK_SHAPE(hd % 16 == 0 && hd >= 16 && hd <= 128, "clip_plan_create: head_dim=%d must be a multiple of 16 in [16, 128]", hd);
  CTRLV_CHECK_SHAPE(c.patch_size > 0 && c.patch_size <= 64 && c.image_size > 0 && c.image_size % c.patch_size == 0,
                    "clip_plan_create: image_size=%d is not a whole number of patches of %d", c.image_size, c.patch_size);
  const int side = c.image_size / c.patch_size;
  CTRLV_CHECK_SHAPE(side * side + 1 <= 4096, "clip_plan_create: %d tokens, at most 4096", side * side + 1);
  CTRLV_CHECK_ARG(c.hidden_act == 0 || c.hidden_act == 1, "clip_plan_create: hidden_act %d (0 gelu, 1 quick_gelu)", c.hidden_act);
  CTRLV_CHECK_ARG(c.layer_norm_eps > 0.f, "clip_plan_create: layer_norm_eps must be positive");
  ctrlv_clip_plan* p = new ctrlv_clip_plan();
  p->cfg = c;
  p->device = device;
  p->tokens = side * side + 1;
  p->kp = (3 * c.patch_size * c.patch_size + 63) / 64 * 64;
  *out = p;
  return CTRLV_OK;
}

extern "C" int ctrlv_clip_plan_destroy(ctrlv_clip_plan* p) {
  if (!p) return CTRLV_OK;
  if (!p->owned.empty()) {
    ctrlv_walk::DeviceScope on(p->device);
    free_owned(p);
  }
  delete p;
  return CTRLV_OK;
}

extern "C" int ctrlv_clip_plan_load_weights(ctrlv_clip_plan* p, const ctrlv_tensor_desc* tensors, size_t n) {
  CTRLV_CHECK_ARG(p && tensors, "clip_plan_load_weights: null argument");
  WeightLoader L("clip_plan_load_weights", &p->owned);
  const int rc = ctrlv_load::run_load(L, p->device, true, [&]() -> int {       // (the caller's device, as _destroy leaves it)
    free_owned(p);
    L.add(tensors, n);
    return load_all(L, p);
  });
  if (rc != CTRLV_OK) { free_owned(p); return rc; }
  p->loaded = true;
  return CTRLV_OK;
}

extern "C" size_t ctrlv_clip_plan_workspace_bytes(ctrlv_clip_plan* p, int n_img) {
  if (!p || !p->loaded) { ctrlv_set_error("clip_plan_workspace_bytes: plan not loaded"); return 0; }
  if (n_img < 1 || n_img > 65535) { ctrlv_set_error("clip_plan_workspace_bytes: n_img=%d must be in [1, 65535]", n_img); return 0; }
  return carve(p, n_img, nullptr).total;
}

extern "C" int ctrlv_clip_forward(ctrlv_clip_plan* p, const void* pixel_values, int dtype, int n_img, void* image_embeds,
                                  void* last_hidden_state, void* workspace, size_t workspace_bytes, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(p && p->loaded, "clip_forward: plan not loaded");
  CTRLV_CHECK_ARG(pixel_values && image_embeds && workspace, "clip_forward: null pointer");
  CTRLV_CHECK_DTYPE(dtype >= 0 && dtype <= 2, "clip_forward: dtype code %d (0 fp32, 1 fp16, 2 bf16)", dtype);
  CTRLV_CHECK_SHAPE(n_img >= 1 && n_img <= 65535, "clip_forward: n_img=%d must be in [1, 65535]", n_img);
  CTRLV_CHECK_ARG(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)image_embeds & 15) == 0 && ((uintptr_t)last_hidden_state & 15) == 0,
                  "clip_forward: workspace must be 256-byte aligned, outputs 16-byte aligned");
  const Regions r = carve(p, n_img, (char*)workspace);
  if (workspace_bytes < r.total) {
    ctrlv_set_error("clip_forward: workspace of %zu bytes, %zu needed (ctrlv_clip_plan_workspace_bytes)", workspace_bytes, r.total);
    return CTRLV_E_WORKSPACE;
  }
  return forward(p, r, pixel_values, dtype, n_img, (el_t*)image_embeds, (el_t*)last_hidden_state, (hipStream_t)stream);
}
