// The CLIP vision tower as ONE C call (include/ctrlv_hip.h "CLIP vision tower as ONE call"): what csrc/plan.hip is for the UNet
// and the ControlNet.  The per-op Python executor (models/clip_vision_hip.py encode) pays a ctypes call, a descriptor build and a
// split-plan query per launch, 262 times per ViT-H encode; here the walk is a C++ loop over packed, library-owned weights, fc1
// and its activation are one launch (ctrlv_gemm_tokens), and a host in any language can run it.
//
// Launches of one forward: 4 + 7 L + 2 kernels, one memset node per sliced weight shape (the K-slice counters of
// ctrlv_gemm_tokens, cleared once per forward: every sliced launch leaves them zero for the next; two shapes for ViT-H) and
// one strided copy node (the class rows).  One stream, one chain.
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

struct ClipLinear { el_t* w = nullptr; float* b = nullptr; int n = 0, k = 0; };
struct ClipNorm { float* g = nullptr; float* b = nullptr; };
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

__device__ __forceinline__ float ld_any(const void* p, int dtype, long i) {
  if (dtype == 0) return ((const float*)p)[i];
  if (dtype == 1) return (float)((const _Float16*)p)[i];
  return bf16_to_f32(((const bf16_t*)p)[i]);
}
// dst[(n_off + n) * ld + c] = src[n * C + c]   (dst pre-zeroed: the K padding)
__global__ void clip_pack_rows_kernel(const void* __restrict__ src, int dtype, long total, int C, el_t* __restrict__ dst, int ld,
                                      int n_off) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x)
    dst[(i / C + n_off) * ld + i % C] = f32_to_el(ld_any(src, dtype, i));
}
__global__ void clip_pack_f32_kernel(const void* __restrict__ src, int dtype, long total, float* __restrict__ dst) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x)
    dst[i] = ld_any(src, dtype, i);
}

inline unsigned blocks_for(long total) { return (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096); }

struct ClipLoader {
  ctrlv_clip_plan* p;
  std::unordered_map<std::string, const ctrlv_tensor_desc*> map;
  std::vector<void*> staged;

  int find(const std::string& name, long numel, const void** src, int* dtype) {
    auto it = map.find(name);
    if (it == map.end()) { ctrlv_set_error("clip_plan_load_weights: missing tensor '%s'", name.c_str()); return CTRLV_E_BAD_ARG; }
    const ctrlv_tensor_desc* t = it->second;
    if (t->numel != numel) {
      ctrlv_set_error("clip_plan_load_weights: '%s' has %ld elements, expected %ld", name.c_str(), (long)t->numel, numel);
      return CTRLV_E_BAD_SHAPE;
    }
    if (t->dtype < 0 || t->dtype > 2 || !t->data) {
      ctrlv_set_error("clip_plan_load_weights: '%s': dtype code %d / null data", name.c_str(), t->dtype);
      return CTRLV_E_BAD_DTYPE;
    }
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
  int alloc(size_t bytes, void** out, bool zero) {
    void* d = nullptr;
    CTRLV_HIP_TRY(hipMalloc(&d, bytes ? bytes : 256));
    p->owned.push_back(d);
    if (zero) CTRLV_HIP_TRY(hipMemsetAsync(d, 0, bytes ? bytes : 256, nullptr));
    *out = d;
    return CTRLV_OK;
  }
  int rows(const std::string& name, int N, int C, ClipLinear& l, int n_off) {
    const void* src;
    int dt;
    TRY(find(name, (long)N * C, &src, &dt));
    clip_pack_rows_kernel<<<blocks_for((long)N * C), 256, 0, nullptr>>>(src, dt, (long)N * C, C, l.w, l.k, n_off);
    CTRLV_LAUNCH_CHECK();
    return CTRLV_OK;
  }
  int vec(const std::string& name, long n, float* dst) {
    const void* src;
    int dt;
    TRY(find(name, n, &src, &dt));
    clip_pack_f32_kernel<<<blocks_for(n), 256, 0, nullptr>>>(src, dt, n, dst);
    CTRLV_LAUNCH_CHECK();
    return CTRLV_OK;
  }
  int new_linear(ClipLinear& l, int N, int K, bool bias) {
    l.n = (N + 31) / 32 * 32;
    l.k = (K + 63) / 64 * 64;
    TRY(alloc((size_t)l.n * l.k * 2, (void**)&l.w, true));
    l.b = nullptr;
    if (bias) TRY(alloc((size_t)l.n * 4, (void**)&l.b, true));
    return CTRLV_OK;
  }
  int linear(const std::string& mod, int N, int K, ClipLinear& l, bool bias) {
    TRY(new_linear(l, N, K, bias));
    TRY(rows(mod + ".weight", N, K, l, 0));
    if (bias) TRY(vec(mod + ".bias", N, l.b));
    return CTRLV_OK;
  }
  int norm(const std::string& mod, int C, ClipNorm& nm) {
    TRY(alloc((size_t)C * 4, (void**)&nm.g, false));
    TRY(alloc((size_t)C * 4, (void**)&nm.b, false));
    TRY(vec(mod + ".weight", C, nm.g));
    return vec(mod + ".bias", C, nm.b);
  }
};

void free_owned(ctrlv_clip_plan* p) {
  for (void* d : p->owned) (void)hipFree(d);
  p->owned.clear();
  p->layers.clear();
  p->loaded = false;
}

int load_all(ClipLoader& L) {
  ctrlv_clip_plan* p = L.p;
  const ctrlv_clip_config& c = p->cfg;
  const int C = c.hidden_size, I = c.intermediate_size, pp3 = 3 * c.patch_size * c.patch_size;
  const std::string vm = "vision_model.";
  TRY(L.linear(vm + "embeddings.patch_embedding", C, pp3, p->patch, false));
  TRY(L.alloc((size_t)C * 4, (void**)&p->cls, false));
  TRY(L.vec(vm + "embeddings.class_embedding", C, p->cls));
  TRY(L.alloc((size_t)p->tokens * C * 4, (void**)&p->pos, false));
  TRY(L.vec(vm + "embeddings.position_embedding.weight", (long)p->tokens * C, p->pos));
  TRY(L.norm(vm + "pre_layrnorm", C, p->pre));
  p->layers.resize(c.num_hidden_layers);
  for (int i = 0; i < c.num_hidden_layers; ++i) {
    ClipLayer& l = p->layers[i];
    const std::string b = vm + "encoder.layers." + std::to_string(i) + ".";
    TRY(L.norm(b + "layer_norm1", C, l.ln1));
    TRY(L.norm(b + "layer_norm2", C, l.ln2));
    TRY(L.new_linear(l.qkv, 3 * C, C, true));
    const char* names[3] = {"q_proj", "k_proj", "v_proj"};
    for (int j = 0; j < 3; ++j) {
      TRY(L.rows(b + "self_attn." + names[j] + ".weight", C, C, l.qkv, j * C));
      TRY(L.vec(b + "self_attn." + names[j] + ".bias", C, l.qkv.b + j * C));
    }
    TRY(L.linear(b + "self_attn.out_proj", C, C, l.out, true));
    TRY(L.linear(b + "mlp.fc1", I, C, l.fc1, true));
    TRY(L.linear(b + "mlp.fc2", C, I, l.fc2, true));
  }
  TRY(L.norm(vm + "post_layernorm", C, p->post));
  return L.linear("visual_projection", c.projection_dim, C, p->proj, false);
}

inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

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
  ctrlv_gemm_desc d;
  memset(&d, 0, sizeof d);
  d.A = A; d.W = l.w; d.out = out; d.bias = l.b; d.R1 = R1;
  d.M = M; d.N = N; d.Cin = l.k; d.taps = 1;
  d.lda = l.k; d.ldo = N; d.n_store = N; d.ldr1 = R1 ? N : 0;
  d.s_acc = 1.0f; d.s1 = 1.0f; d.s2 = 1.0f;
  d.vdiv = 1; d.vmod = 1 << 30; d.vS = 1;
  return ctrlv_gemm(&d, f.st);
}

int forward(ctrlv_clip_plan* p, const Regions& r, const void* px, int dtype, int n, el_t* embeds, el_t* lhs, hipStream_t st) {
  const ctrlv_clip_config& c = p->cfg;
  const int C = c.hidden_size, I = c.intermediate_size, S = p->tokens, P = S - 1, M = n * S;
  const float eps = c.layer_norm_eps;
  const Fwd f{&r, st};
  for (int i = 0; i < r.n_tws; ++i) CTRLV_HIP_TRY(hipMemsetAsync(r.tws[i].p, 0, r.tws[i].cnt, st));
  TRY(ctrlv_clip_patch_rows(px, dtype, n, c.image_size, c.image_size, c.patch_size, r.pr, p->kp, st));
  TRY(gemm_any(f, r.pr, p->patch, n * P, C, r.pe, nullptr, 0));
  TRY(ctrlv_clip_tokens(r.pe, p->cls, p->pos, n, P, C, r.tok, st));
  el_t* x = r.x;
  el_t* x2 = r.x2;
  TRY(ctrlv_layernorm(r.tok, M, C, p->pre.g, p->pre.b, eps, nullptr, 1, 1 << 30, 0, x, st));
  const int L = (int)p->layers.size();
  for (int i = 0; i < L; ++i) {
    const ClipLayer& l = p->layers[i];
    TRY(ctrlv_layernorm(x, M, C, l.ln1.g, l.ln1.b, eps, nullptr, 1, 1 << 30, 0, r.hn, st));
    TRY(gemm_any(f, r.hn, l.qkv, M, 3 * C, r.qkv, nullptr, 0));
    TRY(ctrlv_attention_tokens(r.qkv, r.att, n, S, C, C / c.num_attention_heads, st));
    TRY(gemm_any(f, r.att, l.out, M, C, x2, x, 0));
    std::swap(x, x2);
    TRY(ctrlv_layernorm(x, M, C, l.ln2.g, l.ln2.b, eps, nullptr, 1, 1 << 30, 0, r.hn, st));
    TRY(gemm_any(f, r.hn, l.fc1, M, I, r.u, nullptr, 1 + c.hidden_act));
    el_t* dst = (i == L - 1 && lhs) ? lhs : x2;        // the last layer writes last_hidden_state in place
    TRY(gemm_any(f, r.u, l.fc2, M, C, dst, x, 0));
    x2 = x;
    x = dst;
  }
  // class rows: row 0 of every image (a strided copy node), then post_layernorm and the projection at M = n
  CTRLV_HIP_TRY(hipMemcpy2DAsync(r.cls, (size_t)C * 2, x, (size_t)S * C * 2, (size_t)C * 2, n, hipMemcpyDeviceToDevice, st));
  TRY(ctrlv_layernorm(r.cls, n, C, p->post.g, p->post.b, eps, nullptr, 1, 1 << 30, 0, r.pn, st));
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
    int dev = 0;
    const bool sw = hipGetDevice(&dev) == hipSuccess && dev != p->device;
    if (sw) (void)hipSetDevice(p->device);
    free_owned(p);
    if (sw) (void)hipSetDevice(dev);
  }
  delete p;
  return CTRLV_OK;
}

extern "C" int ctrlv_clip_plan_load_weights(ctrlv_clip_plan* p, const ctrlv_tensor_desc* tensors, size_t n) {
  CTRLV_CHECK_ARG(p && tensors, "clip_plan_load_weights: null argument");
  int prev = 0;
  const bool sw = hipGetDevice(&prev) == hipSuccess && prev != p->device;
  CTRLV_HIP_TRY(hipSetDevice(p->device));
  free_owned(p);
  ClipLoader L;
  L.p = p;
  for (size_t i = 0; i < n; ++i)
    if (tensors[i].name) L.map[tensors[i].name] = &tensors[i];
  const int rc = load_all(L);
  const hipError_t e = hipDeviceSynchronize();
  for (void* d : L.staged) (void)hipFree(d);
  if (sw) (void)hipSetDevice(prev);                              // the caller's device, as ctrlv_clip_plan_destroy leaves it
  if (rc != CTRLV_OK) { free_owned(p); return rc; }
  if (e != hipSuccess) {
    free_owned(p);
    ctrlv_set_error("clip_plan_load_weights: %s", hipGetErrorString(e));
    return CTRLV_E_HIP;
  }
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
  if (dtype < 0 || dtype > 2) {
    ctrlv_set_error("clip_forward: dtype code %d (0 fp32, 1 fp16, 2 bf16)", dtype);
    return CTRLV_E_BAD_DTYPE;
  }
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
