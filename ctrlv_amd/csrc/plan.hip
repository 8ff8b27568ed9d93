// Plan-level C ABI: the execution plan of one UNetSpatioTemporalConditionModel / ControlNetModel instance.
//
//   ctrlv_plan_create        builds the module graph from the diffusers-style config (the wiring of
//                            src/ctrlv/models/controlnet.py:100-195 and of the diffusers parent UNet class)
//   ctrlv_plan_load_weights  takes every parameter by its diffusers state-dict key and packs it ON THE DEVICE into the
//                            layouts the kernels consume (include/ctrlv_hip.h: ctrlv_gemm_desc)
//   ctrlv_{unet,controlnet}_forward   walk the layer list and issue the kernels of this library on the caller's stream,
//                            with every activation in a stack-discipline arena over the caller's workspace
//
// The walk is the C++ twin of ctrlv_amd/models/{blocks,encoder,unet_spatio_temporal_condition,controlnet}.py: same
// kernels, same descriptors, same order -- the two executors produce bit-identical outputs (tests/test_plan_gpu.py).
#include <math.h>

#include <string>
#include <vector>

#include "plan_walk.h"
#include "weight_loader.h"

namespace {

using ctrlv_load::WeightLoader;
using ctrlv_walk::conv2d;
using ctrlv_walk::conv_t;
using ctrlv_walk::DeviceScope;
using ctrlv_walk::resid;
using Linear = ctrlv_load::PackedLinear;
using Norm = ctrlv_load::NormParams;

__global__ void arange_kernel(float* dst, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = (float)i;
}
__global__ void expand_f32_kernel(const float* __restrict__ src, int n_src, float* __restrict__ dst, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[n_src == 1 ? 0 : i];
}

// ------------------------------------------------------------------------------------------------ plan data
struct ResBlock {
  int cin = 0, cout = 0;
  float eps = 1e-6f;
  double alpha = 0.5;     // sigmoid(mix_factor), kept in double: 1 - alpha is formed in double like the Python executor does
  Norm n1, n2, tn1, tn2;
  Linear c1, c2, tc1, tc2, sc;
  bool has_sc = false;
  int temb_off[2] = {0, 0};
  std::string name;
};
struct FeedFwd {
  Linear proj, out;
  el_t* w1f = nullptr;      // C = 320 only: the fragment-major forms of ctrlv_ff_fused (ff_fused.hip), else null
  el_t* w2f = nullptr;
  // FF precision 1 (ctrlv_plan_set_ff_precision): the e4m3 codes of proj.w / out.w and their per-row scales
  // (ctrlv_quant_rows_f8 of the packed weights; only where both K are multiples of 128), else null
  uint8_t* proj8 = nullptr; float* proj8_s = nullptr;
  uint8_t* out8 = nullptr; float* out8_s = nullptr;
};
struct Transformer {
  int C = 0;
  double alpha = 0.5;
  Norm gn, s_ln1, s_ln3, t_lnin, t_ln1, t_ln3;
  Linear pin, pout, s_qkv, s_o, t_qkv, t_o, tpe1, tpe2;
  FeedFwd s_ff, t_ffin, t_ff;
  el_t* t_wf = nullptr;           // C = 320 only: fragment-major q|k|v + to_out of the temporal attention (temporal_fused.hip)
  el_t* se_wf = nullptr;          // C = 320 only: fragment-major proj_in + spatial q|k|v (spatial_entry_fused.hip)
  int xattn_off[2] = {0, 0};
  float* frame_emb = nullptr;     // [cfg.num_frames][C] fp32, prepared at load time
  std::string name;
};
struct Resample {
  int C = 0; Linear conv; bool present = false;
  el_t* wph = nullptr;      // up-sampler only: the four 2x2 phase panels [4][C][4 C] (ctrlv_pack_up_phase_weight), for up = 2
};
struct DownBlock { std::vector<ResBlock> res; std::vector<Transformer> attn; Resample down; };
struct UpBlock { std::vector<ResBlock> res; std::vector<Transformer> attn; Resample up; };
struct CrossOut { int off, c; Linear to_out; };

}  // namespace

struct ctrlv_plan {
  ctrlv_model_config cfg;
  int device = 0;
  bool loaded = false;
  int trunk_mode = 0;         // 0: plain residual trunk, 1: SPLIT hi + lo planes (ctrlv_plan_set_trunk_mode)
  int ff_precision = 0;       // 0: feed-forward GEMMs in the element type, 1: e4m3 operands (ctrlv_plan_set_ff_precision)
  std::vector<void*> owned_f8;   // the e4m3 feed-forward weights and scales (made when the mode is set / at load_weights)
  std::vector<DownBlock> down;
  ResBlock mid_r0, mid_r1;
  Transformer mid_attn;
  std::vector<UpBlock> up;
  Linear cin, te1, te2, ae1, ae2, temb, xv, cout;
  int cin_cp = 0, cin_kp = 0, temb_n = 0, xattn_n = 0;
  std::vector<CrossOut> xouts;
  Norm gno;
  std::vector<Linear> zc;     // controlnet_down_blocks
  Linear zc_mid;
  std::vector<void*> owned;   // every device allocation of load_weights
  struct WsEntry { int B, F, H, W; size_t bytes; };
  std::vector<WsEntry> ws_cache;   // ctrlv_plan_workspace_bytes per input shape (check_workspace)
  // per-launch profile of the plan's OWN launches (ctrlv_plan_profile): HIP events on the launch stream around every
  // kernel the walk issues, with the launch's algorithmic FLOPs / bytes -- bench.py's roofline leg and tools/shape_table.py
  struct ProfRec { ctrlv_profile_record r; hipEvent_t e0, e1; };
  bool profiling = false;
  std::vector<ProfRec> prof;
};

const ctrlv_model_config* ctrlv_plan_info(const ctrlv_plan* p, int* device, int* loaded) {
  if (device) *device = p->device;
  if (loaded) *loaded = p->loaded ? 1 : 0;
  return &p->cfg;
}

namespace {

// ------------------------------------------------------------------------------------------------ graph construction
void make_res(ResBlock& r, int cin, int cout, float eps, const std::string& name) {
  r.cin = cin; r.cout = cout; r.eps = eps; r.has_sc = cin != cout; r.name = name;
}
void make_tr(Transformer& t, int C, const std::string& name) { t.C = C; t.name = name; }

int build_graph(ctrlv_plan* p) {
  const ctrlv_model_config& c = p->cfg;
  const int n = c.n_blocks;
  CTRLV_CHECK_ARG(n >= 1 && n <= CTRLV_MAX_BLOCKS, "plan: n_blocks=%d out of range", n);
  CTRLV_CHECK_ARG(c.kind == 0 || c.kind == 1, "plan: kind must be 0 (UNet) or 1 (ControlNet)");
  for (int i = 0; i < n; ++i) {
    const int ch = c.block_out_channels[i];
    CTRLV_CHECK_SHAPE(ch > 0 && ch % 32 == 0, "plan: block_out_channels[%d]=%d must be a multiple of 32", i, ch);
    const bool attn = c.down_cross_attn[i] || (c.kind == 0 && c.up_cross_attn[n - 1 - i]) || i == n - 1;   // (mid block)
    if (attn)
      CTRLV_CHECK_SHAPE(c.num_attention_heads[i] > 0 && ch == c.num_attention_heads[i] * 64,
                        "plan: attention kernels are specialised for head_dim 64 (block %d: %d channels / %d heads)", i,
                        ch, c.num_attention_heads[i]);
    CTRLV_CHECK_ARG(c.layers_per_block[i] >= 1, "plan: layers_per_block[%d] must be >= 1", i);
  }
  p->down.resize(n);
  int out_ch = c.block_out_channels[0];
  for (int i = 0; i < n; ++i) {
    const int in_ch = out_ch;
    out_ch = c.block_out_channels[i];
    DownBlock& b = p->down[i];
    const std::string base = "down_blocks." + std::to_string(i);
    // get_down_block: CrossAttnDownBlockSpatioTemporal resnets eps 1e-6, DownBlockSpatioTemporal 1e-5
    const float eps = c.down_cross_attn[i] ? 1e-6f : 1e-5f;
    b.res.resize(c.layers_per_block[i]);
    for (int j = 0; j < c.layers_per_block[i]; ++j)
      make_res(b.res[j], j == 0 ? in_ch : out_ch, out_ch, eps, base + ".resnets." + std::to_string(j));
    if (c.down_cross_attn[i]) {
      b.attn.resize(c.layers_per_block[i]);
      for (int j = 0; j < c.layers_per_block[i]; ++j) make_tr(b.attn[j], out_ch, base + ".attentions." + std::to_string(j));
    }
    b.down.present = i != n - 1;
    b.down.C = out_ch;
  }
  const int cm = c.block_out_channels[n - 1];
  make_res(p->mid_r0, cm, cm, 1e-5f, "mid_block.resnets.0");
  make_res(p->mid_r1, cm, cm, 1e-5f, "mid_block.resnets.1");
  make_tr(p->mid_attn, cm, "mid_block.attentions.0");
  if (c.kind == 0) {
    p->up.resize(n);
    int prev = c.block_out_channels[n - 1];
    for (int i = 0; i < n; ++i) {
      const int oc = c.block_out_channels[n - 1 - i];
      const int ic = c.block_out_channels[n - 1 - (i + 1 < n ? i + 1 : n - 1)];
      const int layers = c.layers_per_block[n - 1 - i] + 1;
      UpBlock& b = p->up[i];
      const std::string base = "up_blocks." + std::to_string(i);
      b.res.resize(layers);
      for (int j = 0; j < layers; ++j) {
        const int skip = j == layers - 1 ? ic : oc;
        const int rin = j == 0 ? prev : oc;
        make_res(b.res[j], rin + skip, oc, 1e-6f, base + ".resnets." + std::to_string(j));
      }
      if (c.up_cross_attn[i]) {
        b.attn.resize(layers);
        for (int j = 0; j < layers; ++j) make_tr(b.attn[j], oc, base + ".attentions." + std::to_string(j));
      }
      b.up.present = i != n - 1;
      b.up.C = oc;
      prev = oc;
    }
  }
  return CTRLV_OK;
}

template <class Fn>
void for_each_res(ctrlv_plan* p, Fn fn) {
  for (auto& b : p->down) for (auto& r : b.res) fn(r);
  fn(p->mid_r0); fn(p->mid_r1);
  for (auto& b : p->up) for (auto& r : b.res) fn(r);
}
template <class Fn>
void for_each_tr(ctrlv_plan* p, Fn fn) {
  for (auto& b : p->down) for (auto& t : b.attn) fn(t);
  fn(p->mid_attn);
  for (auto& b : p->up) for (auto& t : b.attn) fn(t);
}

// ------------------------------------------------------------------------------------------------ weight loading
// the phase panels of an up-sampler conv (ctrlv_gemm_desc.up = 2), from the parameter itself: taps summed in fp32, one rounding
int up_phase(WeightLoader& L, const std::string& mod, int N, int C, el_t** dst) {
  const ctrlv_tensor_desc* t;
  CTRLV_TRY(L.find(mod + ".weight", (long)N * C * 9, &t));
  const void* src;
  CTRLV_TRY(L.dev_ptr(t, &src));
  CTRLV_TRY(L.alloc((size_t)16 * N * C * 2, (void**)dst, false));
  return ctrlv_pack_up_phase_weight(src, t->dtype, N, C, *dst, L.st);
}
int ff(WeightLoader& L, const std::string& mod, int C, int C_out, FeedFwd& f) {     // FeedForward: GEGLU(C -> 8C) then Linear(4C -> C_out)
  CTRLV_TRY(L.linear(mod + ".net.0.proj", 8 * C, C, f.proj, true, 1));
  CTRLV_TRY(L.linear(mod + ".net.2", C_out, 4 * C, f.out));
  if (C == 320 && C_out == 320 && f.proj.n == 2560 && f.proj.k == 320 && f.out.n == 320 && f.out.k == 1280) {
    CTRLV_TRY(L.alloc((size_t)ctrlv_ff_fused_w1f_bytes(), (void**)&f.w1f, false));
    CTRLV_TRY(L.alloc((size_t)320 * 1280 * 2, (void**)&f.w2f, false));
    CTRLV_TRY(ctrlv_ff_fused_pack(f.proj.w, f.proj.b, f.out.w, f.w1f, f.w2f, L.st));
  }
  return CTRLV_OK;
}
int qkv(WeightLoader& L, const std::string& mod, int C, Linear& l) {
  CTRLV_TRY(L.new_linear(l, 3 * C, pad_to(C, 64), false));
  CTRLV_TRY(L.pack_w(mod + ".to_q.weight", C, C, 1, l, 0, 0, 0, 0));
  CTRLV_TRY(L.pack_w(mod + ".to_k.weight", C, C, 1, l, 0, 0, C, 0));
  return L.pack_w(mod + ".to_v.weight", C, C, 1, l, 0, 0, 2 * C, 0);
}

int load_res(WeightLoader& L, ctrlv_plan* p, ResBlock& r, int ted) {
  const std::string s = r.name + ".spatial_res_block", t = r.name + ".temporal_res_block";
  CTRLV_TRY(L.norm(s + ".norm1", r.cin, r.n1));
  CTRLV_TRY(L.conv3x3(s + ".conv1", r.cout, r.cin, r.c1));
  CTRLV_TRY(L.norm(s + ".norm2", r.cout, r.n2));
  CTRLV_TRY(L.conv3x3(s + ".conv2", r.cout, r.cout, r.c2));
  if (r.has_sc) CTRLV_TRY(L.linear(s + ".conv_shortcut", r.cout, r.cin, r.sc));
  CTRLV_TRY(L.norm(t + ".norm1", r.cout, r.tn1));
  CTRLV_TRY(L.conv_t(t + ".conv1", r.cout, r.cout, r.tc1));
  CTRLV_TRY(L.norm(t + ".norm2", r.cout, r.tn2));
  CTRLV_TRY(L.conv_t(t + ".conv2", r.cout, r.cout, r.tc2));
  CTRLV_TRY(L.mix_alpha(r.name + ".time_mixer.mix_factor", &r.alpha));
  // the two time_emb_proj rows go into the model-wide [sum Cout, ted] GEMM
  const std::string tp[2] = {s + ".time_emb_proj", t + ".time_emb_proj"};
  for (int k = 0; k < 2; ++k) {
    CTRLV_TRY(L.pack_w(tp[k] + ".weight", r.cout, ted, 1, p->temb, 0, 0, r.temb_off[k], 0));
    CTRLV_TRY(L.pack_v(tp[k] + ".bias", r.cout, p->temb.b, r.temb_off[k], 0, 0));
  }
  return CTRLV_OK;
}

int load_tr(WeightLoader& L, ctrlv_plan* p, Transformer& t, int cross_dim) {
  const int C = t.C;
  const std::string sb = t.name + ".transformer_blocks.0", tb = t.name + ".temporal_transformer_blocks.0";
  CTRLV_TRY(L.norm(t.name + ".norm", C, t.gn));
  CTRLV_TRY(L.linear(t.name + ".proj_in", C, C, t.pin));
  CTRLV_TRY(L.linear(t.name + ".proj_out", C, C, t.pout));
  CTRLV_TRY(L.norm(sb + ".norm1", C, t.s_ln1));
  CTRLV_TRY(L.norm(sb + ".norm3", C, t.s_ln3));
  CTRLV_TRY(qkv(L, sb + ".attn1", C, t.s_qkv));
  CTRLV_TRY(L.linear(sb + ".attn1.to_out.0", C, C, t.s_o));
  CTRLV_TRY(ff(L, sb + ".ff", C, C, t.s_ff));
  CTRLV_TRY(L.norm(tb + ".norm_in", C, t.t_lnin));
  CTRLV_TRY(L.norm(tb + ".norm1", C, t.t_ln1));
  CTRLV_TRY(L.norm(tb + ".norm3", C, t.t_ln3));
  CTRLV_TRY(ff(L, tb + ".ff_in", C, C, t.t_ffin));
  CTRLV_TRY(qkv(L, tb + ".attn1", C, t.t_qkv));
  CTRLV_TRY(L.linear(tb + ".attn1.to_out.0", C, C, t.t_o));
  CTRLV_TRY(ff(L, tb + ".ff", C, C, t.t_ff));
  if (C == 320 && t.t_qkv.n == 960 && t.t_qkv.k == 320 && t.t_o.n == 320 && t.t_o.k == 320) {
    CTRLV_TRY(L.alloc(ctrlv_temporal_fused_weight_bytes(), (void**)&t.t_wf, false));
    CTRLV_TRY(ctrlv_temporal_fused_pack(t.t_qkv.w, t.t_qkv.k, t.t_o.w, t.t_o.k, t.t_wf, L.st));
  }
  if (C == 320 && t.pin.n == 320 && t.pin.k == 320 && t.s_qkv.n == 960 && t.s_qkv.k == 320) {
    CTRLV_TRY(L.alloc(ctrlv_spatial_entry_fused_weight_bytes(), (void**)&t.se_wf, false));
    CTRLV_TRY(ctrlv_spatial_entry_fused_pack(t.pin.w, t.pin.k, t.s_qkv.w, t.s_qkv.k, t.se_wf, L.st));
  }
  CTRLV_TRY(L.linear(t.name + ".time_pos_embed.linear_1", 4 * C, C, t.tpe1));
  CTRLV_TRY(L.linear(t.name + ".time_pos_embed.linear_2", C, 4 * C, t.tpe2));
  CTRLV_TRY(L.mix_alpha(t.name + ".time_mixer.mix_factor", &t.alpha));
  // cross-attentions (1 key: attn2(x) = to_out(to_v(e)), SURVEY finding 8): to_v rows into the model-wide GEMM
  const std::string a2[2] = {sb + ".attn2", tb + ".attn2"};
  for (int k = 0; k < 2; ++k) {
    CTRLV_TRY(L.pack_w(a2[k] + ".to_v.weight", C, cross_dim, 1, p->xv, 0, 0, t.xattn_off[k], 0));
    CrossOut xo;
    xo.off = t.xattn_off[k];
    xo.c = C;
    CTRLV_TRY(L.linear(a2[k] + ".to_out.0", C, C, xo.to_out));
    p->xouts.push_back(xo);
  }
  return CTRLV_OK;
}

// ------------------------------------------------------------------------------------------------ execution context
// A tensor of the RESIDUAL TRUNK (block inputs / outputs, the tensors every branch result is added back into).  In trunk
// mode 1 it carries a second plane: value = hi + lo (include/ctrlv_hip.h, ctrlv_gemm_desc.out_lo).  GEMM A operands and
// the ABI's tensors read `hi`; residual operands (R1 / R2) and norm inputs read both.
struct Trk {
  el_t* hi = nullptr;
  lo_t* lo = nullptr;        // one byte per element (e5m2: common.h lo_t)
};
// The profile record of one launch (or launch group) of the walk: its family and algorithmic work.  family < 0: none (the
// layout kernels and copies around the model's inputs and outputs).
struct Prof { int family = -1; double flops = 0, bytes = 0; int M = 0, N = 0, K = 0, flags = 0; };
// While the plan is profiling: events on the launch stream before / after what runs in this scope.
struct ProfScope {
  ctrlv_plan* p = nullptr;
  hipStream_t st;
  size_t idx = 0;
  ProfScope(ctrlv_plan* plan, hipStream_t st_, const Prof& w) : st(st_) {
    if (w.family < 0 || !plan->profiling) return;
    ctrlv_plan::ProfRec pr;
    memset(&pr.r, 0, sizeof(pr.r));
    pr.r.family = w.family; pr.r.M = w.M; pr.r.N = w.N; pr.r.K = w.K; pr.r.flags = w.flags; pr.r.flops = w.flops; pr.r.bytes = w.bytes;
    if (hipEventCreate(&pr.e0) != hipSuccess || hipEventCreate(&pr.e1) != hipSuccess) return;
    (void)hipEventRecord(pr.e0, st);
    p = plan;
    idx = p->prof.size();
    p->prof.push_back(pr);
  }
  ~ProfScope() {
    if (p) (void)hipEventRecord(p->prof[idx].e1, st);
  }
};
struct Ctx : ctrlv_walk::LaunchGate {      // dry: the measuring pass of ctrlv_plan_workspace_bytes (no launches, no dereferences)
  ctrlv_plan* p;
  char* base;
  size_t cap, off = 0, peak = 0;
  bool overflow = false;
  int B, F;
  Ctx(ctrlv_plan* p_, hipStream_t st_, bool dry_, char* base_, size_t cap_, int B_, int F_)
      : LaunchGate{st_, dry_}, p(p_), base(base_), cap(cap_), B(B_), F(F_) {}
  float* temb = nullptr; int ldtemb = 0;
  float* xattn = nullptr; int ldx = 0;
  bool quirk = false;
  // GroupNorm chunk partials that cross a block boundary: written by the last GEMM of a res block (temporal conv2) for
  // the GroupNorm that opens the transformer behind it (one buffer per forward, used in stream order)
  float* gn_cross = nullptr; size_t gn_cross_floats = 0; bool gn_cross_valid = false;

  void* alloc(size_t bytes) {
    const size_t a = (bytes + 255) & ~(size_t)255;
    const size_t o = off;
    off += a;
    if (off > peak) peak = off;
    if (off > cap) overflow = true;
    return base + o;
  }
  // EVERY launch of the walk goes through here.  Measuring walk: nothing happens.  Live walk: `fn` runs between the events of
  // its profile record.  The refusal is a second line of defence that no entry point can reach: check_workspace has sized
  // the workspace with this same walk, whose peak bounds the live walk's, before anything was launched.
  template <class Fn>
  int launch(const Prof& work, Fn&& fn) {
    return run([&]() -> int {
      if (overflow) {
        ctrlv_set_error("plan forward: workspace too small (need >= %zu bytes)", peak);
        return CTRLV_E_WORKSPACE;
      }
      ProfScope ps(p, st, work);
      return fn();
    });
  }
  el_t* rows(long m, int c) { return (el_t*)alloc((size_t)m * c * 2); }
  Trk trunk(long m, int c) {          // a trunk tensor: one plane, or hi + lo in trunk mode 1
    Trk t;
    t.hi = rows(m, c);
    if (p->trunk_mode == 1) t.lo = (lo_t*)alloc((size_t)m * c);
    return t;
  }
  size_t mark() const { return off; }
  void release(size_t m) { off = m; }
};

// algorithmic work of a gather-GEMM launch (the accounting of ops.py: 2 MAC per output element and K step; operands once)
Prof gemm_work(const ctrlv_gemm_desc& d) {
  Prof w;
  w.family = d.mode == 1 ? CTRLV_FAM_GEMM_CONV3X3 : (d.mode == 2 ? CTRLV_FAM_GEMM_CONV_TEMPORAL : CTRLV_FAM_GEMM_LINEAR);
  const double n_alg = d.geglu ? d.N : (d.N < d.n_store ? d.N : d.n_store);
  const double n_out = d.geglu ? (d.n_store < d.N / 2 ? d.n_store : d.N / 2) : d.n_store;
  w.K = (d.mode == 1 && d.up == 2 ? 4 : d.taps) * d.Cin;                          // (phase form: 2x2 taps per output pixel)
  const double K = w.K;
  w.flops = 2.0 * d.M * n_alg * K;
  w.bytes = (double)d.M * d.Cin * 2 + (double)d.M * n_out * ((d.out_f32 & 1) ? 4 : 2) + (double)d.N * K * 2 * (d.mode == 1 && d.up == 2 ? 4 : 1) +
            (d.R1 ? (double)d.M * n_out * 2 : 0) + (d.R2 ? (double)d.M * n_out * 2 : 0) +
            ((d.R1_lo ? 1 : 0) + (d.R2_lo ? 1 : 0) + (d.out_lo ? 1 : 0)) * (double)d.M * n_out;       // (lo planes: 1 byte)
  w.M = d.M; w.N = d.N;
  w.flags = (d.geglu ? 1 : 0) | ((d.R1 ? 1 : 0) + (d.R2 ? 1 : 0)) << 1 | d.vmode << 3;
  return w;
}
// residual operand / output of a GEMM from a trunk tensor
inline void set_r1(ctrlv_gemm_desc& d, const Trk& t, int ld) { d.R1 = t.hi; d.R1_lo = t.lo; d.ldr1 = ld; }
inline void set_r2(ctrlv_gemm_desc& d, const Trk& t, int ld) { d.R2 = t.hi; d.R2_lo = t.lo; d.ldr2 = ld; }
inline void set_out(ctrlv_gemm_desc& d, const Trk& t) { d.out = t.hi; d.out_lo = t.lo; }
// a GroupNorm's record (algorithmic: 1 read + 1 write); flags 1: its statistics came from the producing GEMM's epilogue
inline Prof gn_work(int n_img, int S, int C, int flags) {
  return {CTRLV_FAM_GROUPNORM, 0.0, 2.0 * 2 * n_img * (double)S * C, n_img * S, C, 0, flags};
}

int gemm(Ctx& c, const ctrlv_gemm_desc& d0) {
  // split contraction of the small-image long-K convs (gemm.hip splitk_plan): its scratch comes from the arena for the
  // duration of the launch (the plan depends on the layer's shape only, so the measuring walk sees the same sizes)
  ctrlv_gemm_desc d = d0;
  const size_t mk = c.mark();
  const size_t ws = ctrlv_gemm_splitk_ws_bytes(&d);
  if (ws) d.splitk_ws = c.alloc(ws);
  const int rc = c.launch(gemm_work(d), [&] { return ctrlv_gemm(&d, c.st); });
  c.release(mk);
  return rc;
}
int groupnorm(Ctx& c, const Trk& x, const Trk& x2, int c_split, int n_img, int S, int C, int ips, const Norm& nm,
              float eps, int silu, el_t* y) {
  const int chunks = ctrlv_groupnorm_chunks(n_img, S, C, ips);
  if (chunks < 0) return chunks;
  const size_t m = c.mark();
  float* part = (float*)c.alloc(((size_t)n_img * chunks + n_img / ips) * 64 * 4);
  const int rc = c.launch(gn_work(n_img, S, C, 0), [&]() -> int {
    CTRLV_TRY(ctrlv_groupnorm_stats_split(x.hi, x.lo, x2.hi, x2.lo, c_split, n_img, S, C, ips, eps, part, c.st));
    return ctrlv_groupnorm_apply_split(x.hi, x.lo, x2.hi, x2.lo, c_split, n_img, S, C, ips, part, nm.g, nm.b, silu, y, c.st);
  });
  c.release(m);          // stream order keeps the scratch alive until the apply pass has read it
  return rc;
}
// A GEMM whose output goes straight into a GroupNorm (conv1 -> norm2, conv2 -> temporal norm1, temporal conv1 -> temporal
// norm2 of a res block): where the launch serves it, its epilogue writes the norm's chunk partials and the norm is
// finalize + apply -- one read and one write of the tensor instead of two reads.  The scratch is sized from the shape alone
// (the measuring walk has no operand pointers to ask the predicate with).
int gemm_groupnorm(Ctx& c, ctrlv_gemm_desc d, int n_img, int S, int C, int ips, const Norm& nm, float eps, int silu, el_t* y) {
  const Trk dout{(el_t*)d.out, (lo_t*)d.out_lo};
  if (S % 64 != 0) {
    CTRLV_TRY(gemm(c, d));
    return groupnorm(c, dout, Trk{}, 0, n_img, S, C, ips, nm, eps, silu, y);
  }
  const size_t m = c.mark();
  float* part = (float*)c.alloc(((size_t)n_img * (S / 64) + n_img / ips) * 64 * 4);
  if (!c.dry && ctrlv_gemm_gn_partials_serves(&d)) {      // (the predicate reads the operand pointers: live walk only)
    d.gn_partials = part;
    int rc = gemm(c, d);
    if (rc == CTRLV_OK)
      rc = c.launch(gn_work(n_img, S, C, 1), [&] {
        return ctrlv_groupnorm_from_partials_split(d.out, d.out_lo, n_img, S, C, ips, eps, part, nm.g, nm.b, silu, y, c.st);
      });
    c.release(m);
    return rc;
  }
  c.release(m);
  CTRLV_TRY(gemm(c, d));
  return groupnorm(c, dout, Trk{}, 0, n_img, S, C, ips, nm, eps, silu, y);
}
int layernorm(Ctx& c, const Trk& x, int M, int C, const Norm& nm, el_t* y, const float* V = nullptr, int vdiv = 1,
              int vmod = 1 << 30, int ldv = 0) {
  return c.launch({CTRLV_FAM_LAYERNORM, 0.0, 2.0 * 2 * (double)M * C, M, C},
                  [&] { return ctrlv_layernorm_split(x.hi, x.lo, M, C, nm.g, nm.b, 1e-5f, V, vdiv, vmod, ldv, y, c.st); });
}

// ---- SpatioTemporalResBlock (blocks.py::SpatioTemporalResBlock.run)
int run_res(Ctx& c, const ResBlock& r, const Trk& x, const Trk& x2, int c1, int H, int W, Trk* out_,
            bool feeds_norm = false) {
  const int N = c.B * c.F, S = H * W, F = c.F;
  const long M = (long)N * S;
  const int cin = r.cin, cout = r.cout;
  c.gn_cross_valid = false;
  if (feeds_norm && S % 64 == 0) {      // (sized from the shape alone, outside this block's scratch region)
    const size_t need = ((size_t)N * (S / 64) + N) * 64;
    if (c.gn_cross_floats < need) { c.gn_cross = (float*)c.alloc(need * 4); c.gn_cross_floats = need; }
  }
  const Trk out = c.trunk(M, cout);
  const size_t mk = c.mark();
  const int lda_x = x2.hi ? c1 : cin;
  el_t* xn = c.rows(M, cin);
  CTRLV_TRY(groupnorm(c, x, x2, x2.hi ? c1 : 0, N, S, cin, 1, r.n1, r.eps, 1, xn));
  el_t* h = c.rows(M, cout);
  el_t* hn = nullptr;
  {
    ctrlv_gemm_desc d = ctrlv_linear_desc(xn, cin, r.c1, h, cout, (int)M, cout, cin, cout);
    conv2d(d, H, W, H, W);
    d.V = c.temb + r.temb_off[0]; d.ldv = c.ldtemb; d.vmode = 1; d.vdiv = F * S;
    hn = c.rows(M, cout);
    CTRLV_TRY(gemm_groupnorm(c, d, N, S, cout, 1, r.n2, r.eps, 1, hn));
  }
  Trk res = x;
  int ldres = cin;
  if (r.has_sc) {
    const Trk rs = c.trunk(M, cout);
    ctrlv_gemm_desc d = ctrlv_linear_desc(x.hi, lda_x, r.sc, rs.hi, cout, (int)M, cout, cin, cout);
    set_out(d, rs);
    if (x2.hi) { d.A2 = x2.hi; d.lda2 = cin - c1; d.c_split = c1; }
    CTRLV_TRY(gemm(c, d));
    res = rs;
    ldres = cout;
  }
  const Trk xs = c.trunk(M, cout);
  {
    ctrlv_gemm_desc d = ctrlv_linear_desc(hn, cout, r.c2, xs.hi, cout, (int)M, cout, cout, cout);
    conv2d(d, H, W, H, W);
    set_out(d, xs);
    set_r1(d, res, ldres);
    CTRLV_TRY(gemm_groupnorm(c, d, N, S, cout, F, r.tn1, r.eps, 1, hn));
  }
  {
    ctrlv_gemm_desc d = ctrlv_linear_desc(hn, cout, r.tc1, h, cout, (int)M, cout, cout, cout);
    conv_t(d, F, S);
    d.V = c.temb + r.temb_off[1]; d.ldv = c.ldtemb; d.vmode = 1; d.vdiv = F * S;
    CTRLV_TRY(gemm_groupnorm(c, d, N, S, cout, F, r.tn2, r.eps, 1, hn));
  }
  {   // AlphaBlender: a*xs + (1-a)*(xs + conv2) = xs + (1-a)*conv2
    ctrlv_gemm_desc d = ctrlv_linear_desc(hn, cout, r.tc2, out.hi, cout, (int)M, cout, cout, cout);
    conv_t(d, F, S);
    d.s_acc = (float)(1.0 - r.alpha);
    set_out(d, out);
    set_r1(d, xs, cout);
    // (live walk only: the predicate reads the operand pointers, so gn_cross_valid is never set on the measuring walk)
    if (feeds_norm && S % 64 == 0 && !c.dry && ctrlv_gemm_gn_partials_serves(&d)) {
      d.gn_partials = c.gn_cross;       // the transformer behind this block opens with a GroupNorm of `out`
      c.gn_cross_valid = true;
    }
    CTRLV_TRY(gemm(c, d));
  }
  c.release(mk);
  *out_ = out;
  return CTRLV_OK;
}

// frame positional embedding table [F][C] fp32 = time_pos_embed(time_proj(arange(F)))  (depends on the weights and F only)
int frame_embedding(Ctx& c, const Transformer& t, int F, float* e) {
  const int C = t.C, kp = t.tpe1.k;
  const size_t mk = c.mark();
  float* ar = (float*)c.alloc((size_t)F * 4);
  el_t* te = c.rows(F, kp);
  el_t* hh = c.rows(F, 4 * C);
  el_t* tmp = kp != C ? c.rows(F, C) : nullptr;
  CTRLV_TRY(c.launch({}, [&]() -> int {
    hipLaunchKernelGGL(arange_kernel, dim3((F + 63) / 64), dim3(64), 0, c.st, ar, F);
    CTRLV_LAUNCH_CHECK();
    if (kp == C) return ctrlv_timestep_embedding(ar, F, C, te, c.st);
    // K zero padding (tiny configs only): sinusoid into a compact buffer, then strided copy
    CTRLV_HIP_TRY(hipMemsetAsync(te, 0, (size_t)F * kp * 2, c.st));
    CTRLV_TRY(ctrlv_timestep_embedding(ar, F, C, tmp, c.st));
    CTRLV_HIP_TRY(hipMemcpy2DAsync(te, (size_t)kp * 2, tmp, (size_t)C * 2, (size_t)C * 2, F, hipMemcpyDeviceToDevice, c.st));
    return CTRLV_OK;
  }));
  {
    ctrlv_gemm_desc d = ctrlv_linear_desc(te, kp, t.tpe1, hh, 4 * C, F, t.tpe1.n, kp, 4 * C);
    d.act = 1;
    CTRLV_TRY(gemm(c, d));
  }
  {
    ctrlv_gemm_desc d = ctrlv_linear_desc(hh, 4 * C, t.tpe2, e, C, F, t.tpe2.n, 4 * C, C);
    d.out_f32 = 1;
    CTRLV_TRY(gemm(c, d));
  }
  c.release(mk);
  return CTRLV_OK;
}

// `u` = the 4C-wide intermediate of the two-launch path, allocated HERE on first need (a transformer whose three
// feed-forwards all run fused never reserves it: 1.2 GB per lane at the 72 x 128 level); proj.out / outd.A are set from it.
int ff_pair(Ctx& c, const FeedFwd& f, ctrlv_gemm_desc proj, ctrlv_gemm_desc outd, int C, el_t** u) {
  // C = 320: one fused launch, the 4C-wide intermediate stays on chip (ff_fused.hip): 234.5 -> 231.3 ms per step (three
  // alternations on one device).  CTRLV_FF_FUSED=0: the two launches.
  if (ctrlv_debug().ff_fused && f.w1f && ctrlv_ff_fused_serves(&outd, proj.lda)) {
    return c.launch({CTRLV_FAM_GEMM_LINEAR, 2.0 * outd.M * 320.0 * (2560 + 1280),
                     (double)outd.M * 320 * (2 * (2 + (outd.R1 ? 1 : 0) + (outd.R2 ? 1 : 0)) + (outd.R1_lo ? 1 : 0) + (outd.R2_lo ? 1 : 0) +
                                             (outd.out_lo ? 1 : 0)), outd.M, 320, 320, 0x100},
                    [&] { return ctrlv_ff_fused(proj.A, proj.lda, f.w1f, f.w2f, &outd, c.st); });
  }
  if (*u == nullptr) *u = c.rows(proj.M, 4 * C);
  proj.out = *u;
  outd.A = *u;
  CTRLV_TRY(gemm(c, proj));
  CTRLV_TRY(gemm(c, outd));
  return CTRLV_OK;
}

// LayerNorm -> feed-forward (blocks.py::_ln_ff).  OPT-IN (CTRLV_FF_LN=1): the norm folded into the fused kernel's tile
// prologue (ctrlv_ff_fused_ln: one launch and one write + read of the activation less).  Measured equal in the model
// (224.2 vs 224.2 and 230.3 vs 230.4 ms per step, three alternations each: the LayerNorm family drops 7.9 -> 5.3 ms, the
// fused kernel's per-tile prologue takes it back), so the default keeps ctrlv_layernorm in front of the fused kernel.
int ln_ff(Ctx& c, const FeedFwd& f, const Norm& nm, const Trk& xraw, const float* lnV, int lnvdiv, int lnvmod, int lnldv,
          el_t* tt, const ctrlv_gemm_desc& proj, const ctrlv_gemm_desc& outd, int C, el_t** u) {
  if (ctrlv_debug().ff_fused && ctrlv_debug().ff_ln && f.w1f && !xraw.lo && ctrlv_ff_fused_serves(&outd, C)) {
    return c.launch({CTRLV_FAM_GEMM_LINEAR, 2.0 * outd.M * 320.0 * (2560 + 1280),
                     (double)outd.M * 320 * 2 * (2 + (outd.R1 ? 1 : 0) + (outd.R2 ? 1 : 0)), outd.M, 320, 320, 0x300}, [&] {
      return ctrlv_ff_fused_ln(xraw.hi, C, nm.g, nm.b, 1e-5f, lnV, lnvdiv, lnvmod, lnldv, f.w1f, f.w2f, &outd, c.st);
    });
  }
  if (c.p->ff_precision == 1 && f.proj8 && f.out8 && !xraw.lo) {
    // FF precision 1: LayerNorm + row quantisation in one pass, the GEGLU projection on e4m3 operands, the
    // row quantisation of u, the output projection on e4m3 operands with the layer's epilogue -- four launches for the three
    // above, wherever ctrlv_gemm_f8_serves accepts both descriptors (a function of the layer's shape only)
    ctrlv_gemm_desc p8 = proj, o8 = outd;
    p8.W = f.proj8; o8.W = f.out8; o8.lda = 4 * C; o8.S = 0;
    if (ctrlv_gemm_f8_serves(&p8) && ctrlv_gemm_f8_serves(&o8)) {
      if (*u == nullptr) *u = c.rows(proj.M, 4 * C);
      const size_t mk = c.mark();
      const long M = proj.M;
      uint8_t* q = (uint8_t*)c.alloc((size_t)M * 4 * C);       // codes of the normalised rows (C wide), then of u (4C wide)
      float* qs = (float*)c.alloc((size_t)M * 4);
      p8.A = q; p8.lda = C; p8.out = *u;
      o8.A = q; o8.lda = 4 * C;
      int rc = c.launch({CTRLV_FAM_LAYERNORM, 0.0, 3.0 * (double)M * C, (int)M, C, 0, 0x400}, [&] {
        return ctrlv_quant_rows_f8(xraw.hi, (int)M, C, C, nm.g, nm.b, 1e-5f, lnV, lnvdiv, lnvmod, lnldv, q, C, qs, c.st);
      });
      if (rc == CTRLV_OK)
        rc = c.launch({CTRLV_FAM_GEMM_LINEAR, 2.0 * M * 8.0 * C * C, (double)M * C + (double)M * 4 * C * 2 + 8.0 * C * C, (int)M, 8 * C, C, 0x401},
                      [&] { return ctrlv_gemm_f8(&p8, qs, f.proj8_s, c.st); });
      if (rc == CTRLV_OK)
        rc = c.launch({CTRLV_FAM_LAYERNORM, 0.0, 3.0 * (double)M * 4 * C, (int)M, 4 * C, 0, 0x400}, [&] {
          return ctrlv_quant_rows_f8(*u, (int)M, 4 * C, 4 * C, nullptr, nullptr, 0.f, nullptr, 1, 1, 0, q, 4 * C, qs, c.st);
        });
      if (rc == CTRLV_OK)
        rc = c.launch({CTRLV_FAM_GEMM_LINEAR, 2.0 * M * 4.0 * C * C,
                       (double)M * 4 * C + (double)M * C * 2 * (1 + (o8.R1 ? 1 : 0) + (o8.R2 ? 1 : 0)) + 4.0 * C * C, (int)M, C, 4 * C,
                       0x400 | ((o8.R1 ? 1 : 0) + (o8.R2 ? 1 : 0)) << 1 | o8.vmode << 3},
                      [&] { return ctrlv_gemm_f8(&o8, qs, f.out8_s, c.st); });
      c.release(mk);
      return rc;
    }
  }
  CTRLV_TRY(layernorm(c, xraw, proj.M, C, nm, tt, lnV, lnvdiv, lnvmod, lnldv));
  return ff_pair(c, f, proj, outd, C, u);
}

// ---- TransformerSpatioTemporalModel (blocks.py::TransformerSpatioTemporalModel.run)
int run_tr(Ctx& c, const Transformer& t, const Trk& x, int H, int W, Trk* out_) {
  const int B = c.B, F = c.F, C = t.C, N = B * F, S = H * W;
  const long M = (long)N * S;
  const Trk out = c.trunk(M, C);
  const size_t mk = c.mark();
  const float* emb = t.frame_emb;
  if (F != c.p->cfg.num_frames || emb == nullptr) {
    float* e = (float*)c.alloc((size_t)F * C * 4);
    CTRLV_TRY(frame_embedding(c, t, F, e));
    emb = e;
  }
  el_t* tt = c.rows(M, C);
  Trk h0;
  el_t* qkv = nullptr;
  // GroupNorm apply + proj_in + norm1 + q|k|v: at C = 320 ONE launch behind the statistics (or the finalize of the producer's
  // partials) -- the normalised rows never reach HBM (spatial_entry_fused.hip; CTRLV_SPATIAL_ENTRY=0: the four launches).  The
  // predicate reads shapes and the trunk mode only, so the measuring walk takes the same route.
  ctrlv_spatial_entry_desc sd;
  memset(&sd, 0, sizeof(sd));
  sd.ldx = C; sd.ldh = C; sd.ldq = 3 * C; sd.n_img = N; sd.S = S; sd.C = C; sd.head_dim = 64;
  const bool split = c.p->trunk_mode == 1;
  const bool entry_fused = ctrlv_debug().spatial_entry && t.se_wf && !split && ctrlv_spatial_entry_fused_serves(&sd);
  if (entry_fused) {
    h0 = c.trunk(M, C);
    qkv = c.rows(M, 3 * C);
    const size_t mk2 = c.mark();
    if (c.gn_cross_valid) {   // statistics from the res block's last GEMM (run_res, feeds_norm: set on the live walk only)
      c.gn_cross_valid = false;
      CTRLV_TRY(c.launch({CTRLV_FAM_GROUPNORM, 0.0, 0.0, N * S, C, 0, 3},
                         [&] { return ctrlv_groupnorm_finalize(N, S, C, 1, 1e-6f, c.gn_cross, c.st); }));
      sd.stats = c.gn_cross + (size_t)N * (S / 64) * 64;
    } else {
      const int chunks = ctrlv_groupnorm_chunks(N, S, C, 1);
      if (chunks < 0) return chunks;
      float* part = (float*)c.alloc(((size_t)N * chunks + N) * 64 * 4);
      CTRLV_TRY(c.launch({CTRLV_FAM_GROUPNORM, 0.0, 2.0 * (double)M * C, N * S, C, 0, 2},
                         [&] { return ctrlv_groupnorm_stats_split(x.hi, nullptr, nullptr, nullptr, 0, N, S, C, 1, 1e-6f, part, c.st); }));
      sd.stats = part + (size_t)N * chunks * 64;
    }
    sd.x = x.hi; sd.wf = t.se_wf; sd.bias_in = t.pin.b; sd.bias_qkv = t.s_qkv.b;
    sd.gn_gamma = t.gn.g; sd.gn_beta = t.gn.b; sd.ln_gamma = t.s_ln1.g; sd.ln_beta = t.s_ln1.b; sd.ln_eps = 1e-5f;
    sd.h0 = h0.hi; sd.qkv = qkv; sd.q_scale = 0.125f * 1.44269504088896340736f;      // q block pre-scaled: (1/sqrt(64)) log2(e)
    CTRLV_TRY(c.launch({CTRLV_FAM_GEMM_SPATIAL_ENTRY, 2.0 * M * C * 4.0 * C, (double)M * C * 2 * 5, (int)M, 4 * C, C},
                       [&] { return ctrlv_spatial_entry_fused(&sd, c.st); }));
    c.release(mk2);           // stream order keeps the statistics alive until the launch has read them
  } else {
    if (c.gn_cross_valid) {     // statistics from the res block's last GEMM (run_res, feeds_norm: set on the live walk only)
      c.gn_cross_valid = false;
      CTRLV_TRY(c.launch(gn_work(N, S, C, 1), [&] {
        return ctrlv_groupnorm_from_partials_split(x.hi, x.lo, N, S, C, 1, 1e-6f, c.gn_cross, t.gn.g, t.gn.b, 0, tt, c.st);
      }));
    } else {
      CTRLV_TRY(groupnorm(c, x, Trk{}, 0, N, S, C, 1, t.gn, 1e-6f, 0, tt));
    }
    h0 = c.trunk(M, C);
    {
      ctrlv_gemm_desc d = ctrlv_linear_desc(tt, C, t.pin, h0.hi, C, (int)M, C, C, C);
      set_out(d, h0);
      CTRLV_TRY(gemm(c, d));
    }
    // ---- spatial BasicTransformerBlock
    CTRLV_TRY(layernorm(c, h0, (int)M, C, t.s_ln1, tt));
    qkv = c.rows(M, 3 * C);
    {
      ctrlv_gemm_desc d = ctrlv_linear_desc(tt, C, t.s_qkv, qkv, 3 * C, (int)M, 3 * C, C, 3 * C);
      d.n_scale2 = C; d.s_acc2 = 0.125f * 1.44269504088896340736f;      // q block pre-scaled: (1/sqrt(64)) log2(e)
      CTRLV_TRY(gemm(c, d));
    }
  }
  el_t* a = c.rows(M, C);
  CTRLV_TRY(c.launch({CTRLV_FAM_ATTENTION_SPATIAL, 4.0 * N * (C / 64) * (double)S * S * 64, 2.0 * 4 * N * (double)S * C, N, S, C},
                     [&] { return ctrlv_attention_spatial_prescaled(qkv, a, N, S, C, c.st); }));
  const Trk h1 = c.trunk(M, C);
  {   // attn2 with one key == to_out(to_v(ehs[b])) for every query: a per-clip row vector
    ctrlv_gemm_desc d = ctrlv_linear_desc(a, C, t.s_o, h1.hi, C, (int)M, C, C, C);
    set_out(d, h1);
    set_r1(d, h0, C);
    d.V = c.xattn + t.xattn_off[0]; d.ldv = c.ldx; d.vmode = 1; d.vdiv = F * S;
    CTRLV_TRY(gemm(c, d));
  }
  el_t* u = nullptr;  // 4C-wide GEGLU output of the two-launch path: allocated by ff_pair on first need
  const Trk h2 = h0;  // h0 is dead from here on
  {
    ctrlv_gemm_desc dp = ctrlv_linear_desc(tt, C, t.s_ff.proj, u, 4 * C, (int)M, 8 * C, C, 4 * C);
    dp.geglu = 1;
    ctrlv_gemm_desc d = ctrlv_linear_desc(u, 4 * C, t.s_ff.out, h2.hi, C, (int)M, C, 4 * C, C);
    set_out(d, h2);
    set_r1(d, h1, C);
    d.S = S;                              // (S: rows per image, the split plan's shape key for a mode-0 launch)
    CTRLV_TRY(ln_ff(c, t.s_ff, t.s_ln3, h1, nullptr, 1, 1 << 30, 0, tt, dp, d, C, &u));
  }
  // ---- temporal block on tokens (b, s) x frames; rows stay ordered (b, f, s)
  const Trk g0 = h1;  // h1 is dead
  {
    ctrlv_gemm_desc dp = ctrlv_linear_desc(tt, C, t.t_ffin.proj, u, 4 * C, (int)M, 8 * C, C, 4 * C);
    dp.geglu = 1;
    ctrlv_gemm_desc d = ctrlv_linear_desc(u, 4 * C, t.t_ffin.out, g0.hi, C, (int)M, C, 4 * C, C);
    set_out(d, g0);
    set_r1(d, h2, C);
    d.S = S;
    d.V = emb; d.ldv = C; d.vmode = 1; d.vdiv = S; d.vmod = F;
    CTRLV_TRY(ln_ff(c, t.t_ffin, t.t_lnin, h2, emb, S, F, C, tt, dp, d, C, &u));
  }
  const Trk g1 = c.trunk(M, C);
  {
    // norm1 + attn1 over the frames + residual + the one-key cross-attention vector (attn2): at C = 320 ONE launch -- the
    // normalised rows, q|k|v and the attention output never reach HBM (temporal_fused.hip; CTRLV_TEMPORAL_FUSED=0: the four
    // launches).  With split trunk planes the norm input of a block that HAS the fused form (C = 320: t_wf) is the hi plane
    // (the element-rounded branch input: one more rounding on this branch's input, none on the trunk -- the residual operand
    // stays hi + lo; the complete step's rel-L2 against the oracle is unchanged within 1e-5, bench.py's parity leg), on
    // BOTH routes, so that such a block gives the same numbers fused and as the four launches (the routing test of
    // tests/test_split_exact_gpu.py).  The kernel's prologue reads hi only because its LO + LN instantiation already uses
    // 248 of 256 VGPRs (tests/test_build_resources.py): there is no room to hold the row's lo bytes through its three passes.
    // The blocks the fused kernel never serves (C = 640 / 1280: the fallback is their only route) normalise hi + lo like
    // every other norm of the split trunk (hi-only norms cost 8.0e-4 -> 9.5e-4 on the complete step).
    ctrlv_temporal_fused_desc fd;
    memset(&fd, 0, sizeof(fd));
    fd.x = tt; fd.ldx = C; fd.wf = t.t_wf; fd.bias = t.t_o.b;
    const bool fuse = ctrlv_debug().temporal_fused && t.t_wf;
    bool ln_in = fuse;
    if (ln_in) { fd.x = g0.hi; fd.ln_gamma = t.t_ln1.g; fd.ln_beta = t.t_ln1.b; fd.ln_eps = 1e-5f; }
    fd.R1 = g0.hi; fd.R1_lo = g0.lo; fd.ldr1 = C;
    fd.V = c.xattn + t.xattn_off[1]; fd.ldv = c.ldx; fd.vdiv = F * S; fd.vS = 1; fd.vmod = 1 << 30;
    if (c.quirk && B > 1) { fd.vmode = 2; fd.vS = S; fd.vmod = B; }   // diffusers 0.27.2: context rows (s, b), tokens (b, s)
    else fd.vmode = 1;
    fd.out = g1.hi; fd.out_lo = g1.lo; fd.ldo = C;
    fd.B = B; fd.F = F; fd.S = S; fd.C = C;
    const bool fused = fuse && ctrlv_temporal_fused_serves(&fd);
    if (!fused || !ln_in) {
      if (ln_in) { ln_in = false; fd.x = tt; fd.ln_gamma = fd.ln_beta = nullptr; }
      CTRLV_TRY(layernorm(c, t.t_wf ? Trk{g0.hi, nullptr} : g0, (int)M, C, t.t_ln1, tt));   // (C = 320: hi, as the prologue)
    }
    if (fused) {
      CTRLV_TRY(c.launch({CTRLV_FAM_GEMM_TEMPORAL_BLOCK, 2.0 * M * C * 4.0 * C + 4.0 * B * S * (C / 64) * (double)F * F * 64,
                          (double)M * C * (2 * (ln_in ? 2 : 3) + (g0.lo ? 1 : 0) + (g1.lo ? 1 : 0)), (int)M, 4 * C, C, ln_in ? 1 : 0},
                         [&] { return ctrlv_temporal_fused(&fd, c.st); }));
    } else {
      CTRLV_TRY(gemm(c, ctrlv_linear_desc(tt, C, t.t_qkv, qkv, 3 * C, (int)M, 3 * C, C, 3 * C)));
      CTRLV_TRY(c.launch({CTRLV_FAM_ATTENTION_TEMPORAL, 4.0 * B * S * (C / 64) * (double)F * F * 64, 2.0 * 4 * B * F * (double)S * C, B * S, F, C},
                         [&] { return ctrlv_attention_temporal(qkv, a, B, F, S, C, c.st); }));
      ctrlv_gemm_desc d = ctrlv_linear_desc(a, C, t.t_o, g1.hi, C, (int)M, C, C, C);
      set_out(d, g1);
      set_r1(d, g0, C);
      d.V = fd.V; d.ldv = fd.ldv; d.vdiv = fd.vdiv; d.vmode = fd.vmode;
      if (fd.vmode == 2) { d.vS = S; d.vmod = B; }
      CTRLV_TRY(gemm(c, d));
    }
  }
  const Trk h3 = g0;
  {   // AlphaBlender folded: h3 = a*h2 + (1-a)*(g1 + ff)
    ctrlv_gemm_desc dp = ctrlv_linear_desc(tt, C, t.t_ff.proj, u, 4 * C, (int)M, 8 * C, C, 4 * C);
    dp.geglu = 1;
    ctrlv_gemm_desc d = ctrlv_linear_desc(u, 4 * C, t.t_ff.out, h3.hi, C, (int)M, C, 4 * C, C);
    set_out(d, h3);
    d.s_acc = (float)(1.0 - t.alpha); d.s1 = (float)(1.0 - t.alpha); d.s2 = (float)t.alpha; d.S = S;
    set_r1(d, g1, C);
    set_r2(d, h2, C);
    CTRLV_TRY(ln_ff(c, t.t_ff, t.t_ln3, g1, nullptr, 1, 1 << 30, 0, tt, dp, d, C, &u));
  }
  {
    ctrlv_gemm_desc d = ctrlv_linear_desc(h3.hi, C, t.pout, out.hi, C, (int)M, C, C, C);
    set_out(d, out);
    set_r1(d, x, C);
    CTRLV_TRY(gemm(c, d));
  }
  c.release(mk);
  *out_ = out;
  return CTRLV_OK;
}

int run_resample(Ctx& c, const Resample& r, const Trk& x, int H, int W, bool up, Trk* out_, int* Ho_, int* Wo_) {
  const int N = c.B * c.F;
  const int Ho = up ? 2 * H : (H + 2 - 3) / 2 + 1, Wo = up ? 2 * W : (W + 2 - 3) / 2 + 1;
  const long M = (long)N * Ho * Wo;
  const Trk out = c.trunk(M, r.C);
  ctrlv_gemm_desc d = ctrlv_linear_desc(x.hi, r.C, r.conv, out.hi, r.C, (int)M, r.C, r.C, r.C);
  set_out(d, out);
  conv2d(d, H, W, Ho, Wo, up ? 1 : 2, up ? 1 : 0);
  // the up-sampler in phase form (four 2x2 convs, 4/9 of the multiply-adds) where the LAYER's shape is served
  if (up && r.wph && ctrlv_gemm_up_phase_serves(&d)) { d.up = 2; d.W = r.wph; }
  CTRLV_TRY(gemm(c, d));
  *out_ = out; *Ho_ = Ho; *Wo_ = Wo;
  return CTRLV_OK;
}

struct Tap { Trk x; int H, W, C; };

// ---- embeddings + per-clip row-vector tables (encoder.py::_context)
int run_context(Ctx& c, int dtype, const float* timestep, int n_t, const void* ehs, const float* ids32, int n_ids) {
  ctrlv_plan* p = c.p;
  const ctrlv_model_config& cfg = p->cfg;
  const int B = c.B, boc0 = cfg.block_out_channels[0], ted = 4 * boc0;
  CTRLV_CHECK_ARG(n_t == 1 || n_t == B, "plan forward: timestep must have 1 or B=%d entries (got %d)", B, n_t);
  const int add_dim = cfg.addition_time_embed_dim;
  CTRLV_CHECK_SHAPE(add_dim * n_ids == cfg.projection_class_embeddings_input_dim,
                    "Model expects an added time embedding vector of length %d, but a vector of %d was created.",
                    cfg.projection_class_embeddings_input_dim, add_dim * n_ids);
  float* t32 = (float*)c.alloc((size_t)B * 4);
  const int kt = p->te1.k, ka = p->ae1.k, kx = p->xv.k;
  el_t* te = c.rows(B, kt);
  el_t* ae = c.rows(B, ka);
  el_t* te_tmp = kt != boc0 ? c.rows(B, boc0) : nullptr;
  el_t* ae_tmp = ka != n_ids * add_dim ? c.rows((long)B * n_ids, add_dim) : nullptr;
  el_t* h = c.rows(B, ted);
  el_t* emb_t = c.rows(B, ted);
  el_t* emb_s = c.rows(B, ted);
  c.ldtemb = p->temb.n;
  c.temb = (float*)c.alloc((size_t)B * c.ldtemb * 4);
  CTRLV_TRY(c.launch({}, [&]() -> int {
    hipLaunchKernelGGL(expand_f32_kernel, dim3((B + 63) / 64), dim3(64), 0, c.st, timestep, n_t, t32, B);
    CTRLV_LAUNCH_CHECK();
    if (kt != boc0) {
      CTRLV_HIP_TRY(hipMemsetAsync(te, 0, (size_t)B * kt * 2, c.st));
      CTRLV_TRY(ctrlv_timestep_embedding(t32, B, boc0, te_tmp, c.st));
      CTRLV_HIP_TRY(hipMemcpy2DAsync(te, (size_t)kt * 2, te_tmp, (size_t)boc0 * 2, (size_t)boc0 * 2, B, hipMemcpyDeviceToDevice, c.st));
    } else {
      CTRLV_TRY(ctrlv_timestep_embedding(t32, B, boc0, te, c.st));
    }
    // added ids: sinusoid of every id -> [B*n_ids, add_dim] == [B, n_ids*add_dim]
    if (ka != n_ids * add_dim) {
      CTRLV_HIP_TRY(hipMemsetAsync(ae, 0, (size_t)B * ka * 2, c.st));
      CTRLV_TRY(ctrlv_timestep_embedding(ids32, B * n_ids, add_dim, ae_tmp, c.st));
      CTRLV_HIP_TRY(hipMemcpy2DAsync(ae, (size_t)ka * 2, ae_tmp, (size_t)n_ids * add_dim * 2, (size_t)n_ids * add_dim * 2, B,
                                     hipMemcpyDeviceToDevice, c.st));
    } else {
      CTRLV_TRY(ctrlv_timestep_embedding(ids32, B * n_ids, add_dim, ae, c.st));
    }
    return CTRLV_OK;
  }));
  // (tile 11: per-clip rows -- one kernel for these launches whatever B is, so a clip's conditioning vectors have the same
  //  bits alone and in any batch: csrc/gemm.hip gemv_small_kernel)
  constexpr int kClipRows = 11;
  { ctrlv_gemm_desc d = ctrlv_linear_desc(te, kt, p->te1, h, ted, B, ted, kt, ted); d.act = 1; d.tile = kClipRows; CTRLV_TRY(gemm(c, d)); }
  { ctrlv_gemm_desc d = ctrlv_linear_desc(h, ted, p->te2, emb_t, ted, B, ted, ted, ted); d.tile = kClipRows; CTRLV_TRY(gemm(c, d)); }
  { ctrlv_gemm_desc d = ctrlv_linear_desc(ae, ka, p->ae1, h, ted, B, ted, ka, ted); d.act = 1; d.tile = kClipRows; CTRLV_TRY(gemm(c, d)); }
  {   // silu(emb + aug_emb): the SiLU in front of every time_emb_proj
    ctrlv_gemm_desc d = ctrlv_linear_desc(h, ted, p->ae2, emb_s, ted, B, ted, ted, ted);
    resid(d, emb_t, ted); d.act = 1; d.tile = kClipRows;
    CTRLV_TRY(gemm(c, d));
  }
  { ctrlv_gemm_desc d = ctrlv_linear_desc(emb_s, ted, p->temb, c.temb, c.ldtemb, B, p->temb.n, ted, c.ldtemb); d.out_f32 = 1; d.tile = kClipRows; CTRLV_TRY(gemm(c, d)); }
  if (p->xattn_n) {
    const int dc = cfg.cross_attention_dim, nx = p->xv.n;
    el_t* e = c.rows(B, kx);
    el_t* v_all = c.rows(B, nx);
    c.ldx = nx;
    c.xattn = (float*)c.alloc((size_t)B * nx * 4);
    CTRLV_TRY(c.launch({}, [&]() -> int {
      if (kx != dc) CTRLV_HIP_TRY(hipMemsetAsync(e, 0, (size_t)B * kx * 2, c.st));
      return ctrlv_nchw_to_rows(ehs, dtype, B, dc, 1, e, kx, 0, c.st);      // (B, 1, dc) any dtype -> bf16 rows [B, kx]
    }));
    { ctrlv_gemm_desc d = ctrlv_linear_desc(e, kx, p->xv, v_all, nx, B, nx, kx, nx); d.tile = kClipRows; CTRLV_TRY(gemm(c, d)); }
    for (const CrossOut& xo : p->xouts) {
      ctrlv_gemm_desc d = ctrlv_linear_desc(v_all + xo.off, nx, xo.to_out, c.xattn + xo.off, nx, B, xo.c, xo.c, xo.c);
      d.out_f32 = 1; d.tile = kClipRows;
      CTRLV_TRY(gemm(c, d));
    }
  }
  c.quirk = cfg.time_context_order == 0;
  return CTRLV_OK;
}

// conv_in (+ control_conv_in) as ONE im2col GEMM over the [conv_in channels | control channels | pad] slots
int run_input(Ctx& c, int dtype, const void* sample, const void* control, int h, int w, Trk* out_) {
  ctrlv_plan* p = c.p;
  const int N = c.B * c.F, cin = p->cfg.in_channels, c0 = p->cfg.block_out_channels[0];
  const long M = (long)N * h * w;
  el_t* x16 = c.rows(M, p->cin_cp);
  el_t* col = c.rows(M, p->cin_kp);
  const Trk x = c.trunk(M, c0);
  CTRLV_TRY(c.launch({}, [&]() -> int {
    CTRLV_HIP_TRY(hipMemsetAsync(x16, 0, (size_t)M * p->cin_cp * 2, c.st));
    CTRLV_TRY(ctrlv_nchw_to_rows(sample, dtype, N, cin, h * w, x16, p->cin_cp, 0, c.st));
    if (control) CTRLV_TRY(ctrlv_nchw_to_rows(control, dtype, N, cin / 2, h * w, x16, p->cin_cp, cin, c.st));
    return ctrlv_im2col3x3(x16, N, h, w, p->cin_cp, col, p->cin_kp, c.st);
  }));
  {
    ctrlv_gemm_desc d = ctrlv_linear_desc(col, p->cin_kp, p->cin, x.hi, c0, (int)M, p->cin.n, p->cin_kp, c0);
    set_out(d, x);
    CTRLV_TRY(gemm(c, d));
  }
  *out_ = x;
  return CTRLV_OK;
}

int run_down_mid(Ctx& c, Trk x, int h, int w, std::vector<Tap>& taps, Trk* mid_, int* H_, int* W_) {
  ctrlv_plan* p = c.p;
  int H = h, W = w;
  taps.push_back({x, H, W, p->cfg.block_out_channels[0]});
  for (auto& b : p->down) {
    for (size_t j = 0; j < b.res.size(); ++j) {
      Trk y;
      CTRLV_TRY(run_res(c, b.res[j], x, Trk{}, 0, H, W, &y, !b.attn.empty()));
      x = y;
      if (!b.attn.empty()) { CTRLV_TRY(run_tr(c, b.attn[j], x, H, W, &y)); x = y; }
      taps.push_back({x, H, W, b.res[j].cout});
    }
    if (b.down.present) {
      Trk y; int Ho, Wo;
      CTRLV_TRY(run_resample(c, b.down, x, H, W, false, &y, &Ho, &Wo));
      x = y; H = Ho; W = Wo;
      taps.push_back({x, H, W, b.down.C});
    }
  }
  Trk y;
  CTRLV_TRY(run_res(c, p->mid_r0, x, Trk{}, 0, H, W, &y, true)); x = y;
  CTRLV_TRY(run_tr(c, p->mid_attn, x, H, W, &y)); x = y;
  CTRLV_TRY(run_res(c, p->mid_r1, x, Trk{}, 0, H, W, &y)); x = y;
  *mid_ = x; *H_ = H; *W_ = W;
  return CTRLV_OK;
}

int check_common(ctrlv_plan* p, int B, int F, int H, int W) {
  CTRLV_CHECK_ARG(p != nullptr, "plan: null plan");
  CTRLV_CHECK_ARG(p->loaded, "plan: weights not loaded (ctrlv_plan_load_weights)");
  CTRLV_CHECK_SHAPE(B > 0 && F > 0 && H > 0 && W > 0, "plan forward: B, F, H, W must be positive");
  const int m = 1 << (p->cfg.n_blocks - 1);
  CTRLV_CHECK_SHAPE(H % m == 0 && W % m == 0, "latent height and width have to be divisible by %d but are %d and %d.", m, H, W);
  return CTRLV_OK;
}

int unet_forward(ctrlv_plan* p, Ctx& c, const void* sample, int dtype, const float* timestep, int n_t, const void* ehs,
                 const float* ids, int n_ids, const void* const* down_res, const void* mid_res, void* res_event, void* out,
                 int h, int w) {
  const int N = c.B * c.F;
  CTRLV_TRY(run_context(c, dtype, timestep, n_t, ehs, ids, n_ids));
  Trk x;
  CTRLV_TRY(run_input(c, dtype, sample, nullptr, h, w, &x));
  std::vector<Tap> taps;
  int H, W;
  CTRLV_TRY(run_down_mid(c, x, h, w, taps, &x, &H, &W));
  // the ControlNet residual add on a trunk tensor: in place; in trunk mode 1 the sum is split again
  auto add_res = [&](const Trk& t, const void* r, size_t n) -> int {
    if (t.lo) return ctrlv_axpby_split(t.hi, t.lo, r, 1.0f, 1.0f, t.hi, t.lo, n, c.st);
    return ctrlv_axpby(t.hi, r, 1.0f, 1.0f, t.hi, n, c.st);
  };
  // (the measuring walk comes without residuals: they need no workspace)
  if (down_res && mid_res) {        // unet_spatio_temporal_condition.py:61,119-127,136-137
    if (res_event) CTRLV_TRY(c.launch({}, [&]() -> int { CTRLV_HIP_TRY(hipStreamWaitEvent(c.st, (hipEvent_t)res_event, 0)); return CTRLV_OK; }));
    taps.push_back({x, H, W, p->cfg.block_out_channels[p->cfg.n_blocks - 1]});      // (the mid residual, like the others)
    for (size_t i = 0; i < taps.size(); ++i) {
      const void* r = i + 1 < taps.size() ? down_res[i] : mid_res;
      CTRLV_CHECK_ARG(r != nullptr, "unet_forward: down_res[%zu] is null", i);
      const size_t n = (size_t)N * taps[i].H * taps[i].W * taps[i].C;
      CTRLV_TRY(c.launch({CTRLV_FAM_RESIDUAL_ADD, 0.0, 2.0 * 3 * (double)n, (int)(n / taps[i].C), taps[i].C},
                         [&] { return add_res(taps[i].x, r, n); }));
    }
    taps.pop_back();
  }
  for (auto& b : p->up) {           // :140-158 -- torch.cat([hidden, skip], dim=1) is read in place (x | x2)
    for (size_t j = 0; j < b.res.size(); ++j) {
      const Tap skip = taps.back();
      taps.pop_back();
      Trk y;
      CTRLV_TRY(run_res(c, b.res[j], x, skip.x, b.res[j].cin - skip.C, H, W, &y, !b.attn.empty()));
      x = y;
      if (!b.attn.empty()) { CTRLV_TRY(run_tr(c, b.attn[j], x, H, W, &y)); x = y; }
    }
    if (b.up.present) {
      Trk y; int Ho, Wo;
      CTRLV_TRY(run_resample(c, b.up, x, H, W, true, &y, &Ho, &Wo));
      x = y; H = Ho; W = Wo;
    }
  }
  const int c0 = p->cfg.block_out_channels[0], co = p->cfg.out_channels, co_p = pad_to(co, 4);
  const long M = (long)N * H * W;
  el_t* xn = c.rows(M, c0);
  CTRLV_TRY(groupnorm(c, x, Trk{}, 0, N, H * W, c0, 1, p->gno, 1e-5f, 1, xn));         // :161-163
  el_t* y = c.rows(M, co_p);
  {
    ctrlv_gemm_desc d = ctrlv_linear_desc(xn, c0, p->cout, y, co_p, (int)M, p->cout.n, c0, co_p);
    conv2d(d, H, W, H, W);
    CTRLV_TRY(gemm(c, d));
  }
  return c.launch({}, [&] { return ctrlv_rows_to_nchw(y, co_p, N, co, H * W, out, dtype, c.st); });  // :166
}

int controlnet_forward(ctrlv_plan* p, Ctx& c, const void* sample, const void* control, int dtype, const float* timestep,
                       int n_t, const void* ehs, const float* ids, int n_ids, float scale, void* const* out_down,
                       void* out_mid, int h, int w) {
  const int N = c.B * c.F;
  CTRLV_TRY(run_context(c, dtype, timestep, n_t, ehs, ids, n_ids));
  Trk x;
  CTRLV_TRY(run_input(c, dtype, sample, control, h, w, &x));
  std::vector<Tap> taps;
  int H, W;
  CTRLV_TRY(run_down_mid(c, x, h, w, taps, &x, &H, &W));
  CTRLV_CHECK_ARG(taps.size() == p->zc.size(), "controlnet_forward: %zu taps but %zu zero-convs", taps.size(), p->zc.size());
  for (size_t i = 0; i < taps.size(); ++i) {       // controlnet.py:331-344: zero-conv * conditioning_scale, one GEMM
    const long M = (long)N * taps[i].H * taps[i].W;
    const int C = taps[i].C;
    // (the measuring walk has no output list to read the pointer from)
    if (!c.dry) CTRLV_CHECK_ARG(out_down && out_down[i], "controlnet_forward: out_down[%zu] is null", i);
    ctrlv_gemm_desc d = ctrlv_linear_desc(taps[i].x.hi, C, p->zc[i], c.dry ? nullptr : out_down[i], C, (int)M, p->zc[i].n, C, C);
    d.s_acc = scale;
    CTRLV_TRY(gemm(c, d));
  }
  {
    const int C = p->cfg.block_out_channels[p->cfg.n_blocks - 1];
    ctrlv_gemm_desc d = ctrlv_linear_desc(x.hi, C, p->zc_mid, out_mid, C, (int)((long)N * H * W), p->zc_mid.n, C, C);
    d.s_acc = scale;
    CTRLV_TRY(gemm(c, d));
  }
  return CTRLV_OK;
}

void free_f8(ctrlv_plan* p) {
  for (void* d : p->owned_f8) (void)hipFree(d);
  p->owned_f8.clear();
  for_each_tr(p, [&](Transformer& t) {
    for (FeedFwd* f : {&t.s_ff, &t.t_ffin, &t.t_ff}) { f->proj8 = f->out8 = nullptr; f->proj8_s = f->out8_s = nullptr; }
  });
}
// e4m3 codes + per-row scales of every feed-forward whose two contractions the FP8 GEMM can serve (K multiples of 128), from
// the packed element weights (ctrlv_quant_rows_f8: one scale per output channel, GEGLU rows keep their interleaving)
int make_f8(ctrlv_plan* p, hipStream_t st) {
  free_f8(p);
  int rc = CTRLV_OK;
  auto one = [&](const Linear& l, uint8_t** q, float** s) -> int {
    void* d = nullptr;
    CTRLV_HIP_TRY(hipMalloc(&d, (size_t)l.n * l.k));
    p->owned_f8.push_back(d);
    *q = (uint8_t*)d;
    CTRLV_HIP_TRY(hipMalloc(&d, (size_t)l.n * 4));
    p->owned_f8.push_back(d);
    *s = (float*)d;
    return ctrlv_quant_rows_f8(l.w, l.n, l.k, l.k, nullptr, nullptr, 0.f, nullptr, 1, 1, 0, *q, l.k, *s, st);
  };
  for_each_tr(p, [&](Transformer& t) {
    for (FeedFwd* f : {&t.s_ff, &t.t_ffin, &t.t_ff}) {
      if (rc != CTRLV_OK || !f->proj.w || !f->out.w || f->proj.k % 128 || f->out.k % 128 || f->out.k > 5120) continue;
      rc = one(f->proj, &f->proj8, &f->proj8_s);
      if (rc == CTRLV_OK) rc = one(f->out, &f->out8, &f->out8_s);
    }
  });
  if (rc != CTRLV_OK) free_f8(p);
  return rc;
}
void free_owned(ctrlv_plan* p) {
  free_f8(p);
  for (void* d : p->owned) (void)hipFree(d);
  p->owned.clear();
  p->xouts.clear();
  p->zc.clear();
  p->loaded = false;
}

}  // namespace

// ================================================================================================== C entry points
extern "C" int ctrlv_plan_create(const ctrlv_model_config* cfg, int device, ctrlv_plan** out) {
  CTRLV_CHECK_ARG(cfg && out, "plan_create: null argument");
  ctrlv_plan* p = new ctrlv_plan();
  p->cfg = *cfg;
  p->device = device;
  const int rc = build_graph(p);
  if (rc != CTRLV_OK) { delete p; return rc; }
  *out = p;
  return CTRLV_OK;
}

extern "C" int ctrlv_plan_destroy(ctrlv_plan* p) {
  if (!p) return CTRLV_OK;
  {
    DeviceScope on(p->device);
    free_owned(p);
    for (auto& r : p->prof) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  }
  delete p;
  return CTRLV_OK;
}

extern "C" int ctrlv_plan_load_weights(ctrlv_plan* p, const ctrlv_tensor_desc* tensors, size_t n) {
  CTRLV_CHECK_ARG(p && tensors, "plan_load_weights: null argument");
  WeightLoader L("plan_load_weights", &p->owned);
  const ctrlv_model_config& c = p->cfg;
  const int nb = c.n_blocks, c0 = c.block_out_channels[0], ted = 4 * c0;
  auto body = [&]() -> int {
    free_owned(p);
    for (size_t i = 0; i < n; ++i)
      CTRLV_CHECK_ARG(tensors[i].name && tensors[i].data && tensors[i].dtype >= 0 && tensors[i].dtype <= 2,
                      "plan_load_weights: bad tensor descriptor %zu", i);
    L.add(tensors, n);
    // input convs: slots [conv_in channels | control_conv_in channels | pad], biases summed (controlnet.py:297-299)
    const int cin_tot = c.in_channels + (c.kind == 1 ? c.in_channels / 2 : 0);
    CTRLV_TRY(L.conv_in("conv_in", c0, c.in_channels, cin_tot, p->cin, &p->cin_cp, &p->cin_kp));
    if (c.kind == 1) {
      CTRLV_TRY(L.pack_w("control_conv_in.weight", c0, c.in_channels / 2, 9, p->cin, p->cin_cp, c.in_channels, 0, 0));
      CTRLV_TRY(L.pack_v("control_conv_in.bias", c0, p->cin.b, 0, 0, 1));
    }
    CTRLV_TRY(L.linear("time_embedding.linear_1", ted, c0, p->te1));
    CTRLV_TRY(L.linear("time_embedding.linear_2", ted, ted, p->te2));
    CTRLV_TRY(L.linear("add_embedding.linear_1", ted, c.projection_class_embeddings_input_dim, p->ae1));
    CTRLV_TRY(L.linear("add_embedding.linear_2", ted, ted, p->ae2));
    // model-wide row-vector GEMMs: offsets first, then storage, then the blocks fill their rows
    int off = 0;
    for_each_res(p, [&](ResBlock& r) { r.temb_off[0] = off; off += r.cout; r.temb_off[1] = off; off += r.cout; });
    p->temb_n = off;
    CTRLV_TRY(L.new_linear(p->temb, off, pad_to(ted, 64), true));
    off = 0;
    for_each_tr(p, [&](Transformer& t) { t.xattn_off[0] = off; off += t.C; t.xattn_off[1] = off; off += t.C; });
    p->xattn_n = off;
    if (off) CTRLV_TRY(L.new_linear(p->xv, off, pad_to(c.cross_attention_dim, 64), false));
    int rc = CTRLV_OK;
    for_each_res(p, [&](ResBlock& r) { if (rc == CTRLV_OK) rc = load_res(L, p, r, ted); });
    CTRLV_TRY(rc);
    for_each_tr(p, [&](Transformer& t) { if (rc == CTRLV_OK) rc = load_tr(L, p, t, c.cross_attention_dim); });
    CTRLV_TRY(rc);
    for (int i = 0; i < nb; ++i) {
      if (p->down[i].down.present)
        CTRLV_TRY(L.conv3x3("down_blocks." + std::to_string(i) + ".downsamplers.0.conv", p->down[i].down.C, p->down[i].down.C,
                      p->down[i].down.conv));
      if (c.kind == 0 && p->up[i].up.present) {
        Resample& u = p->up[i].up;
        const std::string mod = "up_blocks." + std::to_string(i) + ".upsamplers.0.conv";
        CTRLV_TRY(L.conv3x3(mod, u.C, u.C, u.conv));
        if (u.conv.n == u.C) CTRLV_TRY(up_phase(L, mod, u.C, u.C, &u.wph));      // (no padded weight rows: the panels are [C][4 C])
      }
    }
    if (c.kind == 0) {
      CTRLV_TRY(L.norm("conv_norm_out", c0, p->gno));
      CTRLV_TRY(L.conv3x3("conv_out", c.out_channels, c0, p->cout));
    } else {
      // controlnet.py:148-185: one zero-conv per encoder tap (conv_in, every layer, every downsampler) + the mid block
      std::vector<int> ch;
      ch.push_back(c0);
      for (int i = 0; i < nb; ++i) {
        for (int j = 0; j < c.layers_per_block[i]; ++j) ch.push_back(c.block_out_channels[i]);
        if (i != nb - 1) ch.push_back(c.block_out_channels[i]);
      }
      p->zc.resize(ch.size());
      for (size_t i = 0; i < ch.size(); ++i) CTRLV_TRY(L.linear("controlnet_down_blocks." + std::to_string(i), ch[i], ch[i], p->zc[i]));
      CTRLV_TRY(L.linear("controlnet_mid_block", c.block_out_channels[nb - 1], c.block_out_channels[nb - 1], p->zc_mid));
    }
    // frame positional embedding tables for cfg.num_frames (weights-only constants)
    if (c.num_frames > 0) {
      size_t need = 0;
      for_each_tr(p, [&](Transformer& t) {
        const size_t a = ((size_t)c.num_frames * 4 + 255) / 256 * 256 + ((size_t)c.num_frames * t.tpe1.k * 2 + 255) / 256 * 256 +
                         ((size_t)c.num_frames * 4 * t.C * 2 + 255) / 256 * 256 + ((size_t)c.num_frames * t.C * 2 + 255) / 256 * 256;
        if (a > need) need = a;
      });
      void* scratch = nullptr;
      CTRLV_HIP_TRY(hipMalloc(&scratch, need + 1024));
      L.staged.push_back(scratch);
      for_each_tr(p, [&](Transformer& t) {
        if (rc != CTRLV_OK) return;
        rc = L.alloc((size_t)c.num_frames * t.C * 4, (void**)&t.frame_emb, false);
        if (rc != CTRLV_OK) return;
        Ctx cx(p, L.st, false, (char*)scratch, need + 1024, 1, c.num_frames);
        rc = frame_embedding(cx, t, c.num_frames, t.frame_emb);
      });
      CTRLV_TRY(rc);
    }
    if (p->ff_precision == 1) CTRLV_TRY(make_f8(p, L.st));
    return CTRLV_OK;
  };
  const int rc = ctrlv_load::run_load(L, p->device, false, body);       // (the plan's device stays current)
  if (rc != CTRLV_OK) { free_owned(p); return rc; }
  p->loaded = true;
  return CTRLV_OK;
}

extern "C" int ctrlv_plan_set_time_context_order(ctrlv_plan* p, int order) {
  CTRLV_CHECK_ARG(p != nullptr && (order == 0 || order == 1), "plan_set_time_context_order: order must be 0 (sb) or 1 (bs)");
  p->cfg.time_context_order = order;
  return CTRLV_OK;
}

extern "C" int ctrlv_plan_set_trunk_mode(ctrlv_plan* p, int mode) {
  CTRLV_CHECK_ARG(p != nullptr && (mode == 0 || mode == 1), "plan_set_trunk_mode: mode must be 0 (plain) or 1 (split hi + lo planes)");
  CTRLV_CHECK_ARG(mode == 0 || CTRLV_ELEM_DTYPE == 1, "plan_set_trunk_mode: the split trunk needs the fp16 element library "
                                                      "(libctrlv_hip_f16.so)");
  CTRLV_CHECK_ARG(mode == 0 || p->ff_precision == 0, "plan_set_trunk_mode: the split trunk does not combine with FF precision 1 "
                                                     "(ctrlv_plan_set_ff_precision)");
  if (p->trunk_mode != mode) p->ws_cache.clear();       // the workspace grows with the lo planes
  p->trunk_mode = mode;
  return CTRLV_OK;
}

extern "C" int ctrlv_plan_set_ff_precision(ctrlv_plan* p, int mode) {
  CTRLV_CHECK_ARG(p != nullptr && (mode == 0 || mode == 1), "plan_set_ff_precision: mode must be 0 (element type) or 1 (e4m3)");
  CTRLV_CHECK_ARG(mode == 0 || p->trunk_mode == 0, "plan_set_ff_precision: e4m3 feed-forwards do not combine with the split trunk "
                                                   "(ctrlv_plan_set_trunk_mode)");
  if (p->ff_precision == mode) return CTRLV_OK;
  p->ws_cache.clear();                                  // the workspace grows with the codes and scales
  if (mode == 1 && p->loaded) {                         // (not loaded yet: ctrlv_plan_load_weights makes them)
    DeviceScope on(p->device);
    CTRLV_TRY(on.status());
    int rc = make_f8(p, nullptr);
    if (rc == CTRLV_OK && hipDeviceSynchronize() != hipSuccess) { ctrlv_set_error("plan_set_ff_precision: quantising the weights failed"); rc = CTRLV_E_HIP; }
    if (rc != CTRLV_OK) { free_f8(p); return rc; }
  }
  if (mode == 0) free_f8(p);
  p->ff_precision = mode;
  return CTRLV_OK;
}

extern "C" int ctrlv_plan_num_down_residuals(ctrlv_plan* p) {
  CTRLV_CHECK_ARG(p != nullptr, "plan: null plan");
  int n = 1;
  for (int i = 0; i < p->cfg.n_blocks; ++i) n += p->cfg.layers_per_block[i] + (i != p->cfg.n_blocks - 1 ? 1 : 0);
  return n;
}

extern "C" int ctrlv_plan_residual_shape(ctrlv_plan* p, int idx, int B, int F, int H, int W, int64_t* rows, int32_t* channels) {
  CTRLV_CHECK_ARG(p && rows && channels, "plan_residual_shape: null argument");
  const int n = ctrlv_plan_num_down_residuals(p);
  CTRLV_CHECK_ARG(idx >= 0 && idx <= n, "plan_residual_shape: index %d out of range [0, %d]", idx, n);
  int k = 0, h = H, w = W, ch = p->cfg.block_out_channels[0];
  auto hit = [&]() { if (k == idx) { *rows = (int64_t)B * F * h * w; *channels = ch; } ++k; };
  hit();
  for (int i = 0; i < p->cfg.n_blocks; ++i) {
    ch = p->cfg.block_out_channels[i];
    for (int j = 0; j < p->cfg.layers_per_block[i]; ++j) hit();
    if (i != p->cfg.n_blocks - 1) { h = (h + 2 - 3) / 2 + 1; w = (w + 2 - 3) / 2 + 1; hit(); }
  }
  hit();      // idx == n: the mid residual (same shape as the last tap)
  return CTRLV_OK;
}

extern "C" size_t ctrlv_plan_workspace_bytes(ctrlv_plan* p, int B, int F, int H, int W) {
  if (check_common(p, B, F, H, W) != CTRLV_OK) return 0;
  Ctx c(p, nullptr, true, nullptr, 0, B, F);
  const int n_ids = p->cfg.projection_class_embeddings_input_dim / (p->cfg.addition_time_embed_dim > 0 ? p->cfg.addition_time_embed_dim : 1);
  int rc;
  if (p->cfg.kind == 0) {
    // residual adds need no workspace; the dry walk is the same with or without them
    rc = unet_forward(p, c, nullptr, 2, nullptr, 1, nullptr, nullptr, n_ids, nullptr, nullptr, nullptr, nullptr, H, W);
  } else {
    rc = controlnet_forward(p, c, nullptr, nullptr, 2, nullptr, 1, nullptr, nullptr, n_ids, 1.0f, nullptr, nullptr, H, W);
  }
  return rc == CTRLV_OK ? c.peak + 256 : 0;
}

// A workspace below the measuring walk's answer is refused BEFORE anything is launched.  That answer is an upper bound of
// what the live walk takes, so the refusal inside Ctx::launch, which every launch passes, never fires behind this one
// (tests/test_plan_entries_gpu.py runs the forwards in exactly this many bytes).  The dry walk's result is cached per
// (B, F, H, W).
static int check_workspace(ctrlv_plan* p, const char* who, int B, int F, int H, int W, size_t have) {
  size_t need = 0;
  for (const auto& e : p->ws_cache)
    if (e.B == B && e.F == F && e.H == H && e.W == W) need = e.bytes;
  if (need == 0) {
    need = ctrlv_plan_workspace_bytes(p, B, F, H, W);
    if (need == 0) return CTRLV_E_BAD_SHAPE;           // (message set by the dry walk)
    if (p->ws_cache.size() >= 16) p->ws_cache.clear();
    p->ws_cache.push_back({B, F, H, W, need});
  }
  if (have < need) {
    ctrlv_set_error("%s: workspace too small (%zu bytes, need >= %zu: ctrlv_plan_workspace_bytes)", who, have, need);
    return CTRLV_E_WORKSPACE;
  }
  return CTRLV_OK;
}

// The common shape of the three forward entries, in the order their refusals always had: the plan and the shape, the plan's
// kind, the entry's own pointer list (`null_msg`: its refusal, or null), the dtype code, what else the entry refuses
// (`arg_msg`), the workspace size; then the live walk over the 256-aligned workspace.
template <class Walk>
static int forward_entry(ctrlv_plan* p, const char* who, int kind, const char* null_msg, int dtype, const char* arg_msg, int B,
                         int F, int H, int W, void* workspace, size_t workspace_bytes, ctrlv_stream_t stream, Walk&& walk) {
  CTRLV_TRY(check_common(p, B, F, H, W));
  CTRLV_CHECK_ARG(p->cfg.kind == kind, "%s: the plan is a %s", who, kind == 0 ? "ControlNet" : "UNet");
  CTRLV_CHECK_ARG(null_msg == nullptr, "%s: %s", who, null_msg);
  CTRLV_CHECK_DTYPE(dtype >= 0 && dtype <= 2, "%s: dtype must be 0 (fp32), 1 (fp16) or 2 (bf16)", who);
  CTRLV_CHECK_ARG(arg_msg == nullptr, "%s: %s", who, arg_msg);
  CTRLV_TRY(check_workspace(p, who, B, F, H, W, workspace_bytes));
  char* base = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  Ctx c(p, (hipStream_t)stream, false, base, workspace_bytes - (size_t)(base - (char*)workspace), B, F);
  return walk(c);
}

extern "C" int ctrlv_unet_forward(ctrlv_plan* p, const void* sample, int dtype, const float* timestep, int n_timestep,
                                  const void* ehs, const float* added_time_ids, int n_ids, const void* const* down_res,
                                  const void* mid_res, void* residual_event, void* out, int B, int F, int H, int W,
                                  void* workspace, size_t workspace_bytes, ctrlv_stream_t stream) {
  return forward_entry(p, "unet_forward", 0, sample && timestep && ehs && added_time_ids && out && workspace ? nullptr : "null pointer",
                       dtype, (down_res == nullptr) == (mid_res == nullptr) ? nullptr : "pass both down_res and mid_res or neither",
                       B, F, H, W, workspace, workspace_bytes, stream, [&](Ctx& c) {
    return unet_forward(p, c, sample, dtype, timestep, n_timestep, ehs, added_time_ids, n_ids, down_res, mid_res, residual_event, out, H, W);
  });
}

// Down + mid path of the UNet only (the frozen-UNet half of the training step): the skip tensors and the mid output are
// COPIED out of the arena into the caller's buffers (the caller adds the ControlNet residuals with autograd attached).
static int unet_encoder(ctrlv_plan* p, Ctx& c, const void* sample, int dtype, const float* timestep, int n_t, const void* ehs,
                        const float* ids, int n_ids, void* const* out_taps, void* out_mid, int h, int w) {
  const int N = c.B * c.F;
  CTRLV_TRY(run_context(c, dtype, timestep, n_t, ehs, ids, n_ids));
  Trk x;
  CTRLV_TRY(run_input(c, dtype, sample, nullptr, h, w, &x));
  std::vector<Tap> taps;
  int H, W;
  CTRLV_TRY(run_down_mid(c, x, h, w, taps, &x, &H, &W));
  // (live walk only -- the size query measures the whole forward; the training step's tensors are plain element rows: the hi planes)
  auto copy = [&](const el_t* src, void* dst, size_t n) { return c.launch({}, [&] { return ctrlv_axpby(src, src, 1.0f, 0.0f, dst, n, c.st); }); };
  for (size_t i = 0; i < taps.size(); ++i) {
    CTRLV_CHECK_ARG(out_taps[i] != nullptr, "unet_encoder_forward: out_taps[%zu] is null", i);
    CTRLV_TRY(copy(taps[i].x.hi, out_taps[i], (size_t)N * taps[i].H * taps[i].W * taps[i].C));
  }
  return copy(x.hi, out_mid, (size_t)N * H * W * p->cfg.block_out_channels[p->cfg.n_blocks - 1]);
}

extern "C" int ctrlv_unet_encoder_forward(ctrlv_plan* p, const void* sample, int dtype, const float* timestep, int n_timestep,
                                          const void* ehs, const float* added_time_ids, int n_ids, void* const* out_taps,
                                          void* out_mid, int B, int F, int H, int W, void* workspace,
                                          size_t workspace_bytes, ctrlv_stream_t stream) {
  return forward_entry(p, "unet_encoder_forward", 0,
                       sample && timestep && ehs && added_time_ids && out_taps && out_mid && workspace ? nullptr : "null pointer", dtype,
                       nullptr, B, F, H, W, workspace, workspace_bytes, stream, [&](Ctx& c) {      // (workspace: sized for the whole forward)
    return unet_encoder(p, c, sample, dtype, timestep, n_timestep, ehs, added_time_ids, n_ids, out_taps, out_mid, H, W);
  });
}

extern "C" int ctrlv_controlnet_forward(ctrlv_plan* p, const void* sample, const void* control_cond, int dtype,
                                        const float* timestep, int n_timestep, const void* ehs,
                                        const float* added_time_ids, int n_ids, float conditioning_scale,
                                        void* const* out_down, void* out_mid, int B, int F, int H, int W, void* workspace,
                                        size_t workspace_bytes, ctrlv_stream_t stream) {
  return forward_entry(p, "controlnet_forward", 1,
                       sample && control_cond && timestep && ehs && added_time_ids && out_down && out_mid && workspace
                           ? nullptr : "null pointer (control_cond is required, controlnet.py:289)",
                       dtype, nullptr, B, F, H, W, workspace, workspace_bytes, stream, [&](Ctx& c) {
    return controlnet_forward(p, c, sample, control_cond, dtype, timestep, n_timestep, ehs, added_time_ids, n_ids,
                              conditioning_scale, out_down, out_mid, H, W);
  });
}

// ---- per-launch profile of the plan's own launches (include/ctrlv_hip.h)
extern "C" int ctrlv_plan_profile(ctrlv_plan* p, int enable) {
  CTRLV_CHECK_ARG(p != nullptr, "plan_profile: null plan");
  for (auto& r : p->prof) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  p->prof.clear();
  p->profiling = enable != 0;
  return CTRLV_OK;
}
extern "C" int ctrlv_plan_profile_read(ctrlv_plan* p, ctrlv_profile_record* out, int max_records) {
  CTRLV_CHECK_ARG(p != nullptr && (out != nullptr || max_records == 0), "plan_profile_read: null pointer");
  const int n = (int)p->prof.size();
  if (max_records == 0) return n;                            // (count query)
  const int m = n < max_records ? n : max_records;
  for (int i = 0; i < m; ++i) {
    auto& r = p->prof[i];
    CTRLV_HIP_TRY(hipEventSynchronize(r.e1));
    float ms = 0.f;
    CTRLV_HIP_TRY(hipEventElapsedTime(&ms, r.e0, r.e1));
    r.r.ms = ms;
    out[i] = r.r;
  }
  for (auto& r : p->prof) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  p->prof.clear();
  return m;
}
