// A whole clip as one C call: the driver behind ctrlv_pipeline_generate (include/ctrlv_hip.h).  It owns nothing but a side
// stream and two events; the four plans are borrowed, every buffer is carved out of the caller's workspace.  What it enqueues is
// what prepare_clip -> DenoiseStepper (eager) -> finish_clip of ctrlv_amd/pipelines/pipeline_utils.py enqueue, call for call:
// the plan-level entry points plus the glue kernels of csrc/pipeline_io.hip.  ctrlv_pipeline_predict_boxes is the same clip with
// the box frames written over the conditioning channels and the decoded frames clamped (VideoDiffusionPipeline.__call__ with
// bbox_images); ctrlv_pipeline_boxes_to_video chains it, the kernels of csrc/box_frames.hip and generate.
// ctrlv_pipeline_best_boxes runs that first stage once per candidate request, scores every result against ground-truth box frames
// and keeps the best one per clip without coming back to the host (the kernels of csrc/box_eval.hip);
// ctrlv_pipeline_best_boxes_to_video puts generate behind it.
#include <math.h>

#include <vector>

#include "pipeline_io.h"

constexpr uint32_t kPipelineTag = 0x43564c00u | CTRLV_ELEM_DTYPE;      // "CVL" + the element code of the library that made it

struct ctrlv_pipeline {
  uint32_t tag = kPipelineTag;           // first member: ctrlv_pipeline_boxes_to_video tells a handle of the other library by it
  ctrlv_plan* unet = nullptr;
  ctrlv_plan* cn = nullptr;
  ctrlv_vae_plan* vae = nullptr;
  ctrlv_clip_plan* clip = nullptr;
  int device = 0;
  int overlap = 1;
  hipStream_t side = nullptr;            // created by the first generate that overlaps
  hipEvent_t ev_fork = nullptr, ev_res = nullptr;
  std::vector<float> consts;             // host staging of the one upload (timesteps | guidance | added time ids)
  std::vector<float> sched;              // sigmas | timesteps of a generate_seeded call whose host gave no arrays
};

namespace {

constexpr int kMaxSteps = 1024;
constexpr size_t kAlign = 256;
inline size_t up(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

struct Carver {              // regions of a workspace, one behind the other, each on a kAlign boundary
  size_t o = 0;
  size_t take(size_t bytes) { const size_t at = o; o += up(bytes); return at; }
};

// What the driver knows of a stage beyond its request.  The fields it will supply from its own workspace count as present for
// the null checks and for `decode`; the request itself keeps NULL there until the workspace's base is known.
enum : unsigned {
  kCond = 1, kOutFrames = 2,                       // the chains: stage 2's ControlNet condition, stage 1's frames
  kImage = 4, kAugNoise = 8, kLatents = 16,        // prepare: the resized image and the two draws
  kBoxStage = 32,                                  // a box predictor's stage: the box condition is required
};

// the element type's rounding on the host (added time ids: torch.tensor([...], dtype=<model dtype>))
float round_el(float v) {
#ifdef CTRLV_ELEM_F16
  return (float)(_Float16)v;
#else
  uint32_t u;
  memcpy(&u, &v, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  u &= 0xffff0000u;
  float r;
  memcpy(&r, &u, 4);
  return r;
#endif
}

struct Geo {                 // a validated request's derived sizes
  int B, F, H, W, h, w, hw, L, nb, cfg, D, S;      // nb = model batch (2 B with cfg), D = embedding width, S = CLIP image size
  bool decode, frames_out;    // frames_out: out_frames is the caller's or the driver's (the decoder writes there, not in its phase)
};

struct BoxGeo {              // a validated ctrlv_box_condition
  int K, take;               // take = min(K + 1, F): the frames [0, K) and F - 1
  bool encode;               // 3-channel pixels: the taken frames go through the VAE encoder first
};

struct Layout {              // byte offsets into the workspace
  size_t consts, ehs, first, lmi, scaled, pred, cond_em, res[CTRLV_MAX_BLOCKS * 8 + 1], phase, total;
  int n_res;                 // residual tensors (down + mid), 0 without a ControlNet
  // loop phase
  size_t unet_ws, unet_bytes, cn_ws, cn_bytes;
  // CLIP phase
  size_t clip_px, clip_emb, clip_ws, clip_bytes;
  // VAE encode phase
  size_t enc_px, enc_lat, enc_ws, enc_bytes;
  // decode phase
  size_t dec_z, dec_frames, dec_ws, dec_bytes;
};

int validate(const ctrlv_pipeline* p, const ctrlv_clip_request* r, unsigned supplied, Geo* g) {
  CTRLV_CHECK_ARG(p != nullptr, "pipeline: null pipeline");
  CTRLV_CHECK_ARG(r != nullptr, "pipeline: null request");
  const ctrlv_model_config* uc = ctrlv_plan_info(p->unet, nullptr, nullptr);
  const ctrlv_vae_config* vc = ctrlv_vae_plan_info(p->vae, nullptr, nullptr);
  const ctrlv_clip_config* cc = ctrlv_clip_plan_info(p->clip, nullptr, nullptr);
  CTRLV_CHECK_SHAPE(r->n_clips >= 1 && r->n_clips <= 4096, "pipeline: n_clips=%d must be in [1, 4096]", r->n_clips);
  CTRLV_CHECK_SHAPE(r->num_frames >= 1 && r->num_frames <= 32, "pipeline: num_frames=%d must be in [1, 32] (the temporal "
                    "attention's limit)", r->num_frames);
  const int m = 8 * (1 << (uc->n_blocks - 1));
  CTRLV_CHECK_SHAPE(r->height > 0 && r->width > 0 && r->height % m == 0 && r->width % m == 0,
                    "pipeline: height=%d / width=%d must be positive multiples of %d (8 for the VAE times %d for the UNet's levels)",
                    r->height, r->width, m, m / 8);
  const int h = r->height / 8, w = r->width / 8;
  CTRLV_CHECK_SHAPE((h * w) % 64 == 0 && h * w <= 16384, "pipeline: height=%d / width=%d give %d latent pixels; the VAE's attention "
                    "takes a multiple of 64, at most 16384", r->height, r->width, h * w);
  CTRLV_CHECK_ARG(r->image_u8 != nullptr || (supplied & kImage), "pipeline: image_u8 is null");
  CTRLV_CHECK_ARG(r->latents != nullptr || (supplied & kLatents), "pipeline: latents is null");
  CTRLV_CHECK_ARG(r->out_latents != nullptr, "pipeline: out_latents is null");
  if (p->cn) {
    CTRLV_CHECK_ARG(r->cond != nullptr || (supplied & kCond), "pipeline: cond is null but the pipeline has a ControlNet");
  }
  if (r->cond) {
    CTRLV_CHECK_SHAPE(r->cond_channels == 3 || r->cond_channels == vc->latent_channels,
                      "pipeline: cond_channels=%d must be 3 (pixels) or %d (latents)", r->cond_channels, vc->latent_channels);
    CTRLV_CHECK_DTYPE(r->cond_dtype >= 0 && r->cond_dtype <= 2, "pipeline: cond_dtype code %d (0 fp32, 1 fp16, 2 bf16)", r->cond_dtype);
  }
  CTRLV_CHECK_SHAPE(r->num_steps >= 1 && r->num_steps <= kMaxSteps, "pipeline: num_steps=%d must be in [1, %d]", r->num_steps,
                    kMaxSteps);
  CTRLV_CHECK_ARG(r->sigmas != nullptr && r->timesteps != nullptr, "pipeline: sigmas / timesteps are null (host arrays)");
  for (int i = 0; i < r->num_steps; ++i) {
    CTRLV_CHECK_ARG(isfinite(r->sigmas[i]) && r->sigmas[i] > 0.f && r->sigmas[i + 1] >= 0.f && r->sigmas[i + 1] < r->sigmas[i],
                    "pipeline: sigmas must be positive and strictly decreasing (sigmas[%d]=%g, sigmas[%d]=%g)", i,
                    (double)r->sigmas[i], i + 1, (double)r->sigmas[i + 1]);
  }
  CTRLV_CHECK_ARG(r->noise_aug_strength >= 0.f && isfinite(r->noise_aug_strength), "pipeline: noise_aug_strength=%g",
                  (double)r->noise_aug_strength);
  CTRLV_CHECK_ARG(isfinite(r->min_guidance) && isfinite(r->max_guidance), "pipeline: min_guidance / max_guidance are not finite");
  const bool frames_out = r->out_frames != nullptr || (supplied & kOutFrames);
  const bool decode = frames_out || r->out_frames_u8 != nullptr;
  if (decode) {
    CTRLV_CHECK_SHAPE(r->decode_chunk >= 1, "pipeline: decode_chunk=%d must be >= 1 when frames are asked for", r->decode_chunk);
    CTRLV_CHECK_ARG(((uintptr_t)r->out_frames_u8 & 3) == 0, "pipeline: out_frames_u8 must be 4-byte aligned");
  }
  bool zero = true;
  for (int c = 0; c < 3; ++c) zero = zero && r->clip_mean[c] == 0.f && r->clip_std[c] == 0.f;
  if (!zero) {
    for (int c = 0; c < 3; ++c) CTRLV_CHECK_ARG(r->clip_std[c] > 0.f, "pipeline: clip_std[%d]=%g", c, (double)r->clip_std[c]);
  }
  const int rc = ctrlv_resize_check(r->n_clips, r->height, r->width, cc->image_size, cc->image_size);
  if (rc != CTRLV_OK) return rc;
  g->B = r->n_clips; g->F = r->num_frames; g->H = r->height; g->W = r->width; g->h = h; g->w = w; g->hw = h * w;
  g->L = vc->latent_channels;
  g->cfg = r->max_guidance > 1.f ? 1 : 0;
  g->nb = g->cfg ? 2 * g->B : g->B;
  g->D = cc->projection_dim;
  g->S = cc->image_size;
  g->decode = decode;
  g->frames_out = frames_out;
  return CTRLV_OK;
}

// The box condition of ctrlv_pipeline_predict_boxes against a validated request: the refusals that name the box predictor come
// first (a ControlNet pipeline would otherwise be refused for its missing cond), then the request as generate validates it.
int validate_boxes(const ctrlv_pipeline* p, const ctrlv_clip_request* r, const ctrlv_box_condition* bc, unsigned supplied, Geo* g,
                   BoxGeo* bg) {
  CTRLV_CHECK_ARG(p != nullptr, "predict_boxes: null pipeline");
  CTRLV_CHECK_ARG(r != nullptr, "predict_boxes: null request");
  CTRLV_CHECK_ARG(bc != nullptr, "predict_boxes: null box condition");
  CTRLV_CHECK_ARG(p->cn == nullptr, "predict_boxes: the pipeline has a ControlNet; the box predictor is a UNet-only pipeline "
                  "(ctrlv_pipeline_create with controlnet = NULL)");
  CTRLV_CHECK_ARG(r->cond == nullptr, "predict_boxes: cond is set; the box predictor takes its box frames through "
                  "ctrlv_box_condition, not the ControlNet condition");
  CTRLV_TRY(validate(p, r, supplied, g));
  CTRLV_CHECK_ARG(bc->reserved == 0, "predict_boxes: box condition reserved=%d must be 0", bc->reserved);
  CTRLV_CHECK_ARG(bc->frames != nullptr, "predict_boxes: box condition frames is null");
  CTRLV_CHECK_SHAPE(bc->channels == 3 || bc->channels == g->L, "predict_boxes: box condition channels=%d must be 3 (pixels) or "
                    "%d (latents)", bc->channels, g->L);
  CTRLV_CHECK_DTYPE(bc->dtype >= 0 && bc->dtype <= 2, "predict_boxes: box condition dtype code %d (0 fp32, 1 fp16, 2 bf16)",
                    bc->dtype);
  CTRLV_CHECK_SHAPE(bc->num_cond_frames >= 0 && bc->num_cond_frames <= g->F, "predict_boxes: num_cond_frames=%d must be in "
                    "[0, %d] (num_frames)", bc->num_cond_frames, g->F);
  bg->K = bc->num_cond_frames;
  bg->take = bg->K + 1 < g->F ? bg->K + 1 : g->F;
  bg->encode = bc->channels == 3;
  return CTRLV_OK;
}

// bx: the box condition of predict_boxes (its encoder call and the latents of the taken frames join the VAE-encode phase)
int layout(ctrlv_pipeline* p, const ctrlv_clip_request* r, const Geo& g, const BoxGeo* bx, Layout* L) {
  int lu = 0, lv = 0, lc = 0, ln = 1;
  ctrlv_plan_info(p->unet, nullptr, &lu);
  ctrlv_vae_plan_info(p->vae, nullptr, &lv);
  ctrlv_clip_plan_info(p->clip, nullptr, &lc);
  if (p->cn) ctrlv_plan_info(p->cn, nullptr, &ln);
  CTRLV_CHECK_ARG(lu && lv && lc && ln, "pipeline: plan not loaded (load the weights of every plan first)");
  const size_t el = sizeof(el_t);
  const size_t lat = (size_t)g.B * g.F * g.L * g.hw;              // elements of the latents of the B clips
  Carver cv;
  L->consts = cv.take((size_t)(kMaxSteps + 32 + 3 * 2 * 4096) * sizeof(float));
  L->ehs = cv.take((size_t)g.nb * g.D * el);
  L->first = cv.take((size_t)g.B * g.L * g.hw * el);
  L->lmi = cv.take((size_t)g.nb * g.F * 2 * g.L * g.hw * el);
  L->scaled = cv.take(lat * el);
  L->pred = cv.take((size_t)g.nb * g.F * g.L * g.hw * el);
  L->cond_em = 0;
  L->n_res = 0;
  if (p->cn) {
    L->cond_em = cv.take((size_t)g.nb * g.F * g.L * g.hw * el);
    const int nd = ctrlv_plan_num_down_residuals(p->cn);
    CTRLV_CHECK_SHAPE(nd + 1 <= (int)(sizeof(L->res) / sizeof(L->res[0])), "pipeline: %d residual tensors", nd + 1);
    for (int i = 0; i <= nd; ++i) {
      int64_t rows = 0;
      int32_t ch = 0;
      const int rc = ctrlv_plan_residual_shape(p->cn, i, g.nb, g.F, g.h, g.w, &rows, &ch);
      if (rc != CTRLV_OK) return rc;
      L->res[i] = cv.take((size_t)rows * ch * el);
    }
    L->n_res = nd + 1;
  }
  L->phase = cv.o;
  size_t end = cv.o;
  // the loop: UNet and ControlNet work side by side in disjoint regions
  L->unet_bytes = ctrlv_plan_workspace_bytes(p->unet, g.nb, g.F, g.h, g.w);
  if (L->unet_bytes == 0) return CTRLV_E_BAD_SHAPE;
  L->cn_bytes = 0;
  if (p->cn) {
    L->cn_bytes = ctrlv_plan_workspace_bytes(p->cn, g.nb, g.F, g.h, g.w);
    if (L->cn_bytes == 0) return CTRLV_E_BAD_SHAPE;
  }
  cv.o = L->phase;
  L->unet_ws = cv.take(L->unet_bytes);
  L->cn_ws = cv.take(L->cn_bytes);
  end = cv.o > end ? cv.o : end;
  // CLIP: resized pixels, embeddings, the tower's workspace
  L->clip_bytes = ctrlv_clip_plan_workspace_bytes(p->clip, g.B);
  if (L->clip_bytes == 0) return CTRLV_E_BAD_SHAPE;
  cv.o = L->phase;
  L->clip_px = cv.take((size_t)g.B * 3 * g.S * g.S * el);
  L->clip_emb = cv.take((size_t)g.B * g.D * el);
  L->clip_ws = cv.take(L->clip_bytes);
  end = cv.o > end ? cv.o : end;
  // VAE encode: the image's pixels, the condition's latents, the encoder's workspace (the larger of the two calls)
  L->enc_bytes = ctrlv_vae_plan_workspace_bytes(p->vae, 0, g.B, 1, g.H, g.W);
  if (L->enc_bytes == 0) return CTRLV_E_BAD_SHAPE;
  const bool enc_cond = p->cn && r->cond_channels == 3;
  if (enc_cond) {
    const size_t b2 = ctrlv_vae_plan_workspace_bytes(p->vae, 0, g.B * g.F, 1, g.H, g.W);
    if (b2 == 0) return CTRLV_E_BAD_SHAPE;
    L->enc_bytes = b2 > L->enc_bytes ? b2 : L->enc_bytes;
  }
  size_t box_lat = 0;
  if (bx && bx->encode) {      // one call over all the clips' frames when every frame is taken, else [0, K) and F - 1 per clip
    const int calls[2] = {bx->take == g.F ? g.B * g.F : bx->K, bx->take == g.F ? 0 : 1};
    for (int n : calls) {
      if (n == 0) continue;
      const size_t b2 = ctrlv_vae_plan_workspace_bytes(p->vae, 0, n, 1, g.H, g.W);
      if (b2 == 0) return CTRLV_E_BAD_SHAPE;
      L->enc_bytes = b2 > L->enc_bytes ? b2 : L->enc_bytes;
    }
    box_lat = (size_t)g.B * bx->take * g.L * g.hw * el;
  }
  cv.o = L->phase;
  L->enc_px = cv.take((size_t)g.B * 3 * g.H * g.W * el);
  L->enc_lat = cv.take(enc_cond ? lat * el : box_lat);
  L->enc_ws = cv.take(L->enc_bytes);
  end = cv.o > end ? cv.o : end;
  // decode: the scaled latents, the frames (unless the caller takes them), the decoder's workspace
  L->dec_bytes = 0;
  if (g.decode) {
    const int total = g.B * g.F, chunk = r->decode_chunk < total ? r->decode_chunk : total, last = total % chunk;
    L->dec_bytes = ctrlv_vae_plan_workspace_bytes(p->vae, 1, chunk, chunk, g.h, g.w);
    if (L->dec_bytes == 0) return CTRLV_E_BAD_SHAPE;
    if (last) {
      const size_t b2 = ctrlv_vae_plan_workspace_bytes(p->vae, 1, last, last, g.h, g.w);
      if (b2 == 0) return CTRLV_E_BAD_SHAPE;
      L->dec_bytes = b2 > L->dec_bytes ? b2 : L->dec_bytes;
    }
    cv.o = L->phase;
    L->dec_z = cv.take(lat * el);
    L->dec_frames = cv.take(g.frames_out ? 0 : (size_t)total * 3 * g.H * g.W * el);
    L->dec_ws = cv.take(L->dec_bytes);
    end = cv.o > end ? cv.o : end;
  }
  L->total = end;
  return CTRLV_OK;
}

struct Stage {               // everything one clip needs: ctrlv_pipeline_generate's, or with bc ctrlv_pipeline_predict_boxes'
  ctrlv_pipeline* p;
  ctrlv_clip_request r;      // the request as the stage sees it: what the driver supplies is NULL until its call knows the base
  const ctrlv_box_condition* bc;     // NULL: no box condition (bx is unset)
  Geo g;
  BoxGeo bx;
  Layout L;
};

// every refusal of a stage that needs no loaded plan
int validate_stage(ctrlv_pipeline* p, const ctrlv_clip_request* r, const ctrlv_box_condition* bc, unsigned supplied, Stage* st) {
  if (supplied & kBoxStage) {
    CTRLV_TRY(validate_boxes(p, r, bc, supplied, &st->g, &st->bx));
  } else {
    CTRLV_TRY(validate(p, r, supplied, &st->g));
  }
  st->p = p;
  st->r = *r;
  st->bc = (supplied & kBoxStage) ? bc : nullptr;
  return CTRLV_OK;
}

int layout_stage(Stage* st) { return layout(st->p, &st->r, st->g, st->bc ? &st->bx : nullptr, &st->L); }

int plan_stage(ctrlv_pipeline* p, const ctrlv_clip_request* r, const ctrlv_box_condition* bc, unsigned supplied, Stage* st) {
  CTRLV_TRY(validate_stage(p, r, bc, supplied, st));
  return layout_stage(st);
}

}  // namespace

extern "C" int ctrlv_pipeline_create(ctrlv_plan* unet, ctrlv_plan* controlnet, ctrlv_vae_plan* vae, ctrlv_clip_plan* clip,
                                     int device, ctrlv_pipeline** out) {
  CTRLV_CHECK_ARG(out != nullptr, "pipeline_create: null output");
  *out = nullptr;
  CTRLV_CHECK_ARG(unet != nullptr, "pipeline_create: the UNet plan is null");
  CTRLV_CHECK_ARG(vae != nullptr, "pipeline_create: the VAE plan is null");
  CTRLV_CHECK_ARG(clip != nullptr, "pipeline_create: the CLIP plan is null");
  CTRLV_CHECK_ARG(device >= 0 && device < CTRLV_MAX_DEVICES, "pipeline_create: device %d", device);
  int du = 0, dv = 0, dc = 0, dn = device;
  const ctrlv_model_config* uc = ctrlv_plan_info(unet, &du, nullptr);
  const ctrlv_vae_config* vc = ctrlv_vae_plan_info(vae, &dv, nullptr);
  const ctrlv_clip_config* cc = ctrlv_clip_plan_info(clip, &dc, nullptr);
  CTRLV_CHECK_ARG(uc->kind == 0, "pipeline_create: the first plan must be a UNet plan (kind 0)");
  if (controlnet) {
    const ctrlv_model_config* nc = ctrlv_plan_info(controlnet, &dn, nullptr);
    CTRLV_CHECK_ARG(nc->kind == 1, "pipeline_create: the second plan must be a ControlNet plan (kind 1)");
    CTRLV_CHECK_SHAPE(nc->in_channels == uc->in_channels && nc->n_blocks == uc->n_blocks &&
                      nc->cross_attention_dim == uc->cross_attention_dim,
                      "pipeline_create: the ControlNet's in_channels / blocks / cross_attention_dim differ from the UNet's");
  }
  CTRLV_CHECK_ARG(du == device && dv == device && dc == device && dn == device,
                  "pipeline_create: the plans live on devices %d / %d / %d / %d, the pipeline on %d", du, dn, dv, dc, device);
  CTRLV_CHECK_SHAPE(uc->in_channels == 2 * vc->latent_channels && uc->out_channels == vc->latent_channels,
                    "pipeline_create: the UNet takes %d and gives %d channels, the VAE has %d latent channels", uc->in_channels,
                    uc->out_channels, vc->latent_channels);
  CTRLV_CHECK_SHAPE(cc->projection_dim == uc->cross_attention_dim, "pipeline_create: the CLIP projection has %d columns, the "
                    "UNet's cross_attention_dim is %d", cc->projection_dim, uc->cross_attention_dim);
  CTRLV_CHECK_SHAPE(vc->in_channels == 3 && vc->out_channels == 3, "pipeline_create: the VAE has %d / %d image channels, not 3",
                    vc->in_channels, vc->out_channels);
  CTRLV_CHECK_ARG(vc->scaling_factor > 0.f, "pipeline_create: the VAE's scaling_factor is %g", (double)vc->scaling_factor);
  ctrlv_pipeline* p = new ctrlv_pipeline();
  p->unet = unet; p->cn = controlnet; p->vae = vae; p->clip = clip; p->device = device;
  *out = p;
  return CTRLV_OK;
}

extern "C" int ctrlv_pipeline_set_overlap(ctrlv_pipeline* p, int on) {
  CTRLV_CHECK_ARG(p != nullptr && (on == 0 || on == 1), "pipeline_set_overlap: on must be 0 or 1");
  p->overlap = on;
  return CTRLV_OK;
}

extern "C" int ctrlv_pipeline_destroy(ctrlv_pipeline* p) {
  if (!p) return CTRLV_OK;
  if (p->ev_fork) (void)hipEventDestroy(p->ev_fork);
  if (p->ev_res) (void)hipEventDestroy(p->ev_res);
  if (p->side) (void)hipStreamDestroy(p->side);
  delete p;
  return CTRLV_OK;
}

namespace {

int check_workspace(const char* who, const char* query, const void* ws, size_t ws_bytes, size_t need) {
  CTRLV_CHECK_ARG(ws != nullptr && ((uintptr_t)ws & (kAlign - 1)) == 0, "%s: the workspace must be non-null and 256-byte aligned",
                  who);
  if (ws_bytes < need) {
    ctrlv_set_error("%s: ws_bytes=%zu is smaller than the %zu bytes this request needs (%s)", who, ws_bytes, need, query);
    return CTRLV_E_WORKSPACE;
  }
  return CTRLV_OK;
}

// The clip of a planned stage in a workspace of L.total bytes: ctrlv_pipeline_generate (bc = NULL), or
// ctrlv_pipeline_predict_boxes (bc / bx: the box frames overwrite the conditioning channels, the decoded frames are clamped).
int run_stage(const Stage& st, void* ws, ctrlv_stream_t stream) {
  ctrlv_pipeline* p = st.p;
  const ctrlv_clip_request* r = &st.r;
  const ctrlv_box_condition* bc = st.bc;
  const Geo& g = st.g;
  const BoxGeo* bx = bc ? &st.bx : nullptr;
  const Layout& L = st.L;
  const hipStream_t s = (hipStream_t)stream;
  char* base = (char*)ws;
  const bool overlap = p->cn && p->overlap;
  if (overlap && !p->side) {
    CTRLV_HIP_TRY(hipStreamCreateWithFlags(&p->side, hipStreamNonBlocking));
    CTRLV_HIP_TRY(hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming));
    CTRLV_HIP_TRY(hipEventCreateWithFlags(&p->ev_res, hipEventDisableTiming));
  }
  const int B = g.B, F = g.F, Lc = g.L, hw = g.hw, nb = g.nb;
  const long lat = (long)B * F * Lc * hw;
  const float scaling = ctrlv_vae_plan_info(p->vae, nullptr, nullptr)->scaling_factor;

  // ---- the one upload: timesteps | guidance ramp | added time ids
  float* c_t = (float*)(base + L.consts);
  float* c_g = c_t + kMaxSteps;
  float* c_ids = c_g + 32;
  {
    std::vector<float>& hb = p->consts;
    hb.assign((size_t)kMaxSteps + 32 + 3 * (size_t)nb, 0.f);
    for (int i = 0; i < r->num_steps; ++i) hb[i] = r->timesteps[i];
    // torch.linspace: the first half counts up from the start, the second down from the end
    const float step = F > 1 ? (r->max_guidance - r->min_guidance) / (float)(F - 1) : 0.f;
    for (int f = 0; f < F; ++f)
      hb[kMaxSteps + f] = f < F / 2 ? r->min_guidance + step * (float)f : r->max_guidance - step * (float)(F - 1 - f);
    for (int b = 0; b < nb; ++b) {
      float* id = &hb[(size_t)kMaxSteps + 32 + 3 * (size_t)b];
      id[0] = round_el((float)(r->fps - 1));
      id[1] = round_el((float)r->motion_bucket_id);
      id[2] = round_el(r->noise_aug_strength);
    }
    CTRLV_HIP_TRY(hipMemcpyAsync(c_t, hb.data(), hb.size() * sizeof(float), hipMemcpyHostToDevice, s));
  }

  // ---- 1. CLIP embedding of the conditioning image
  static const float kClipMean[3] = {0.48145466f, 0.4578275f, 0.40821073f}, kClipStd[3] = {0.26862954f, 0.26130258f, 0.27577711f};
  bool own = false;
  for (int c = 0; c < 3; ++c) own = own || r->clip_mean[c] != 0.f || r->clip_std[c] != 0.f;
  CTRLV_TRY(ctrlv_resize_antialias(r->image_u8, 1, B, g.H, g.W, base + L.clip_px, CTRLV_ELEM_DTYPE, g.S, g.S,
                             own ? r->clip_mean : kClipMean, own ? r->clip_std : kClipStd, stream));
  CTRLV_TRY(ctrlv_clip_forward(p->clip, base + L.clip_px, CTRLV_ELEM_DTYPE, B, base + L.clip_emb, nullptr, base + L.clip_ws,
                         L.clip_bytes, stream));
  CTRLV_TRY(ctrlv_pio_cfg_double(base + L.clip_emb, CTRLV_ELEM_DTYPE, base + L.ehs, B, g.D, g.cfg, s));

  // ---- 2. VAE latents of the (noise-augmented) image and of the condition
  CTRLV_TRY(ctrlv_pixels_prepare(r->image_u8, r->aug_noise, r->noise_aug_strength, B, g.H, g.W, base + L.enc_px, stream));
  CTRLV_TRY(ctrlv_vae_encode(p->vae, base + L.enc_px, CTRLV_ELEM_DTYPE, B, g.H, g.W, nullptr, 1.0f, base + L.first, nullptr,
                       CTRLV_ELEM_DTYPE, base + L.enc_ws, L.enc_bytes, stream));
  CTRLV_TRY(ctrlv_pio_lmi_cond(base + L.first, base + L.lmi, B, F, Lc, hw, g.cfg, s));
  if (bx) {
    // the box frames [0, K) and F - 1 of every clip replace the image's latent there.  Only those are encoded: the encoder
    // treats every image on its own, so a frame's latent does not depend on which frames share its call
    if (bx->encode) {
      const size_t px = (size_t)3 * g.H * g.W * (bc->dtype == 0 ? 4 : 2), lt = (size_t)Lc * hw * sizeof(el_t);
      const char* src = (const char*)bc->frames;
      char* dst = base + L.enc_lat;
      auto encode = [&](const char* x, int n, char* out) {
        return ctrlv_vae_encode(p->vae, x, bc->dtype, n, g.H, g.W, nullptr, 1.0f, out, nullptr, CTRLV_ELEM_DTYPE, base + L.enc_ws,
                                L.enc_bytes, stream);
      };
      if (bx->take == F) {
        CTRLV_TRY(encode(src, B * F, dst));
      } else {
        for (int b = 0; b < B; ++b) {
          if (bx->K > 0) CTRLV_TRY(encode(src + (size_t)b * F * px, bx->K, dst + (size_t)b * bx->take * lt));
          CTRLV_TRY(encode(src + ((size_t)b * F + F - 1) * px, 1, dst + ((size_t)b * bx->take + bx->K) * lt));
        }
      }
      CTRLV_TRY(ctrlv_pio_lmi_boxes(dst, CTRLV_ELEM_DTYPE, bx->take, 1, base + L.lmi, B, F, bx->K, Lc, hw, g.cfg, s));
    } else {
      CTRLV_TRY(ctrlv_pio_lmi_boxes(bc->frames, bc->dtype, F, 0, base + L.lmi, B, F, bx->K, Lc, hw, g.cfg, s));
    }
  }
  if (p->cn) {
    if (r->cond_channels == 3) {
      CTRLV_TRY(ctrlv_vae_encode(p->vae, r->cond, r->cond_dtype, B * F, g.H, g.W, nullptr, 1.0f, base + L.enc_lat, nullptr,
                           CTRLV_ELEM_DTYPE, base + L.enc_ws, L.enc_bytes, stream));
      CTRLV_TRY(ctrlv_pio_cfg_double(base + L.enc_lat, CTRLV_ELEM_DTYPE, base + L.cond_em, B, (long)F * Lc * hw, g.cfg, s));
    } else {
      CTRLV_TRY(ctrlv_pio_cfg_double(r->cond, r->cond_dtype, base + L.cond_em, B, (long)F * Lc * hw, g.cfg, s));
    }
  }

  // ---- 3. / 4. the loop
  // torch divides a tensor by a host scalar as a multiplication by the reciprocal, formed in double and rounded once
  const float inv0 = (float)(1.0 / sqrt((double)r->sigmas[0] * (double)r->sigmas[0] + 1.0));
  CTRLV_TRY(ctrlv_pio_scale_latents(r->latents, r->out_latents, base + L.scaled, lat, inv0, s));
  void* res[CTRLV_MAX_BLOCKS * 8 + 1];
  for (int i = 0; i < L.n_res; ++i) res[i] = base + L.res[i];
  for (int i = 0; i < r->num_steps; ++i) {
    CTRLV_TRY(ctrlv_pio_lmi_scatter(base + L.scaled, base + L.lmi, B, F, Lc, hw, g.cfg, s));
    void* ev = nullptr;
    if (p->cn) {
      hipStream_t sc = s;
      if (overlap) {
        CTRLV_HIP_TRY(hipEventRecord(p->ev_fork, s));
        CTRLV_HIP_TRY(hipStreamWaitEvent(p->side, p->ev_fork, 0));
        sc = p->side;
      }
      CTRLV_TRY(ctrlv_controlnet_forward(p->cn, base + L.lmi, base + L.cond_em, CTRLV_ELEM_DTYPE, c_t + i, 1, base + L.ehs, c_ids, 3,
                                   r->conditioning_scale, res, res[L.n_res - 1], nb, F, g.h, g.w, base + L.cn_ws, L.cn_bytes,
                                   (ctrlv_stream_t)sc));
      if (overlap) {
        CTRLV_HIP_TRY(hipEventRecord(p->ev_res, p->side));
        ev = (void*)p->ev_res;
      }
    }
    CTRLV_TRY(ctrlv_unet_forward(p->unet, base + L.lmi, CTRLV_ELEM_DTYPE, c_t + i, 1, base + L.ehs, c_ids, 3,
                           p->cn ? (const void* const*)res : nullptr, p->cn ? res[L.n_res - 1] : nullptr, ev, base + L.pred, nb, F,
                           g.h, g.w, base + L.unet_ws, L.unet_bytes, stream));
    CTRLV_TRY(ctrlv_cfg_euler_step(r->out_latents, base + L.pred, CTRLV_ELEM_DTYPE, g.cfg, c_g, B, F, Lc * hw, r->sigmas[i],
                             r->sigmas[i + 1], base + L.scaled, stream));
  }

  // ---- 5. / 6. decode and convert
  if (g.decode) {
    const float inv_sf = (float)(1.0 / (double)scaling);
    CTRLV_TRY(ctrlv_pio_decode_input(r->out_latents, base + L.dec_z, lat, inv_sf, s));
    char* frames = r->out_frames ? (char*)r->out_frames : base + L.dec_frames;
    const int total = B * F;
    for (int i0 = 0; i0 < total; i0 += r->decode_chunk) {
      const int nf = total - i0 < r->decode_chunk ? total - i0 : r->decode_chunk;
      CTRLV_TRY(ctrlv_vae_decode(p->vae, base + L.dec_z + (size_t)i0 * Lc * hw * sizeof(el_t), CTRLV_ELEM_DTYPE, nf, nf, g.h, g.w,
                           frames + (size_t)i0 * 3 * g.H * g.W * sizeof(el_t), CTRLV_ELEM_DTYPE, base + L.dec_ws, L.dec_bytes,
                           stream));
    }
    if (r->out_frames_u8) CTRLV_TRY(ctrlv_frames_to_u8(frames, total, g.H, g.W, r->out_frames_u8, stream));
    // (the bytes above are those of the clamped frames too: ctrlv_frames_to_u8 clamps x / 2 + 0.5 to [0, 1] itself)
    if (bx && r->out_frames) CTRLV_TRY(ctrlv_pio_clamp_frames(r->out_frames, (long)total * 3 * g.H * g.W, s));
  }
  return CTRLV_OK;
}

}  // namespace

extern "C" size_t ctrlv_pipeline_workspace_bytes(ctrlv_pipeline* p, const ctrlv_clip_request* r) {
  Stage st;
  return plan_stage(p, r, nullptr, 0, &st) == CTRLV_OK ? st.L.total : 0;
}

extern "C" int ctrlv_pipeline_generate(ctrlv_pipeline* p, const ctrlv_clip_request* r, void* ws, size_t ws_bytes,
                                       ctrlv_stream_t stream) {
  Stage st;
  CTRLV_TRY(plan_stage(p, r, nullptr, 0, &st));
  CTRLV_TRY(check_workspace("pipeline_generate", "ctrlv_pipeline_workspace_bytes", ws, ws_bytes, st.L.total));
  return run_stage(st, ws, stream);
}

extern "C" size_t ctrlv_pipeline_boxes_workspace_bytes(ctrlv_pipeline* p, const ctrlv_clip_request* r,
                                                       const ctrlv_box_condition* bc) {
  Stage st;
  return plan_stage(p, r, bc, kBoxStage, &st) == CTRLV_OK ? st.L.total : 0;
}

extern "C" int ctrlv_pipeline_predict_boxes(ctrlv_pipeline* p, const ctrlv_clip_request* r, const ctrlv_box_condition* bc, void* ws,
                                            size_t ws_bytes, ctrlv_stream_t stream) {
  Stage st;
  CTRLV_TRY(plan_stage(p, r, bc, kBoxStage, &st));
  CTRLV_TRY(check_workspace("pipeline_predict_boxes", "ctrlv_pipeline_boxes_workspace_bytes", ws, ws_bytes, st.L.total));
  return run_stage(st, ws, stream);
}

namespace {

// ---- the two chains' shared front: the pipeline pair, then stage 2's request as the chain sees it

// Q: ctrlv_two_stage_request or ctrlv_best_chain_request (`reserved` and `video`)
template <class Q>
int check_pair(const char* who, const ctrlv_pipeline* pb, const ctrlv_pipeline* pv, const Q* q) {
  CTRLV_CHECK_ARG(pb != nullptr && pv != nullptr, "%s: null pipeline", who);
  CTRLV_CHECK_ARG(q != nullptr, "%s: null request", who);
  CTRLV_CHECK_ARG(pb->tag == kPipelineTag && pv->tag == kPipelineTag, "%s: both pipelines must come from this library (element "
                  "dtype code %d)", who, CTRLV_ELEM_DTYPE);
  CTRLV_CHECK_ARG(pb->device == pv->device, "%s: the pipelines live on different devices (%d and %d)", who, pb->device, pv->device);
  CTRLV_CHECK_ARG(q->reserved == 0, "%s: reserved=%d must be 0", who, q->reserved);
  CTRLV_CHECK_ARG(pv->cn != nullptr, "%s: the video pipeline has no ControlNet to take the box frames", who);
  CTRLV_CHECK_ARG(q->video.cond == nullptr, "%s: video.cond must be NULL on entry (the driver supplies stage 1's box frames)", who);
  return CTRLV_OK;
}

// first: stage 1's (first) request.  The condition is the driver's: pixels in the element type, validated with kCond
int video_request(const char* who, const ctrlv_clip_request* first, const ctrlv_clip_request* video, ctrlv_clip_request* v) {
  CTRLV_CHECK_SHAPE(first->n_clips == video->n_clips && first->num_frames == video->num_frames && first->height == video->height &&
                    first->width == video->width,
                    "%s: the two stages differ in geometry (boxes %d x %d x %d x %d, video %d x %d x %d x %d)", who, first->n_clips,
                    first->num_frames, first->height, first->width, video->n_clips, video->num_frames, video->height, video->width);
  *v = *video;
  v->cond_channels = 3;
  v->cond_dtype = CTRLV_ELEM_DTYPE;
  return CTRLV_OK;
}

struct Chain {               // ctrlv_pipeline_boxes_to_video: the two stages, and where things lie in the workspace
  Stage boxes, video;
  size_t frames, cond, post, post_bytes, stage, total;
};

int plan_chain(ctrlv_pipeline* pb, ctrlv_pipeline* pv, const ctrlv_two_stage_request* q, Chain* c) {
  CTRLV_TRY(check_pair("boxes_to_video", pb, pv, q));
  CTRLV_CHECK_ARG(isfinite(q->clean_threshold), "boxes_to_video: clean_threshold=%g", (double)q->clean_threshold);
  ctrlv_clip_request v;
  CTRLV_TRY(video_request("boxes_to_video", &q->boxes, &q->video, &v));
  // stage 1 must decode: its frames are what stage 2 is conditioned on.  Without out_frames they go into the chain's workspace
  const bool own_frames = q->boxes.out_frames == nullptr;
  CTRLV_TRY(validate_stage(pb, &q->boxes, &q->box_cond, kBoxStage | (own_frames ? kOutFrames : 0u), &c->boxes));
  CTRLV_TRY(validate_stage(pv, &v, nullptr, kCond, &c->video));
  CTRLV_TRY(layout_stage(&c->boxes));
  CTRLV_TRY(layout_stage(&c->video));
  const Geo& g = c->boxes.g;
  const size_t fr = (size_t)g.B * g.F * 3 * g.H * g.W * sizeof(el_t);
  Carver cv;
  c->frames = cv.take(own_frames ? fr : 0);
  c->cond = cv.take(fr);
  c->post_bytes = ctrlv_box_frames_post_ws_bytes(g.B, g.F);
  c->post = cv.take(c->post_bytes);
  c->stage = cv.o;
  c->total = cv.o + (c->boxes.L.total > c->video.L.total ? c->boxes.L.total : c->video.L.total);
  return CTRLV_OK;
}

// the three calls a host would make by hand; the two stages' own workspaces share one region
int run_chain(Chain* c, const ctrlv_two_stage_request* q, void* ws, ctrlv_stream_t stream) {
  char* base = (char*)ws;
  if (!c->boxes.r.out_frames) c->boxes.r.out_frames = base + c->frames;
  c->video.r.cond = base + c->cond;
  const Geo& g = c->boxes.g;
  CTRLV_TRY(run_stage(c->boxes, base + c->stage, stream));
  CTRLV_TRY(ctrlv_box_frames_post(c->boxes.r.out_frames, g.B, g.F, g.H, g.W, q->clean_threshold, nullptr, base + c->cond,
                                  q->out_box_frames_u8, base + c->post, c->post_bytes, stream));
  return run_stage(c->video, base + c->stage, stream);
}

}  // namespace

extern "C" size_t ctrlv_pipeline_chain_workspace_bytes(ctrlv_pipeline* boxes, ctrlv_pipeline* video,
                                                       const ctrlv_two_stage_request* q) {
  Chain c;
  return plan_chain(boxes, video, q, &c) == CTRLV_OK ? c.total : 0;
}

extern "C" int ctrlv_pipeline_boxes_to_video(ctrlv_pipeline* boxes, ctrlv_pipeline* video, const ctrlv_two_stage_request* q,
                                             void* ws, size_t ws_bytes, ctrlv_stream_t stream) {
  Chain c;
  CTRLV_TRY(plan_chain(boxes, video, q, &c));
  CTRLV_TRY(check_workspace("pipeline_boxes_to_video", "ctrlv_pipeline_chain_workspace_bytes", ws, ws_bytes, c.total));
  return run_chain(&c, q, ws, stream);
}

namespace {

struct Sched {               // where a schedule the request asks for is written
  float *sig, *ts;
};

struct Prep {                // ctrlv_pipeline_prepare: the filled request and the layout of prep_ws
  ctrlv_clip_request filled; // (what prepare places in prep_ws -- `supplied` -- is NULL until place_prepared)
  unsigned supplied;         // kImage (a Lanczos resize) | kAugNoise | kLatents (the two draws)
  size_t resize_ws, resize_bytes, image, aug, lat, front;      // front: the bytes of prep_ws, at least kAlign
  bool schedule;
  double init_noise_sigma;
  Geo g;
};

// Everything prepare decides on the host.  sc: the caller's arrays, the pipeline's, or a size query's scratch.  The filled
// request is validated as generate validates it.
int plan_prepare(const ctrlv_pipeline* p, const ctrlv_clip_request* in, const ctrlv_seed_request* s, Sched sc, Prep* q) {
  CTRLV_CHECK_ARG(p != nullptr, "pipeline_prepare: null pipeline");
  CTRLV_CHECK_ARG(in != nullptr, "pipeline_prepare: null request");
  CTRLV_CHECK_ARG(s != nullptr, "pipeline_prepare: null seed request");
  CTRLV_CHECK_ARG(s->reserved == 0, "pipeline_prepare: seed request reserved=%d must be 0", s->reserved);
  ctrlv_clip_request& f = q->filled;
  f = *in;
  q->schedule = in->sigmas == nullptr || in->timesteps == nullptr;
  if (q->schedule) {
    CTRLV_CHECK_SHAPE(in->num_steps >= 1 && in->num_steps <= kMaxSteps, "pipeline_prepare: num_steps=%d must be in [1, %d]",
                      in->num_steps, kMaxSteps);
    CTRLV_CHECK_ARG(sc.sig != nullptr && sc.ts != nullptr, "pipeline_prepare: the request leaves sigmas / timesteps NULL, and "
                    "sigmas_host / timesteps_host of the seed request are null (host arrays of num_steps + 1 and num_steps floats)");
    // into scratch first: a table the caller did set is kept
    std::vector<float> tmp((size_t)2 * in->num_steps + 1);
    CTRLV_TRY(ctrlv_euler_schedule(in->num_steps, s->sigma_min, s->sigma_max, tmp.data(), tmp.data() + in->num_steps + 1, nullptr));
    if (!in->sigmas) {
      memcpy(sc.sig, tmp.data(), ((size_t)in->num_steps + 1) * sizeof(float));
      f.sigmas = sc.sig;
    }
    if (!in->timesteps) {
      memcpy(sc.ts, tmp.data() + in->num_steps + 1, (size_t)in->num_steps * sizeof(float));
      f.timesteps = sc.ts;
    }
  }
  q->init_noise_sigma = sqrt((double)f.sigmas[0] * (double)f.sigmas[0] + 1.0);
  Carver cv;
  q->supplied = 0;
  q->resize_ws = q->resize_bytes = q->image = q->aug = q->lat = 0;
  if (s->src_image_u8) {
    CTRLV_CHECK_ARG(in->image_u8 == nullptr, "pipeline_prepare: image_u8 and src_image_u8 are both set");
    CTRLV_CHECK_SHAPE(s->src_height > 0 && s->src_width > 0, "pipeline_prepare: src_image_u8 without sizes (src_height=%d, "
                      "src_width=%d)", s->src_height, s->src_width);
    if (s->src_height == in->height && s->src_width == in->width) {
      f.image_u8 = s->src_image_u8;
    } else {
      CTRLV_CHECK_SHAPE(in->n_clips >= 1 && in->height > 0 && in->width > 0, "pipeline_prepare: n_clips=%d, height=%d, width=%d "
                        "must be positive", in->n_clips, in->height, in->width);
      CTRLV_TRY(ctrlv_resize_lanczos_check(in->n_clips, s->src_height, s->src_width, in->height, in->width));
      q->supplied |= kImage;
      q->resize_bytes = ctrlv_resize_lanczos_ws_bytes(in->n_clips, s->src_height, s->src_width, in->height, in->width);
      q->resize_ws = cv.take(q->resize_bytes);
      q->image = cv.take((size_t)in->n_clips * in->height * in->width * 3);
    }
  }
  if (!in->aug_noise) q->supplied |= kAugNoise;
  if (!in->latents) q->supplied |= kLatents;
  // (a ControlNet pipeline's request may still lack its cond here -- kCond --: stage 2 of a ctrlv_two_stage_request receives it
  // from the chain.  The consuming call validates the request it is given)
  const Geo& g = q->g;
  CTRLV_TRY(validate(p, &f, q->supplied | kCond, &q->g));
  if (q->supplied & kAugNoise) q->aug = cv.take((size_t)g.B * 3 * g.H * g.W * sizeof(float));
  if (q->supplied & kLatents) q->lat = cv.take((size_t)g.B * g.F * g.L * g.hw * sizeof(float));
  q->front = cv.o > 0 ? cv.o : kAlign;
  return CTRLV_OK;
}

// what prepare supplies gets its address in a request: the one place, where the workspace is known
void place_prepared(const Prep& q, void* prep_ws, ctrlv_clip_request* r) {
  char* base = (char*)prep_ws;
  if (q.supplied & kImage) r->image_u8 = base + q.image;
  if (q.supplied & kAugNoise) r->aug_noise = (const float*)(base + q.aug);
  if (q.supplied & kLatents) r->latents = (const float*)(base + q.lat);
}

int run_prepare(const Prep& q, const ctrlv_seed_request* s, void* prep_ws, ctrlv_stream_t stream) {
  char* base = (char*)prep_ws;
  const ctrlv_clip_request& f = q.filled;
  if (q.supplied & kImage)
    CTRLV_TRY(ctrlv_resize_lanczos_u8(s->src_image_u8, f.n_clips, s->src_height, s->src_width, base + q.image, f.height, f.width,
                                      base + q.resize_ws, q.resize_bytes, stream));
  if (q.supplied & kAugNoise)
    CTRLV_TRY(ctrlv_randn(s->seed, s->clip_index0, s->call, 0, f.n_clips, (size_t)3 * f.height * f.width, 1.0f, 0, base + q.aug, 0,
                          stream));
  if (q.supplied & kLatents)
    CTRLV_TRY(ctrlv_randn(s->seed, s->clip_index0, s->call, 1, f.n_clips,
                          (size_t)q.g.F * q.g.L * q.g.hw, (float)q.init_noise_sigma, 1, base + q.lat,
                          0, stream));
  return CTRLV_OK;
}

// the schedule's home of a size query or of a generate_seeded call without host arrays
Sched sched_store(std::vector<float>* v, const ctrlv_clip_request* r) {
  const int n = r && r->num_steps >= 1 && r->num_steps <= kMaxSteps ? r->num_steps : 1;
  v->assign((size_t)2 * n + 1, 0.f);
  return {v->data(), v->data() + n + 1};
}

struct Seeded {              // ctrlv_pipeline_generate_seeded: prepare in the front of the workspace, the clip behind it
  Prep prep;
  Stage clip;
};

int plan_seeded(ctrlv_pipeline* p, const ctrlv_clip_request* r, const ctrlv_seed_request* s, Sched sc, Seeded* sd) {
  CTRLV_TRY(plan_prepare(p, r, s, sc, &sd->prep));
  return plan_stage(p, &sd->prep.filled, nullptr, sd->prep.supplied, &sd->clip);
}

int run_seeded(Seeded* sd, const ctrlv_seed_request* s, void* ws, ctrlv_stream_t stream) {
  place_prepared(sd->prep, ws, &sd->clip.r);
  CTRLV_TRY(run_prepare(sd->prep, s, ws, stream));
  return run_stage(sd->clip, (char*)ws + sd->prep.front, stream);
}

}  // namespace

extern "C" size_t ctrlv_pipeline_prepare_bytes(ctrlv_pipeline* p, const ctrlv_clip_request* r, const ctrlv_seed_request* s) {
  Prep q;
  std::vector<float> tmp;
  return plan_prepare(p, r, s, sched_store(&tmp, r), &q) == CTRLV_OK ? q.front : 0;
}

extern "C" int ctrlv_pipeline_prepare(ctrlv_pipeline* p, const ctrlv_clip_request* in, const ctrlv_seed_request* s,
                                      ctrlv_clip_request* out, void* prep_ws, size_t prep_bytes, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(out != nullptr, "pipeline_prepare: null output request");
  Prep q;
  CTRLV_TRY(plan_prepare(p, in, s, {s ? s->sigmas_host : nullptr, s ? s->timesteps_host : nullptr}, &q));
  CTRLV_TRY(check_workspace("pipeline_prepare", "ctrlv_pipeline_prepare_bytes", prep_ws, prep_bytes, q.front));
  CTRLV_TRY(run_prepare(q, s, prep_ws, stream));
  place_prepared(q, prep_ws, &q.filled);
  *out = q.filled;
  return CTRLV_OK;
}

extern "C" size_t ctrlv_pipeline_seeded_workspace_bytes(ctrlv_pipeline* p, const ctrlv_clip_request* r,
                                                        const ctrlv_seed_request* s) {
  Seeded sd;
  std::vector<float> tmp;
  return plan_seeded(p, r, s, sched_store(&tmp, r), &sd) == CTRLV_OK ? sd.prep.front + sd.clip.L.total : 0;
}

extern "C" int ctrlv_pipeline_generate_seeded(ctrlv_pipeline* p, const ctrlv_clip_request* r, const ctrlv_seed_request* s, void* ws,
                                              size_t ws_bytes, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(p != nullptr, "pipeline_generate_seeded: null pipeline");
  CTRLV_CHECK_ARG(s != nullptr, "pipeline_generate_seeded: null seed request");
  Sched sc = {s->sigmas_host, s->timesteps_host};
  if (!sc.sig || !sc.ts) {
    const Sched own = sched_store(&p->sched, r);
    if (!sc.sig) sc.sig = own.sig;
    if (!sc.ts) sc.ts = own.ts;
  }
  Seeded sd;
  CTRLV_TRY(plan_seeded(p, r, s, sc, &sd));
  CTRLV_TRY(check_workspace("pipeline_generate_seeded", "ctrlv_pipeline_seeded_workspace_bytes", ws, ws_bytes,
                            sd.prep.front + sd.clip.L.total));
  return run_seeded(&sd, s, ws, stream);
}

// csrc/box_render.hip: every refusal of ctrlv_box_frames_cond that depends on neither its output nor its workspace, and the bytes
// of workspace it needs without an out_u8
int ctrlv_box_frames_cond_check(const void* objects, int n_objects, const void* frames, int n_frames, int Hs, int Ws, int H, int W,
                                size_t* ws_bytes);

namespace {

struct FromBoxes {           // ctrlv_pipeline_generate_from_boxes: the rendered condition in front, the clip behind it
  Stage clip;
  size_t cond, cond_ws_bytes, stage, total;      // the render's own workspace aliases the clip's: it is dead when the clip starts
};

int plan_from_boxes(ctrlv_pipeline* p, const ctrlv_clip_request* r, const ctrlv_box_render_request* b, FromBoxes* fb) {
  CTRLV_CHECK_ARG(p != nullptr, "generate_from_boxes: null pipeline");
  CTRLV_CHECK_ARG(r != nullptr, "generate_from_boxes: null request");
  CTRLV_CHECK_ARG(b != nullptr, "generate_from_boxes: null box render request");
  CTRLV_CHECK_ARG(r->cond == nullptr, "generate_from_boxes: cond is set together with boxes; the driver supplies the rendered frames");
  CTRLV_CHECK_ARG(p->cn != nullptr, "generate_from_boxes: the pipeline has no ControlNet to take the box frames");
  CTRLV_CHECK_ARG(b->reserved[0] == 0 && b->reserved[1] == 0, "generate_from_boxes: box render request reserved must be 0");
  ctrlv_clip_request v = *r;
  v.cond_channels = 3;
  v.cond_dtype = CTRLV_ELEM_DTYPE;
  CTRLV_TRY(validate_stage(p, &v, nullptr, kCond, &fb->clip));
  const Geo& g = fb->clip.g;
  CTRLV_CHECK_SHAPE(b->n_frames == g.B * g.F, "generate_from_boxes: the frame table has n_frames=%d records, the request %d clips "
                    "of %d frames", b->n_frames, g.B, g.F);
  CTRLV_TRY(ctrlv_box_frames_cond_check(b->objects, b->n_objects, b->frames, b->n_frames, b->src_height, b->src_width, g.H, g.W,
                                        &fb->cond_ws_bytes));
  CTRLV_TRY(layout_stage(&fb->clip));
  Carver cv;
  fb->cond = cv.take((size_t)g.B * g.F * 3 * g.H * g.W * sizeof(el_t));
  fb->stage = cv.o;
  fb->total = cv.o + (fb->cond_ws_bytes > fb->clip.L.total ? fb->cond_ws_bytes : fb->clip.L.total);
  return CTRLV_OK;
}

// the two calls a host would make by hand
int run_from_boxes(FromBoxes* fb, const ctrlv_box_render_request* b, void* ws, ctrlv_stream_t stream) {
  char* base = (char*)ws;
  const Geo& g = fb->clip.g;
  fb->clip.r.cond = base + fb->cond;
  CTRLV_TRY(ctrlv_box_frames_cond(b->objects, b->n_objects, b->frames, b->n_frames, b->src_height, b->src_width, g.H, g.W,
                                  base + fb->cond, CTRLV_ELEM_DTYPE, nullptr, base + fb->stage, fb->cond_ws_bytes, stream));
  return run_stage(fb->clip, base + fb->stage, stream);
}

}  // namespace

extern "C" size_t ctrlv_pipeline_from_boxes_workspace_bytes(ctrlv_pipeline* p, const ctrlv_clip_request* r,
                                                            const ctrlv_box_render_request* b) {
  FromBoxes fb;
  return plan_from_boxes(p, r, b, &fb) == CTRLV_OK ? fb.total : 0;
}

extern "C" int ctrlv_pipeline_generate_from_boxes(ctrlv_pipeline* p, const ctrlv_clip_request* r, const ctrlv_box_render_request* b,
                                                  void* ws, size_t ws_bytes, ctrlv_stream_t stream) {
  FromBoxes fb;
  CTRLV_TRY(plan_from_boxes(p, r, b, &fb));
  CTRLV_TRY(check_workspace("pipeline_generate_from_boxes", "ctrlv_pipeline_from_boxes_workspace_bytes", ws, ws_bytes, fb.total));
  return run_from_boxes(&fb, b, ws, stream);
}

namespace {

constexpr int kMaxCandidates = 8;

struct Best {                // ctrlv_pipeline_best_boxes: the candidates' stages, and where things lie in the workspace
  int C;
  Stage cand[kMaxCandidates];
  bool emit;                 // any of out_pt / out_cond / out_u8 (with need_cond: always)
  size_t fr, clip_bytes, slots, scratch, counts, winner, gathered, cond, post, post_bytes, stage, stage_bytes;
};

// every refusal that needs no loaded plan
int validate_best(ctrlv_pipeline* p, const ctrlv_best_boxes_request* q, Best* b) {
  CTRLV_CHECK_ARG(p != nullptr, "best_boxes: null pipeline");
  CTRLV_CHECK_ARG(q != nullptr, "best_boxes: null request");
  CTRLV_CHECK_ARG(p->tag == kPipelineTag, "best_boxes: the pipeline must come from this library (element dtype code %d)",
                  CTRLV_ELEM_DTYPE);
  CTRLV_CHECK_SHAPE(q->n_candidates >= 1 && q->n_candidates <= kMaxCandidates, "best_boxes: n_candidates=%d must be in [1, %d]",
                    q->n_candidates, kMaxCandidates);
  CTRLV_CHECK_ARG(q->reserved == 0 && q->reserved2 == 0, "best_boxes: reserved=%d / reserved2=%d must be 0", q->reserved,
                  q->reserved2);
  CTRLV_CHECK_ARG(q->candidates != nullptr, "best_boxes: the candidates array is null");
  CTRLV_CHECK_ARG(q->gt_u8 != nullptr, "best_boxes: gt_u8 is null");
  CTRLV_CHECK_ARG(isfinite(q->clean_threshold), "best_boxes: clean_threshold=%g", (double)q->clean_threshold);
  CTRLV_CHECK_ARG(((uintptr_t)q->out_counts & 7) == 0, "best_boxes: out_counts must be 8-byte aligned");
  CTRLV_CHECK_ARG(((uintptr_t)q->out_winner & 3) == 0, "best_boxes: out_winner must be 4-byte aligned");
  b->C = q->n_candidates;
  const ctrlv_clip_request& r0 = q->candidates[0];
  for (int c = 0; c < b->C; ++c) {
    const ctrlv_clip_request& r = q->candidates[c];
    CTRLV_CHECK_ARG(r.out_frames == nullptr && r.out_frames_u8 == nullptr, "best_boxes: candidate %d has out_frames / "
                    "out_frames_u8 set; the driver keeps the candidates' frames in the workspace", c);
    CTRLV_CHECK_SHAPE(r.n_clips == r0.n_clips && r.num_frames == r0.num_frames && r.height == r0.height && r.width == r0.width,
                      "best_boxes: the candidates differ in geometry (candidate 0: %d x %d x %d x %d, candidate %d: %d x %d x %d x "
                      "%d)", r0.n_clips, r0.num_frames, r0.height, r0.width, c, r.n_clips, r.num_frames, r.height, r.width);
  }
  for (int c = 0; c < b->C; ++c)       // (kOutFrames: the clip must decode, into its frame slot)
    CTRLV_TRY(validate_stage(p, &q->candidates[c], &q->box_cond, kBoxStage | kOutFrames, &b->cand[c]));
  return CTRLV_OK;
}

// need_cond: the chain's call -- a condition buffer is laid out when the request brings none
int layout_best(const ctrlv_best_boxes_request* q, bool need_cond, Best* b) {
  b->stage_bytes = 0;
  for (int c = 0; c < b->C; ++c) {
    CTRLV_TRY(layout_stage(&b->cand[c]));
    b->stage_bytes = b->cand[c].L.total > b->stage_bytes ? b->cand[c].L.total : b->stage_bytes;
  }
  const Geo& g = b->cand[0].g;
  b->emit = need_cond || q->out_pt || q->out_cond || q->out_u8;
  b->clip_bytes = (size_t)g.F * 3 * g.H * g.W * sizeof(el_t);
  b->fr = (size_t)g.B * b->clip_bytes;
  Carver cv;
  b->slots = cv.take((size_t)b->C * b->fr);                 // (C, n, clip) without gaps: ctrlv_gather_clips reads it as one array
  b->scratch = cv.take((size_t)g.B * g.F * 3 * g.H * g.W);
  b->counts = cv.take(q->out_counts ? 0 : (size_t)b->C * g.B * 6 * sizeof(unsigned long long));
  b->winner = cv.take(q->out_winner ? 0 : (size_t)g.B * sizeof(int32_t));
  b->gathered = cv.take(b->emit ? b->fr : 0);
  b->cond = cv.take(need_cond && !q->out_cond ? b->fr : 0);
  b->post_bytes = ctrlv_box_frames_post_ws_bytes(g.B, g.F);
  b->post = cv.take(b->post_bytes);
  b->stage = cv.o;
  return CTRLV_OK;
}

// out_cond: the request's, or the chain's buffer
int run_best(const ctrlv_best_boxes_request* q, Best* b, char* base, void* out_cond, ctrlv_stream_t stream) {
  const Geo& g = b->cand[0].g;
  unsigned long long* counts = q->out_counts ? q->out_counts : (unsigned long long*)(base + b->counts);
  int32_t* winner = q->out_winner ? q->out_winner : (int32_t*)(base + b->winner);
  for (int c = 0; c < b->C; ++c) {
    char* slot = base + b->slots + (size_t)c * b->fr;
    b->cand[c].r.out_frames = slot;
    CTRLV_TRY(run_stage(b->cand[c], base + b->stage, stream));
    CTRLV_TRY(ctrlv_box_frames_post(slot, g.B, g.F, g.H, g.W, q->clean_threshold, nullptr, nullptr, base + b->scratch,
                                    base + b->post, b->post_bytes, stream));
    CTRLV_TRY(ctrlv_mask_counts(q->gt_u8, base + b->scratch, g.B, g.F, g.H, g.W, counts + (size_t)c * g.B * 6, stream));
  }
  CTRLV_TRY(ctrlv_best_candidate(counts, g.B, b->C, winner, stream));
  if (!b->emit) return CTRLV_OK;
  CTRLV_TRY(ctrlv_gather_clips(base + b->slots, winner, g.B, b->C, b->clip_bytes, base + b->gathered, stream));
  return ctrlv_box_frames_post(base + b->gathered, g.B, g.F, g.H, g.W, q->clean_threshold, q->out_pt, out_cond, q->out_u8,
                               base + b->post, b->post_bytes, stream);
}

int plan_best(ctrlv_pipeline* p, const ctrlv_best_boxes_request* q, Best* b) {
  CTRLV_TRY(validate_best(p, q, b));
  return layout_best(q, false, b);
}

struct BestChain {           // ctrlv_pipeline_best_boxes_to_video
  Best best;
  Stage video;
  size_t total;
};

int plan_best_chain(ctrlv_pipeline* pb, ctrlv_pipeline* pv, const ctrlv_best_chain_request* q, BestChain* c) {
  CTRLV_TRY(check_pair("best_boxes_to_video", pb, pv, q));
  CTRLV_TRY(validate_best(pb, &q->boxes, &c->best));
  ctrlv_clip_request v;
  CTRLV_TRY(video_request("best_boxes_to_video", &q->boxes.candidates[0], &q->video, &v));
  CTRLV_TRY(validate_stage(pv, &v, nullptr, kCond, &c->video));
  CTRLV_TRY(layout_best(&q->boxes, true, &c->best));
  CTRLV_TRY(layout_stage(&c->video));
  c->total = c->best.stage + (c->best.stage_bytes > c->video.L.total ? c->best.stage_bytes : c->video.L.total);
  return CTRLV_OK;
}

int run_best_chain(BestChain* c, const ctrlv_best_chain_request* q, void* ws, ctrlv_stream_t stream) {
  char* base = (char*)ws;
  void* cond = q->boxes.out_cond ? q->boxes.out_cond : (void*)(base + c->best.cond);
  c->video.r.cond = cond;
  CTRLV_TRY(run_best(&q->boxes, &c->best, base, cond, stream));
  return run_stage(c->video, base + c->best.stage, stream);
}

}  // namespace

// (eight stages: Best and BestChain live off the stack)

extern "C" size_t ctrlv_pipeline_best_boxes_workspace_bytes(ctrlv_pipeline* p, const ctrlv_best_boxes_request* q) {
  std::vector<Best> b(1);
  return plan_best(p, q, &b[0]) == CTRLV_OK ? b[0].stage + b[0].stage_bytes : 0;
}

extern "C" int ctrlv_pipeline_best_boxes(ctrlv_pipeline* p, const ctrlv_best_boxes_request* q, void* ws, size_t ws_bytes,
                                         ctrlv_stream_t stream) {
  std::vector<Best> b(1);
  CTRLV_TRY(plan_best(p, q, &b[0]));
  CTRLV_TRY(check_workspace("pipeline_best_boxes", "ctrlv_pipeline_best_boxes_workspace_bytes", ws, ws_bytes,
                            b[0].stage + b[0].stage_bytes));
  return run_best(q, &b[0], (char*)ws, q->out_cond, stream);
}

extern "C" size_t ctrlv_pipeline_best_chain_workspace_bytes(ctrlv_pipeline* boxes, ctrlv_pipeline* video,
                                                            const ctrlv_best_chain_request* q) {
  std::vector<BestChain> c(1);
  return plan_best_chain(boxes, video, q, &c[0]) == CTRLV_OK ? c[0].total : 0;
}

extern "C" int ctrlv_pipeline_best_boxes_to_video(ctrlv_pipeline* boxes, ctrlv_pipeline* video, const ctrlv_best_chain_request* q,
                                                  void* ws, size_t ws_bytes, ctrlv_stream_t stream) {
  std::vector<BestChain> c(1);
  CTRLV_TRY(plan_best_chain(boxes, video, q, &c[0]));
  CTRLV_TRY(check_workspace("pipeline_best_boxes_to_video", "ctrlv_pipeline_best_chain_workspace_bytes", ws, ws_bytes, c[0].total));
  return run_best_chain(&c[0], q, ws, stream);
}
