// A training batch as one C call: the driver behind ctrlv_train_batch_prepare (include/ctrlv_hip.h), beside the clip driver of
// csrc/pipeline.hip and built like it.  It owns nothing: the two plans are borrowed, every buffer is carved out of the caller's
// workspace.  What it enqueues is what a host would call by hand -- ctrlv_resize_antialias_clamped, ctrlv_clip_forward,
// ctrlv_train_draws, ctrlv_randn, ctrlv_vae_encode, ctrlv_train_assemble -- plus the glue kernels of csrc/train_batch.hip.
#include <math.h>

#include "pipeline_io.h"
#include "train_batch.h"

namespace {

constexpr size_t kAlign = 256;
inline size_t up(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

struct Carver {              // regions of a workspace, one behind the other, each on a kAlign boundary
  size_t o = 0;
  size_t take(size_t bytes) { const size_t at = o; o += up(bytes); return at; }
};

constexpr uint32_t kStreamTarget = 4, kStreamImage = 5, kStreamControl = 6;      // posterior noise (the header's stream ids)

struct Geo {                 // a validated request's derived sizes
  int n, F, H, W, h, w, hw, L, D, S, mode, K;
  float scaling;
  size_t lat, img;           // elements of the latents of the n clips, and of their image latents
};

struct Layout {              // byte offsets into the workspace
  size_t img32, keep, mask, first, cond, phase, own, total;
  // CLIP phase
  size_t clip_px, clip_emb, clip_ws, clip_bytes;
  // VAE phase
  size_t enc_noise, enc_ws, enc_bytes;
};

int validate(const ctrlv_vae_plan* vae, const ctrlv_clip_plan* clip, const ctrlv_train_batch_request* r, Geo* g) {
  CTRLV_CHECK_ARG(vae != nullptr, "train_batch: the VAE plan is null");
  CTRLV_CHECK_ARG(clip != nullptr, "train_batch: the CLIP plan is null");
  CTRLV_CHECK_ARG(r != nullptr, "train_batch: null request");
  CTRLV_CHECK_ARG(r->reserved == 0, "train_batch: reserved=%d must be 0", r->reserved);
  int dv = 0, dc = 0;
  const ctrlv_vae_config* vc = ctrlv_vae_plan_info(vae, &dv, nullptr);
  const ctrlv_clip_config* cc = ctrlv_clip_plan_info(clip, &dc, nullptr);
  CTRLV_CHECK_ARG(dv == dc, "train_batch: the plans live on different devices (%d and %d)", dv, dc);
  CTRLV_CHECK_SHAPE(vc->in_channels == 3, "train_batch: the VAE has %d image channels, not 3", vc->in_channels);
  CTRLV_CHECK_SHAPE(r->n_clips >= 1 && r->n_clips <= 4096, "train_batch: n_clips=%d must be in [1, 4096]", r->n_clips);
  CTRLV_CHECK_SHAPE(r->num_frames >= 1 && r->num_frames <= 32, "train_batch: num_frames=%d must be in [1, 32] (the temporal "
                    "attention's limit)", r->num_frames);
  CTRLV_CHECK_SHAPE(r->height > 0 && r->width > 0 && r->height % 8 == 0 && r->width % 8 == 0,
                    "train_batch: height=%d / width=%d must be positive multiples of 8", r->height, r->width);
  const int h = r->height / 8, w = r->width / 8;
  CTRLV_CHECK_SHAPE((h * w) % 64 == 0 && h * w <= 16384, "train_batch: height=%d / width=%d give %d latent pixels; the VAE's attention "
                    "takes a multiple of 64, at most 16384", r->height, r->width, h * w);
  CTRLV_CHECK_ARG(r->mode >= 0 && r->mode <= 2, "train_batch: mode=%d must be 0 (ControlNet step), 1 (stage-1 UNet step) or 2 (box-"
                  "predictor step)", r->mode);
  CTRLV_CHECK_ARG(r->clips != nullptr, "train_batch: clips is null");
  CTRLV_CHECK_DTYPE(r->clips_dtype >= 0 && r->clips_dtype <= 2, "train_batch: clips_dtype code %d (0 fp32, 1 fp16, 2 bf16)",
                    r->clips_dtype);
  if (r->mode == 1) {
    CTRLV_CHECK_ARG(r->box_frames == nullptr, "train_batch: box_frames is set, but mode 1 (stage-1 UNet step) takes none");
  } else {
    CTRLV_CHECK_ARG(r->box_frames != nullptr, "train_batch: box_frames is null, but mode %d needs them", r->mode);
    CTRLV_CHECK_DTYPE(r->box_dtype >= 0 && r->box_dtype <= 2, "train_batch: box_dtype code %d (0 fp32, 1 fp16, 2 bf16)", r->box_dtype);
  }
  if (r->mode == 2)
    CTRLV_CHECK_SHAPE(r->num_cond_frames >= 0 && r->num_cond_frames <= r->num_frames, "train_batch: num_cond_frames=%d must be in "
                      "[0, %d] (num_frames)", r->num_cond_frames, r->num_frames);
  CTRLV_CHECK_ARG(isfinite(r->dropout_prob), "train_batch: dropout_prob=%g is not finite (negative: no dropout)", r->dropout_prob);
  CTRLV_CHECK_ARG(r->sigma_table != nullptr && r->timestep_table != nullptr, "train_batch: sigma_table / timestep_table are null "
                  "(device arrays of table_size floats)");
  CTRLV_CHECK_SHAPE(r->table_size >= 1 && r->table_size <= 65536, "train_batch: table_size=%d must be in [1, 65536]", r->table_size);
  CTRLV_CHECK_ARG(isfinite(r->scaling_factor) && r->scaling_factor >= 0.f, "train_batch: scaling_factor=%g (0: the VAE plan's)",
                  (double)r->scaling_factor);
  const float scaling = r->scaling_factor != 0.f ? r->scaling_factor : vc->scaling_factor;
  CTRLV_CHECK_ARG(scaling > 0.f, "train_batch: the VAE plan's scaling_factor is %g", (double)scaling);
  bool zero = true;
  for (int c = 0; c < 3; ++c) zero = zero && r->clip_mean[c] == 0.f && r->clip_std[c] == 0.f;
  if (!zero) {
    for (int c = 0; c < 3; ++c) CTRLV_CHECK_ARG(r->clip_std[c] > 0.f, "train_batch: clip_std[%d]=%g", c, (double)r->clip_std[c]);
  }
  CTRLV_CHECK_DTYPE(r->sample_dtype == 0 || r->sample_dtype == CTRLV_ELEM_DTYPE, "train_batch: sample_dtype code %d (0 fp32 or %d, "
                    "this library's element type)", r->sample_dtype, CTRLV_ELEM_DTYPE);
  CTRLV_CHECK_ARG(r->target_latents && r->noisy_latents && r->sample && r->encoder_hidden_states && r->sigmas && r->timesteps &&
                  r->indices && r->random_p, "train_batch: a null output (target_latents, noisy_latents, sample, "
                  "encoder_hidden_states, sigmas, timesteps, indices and random_p are required)");
  if (r->mode == 0) {
    CTRLV_CHECK_ARG(r->control_cond != nullptr, "train_batch: control_cond is null, but mode 0 writes it");
  } else {
    CTRLV_CHECK_ARG(r->control_cond == nullptr, "train_batch: control_cond is set, but only mode 0 writes it");
  }
  const uintptr_t f32s = (uintptr_t)r->target_latents | (uintptr_t)r->noisy_latents | (uintptr_t)r->control_cond | (uintptr_t)r->sigmas |
                         (uintptr_t)r->timesteps | (uintptr_t)r->indices | (uintptr_t)r->random_p | (uintptr_t)r->noise |
                         (uintptr_t)r->sigma_table | (uintptr_t)r->timestep_table;
  CTRLV_CHECK_ARG((f32s & 3) == 0 && ((uintptr_t)r->sample & (r->sample_dtype == 0 ? 3 : 1)) == 0 &&
                  ((uintptr_t)r->encoder_hidden_states & 1) == 0, "train_batch: a tensor is not aligned to its element size");
  CTRLV_TRY(ctrlv_resize_check(r->n_clips, r->height, r->width, cc->image_size, cc->image_size));
  CTRLV_TRY(ctrlv_train_assemble_check(r->mode == 2 ? 1 : 0, r->num_cond_frames, r->n_clips, r->num_frames, vc->latent_channels, h, w));
  g->n = r->n_clips; g->F = r->num_frames; g->H = r->height; g->W = r->width; g->h = h; g->w = w; g->hw = h * w;
  g->L = vc->latent_channels;
  g->D = cc->projection_dim;
  g->S = cc->image_size;
  g->mode = r->mode;
  g->K = r->mode == 2 ? r->num_cond_frames : 0;
  g->scaling = scaling;
  g->img = (size_t)g->n * g->L * g->hw;
  g->lat = g->img * g->F;
  return CTRLV_OK;
}

// The driver's own buffers: host arithmetic on the request and the plans' configurations (no weights needed).  L->own is what
// they take up to the end of the fixed part of either phase; the plans' workspaces come behind (layout_plans).
void layout_own(const Geo& g, Layout* L) {
  Carver cv;
  L->img32 = cv.take((size_t)g.n * 3 * g.H * g.W * sizeof(float));
  L->keep = cv.take((size_t)g.n * sizeof(float));
  L->mask = cv.take((size_t)g.n * sizeof(float));
  L->first = cv.take(g.img * sizeof(float));
  L->cond = cv.take(g.mode == 2 ? g.lat * sizeof(float) : 0);
  L->phase = cv.o;
  L->clip_px = cv.take((size_t)g.n * 3 * g.S * g.S * sizeof(el_t));
  L->clip_emb = cv.take((size_t)g.n * g.D * sizeof(el_t));
  L->clip_ws = cv.o;
  cv.o = L->phase;
  L->enc_noise = cv.take(g.lat * sizeof(float));
  L->enc_ws = cv.o;
  L->own = L->clip_ws > L->enc_ws ? L->clip_ws : L->enc_ws;
}

int layout_plans(ctrlv_vae_plan* vae, ctrlv_clip_plan* clip, const Geo& g, Layout* L) {
  int lv = 0, lc = 0;
  ctrlv_vae_plan_info(vae, nullptr, &lv);
  ctrlv_clip_plan_info(clip, nullptr, &lc);
  CTRLV_CHECK_ARG(lv && lc, "train_batch: plan not loaded (load the weights of both plans first)");
  L->clip_bytes = ctrlv_clip_plan_workspace_bytes(clip, g.n);
  if (L->clip_bytes == 0) return CTRLV_E_BAD_SHAPE;
  // the encoder's workspace: the larger of the image's call and the frames' calls
  L->enc_bytes = ctrlv_vae_plan_workspace_bytes(vae, 0, g.n, 1, g.H, g.W);
  if (L->enc_bytes == 0) return CTRLV_E_BAD_SHAPE;
  const size_t b2 = ctrlv_vae_plan_workspace_bytes(vae, 0, g.n * g.F, 1, g.H, g.W);
  if (b2 == 0) return CTRLV_E_BAD_SHAPE;
  L->enc_bytes = b2 > L->enc_bytes ? b2 : L->enc_bytes;
  const size_t end_clip = L->clip_ws + up(L->clip_bytes), end_enc = L->enc_ws + up(L->enc_bytes);
  L->total = end_clip > end_enc ? end_clip : end_enc;
  return CTRLV_OK;
}

int check_workspace(const void* ws, size_t ws_bytes, size_t need, const char* of_what) {
  CTRLV_CHECK_ARG(ws != nullptr && ((uintptr_t)ws & (kAlign - 1)) == 0, "train_batch_prepare: the workspace must be non-null and "
                  "256-byte aligned");
  if (ws_bytes < need) {
    ctrlv_set_error("train_batch_prepare: ws_bytes=%zu is smaller than the %zu bytes %s (ctrlv_train_batch_workspace_bytes)", ws_bytes,
                    need, of_what);
    return CTRLV_E_WORKSPACE;
  }
  return CTRLV_OK;
}

int run(ctrlv_vae_plan* vae, ctrlv_clip_plan* clip, const ctrlv_train_batch_request* r, const Geo& g, const Layout& L, void* ws,
        ctrlv_stream_t stream) {
  const hipStream_t s = (hipStream_t)stream;
  char* base = (char*)ws;
  const int n = g.n, F = g.F;
  float* img32 = (float*)(base + L.img32);
  float* keep = (float*)(base + L.keep);
  float* mask = (float*)(base + L.mask);
  float* first = (float*)(base + L.first);
  float* cond = g.mode == 2 ? (float*)(base + L.cond) : nullptr;
  float* enc_noise = (float*)(base + L.enc_noise);
  const size_t per_frames = (size_t)F * g.L * g.hw, per_image = (size_t)g.L * g.hw;

  // ---- clips[:, 0] as fp32: the CLIP prologue's and the image encoder's input
  CTRLV_TRY(ctrlv_tb_first_frames(r->clips, r->clips_dtype, n, F, (long)3 * g.H * g.W, img32, s));

  // ---- 1. CLIP embedding of the first frame, with the training prologue's clamp
  static const float kClipMean[3] = {0.48145466f, 0.4578275f, 0.40821073f}, kClipStd[3] = {0.26862954f, 0.26130258f, 0.27577711f};
  bool own = false;
  for (int c = 0; c < 3; ++c) own = own || r->clip_mean[c] != 0.f || r->clip_std[c] != 0.f;
  CTRLV_TRY(ctrlv_resize_antialias_clamped(img32, 0, n, g.H, g.W, base + L.clip_px, CTRLV_ELEM_DTYPE, g.S, g.S,
                                           own ? r->clip_mean : kClipMean, own ? r->clip_std : kClipStd, stream));
  CTRLV_TRY(ctrlv_clip_forward(clip, base + L.clip_px, CTRLV_ELEM_DTYPE, n, base + L.clip_emb, nullptr, base + L.clip_ws,
                               L.clip_bytes, stream));

  // ---- 2. / 3. the per-clip draws, the prompt half of the dropout
  CTRLV_TRY(ctrlv_train_draws(r->seed, r->clip_index0, r->call, n, r->sigma_table, r->timestep_table, r->table_size, r->dropout_prob,
                              r->indices, r->sigmas, r->timesteps, r->random_p, keep, mask, stream));
  CTRLV_TRY(ctrlv_tb_keep_rows(base + L.clip_emb, keep, n, g.D, r->encoder_hidden_states, s));

  // ---- 4. / 5. posterior noise and the encoder, one tensor after the other (the CLIP phase's region is free from here on)
  auto encode = [&](const void* px, int dtype, int images, uint32_t stream_id, size_t per_clip, float scale, float* out) {
    CTRLV_TRY(ctrlv_randn(r->seed, r->clip_index0, r->call, stream_id, n, per_clip, 1.0f, 0, enc_noise, 0, stream));
    return ctrlv_vae_encode(vae, px, dtype, images, g.H, g.W, enc_noise, scale, out, nullptr, 0, base + L.enc_ws, L.enc_bytes,
                            stream);
  };
  if (g.mode == 2) {
    CTRLV_TRY(encode(r->box_frames, r->box_dtype, n * F, kStreamTarget, per_frames, 1.0f, cond));
    CTRLV_TRY(ctrlv_tb_scale(cond, g.scaling, (long)g.lat, r->target_latents, s));
  } else {
    CTRLV_TRY(encode(r->clips, r->clips_dtype, n * F, kStreamTarget, per_frames, g.scaling, r->target_latents));
  }
  CTRLV_TRY(encode(img32, 0, n, kStreamImage, per_image, 1.0f, first));
  if (g.mode == 0) CTRLV_TRY(encode(r->box_frames, r->box_dtype, n * F, kStreamControl, per_frames, 1.0f, r->control_cond));

  // ---- 6. noising, the model input and the conditioning channels
  return ctrlv_train_assemble(r->target_latents, nullptr, r->sigmas, mask, cond, first, g.mode == 2 ? 1 : 0, g.K, n, F, g.L, g.h, g.w,
                              r->seed, r->clip_index0, r->call, r->noisy_latents, r->sample, r->sample_dtype, r->noise, stream);
}

}  // namespace

extern "C" size_t ctrlv_train_batch_workspace_bytes(ctrlv_vae_plan* vae, ctrlv_clip_plan* clip, const ctrlv_train_batch_request* r) {
  Geo g;
  Layout L;
  if (validate(vae, clip, r, &g) != CTRLV_OK) return 0;
  layout_own(g, &L);
  return layout_plans(vae, clip, g, &L) == CTRLV_OK ? L.total : 0;
}

extern "C" int ctrlv_train_batch_prepare(ctrlv_vae_plan* vae, ctrlv_clip_plan* clip, const ctrlv_train_batch_request* r, void* ws,
                                         size_t ws_bytes, ctrlv_stream_t stream) {
  Geo g;
  Layout L;
  CTRLV_TRY(validate(vae, clip, r, &g));
  layout_own(g, &L);
  CTRLV_TRY(check_workspace(ws, ws_bytes, L.own, "of the driver's own buffers alone"));
  CTRLV_TRY(layout_plans(vae, clip, g, &L));
  CTRLV_TRY(check_workspace(ws, ws_bytes, L.total, "this request needs"));
  return run(vae, clip, r, g, L, ws, stream);
}
