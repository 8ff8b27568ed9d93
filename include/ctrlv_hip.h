/*
 * ctrlv_hip.h -- C ABI of libctrlv_hip.so: the MI355X (gfx950) implementation of Ctrl-V's denoising hot path.
 *
 * The reference (oooolga/Ctrl-V) has NO native boundary: its hot path is two Python callables whose arithmetic lives
 * in diffusers==0.27.2 torch modules.  Each entry point below names the reference interface (file:line under
 * /root/reference, or the diffusers block it instantiates) that it replaces.  All functions:
 *   - take plain device pointers + sizes (no torch types), enqueue on the caller's hipStream_t, never allocate
 *     device memory, never synchronise the host;
 *   - return 0 on success, <0 on error (CTRLV_E_*); the message is available through ctrlv_last_error();
 *   - read inputs only; outputs are caller-owned buffers.
 *
 * Activations are CHANNELS-LAST rows: a tensor the reference holds as (N, C, H, W) is the row-major matrix
 * [N*H*W, C] of 16-bit ELEMENTS here (row = (n, y, x), n = b*F + f).  fp32 is used for all accumulation and statistics.
 *
 * ELEMENT TYPE.  The same sources and the same ABI are built twice:
 *   libctrlv_hip.so      elements are bf16  (ctrlv_elem_dtype() == 2) -- BASELINE.json's dtype; inference + training step
 *   libctrlv_hip_f16.so  elements are fp16  (ctrlv_elem_dtype() == 1) -- the dtype the reference itself evaluates in (fp16
 *                        autocast: config/a100l.yaml:9, tools/eval_video_controlnet.py:110-118); inference plans of fp16 models
 * Wherever this header says "bf16" for an activation / packed weight / residual buffer, read "the library's element
 * type".  The dtype CODES of the model boundary (0 fp32, 1 fp16, 2 bf16: sample, ehs, parameters, outputs) mean the same
 * in both libraries.  A process may load both (the host layer selects by the model's dtype).
 */
#ifndef CTRLV_HIP_H
#define CTRLV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ctrlv_stream_t; /* hipStream_t */

enum {
  CTRLV_OK = 0,
  CTRLV_E_BAD_ARG = -1,
  CTRLV_E_BAD_SHAPE = -2,
  CTRLV_E_HIP = -3,
  CTRLV_E_BAD_DTYPE = -4,  /* a dtype code outside {0 fp32, 1 fp16, 2 bf16} at the model boundary */
  CTRLV_E_WORKSPACE = -5,  /* caller-supplied workspace smaller than ctrlv_plan_workspace_bytes() */
};

/* Library ABI version (bumped on any signature change; 21: the LoRA entry points; 22: the two backward kernels of the VAE
 * decoder's training walk, ctrlv_softmax_rows_bwd and ctrlv_time_conv_rows_to_nchw_bwd).  Purely ADDITIVE entry points do not
 * bump the number: a host built against 22 runs unchanged on a library that also exports the CLIP vision kernels
 * (ctrlv_attention_tokens, ctrlv_clip_patch_rows, ctrlv_clip_tokens, ctrlv_act_rows) or ctrlv_gemm_tokens and the CLIP plan
 * (ctrlv_clip_*) ctrlv_vae_posterior or the VAE plan (ctrlv_vae_*) or the whole-clip driver and its I/O kernels (ctrlv_pipeline_*,
 * ctrlv_resize_antialias, ctrlv_pixels_prepare, ctrlv_frames_to_u8) or the seeded-clip entry points (ctrlv_randn,
 * ctrlv_euler_schedule, ctrlv_resize_lanczos_u8, ctrlv_pipeline_prepare, ctrlv_pipeline_generate_seeded) or the per-frame quality
 * entry points (ctrlv_frame_stats, ctrlv_frame_ssim, ctrlv_frame_ssim_ws_bytes, ctrlv_resize_frames_u8,
 * ctrlv_resize_frames_ws_bytes) or the LPIPS entry points (ctrlv_lpips_*, ctrlv_relu_maxpool_rows) or the optimiser pass (ctrlv_adamw_step, ctrlv_ema_step)
 * or the gradient-norm clipping in front of it (ctrlv_grad_sumsq, ctrlv_grad_sumsq_partials, ctrlv_grad_finish,
 * ctrlv_adamw_step_dev) or the loss-scaled forms of its last two stages (ctrlv_grad_finish_scaled, ctrlv_adamw_step_scaled)
 * or the box-frame rendering (ctrlv_render_box_frames, ctrlv_box_*, ctrlv_pipeline_generate_from_boxes),
 * and a host that needs them fails at symbol lookup on a library without them.
 * NOT neutral, although the number did not move: ctrlv_gemm_desc.pad_br gives meaning to four bytes that were alignment
 * padding, so descriptors must now be zero-initialised (see the field). */
int ctrlv_abi_version(void);
/* dtype code (1 fp16 / 2 bf16) of the element type this library was built for (see above). */
int ctrlv_elem_dtype(void);
/* Copies the build id (hash of the kernel sources + this header the library was compiled from) into buf; returns its
 * length.  The Python host layer compares it with the sources it sits next to and refuses a stale library. */
int ctrlv_build_id(char* buf, size_t n);
/* Copies the last error message of the calling thread into buf (NUL terminated); returns its length. */
int ctrlv_last_error(char* buf, size_t n);

/* ------------------------------------------------------------------------------------------------------------------
 * Gather-GEMM:  out[m, :] = epilogue( sum_taps A_tap[m, :] . W[:, tap, :]^T )
 *
 * One kernel family replaces every dense contraction of the path:
 *   mode 0  nn.Linear / 1x1 Conv2d ........ to_q/k/v/out, proj_in/out, GEGLU FF, time MLPs, conv_shortcut,
 *                                            controlnet_down_blocks[i] / controlnet_mid_block zero-convs
 *                                            (src/ctrlv/models/controlnet.py:148-185,331-344; `conditioning_scale`
 *                                            of :343-344 is folded into s_acc)
 *   mode 1  Conv2d 3x3 pad 1 .............. ResnetBlock2D.conv1/conv2, Downsample2D (stride 2), Upsample2D
 *                                            (nearest x2 fused: up=1), conv_in / conv_out
 *                                            (unet_spatio_temporal_condition.py:97,163; controlnet.py:297-298)
 *   mode 2  Conv3d (3,1,1) pad (1,0,0) .... TemporalResnetBlock.conv1/conv2 (3 taps along the frame axis)
 *
 * A, A2, R1, R2, out(bf16) are bf16; W is bf16 [N][taps*Cin] (K contiguous, tap-major); bias, V are fp32.
 * Epilogue, in fp32:  v = s_acc*(acc + bias[n]) + s1*R1[m,n] + s2*R2[m,n] + V[vidx(m), n];  v = silu(v) if act;
 * GEGLU (geglu=1): weight rows are interleaved in blocks of 16 (value block, gate block); out[m, j] = a_j * gelu_erf(g_j)
 * (erf-GELU x*Phi(x) evaluated in fp32 by a polynomial, |absolute error| <= 2.1e-6 -- csrc/common.h),
 * out has N/2 columns.  This fuses AlphaBlender, residual adds, the temb broadcast add, the frame
 * positional embedding and the degenerate 1-key CLIP cross-attention (a row vector per clip) into the GEMM.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct ctrlv_gemm_desc {
  const void* A;      /* [rows, lda] bf16 */
  const void* A2;     /* optional second source for channels >= c_split (skip-concat, torch.cat dim=1) or NULL;
                         every mode accepts it (fast path: plain GEMM with a bias-only epilogue, the 1x1 shortcuts) */
  const void* W;      /* [N, taps*Cin] bf16 */
  void* out;          /* [M, ldo] bf16 (or fp32 if out_f32) */
  const float* bias;  /* [N] or NULL */
  const void* R1;     /* [M, ldr1] bf16 or NULL */
  const void* R2;     /* [M, ldr2] bf16 or NULL */
  const float* V;     /* [*, ldv] fp32 row-vector table or NULL */
  int32_t M, N, Cin, taps;
  int32_t lda, lda2, c_split;         /* ROW PITCHES (lda, lda2, ldo, ldr1, ldr2, ldv, ld_raw), in elements of their tensor: a
                                         pitch covers its row -- rows may be views into wider buffers, they never overlap.
                                         lda >= Cin (>= c_split with A2), lda2 >= Cin - c_split; ldo, ldr1, ldr2 and ldv >=
                                         the stored columns = n_store (GEGLU: min(n_store, N / 2)); ld_raw >= N.  Checked for
                                         the operands that are present, before any launch (CTRLV_E_BAD_SHAPE); the same rule
                                         holds for ctrlv_gemm_f8 and the out / R1 / R2 pitches of ctrlv_ff_fused (>= 320) */
  int32_t mode;                       /* 0 plain, 1 conv2d 3x3, 2 temporal (3,1,1) */
  int32_t H, Wd, Ho, Wo, stride, up;  /* mode 1: input H x Wd (before upsample), output Ho x Wo.  up = 1: nearest-x2 upsample
                                         fused into the 3x3 gather (source pixel (y >> 1, x >> 1)), W = [N][9 Cin].
                                         up = 2 (stride 1, Ho = 2 H, Wo = 2 Wd; only where ctrlv_gemm_up_phase_serves(d)): the
                                         same conv in PHASE FORM -- four 2x2 convs on the low-resolution input, one per output
                                         parity p = 2 py + px: out[2 i + py, 2 j + px] = sum_{a, b in {0, 1}} W[p][.][(2 a + b) Cin
                                         + c] x[i - 1 + py + a, j - 1 + px + b][c], pixels outside H x Wd read as zero.  W = the
                                         four panels [4][N][4 Cin] written by ctrlv_pack_up_phase_weight; M, Ho, Wo, taps = 9
                                         and every other field as for up = 1.  4/9 of the multiply-adds; each phase weight is
                                         a sum of 1, 2, 2 or 4 taps rounded once to the element type, so the result equals
                                         the up = 1 launch up to that one rounding (exactly, where the sums are exact). */
  int32_t F, S;                       /* mode 2: frames per clip, pixels per frame.  mode 0: S = optional rows-per-image
                                         hint (0 = unknown), the shape key of the split plan (ctrlv_gemm_splitk_ws_bytes) */
  int32_t ldo, n_store;               /* output leading dimension; columns >= n_store are not written */
  int32_t ldr1, ldr2;
  float s_acc, s1, s2;
  int32_t vmode;                      /* 0 none; 1: vidx = (m / vdiv) % vmod; 2: vidx = ((m / vdiv) * vS + m % vS) % vmod */
  int32_t vdiv, vmod, vS, ldv;
  int32_t act;                        /* 0 none, 1 SiLU */
  int32_t geglu;
  int32_t out_f32;
  int32_t tile;                       /* 0 auto, else forces a tile configuration (testing) */
  int32_t ld_raw;                     /* leading dimension of raw_out (elements) */
  int32_t pad_br;                     /* 1 (mode 1, taps 9, stride 2, up 0 only): the stride-2 conv with the padding on the
                                         BOTTOM and RIGHT only -- F.pad(x, (0, 1, 0, 1)) + Conv2d(3, stride 2, padding 0), the
                                         down-sampler of the VAE encoder: out[yo, xo] = sum_{ky, kx} w[ky, kx] x[2 yo + ky,
                                         2 xo + kx], row H and column Wd read as zero; H and Wd even, Ho = H / 2, Wo = Wd / 2.
                                         The tap centre moves from (2 yo, 2 xo) to (2 yo + 1, 2 xo + 1); inference only (the
                                         backward entry points refuse it), no gn_partials, no K split, no split planes.
                                         LAYOUT AND A REQUIREMENT.  The field occupies the four bytes that were alignment
                                         padding in front of raw_out (offset 196): sizeof and every other offset are those
                                         of ABI 22 and the version number stays 22.  Until this field those bytes had no
                                         meaning and nothing asked a host to initialise them; from now on a descriptor MUST
                                         be zero-initialised (memset / calloc / `= {0}` / ctypes) before its fields are
                                         set.  A host built against an older header that fills a stack descriptor field by
                                         field passes whatever the stack held: a non-zero value is CTRLV_E_BAD_ARG on
                                         launches that worked before, and the value 1 on a stride-2 conv selects THIS
                                         convolution.  Such a host has to be changed to clear the descriptor; the
                                         library's own callers and the documented bindings always did */
  void* raw_out;                      /* GEGLU only, optional (training forward): the projection BEFORE the gate,
                                         [M, ld_raw] bf16 in the packed (16 value | 16 gate) column-block order -- what
                                         ctrlv_geglu_bwd consumes -- written by the same launch (ping-pong tiles) */
  int32_t n_scale2;                   /* output columns [0, n_scale2) take s_acc2 in place of s_acc (multiple of 32; 0 = */
  float s_acc2;                       /* none).  The fused q|k|v projection scales its q block by (1/sqrt(64)) log2(e)
                                         here, in fp32 before the one bf16 rounding: ctrlv_attention_spatial_prescaled */
  float* gn_partials;                 /* optional: GroupNorm(32) chunk partials of `out`, written by the same launch --
                                         [M / 64][32 groups][mean, M2] fp32 over 64-row chunks (what the statistics pass
                                         of ctrlv_groupnorm would compute by re-reading `out`); consumed by
                                         ctrlv_groupnorm_from_partials.  Only where ctrlv_gemm_gn_partials_serves(d) */
  void* splitk_ws;                    /* optional scratch of ctrlv_gemm_splitk_ws_bytes(d) bytes: lets ctrlv_gemm split the
                                         contraction of a small-image, long-K conv into K slices (one launch for all
                                         slices + a streaming sum / epilogue kernel).  NULL = never split */
  int32_t ksplit, w_cin;              /* internal (set by ctrlv_gemm for its slice launch; callers leave 0): number of K
                                         slices; channels per tap of W when Cin is a slice's channel count */
  /* SPLIT ("fp16x2") residual trunk -- libctrlv_hip_f16.so only (round 5).  A tensor of the residual stream may carry a
   * second plane of the same shape and pitch IN ELEMENTS: hi = rne_fp16(v), lo = rne_e5m2(v - hi) -- ABI 20: the lo plane
   * holds ONE BYTE per element (e5m2 / "bf8": fp16's sign and exponent, two mantissa bits; row pitch in bytes = the hi
   * plane's pitch in elements), hi + lo keeps ~15 significant bits in 3 bytes per element (ABI 18-19: a 16-bit lo plane; on
   * the oracle both give the same model-level error, tests/trunk_precision_study.py).  R1_lo / R2_lo (optional, need R1 /
   * R2): the operand is R1 + R1_lo (R2 + R2_lo); out_lo (optional): `out` receives hi, out_lo receives lo.  MFMA operands
   * (A, A2) always read the hi plane: it is the element-rounded tensor.  Not with GEGLU / SiLU / fp32 output / raw_out. */
  const void* R1_lo;
  const void* R2_lo;
  void* out_lo;
} ctrlv_gemm_desc;

int ctrlv_gemm(const ctrlv_gemm_desc* d, ctrlv_stream_t stream);
/* Bytes of splitk_ws a launch of `d` wants (0: the launch is not split).  A function of the layer's shape -- pixels per
 * image, N, Cin, taps -- and of M only through the size of the scratch: a clip is computed with the same summation order
 * alone and in a batch.  A caller that passes the scratch for one batch size must pass it for every batch size. */
size_t ctrlv_gemm_splitk_ws_bytes(const ctrlv_gemm_desc* d);
/* 1 if a launch of `d` can write gn_partials: a 3x3 conv (row-halo eligible geometry) or a temporal conv with a {V} or
 * {R1} epilogue (ResnetBlock2D.conv1 / conv2, TemporalResnetBlock.conv1 / conv2: the producers of norm2, temporal norm1,
 * temporal norm2 and -- conv2 with the AlphaBlender epilogue -- of the GroupNorm that opens the transformer behind the
 * block), N = 320 / 640 / 1280, image size a multiple of 64 pixels.  Depends on the layer's shape only, never on the
 * batch size. */
int ctrlv_gemm_gn_partials_serves(const ctrlv_gemm_desc* d);
/* 1 if ctrlv_gemm serves this nearest-x2 upsampler conv (mode 1, taps 9, stride 1, up = 1 or 2, Ho = 2 H, Wo = 2 Wd) in phase
 * form (ctrlv_gemm_desc.up = 2): Wd a power of two <= 256, Cin a multiple of 64, bias-only epilogue, 8-element pitches; out_lo
 * only in the fp16 library with N a multiple of 320.  Depends on the layer's shape only, never on the image count. */
int ctrlv_gemm_up_phase_serves(const ctrlv_gemm_desc* d);
/* Phase weights of such a conv from its parameter w [N][Cin][3][3] (device; dtype 0 fp32 / 1 fp16 / 2 bf16): dst[p][n][(2 a +
 * b) Cin + c] = sum of w[n][c][ky][kx] over ky in KY(py, a), kx in KY(px, b), p = 2 py + px, where KY(0, 0) = {0}, KY(0, 1) =
 * {1, 2}, KY(1, 0) = {0, 1}, KY(1, 1) = {2}; summed in fp32 (ky outer, kx inner), rounded once to the element type.  dst: 16 N
 * Cin elements. */
int ctrlv_pack_up_phase_weight(const void* w, int dtype, int N, int Cin, void* dst, ctrlv_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * GroupNorm(32) (+SiLU), channels-last.  Replaces nn.GroupNorm + SiLU of ResnetBlock2D.norm1/norm2,
 * TemporalResnetBlock.norm1/norm2 (5-D: statistics over (C/32, F, H, W)), TransformerSpatioTemporalModel.norm and
 * conv_norm_out (unet_spatio_temporal_condition.py:161-162).
 *   x  : [n_img*S, C] bf16, optionally the channel-concat of (x [.., c_split], x2 [.., C-c_split]) (torch.cat dim=1)
 *   statistics are taken per (img / imgs_per_stat, group): imgs_per_stat = 1 (4-D) or F (5-D)
 *   stats pass writes per-chunk fp32 (mean, M2 = sum (x - mean)^2) per group (accumulated about per-channel pilot
 *   values, so |mean| >> std does not cancel), then combines them in fp64 into (mean, rstd) per (statistics row, group),
 *   stored behind the chunk partials; the apply pass streams y = [silu](x * a_c + b_c).
 * `partials` must hold (n_img * n_chunks + n_img / imgs_per_stat) * 64 floats, n_chunks = ctrlv_groupnorm_chunks().
 * ------------------------------------------------------------------------------------------------------------------ */
int ctrlv_groupnorm_chunks(int n_img, int S, int C, int imgs_per_stat);
int ctrlv_groupnorm_stats(const void* x, const void* x2, int c_split, int n_img, int S, int C, int imgs_per_stat,
                          float eps, float* partials, ctrlv_stream_t stream);
int ctrlv_groupnorm_apply(const void* x, const void* x2, int c_split, int n_img, int S, int C, int imgs_per_stat,
                          const float* partials, const float* gamma, const float* beta, int silu, void* y,
                          ctrlv_stream_t stream);
/* GroupNorm(+SiLU) of a tensor whose producer wrote the chunk partials (ctrlv_gemm_desc.gn_partials): combines them
 * into (mean, rstd) and streams y -- 1 read + 1 write of the tensor.  `partials` holds (n_img * S / 64 + n_img /
 * imgs_per_stat) * 64 floats (the producer's part first); S must be a multiple of 64. */
int ctrlv_groupnorm_from_partials(const void* x, int n_img, int S, int C, int imgs_per_stat, float eps, float* partials,
                                  const float* gamma, const float* beta, int silu, void* y, ctrlv_stream_t stream);
/* The same on a SPLIT tensor (ABI 18): x_lo = the lo plane the producing launch wrote beside `x` (ctrlv_gemm_desc.out_lo together
 * with gn_partials: the {R1} row-halo 3x3 and temporal convs, ctrlv_gemm_gn_partials_serves); NULL = plain. */
int ctrlv_groupnorm_from_partials_split(const void* x, const void* x_lo, int n_img, int S, int C, int imgs_per_stat, float eps,
                                        float* partials, const float* gamma, const float* beta, int silu, void* y,
                                        ctrlv_stream_t stream);
/* The finalize step of ctrlv_groupnorm_from_partials alone: the producer's 64-row chunk partials -> (mean, rstd) per
 * (statistics row, group) behind them, at partials + n_img * (S / 64) * 64 (what ctrlv_spatial_entry_fused reads as `stats`). */
int ctrlv_groupnorm_finalize(int n_img, int S, int C, int imgs_per_stat, float eps, float* partials, ctrlv_stream_t stream);
/* The statistics and apply passes on a SPLIT input (ctrlv_gemm_desc.out_lo): x_lo / x2_lo are the lo planes of x / x2 (same shapes and
 * pitches; either may be NULL = that half has no lo plane); the normalised value is x + x_lo.  y is a plain tensor. */
int ctrlv_groupnorm_stats_split(const void* x, const void* x_lo, const void* x2, const void* x2_lo, int c_split, int n_img,
                                int S, int C, int imgs_per_stat, float eps, float* partials, ctrlv_stream_t stream);
int ctrlv_groupnorm_apply_split(const void* x, const void* x_lo, const void* x2, const void* x2_lo, int c_split, int n_img,
                                int S, int C, int imgs_per_stat, const float* partials, const float* gamma,
                                const float* beta, int silu, void* y, ctrlv_stream_t stream);

/* LayerNorm over the channel axis of [M, C] bf16 rows (BasicTransformerBlock.norm1/3,
 * TemporalBasicTransformerBlock.norm_in/1/3).  If V != NULL, normalises x[m,:] + V[(m / vdiv) % vmod, :]
 * (the frame positional embedding add of TransformerSpatioTemporalModel). */
int ctrlv_layernorm(const void* x, int M, int C, const float* gamma, const float* beta, float eps,
                    const float* V, int vdiv, int vmod, int ldv, void* y, ctrlv_stream_t stream);
/* ... of a SPLIT input: normalises x + x_lo (+ V) (x_lo: the lo plane of x, ctrlv_gemm_desc.out_lo). */
int ctrlv_layernorm_split(const void* x, const void* x_lo, int M, int C, const float* gamma, const float* beta, float eps,
                          const float* V, int vdiv, int vmod, int ldv, void* y, ctrlv_stream_t stream);

/* Fused feed-forward pair at C = 320:  out = epilogue( GEGLU(x . W1^T + b1) . W2^T )  with the second projection's
 * epilogue operands taken from `out_desc` (out, bias = b2, R1 / R2 / V, s_acc, s1, s2, M, N = 320, Cin = 1280, mode 0):
 * the two ctrlv_gemm launches of BasicTransformerBlock.ff / TemporalBasicTransformerBlock.ff_in / .ff [DIFF-0.27.2
 * attention.py FeedForward(GEGLU)] without the 4C-wide intermediate in HBM.  x: bf16 [M][ldx]; w1f / w2f: the
 * fragment-major forms written by ctrlv_ff_fused_pack from the packed weights ([2560][320] in the GEGLU-interleaved row
 * order, [320][1280]) and b1 (fp32 [2560], the same row order; it travels inside w1f as a 21st K step).  w1f holds
 * ctrlv_ff_fused_w1f_bytes() bytes, w2f 320 * 1280 * 2.  Results: the arithmetic of the two launches up to the
 * summation order of the second projection and 2^-17 |b1| (csrc/ff_fused.hip). */
int ctrlv_ff_fused_w1f_bytes(void);
int ctrlv_ff_fused_pack(const void* w1_packed, const float* b1, const void* w2_packed, void* w1f, void* w2f,
                        ctrlv_stream_t stream);
int ctrlv_ff_fused(const void* x, int ldx, const void* w1f, const void* w2f, const ctrlv_gemm_desc* out_desc,
                   ctrlv_stream_t stream);
/* The same with the LayerNorm in front of the feed-forward folded in (norm3 / norm_in of the transformer blocks):
 * the kernel's input rows are x' = LayerNorm(x + ln_V[(m / ln_vdiv) % ln_vmod]) * gamma + beta, rounded to bf16 like
 * ctrlv_layernorm's output (ln_V may be null; ln_gamma = null: no LayerNorm, = ctrlv_ff_fused). */
int ctrlv_ff_fused_ln(const void* x, int ldx, const float* ln_gamma, const float* ln_beta, float ln_eps,
                      const float* ln_V, int ln_vdiv, int ln_vmod, int ln_ldv, const void* w1f, const void* w2f,
                      const ctrlv_gemm_desc* out_desc, ctrlv_stream_t stream);
/* 1 if ctrlv_ff_fused serves this second-projection descriptor with input rows of pitch ldx -- N = 320, Cin = 1280,
 * n_store 320, every operand within 32-bit byte offsets, pitches multiples of 8; epilogue bias, +R1 or +R1+R2; a row-vector
 * operand (vmode 1 / 2) with bias or +R1, and with +R1+R2 only in the per-tile form (vmode 1, vdiv a multiple of 256,
 * s_acc == 1) -- 0 = use the two ctrlv_gemm launches.  The launcher applies exactly these conditions. */
int ctrlv_ff_fused_serves(const ctrlv_gemm_desc* out_desc, int ldx);

/* ------------------------------------------------------------------------------------------------------------------
 * FP8 linear GEMM (opt-in throughput mode of the feed-forwards; csrc/quant_f8.hip, csrc/gemm_f8.hip).  Additive entry
 * points: the ABI number does not change.  Codes are OCP e4m3 ("e4m3fn", torch.float8_e4m3fn: largest finite value 448),
 * round-to-nearest-even, saturating; the NaN codes 0x7f / 0xff are never produced from finite input.
 *
 * ctrlv_quant_rows_f8: one pass over [M, K] element rows (pitch ldx elements).  y = x, or with gamma != NULL (beta too)
 * y = ctrlv_layernorm's value LayerNorm(x + V[(m / vdiv) % vmod]) * gamma + beta kept in fp32 (V optional; V needs gamma).
 * a = max |y[m, :]|;  scale[m] = a / 448 (a == 0: 1; never below the smallest normal fp32);  q[m, k] = e4m3(y[m, k] /
 * scale[m]), bytes with pitch ldq.  K a multiple of 8, <= 5120; ldx, ldq multiples of 8.  Weights W[N][K] are quantised by
 * the same call (one scale per output channel; GEGLU-interleaved rows keep their order).
 *
 * ctrlv_gemm_f8: out = epilogue(a_scale[m] w_scale[n] sum_k A[m, k] W[n, k] + bias[n]) with A, W holding e4m3 bytes (lda and
 * the weight pitch Cin in bytes), fp32 accumulation on v_mfma_scale_f32_32x32x64_f8f6f4 with unit block scales, and the
 * mode-0 epilogue of ctrlv_gemm behind it: v = s_acc (..) + s1 R1 + s2 R2 + V[vidx(m)], or GEGLU, n_store, out_f32.
 * ctrlv_gemm_f8_serves (host only) says whether a descriptor is served: mode 0, taps 1, A2 == NULL, no lo planes, no raw_out /
 * gn_partials / n_scale2 / act / pad_br, tile 0 (chosen by the launch's size: both tiles give the same bits) or 1 / 2, Cin a multiple of 128 (so not 320: that feed-forward stays on ctrlv_ff_fused),
 * N a multiple of 32, lda a multiple of 16 and >= Cin, ldo / n_store / ldr1 / ldr2 / ldv multiples of 4, out_f32 0 or 1, GEGLU
 * with bias only, operands aligned (A, W, bias, V 16 bytes; R1, R2, out 8 bytes; out 16 with out_f32).  An unserved
 * descriptor is CTRLV_E_BAD_SHAPE, a null operand or scale vector CTRLV_E_BAD_ARG, both before any HIP call.  A function of
 * the layer's shape only: a row's bits do not depend on M.
 * ------------------------------------------------------------------------------------------------------------------ */
int ctrlv_quant_rows_f8(const void* x, int M, int K, int ldx, const float* gamma, const float* beta, float eps,
                        const float* V, int vdiv, int vmod, int ldv, void* q, int ldq, float* scale, ctrlv_stream_t stream);
int ctrlv_gemm_f8(const ctrlv_gemm_desc* d, const float* a_scale, const float* w_scale, ctrlv_stream_t stream);
int ctrlv_gemm_f8_serves(const ctrlv_gemm_desc* d);

/* Fused temporal self-attention block at C = 320 (ABI 18; csrc/temporal_fused.hip):
 *     out = R1 + to_out( softmax_f( q k^T / 8 ) v ) + bias + V[clip],     (q | k | v) = x . W_qkv^T
 * over the F <= 32 frames of every pixel -- `TemporalBasicTransformerBlock.attn1` with its residual and the one-key
 * cross-attention vector [DIFF-0.27.2; instantiated by get_down_block / UNetMidBlockSpatioTemporal,
 * src/ctrlv/models/controlnet.py:157-170,186-192] in ONE launch instead of ctrlv_gemm (q|k|v) + ctrlv_attention_temporal +
 * ctrlv_gemm (to_out) [+ ctrlv_layernorm with ln_gamma]: neither the 3C-wide q|k|v tensor nor the attention output (nor the
 * normalised rows) reaches HBM.  x = LayerNorm(R1) rows -- or, with ln_gamma / ln_beta, the raw rows (= R1) --
 * [B F S][ldx] ordered (b, f, s); wf = ctrlv_temporal_fused_weight_bytes() bytes written by ctrlv_temporal_fused_pack from the
 * packed [3C][ld_qkv] q|k|v weight and the packed [C][ld_o] output projection; bias fp32 [C] or NULL; V: row-vector table
 * as in ctrlv_gemm_desc (vmode 1: vdiv = F S -- one row per clip; vmode 2: also vS = S); R1_lo / out_lo: SPLIT trunk planes
 * (fp16 element library).  Results: the arithmetic of the three launches up to summation orders (same rounding points:
 * q, k, v, P and the attention output are rounded to the element type). */
typedef struct ctrlv_temporal_fused_desc {
  const void* x; int32_t ldx;
  const void* wf;
  const float* bias;
  const void* R1; const void* R1_lo; int32_t ldr1;
  const float* V; int32_t vmode, vdiv, vmod, vS, ldv;
  void* out; void* out_lo; int32_t ldo;
  int32_t B, F, S, C;
  const float* ln_gamma; const float* ln_beta; float ln_eps;   /* optional: x holds the RAW rows and the kernel normalises them
                                                                  first (LayerNorm over C, ctrlv_layernorm's arithmetic and
                                                                  rounding; with a split trunk x is the hi plane: the branch
                                                                  input is the element-rounded value, the residual operand
                                                                  R1 + R1_lo stays exact).  NULL: x is used as it is */
} ctrlv_temporal_fused_desc;
size_t ctrlv_temporal_fused_weight_bytes(void);
int ctrlv_temporal_fused_pack(const void* wqkv_packed, int ld_qkv, const void* wo_packed, int ld_o, void* wf,
                              ctrlv_stream_t stream);
int ctrlv_temporal_fused(const ctrlv_temporal_fused_desc* d, ctrlv_stream_t stream);
/* 1 if ctrlv_temporal_fused serves this descriptor (C = 320, F <= 32, pitches multiples of 8, 32-bit byte offsets, a per-clip
 * row vector) -- 0 = use the three launches.  The launcher applies exactly these conditions. */
int ctrlv_temporal_fused_serves(const ctrlv_temporal_fused_desc* d);

/* Fused entry of the spatial transformer block at C = 320 (additive entry points; csrc/spatial_entry_fused.hip):
 *     h0 = el( el(GroupNorm(x)) . W_in^T + bias_in ),     q|k|v = el( el(LayerNorm(h0)) . W_qkv^T + bias_qkv ),  q block x q_scale
 * -- the GroupNorm apply pass, proj_in, norm1 and the q|k|v projection of TransformerSpatioTemporalModel's opening in ONE
 * launch instead of ctrlv_groupnorm_apply + ctrlv_gemm + ctrlv_layernorm + ctrlv_gemm (n_scale2 = C): the normalised rows never
 * reach HBM.  x: raw rows [n_img S][ldx]; stats: the finalized (mean, rstd) per (image, group), fp32 [n_img][32][2], as
 * ctrlv_groupnorm_stats leaves it behind its chunk partials (ctrlv_groupnorm_finalize for a producer's partials); wf =
 * ctrlv_spatial_entry_fused_weight_bytes() bytes written by ctrlv_spatial_entry_fused_pack from the packed [C][ld_in] proj_in
 * weight and the packed [3C][ld_qkv] q|k|v weight; bias_in fp32 [C] / bias_qkv fp32 [3C] or NULL.  h0: [M][ldh], qkv: [M][ldq].
 * Results: the arithmetic and rounding points of the four launches (the normalised rows, h0 and q|k|v are rounded to the
 * element type) up to the summation order of the LayerNorm statistics and of the q|k|v contraction. */
typedef struct ctrlv_spatial_entry_desc {
  const void* x; const void* x_lo; int32_t ldx;     /* x_lo / h0_lo: split trunk planes -- NOT served (the predicate says so) */
  const void* wf;
  const float* bias_in; const float* bias_qkv;
  const float* stats;
  const float* gn_gamma; const float* gn_beta;
  const float* ln_gamma; const float* ln_beta; float ln_eps;
  void* h0; void* h0_lo; int32_t ldh;
  void* qkv; int32_t ldq;
  int32_t n_img, S, C, head_dim;
  float q_scale;
} ctrlv_spatial_entry_desc;
size_t ctrlv_spatial_entry_fused_weight_bytes(void);
int ctrlv_spatial_entry_fused_pack(const void* win_packed, int ld_in, const void* wqkv_packed, int ld_qkv, void* wf,
                                   ctrlv_stream_t stream);
int ctrlv_spatial_entry_fused(const ctrlv_spatial_entry_desc* d, ctrlv_stream_t stream);
/* 1 if ctrlv_spatial_entry_fused serves this descriptor (C = 320, head_dim 64, S a multiple of 32, no split planes, pitches
 * multiples of 8, 31-bit byte offsets) -- 0 = use the four launches.  Shape and operands only; the launcher applies exactly these. */
int ctrlv_spatial_entry_fused_serves(const ctrlv_spatial_entry_desc* d);

/* Row softmax of fp32 scores into bf16 probabilities: probs[r, :cols] = softmax(scores[r, :cols]) (cols a multiple of 4,
 * <= 16384).  The VAE mid block's single-head attention (head dim 512; AutoencoderKLTemporalDecoder, called by
 * pipeline_video_control.py:235,278,346) runs as scores GEMM -> this -> P.V GEMM. */
int ctrlv_softmax_rows(const float* scores, int rows, int cols, long ld_scores, void* probs, long ld_probs,
                       ctrlv_stream_t stream);
/* Backward of ctrlv_softmax_rows for one frame's tile (ABI 22; the VAE decoder fine-tuning of
 * tools/train_vae_finetuning.py:303-320 -- the mid block's attention core trains through GEMMs around this kernel):
 * dscores[r, :cols] = scale * probs[r, :] o (dprobs[r, :] - sum_c probs[r, c] * dprobs[r, c]).  probs: the element-type P the
 * forward wrote; dprobs: fp32 (dO . V^T from a GEMM with fp32 output); scale: the factor the scores GEMM folded in
 * (1 / sqrt(C)), so dscores is the gradient of the unscaled q k^T, in the element type.  The row sum is fp32, one
 * workgroup per row; cols as in the forward (a multiple of 4, <= 16384), pitches multiples of 4.  No atomics. */
int ctrlv_softmax_rows_bwd(const void* probs, long ld_probs, const float* dprobs, long ld_dprobs, int rows, int cols,
                           float scale, void* dscores, long ld_dscores, ctrlv_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Self-attention cores (diffusers AttnProcessor2_0 = F.scaled_dot_product_attention, head_dim 64, no mask).
 * qkv: [rows, 3*C] bf16 with q | k | v column blocks (fused to_q/to_k/to_v output), heads = C/64; out: [rows, C].
 *   spatial : rows = n_img*S, attention over the S tokens of each image (BasicTransformerBlock.attn1)
 *   temporal: rows = B*F*S ordered (b, f, s); attention over the F frames of each (b, s) -- the
 *             (b f) s c <-> (b s) f c permutes of TemporalBasicTransformerBlock are index math, F <= 32.
 * ------------------------------------------------------------------------------------------------------------------ */
int ctrlv_attention_spatial(const void* qkv, void* out, int n_img, int S, int C, ctrlv_stream_t stream);
/* The same core for q columns that are ALREADY scaled by (1/sqrt(64)) * log2(e) = 0.18033688 (ctrlv_gemm_desc.n_scale2 /
 * s_acc2 on the q|k|v projection): softmax_2(q' k^T) v.  The scaled scores then come out of the K.Q^T MFMAs and the
 * running max is subtracted through their C operand -- no per-score multiply-add on the vector ALU (the inference
 * plans use this entry; training keeps the unscaled form and its LSE convention). */
int ctrlv_attention_spatial_prescaled(const void* qkv, void* out, int n_img, int S, int C, ctrlv_stream_t stream);
int ctrlv_attention_temporal(const void* qkv, void* out, int B, int F, int S, int C, ctrlv_stream_t stream);
/* Training forward of the spatial core: additionally writes L = m + log2(l) of every softmax row (log2 domain of the
 * scaled scores), lse [n_img][C/64][S] fp32 (NULL = ctrlv_attention_spatial). */
int ctrlv_attention_spatial_lse(const void* qkv, void* out, float* lse, int n_img, int S, int C, ctrlv_stream_t stream);
/* Backward of the two cores (torch autograd of F.scaled_dot_product_attention, cfg5 training step,
 * tools/train_video_controlnet.py:451-488).  dout [rows, C] bf16 -> dqkv [rows, 3C] bf16 (dq | dk | dv, every column
 * written).  spatial: lse from ctrlv_attention_spatial_lse, delta = ctrlv_attention_bwd_scratch_floats() floats of
 * scratch (receives rowsum(dO * O)).  Deterministic (no atomics). */
size_t ctrlv_attention_bwd_scratch_floats(int n_img, int S, int C);
int ctrlv_attention_spatial_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv,
                                float* delta, int n_img, int S, int C, ctrlv_stream_t stream);
int ctrlv_attention_temporal_bwd(const void* qkv, const void* out, const void* dout, void* dqkv, int B, int F, int S, int C,
                                 ctrlv_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * CLIP vision tower (csrc/clip.hip): transformers' CLIPVisionModelWithProjection -- the `image_encoder(pixel_values)
 * .image_embeds` of pipeline_video_control.py:220 and src/ctrlv/utils/util.py:97-125 (ViT-H/14: 257 tokens, 16 heads of 80).
 * Projections, MLP and patch embedding run on ctrlv_gemm, the norms on ctrlv_layernorm; these four are the rest.
 * ------------------------------------------------------------------------------------------------------------------ */
/* Self-attention over the S tokens of each image for ANY 1 <= S <= 4096: qkv [n_img*S, 3C] with q | k | v column blocks (as
 * ctrlv_attention_spatial), heads = C / head_dim, head_dim a multiple of 16 in [16, 128]; out [n_img*S, C].  softmax(q k^T
 * head_dim^-0.5) v with the scale applied in fp32, scores and P.V on MFMA with fp32 accumulation, fp32 softmax; the key tail of
 * the last tile is masked in the kernel, no S x S tensor reaches memory, no atomics.  An image's result does not depend on
 * n_img.  qkv / out 16-byte aligned. */
int ctrlv_attention_tokens(const void* qkv, void* out, int n_img, int S, int C, int head_dim, ctrlv_stream_t stream);
/* NCHW pixels (n, 3, Hpx, Wpx), dtype_code 0 fp32 / 1 fp16 / 2 bf16 -> element rows [n*P, ld], P = (Hpx/patch) (Wpx/patch), one
 * row per patch in row-major patch order, columns in (c, dy, dx) order (= patch_embedding.weight.flatten(1)); columns
 * [3 patch^2, ld) are written as zeros (the GEMM wants Cin % 64 == 0: 588 -> 640).  ld a multiple of 8. */
int ctrlv_clip_patch_rows(const void* pixels, int dtype_code, int n, int Hpx, int Wpx, int patch, void* rows, int ld,
                          ctrlv_stream_t stream);
/* Token rows out [n*(P+1), C]: row 0 of an image = class_emb + pos_emb[0], row p + 1 = patch_out[p] + pos_emb[p + 1]; patch_out
 * [n*P, C] elements, class_emb fp32 [C], pos_emb fp32 [P+1, C]; the sum in fp32, one rounding.  C a multiple of 8. */
int ctrlv_clip_tokens(const void* patch_out, const float* class_emb, const float* pos_emb, int n, int P, int C, void* out,
                      ctrlv_stream_t stream);
/* In place on element rows x [M, ld] (first N columns; N, ld multiples of 8): kind 0 = GELU in the erf form
 * 0.5 x (1 + erf(x / sqrt 2)), kind 1 = quick-GELU x sigmoid(1.702 x); fp32 arithmetic, one rounding. */
int ctrlv_act_rows(void* x, int M, int N, int ld, int kind, ctrlv_stream_t stream);

/* GEMM for a few hundred rows (csrc/gemm_tokens.hip): the tower's projections at batch 1 -- 257 token rows against 1280 -> 3840,
 * 1280 -> 1280, 1280 -> 5120, 5120 -> 1280 -- are weight streaming, and ctrlv_gemm's 256-row tiles put 8-40 workgroups on 256 CUs.
 *     out[m, n] = act( sum_k A[m, k] W[n, k] + bias[n] ) + R1[m, n]
 * A, R1, out: element rows (lda / ldr1 / ldo multiples of 8, 16-byte aligned bases); W: elements [N][K], K contiguous -- what
 * packing.pack_linear / pack_qkv and ctrlv_pack_weight produce; bias fp32 [N] (16-byte aligned) or NULL; R1 optional.
 * act: 0 none, 1 erf-GELU, 2 quick-GELU -- ctrlv_act_rows' formulas (erff, not the GEGLU polynomial) in fp32 on accumulator +
 * bias; the output is rounded ONCE (fc1 + ctrlv_act_rows as one launch).  K % 64 == 0, N % 32 == 0, any M >= 1.  fp32 accumulation
 * on MFMA; rows >= M and columns >= N are never written.
 * DECOMPOSITION: a workgroup owns a column tile of bn weight rows for a block of 288 activation rows and one of `slices` K
 * slices; (bn, slices) are a function of (N, K) only (ctrlv_gemm_tokens_plan) -- never of M, the device or the environment: a
 * row has the same bits alone and in any batch.  With slices > 1 the fp32 partial sums go to `workspace`
 * (ctrlv_gemm_tokens_ws_bytes(M, N, K) bytes, 16-byte aligned; 0 when slices == 1) and are combined INSIDE the launch by the
 * workgroup of each tile that arrives last (agent-scope release / counter / acquire, slabs read past the L1): summed in
 * slice-index order, no float atomics, no second launch, no waiting.  The workspace starts with one counter word per tile;
 * the call clears them on the stream (a captured memset node) unless ws_zeroed, and leaves them zero. */
typedef struct ctrlv_gemm_tokens_desc {
  const void* A;            /* elements [M][lda] */
  const void* W;            /* elements [N][K] */
  const float* bias;        /* fp32 [N] or NULL */
  const void* R1;           /* elements [M][ldr1] or NULL */
  void* out;                /* elements [M][ldo] */
  void* workspace;          /* ctrlv_gemm_tokens_ws_bytes(M, N, K) bytes; may be NULL when that is 0 */
  size_t workspace_bytes;
  int32_t M, N, K;
  int32_t lda, ldr1, ldo;
  int32_t act;              /* 0 none, 1 erf-GELU, 2 quick-GELU */
  int32_t ws_zeroed;        /* 1: the caller vouches that the workspace's counter words are zero (they are after every call):
                               no memset is enqueued.  Only for a workspace that serves ONE (N, K): the counter block is sized
                               by the shape, and another shape's slabs would overwrite it */
} ctrlv_gemm_tokens_desc;
int ctrlv_gemm_tokens(const ctrlv_gemm_tokens_desc* d, ctrlv_stream_t stream);
/* The launch plan of (N, K): bn = weight rows per column tile (64 or 32), slices = K slices (1 whenever K / 64 < 8). */
int ctrlv_gemm_tokens_plan(int N, int K, int* bn, int* slices);
/* counter words (one per row block x column tile, rounded up to 256 bytes) + slices x row blocks x 288 x N fp32; 0 when the
 * shape is not sliced (or invalid: see ctrlv_last_error). */
size_t ctrlv_gemm_tokens_ws_bytes(int M, int N, int K);

/* ------------------------------------------------------------------------------------------------------------------
 * Element-wise / layout kernels.
 * ------------------------------------------------------------------------------------------------------------------ */
/* NCHW (any of fp32/fp16/bf16: src_dtype 0/1/2) -> channels-last bf16 rows [n_img*HW, ldc], writing channels
 * [c_off, c_off+C) and leaving others untouched (used to build the 8|4|pad conv_in input). */
int ctrlv_nchw_to_rows(const void* src, int src_dtype, int n_img, int C, int HW, void* dst, int ldc, int c_off,
                       ctrlv_stream_t stream);
/* channels-last bf16 rows [n_img*HW, ldc] (first C columns) -> NCHW of dst_dtype (0 fp32, 1 fp16, 2 bf16). */
int ctrlv_rows_to_nchw(const void* src, int ldc, int n_img, int C, int HW, void* dst, int dst_dtype,
                       ctrlv_stream_t stream);
/* The (3, 1, 1) time convolution that ends AutoencoderKLTemporalDecoder.decode (`time_conv_out`, C -> C channels, C <= 4,
 * zero padding over the frames of ONE clip; pipeline_video_control.py:346 calls decode per chunk) fused with the
 * rows -> NCHW conversion: src = conv_out rows [n_frames*HW, ldc] bf16, weight fp32 [C][C][3] (out, in, tap), bias
 * fp32 [C]; dst (n_frames, C, H, W) in dst_dtype. */
int ctrlv_time_conv_rows_to_nchw(const void* src, int ldc, int n_frames, int C, int HW, const float* weight,
                                 const float* bias, void* dst, int dst_dtype, ctrlv_stream_t stream);
/* quant_conv + posterior of AutoencoderKLTemporalDecoder.encode (`moments = quant_conv(encoder(x))`,
 * `DiagonalGaussianDistribution(moments).mode() / .sample()`) on the rows the encoder's conv_out GEMM wrote.
 *   rows         [n_img * HW, ld >= 2 L] in the element type: the moments BEFORE quant_conv (L = latent_channels <= 8)
 *   quant_weight [2 L, 2 L] fp32, quant_bias [2 L] fp32 (quant_conv.weight / .bias)
 *   moments_out  (n_img, 2 L, H, W) NCHW, dtype code out_dtype, or NULL: quant_conv(rows), computed in fp32, rounded once
 *   latents_out  (n_img, L, H, W) NCHW, same dtype, or NULL: scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise);
 *                noise (n_img, L, H, W) fp32 from the caller, or NULL for mode() -- the library draws no random numbers
 * At least one output.  One thread per (image, pixel), no atomics, a fixed channel order: the same bits in every run. */
int ctrlv_vae_posterior(const void* rows, int ld, int n_img, int L, int HW, const float* quant_weight, const float* quant_bias,
                        const float* noise, float scale, void* moments_out, void* latents_out, int out_dtype,
                        ctrlv_stream_t stream);
/* Backward of ctrlv_time_conv_rows_to_nchw (ABI 22; the last op of the decoder in tools/train_vae_finetuning.py:303-320).
 * dout: fp32 (n_frames, C, H, W) gradient of the forward's output; src / ldc_src / weight: the forward's operands.  The
 * n_frames frames are whole clips of clip_frames (one forward call each): taps never cross a clip, exactly the forward's
 * zero padding -- with clip_frames = 1 the outer taps of dweight are exactly zero.  Writes drows [n_frames*HW, ldc] in the
 * element type (EVERY one of the ldc columns: the padding columns >= C are zero; C <= ldc <= 64), dweight fp32 [C][C][3]
 * and dbias fp32 [C].  The parameter sums are per-block partials in `scratch` (CTRLV_TIME_CONV_BWD_SCRATCH_FLOATS fp32)
 * added in block order: no atomics, the same bits in every run. */
#define CTRLV_TIME_CONV_BWD_SCRATCH_FLOATS 16384
int ctrlv_time_conv_rows_to_nchw_bwd(const float* dout, const void* src, int ldc_src, int n_frames, int clip_frames, int C,
                                     int HW, const float* weight, void* drows, int ldc, float* dweight, float* dbias,
                                     float* scratch, ctrlv_stream_t stream);
/* im2col for the tiny-channel 3x3 input convs (conv_in, control_conv_in): rows [n_img*H*W, Cp] -> [.., 9*Cp (+pad to Kp)] */
int ctrlv_im2col3x3(const void* x, int n_img, int H, int W, int Cp, void* col, int Kp, ctrlv_stream_t stream);
/* y = a*x + b*r  (bf16 rows, n elements) -- the ControlNet residual add of
 * unet_spatio_temporal_condition.py:119-127,136-137. */
int ctrlv_axpby(const void* x, const void* r, float a, float b, void* y, size_t n, ctrlv_stream_t stream);
/* (y, y_lo) = split(a * (x + x_lo) + b * r): the same add on a SPLIT skip tensor (x_lo may be NULL; y_lo receives the lo
 * plane of the result; in place allowed). */
int ctrlv_axpby_split(const void* x, const void* x_lo, const void* r, float a, float b, void* y, void* y_lo, size_t n,
                      ctrlv_stream_t stream);
/* Sinusoidal `Timesteps` (flip_sin_to_cos=True, shift 0, max_period 1e4): t[n] -> out[n, dim] = [cos | sin], bf16. */
int ctrlv_timestep_embedding(const float* t, int n, int dim, void* out, ctrlv_stream_t stream);
/* y = silu(x) on bf16 (the SiLU in front of every time_emb_proj). */
int ctrlv_silu(const void* x, void* y, size_t n, ctrlv_stream_t stream);
/* Fused CFG combine + Euler (v-prediction) update of pipeline_video_control.py:327-332:
 *   v = uncond + g[f]*(cond - uncond);  x0 = v*(-sigma/sqrt(sigma^2+1)) + x/(sigma^2+1);  x += (x - x0)/sigma*(sigma_next-sigma)
 * latents fp32 [B, F, CHW]; noise_pred bf16/fp32 [(2)B, F, CHW] (uncond first); also writes the next scaled model
 * input (x_next / sqrt(sigma_next^2+1)) as bf16 into `scaled_next` if not NULL. */
int ctrlv_cfg_euler_step(float* latents, const void* noise_pred, int pred_dtype, int cfg, const float* guidance,
                         int B, int F, int CHW, float sigma, float sigma_next, void* scaled_next,
                         ctrlv_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Backward kernels: first slice of the training step (tools/train_video_controlnet.py:451-488 -- ControlNet dgrad +
 * wgrad, UNet up-path dgrad).  DGRAD of the gather-GEMM family is ctrlv_gemm itself on
 * role-swapped weights (ctrlv_amd/autograd.py); these are the reductions the forward kernels cannot express.
 * ------------------------------------------------------------------------------------------------------------------ */
/* dW[n][tap*Cin + c] += sum_m dY[m][n] * A[src(m, tap)][c]  for the forward GEMM described by `fwd` (A, A2/c_split, M, N,
 * Cin, taps, mode and its geometry are read; W / out / epilogue fields are ignored).  dY: bf16 [M][ldy]; dW: fp32
 * [N][taps*Cin] in the packed (tap-major) K order -- or, with torch_layout = 1, [N][Cin][taps], the layout of the
 * nn.Conv2d / nn.Conv3d / nn.Linear parameter itself -- accumulated with atomics: zero it first.  dbias (fp32 [N], or
 * NULL) += scale * column sums of dY, computed by the workgroups that stream dY anyway; dW is scaled by `scale` too
 * (the forward's s_acc).
 * scratch (ctrlv_gemm_wgrad_scratch_bytes(fwd) bytes, or NULL): with it the launch is DETERMINISTIC -- the row slabs write
 * fp32 partial matrices with plain stores and a second kernel adds them to dW / dbias in slab order (a single writer per
 * element): the same gradient bits in every run.  Without it the slabs add with fp32 atomics (arrival order).
 * torch_layout bit 1 (value 2; with scratch only): ASSIGN -- dW / dbias = scale * sum instead of +=, their previous contents
 * are not read (no zero fill in front of the launch).
 * Kernel choice (a function of the layer's shape; the result layout is the same): the LDS-DMA ring of wgrad_pp.hip serves
 * Linear / 1x1, the stride-1 3x3 conv with or without the fused nearest-x2 upsampling, and the temporal conv, with N and
 * Cin multiples of 64 and M >= 1024; the stride-2 conv, the concat operand (A2) and everything else run on the
 * register-staged kernel of backward.hip. */
size_t ctrlv_gemm_wgrad_scratch_bytes(const ctrlv_gemm_desc* fwd);
int ctrlv_gemm_wgrad(const ctrlv_gemm_desc* fwd, const void* dY, int ldy, float* dW, float* dbias, float scale,
                     int torch_layout, void* scratch, size_t scratch_bytes, ctrlv_stream_t stream);
/* One-kernel packing of a PyTorch-layout parameter (fp32 / fp16 / bf16: src_dtype 0 / 1 / 2; [N][C][taps] contiguous:
 * nn.Linear taps 1, Conv2d 3x3 taps 9, Conv3d (3,1,1) taps 3) into the bf16 GEMM layouts -- what a training step does
 * to every trainable weight every step.  form 0: the forward layout dst[n][tap*C + c] (geglu: rows in the packed
 * (value, gate) block order); form 1: the role-swapped dgrad layout dst[c][(taps-1-tap)*Np + n], Np = ld_dst / taps
 * (columns n >= N zero).  Rows of dst beyond those written (row padding to 32) must be zeroed by the caller. */
int ctrlv_pack_weight(const void* src, int src_dtype, int N, int C, int taps, int form, int geglu, void* dst, int ld_dst,
                      ctrlv_stream_t stream);
/* out[idx(m)][n] += scale * x[m][n] summed over rows; idx = 0 (vmode 0: bias gradient) or (m / vdiv) % vmod (vmode 1: the
 * gradient of a per-clip row-vector operand V).  x bf16 [M][ldx], out fp32 [*][ldo], accumulated -- with atomics, or,
 * given `scratch` (ctrlv_colsum_scratch_floats floats; 0 = this row grouping has no deterministic form), per-block sums
 * added in block order: bit-reproducible. */
size_t ctrlv_colsum_scratch_floats(int M, int N, int vmode, int vdiv);
int ctrlv_colsum(const void* x, int M, int N, int ldx, int vmode, int vdiv, int vmod, float scale, float* out, int ldo,
                 float* scratch, ctrlv_stream_t stream);
/* out[0] += scale * sum_i dy[i] * (p[i] - q[i]) over n bf16 elements: the gradient of a folded AlphaBlender's mixing
 * weight (out = xs + (1 - a) * h  =>  dL/da = -sum dy * (out - xs) / (1 - a)).  scratch: 1024 floats (deterministic: block
 * sums added in order) or NULL (one atomic per block). */
int ctrlv_dot_diff(const void* dy, const void* p, const void* q, size_t n, float scale, float* out, float* scratch,
                   ctrlv_stream_t stream);
/* GroupNorm(32)(+SiLU) backward on channels-last rows.  `fwd_partials` is the buffer ctrlv_groupnorm_stats filled for
 * the same x (its (mean, rstd) table is reused); dx bf16; dgamma / dbeta fp32 [C], ACCUMULATED (ordered two-level sums, no
 * atomics: bit-reproducible); scratch fp32 of ctrlv_groupnorm_bwd_scratch_floats() elements. */
int ctrlv_groupnorm_bwd_scratch_floats(int n_img, int S, int C, int imgs_per_stat);
int ctrlv_groupnorm_bwd(const void* x, const void* dy, int n_img, int S, int C, int imgs_per_stat,
                        const float* fwd_partials, const float* gamma, const float* beta, int silu, void* dx,
                        float* dgamma, float* dbeta, float* scratch, ctrlv_stream_t stream);
/* ... + add (element rows like dy, or NULL): dx = (norm backward) + add in the same pass.  x feeds the norm that opens a
 * residual branch AND the skip connection around it; `add` is the gradient that arrives through the skip (what autograd would
 * otherwise sum in a separate pass over both tensors: 181 such sums per cfg5 step).  ABI 19. */
int ctrlv_groupnorm_bwd_add(const void* x, const void* dy, const void* add, int n_img, int S, int C, int imgs_per_stat,
                            const float* fwd_partials, const float* gamma, const float* beta, int silu, void* dx,
                            float* dgamma, float* dbeta, float* scratch, ctrlv_stream_t stream);

/* LayerNorm backward over [M, C] rows (optionally of x + V[(m / vdiv) % vmod], as the forward): dx bf16; dgamma / dbeta
 * fp32 [C], ACCUMULATED; scratch = ctrlv_layernorm_bwd_scratch_floats(M, C) floats (per-wave column partials, folded by a
 * second kernel).  The gradient of V's rows is ctrlv_colsum(dx, vmode 1). */
size_t ctrlv_layernorm_bwd_scratch_floats(int M, int C);
int ctrlv_layernorm_bwd(const void* x, const void* dy, int M, int C, const float* gamma, float eps, const float* V, int vdiv,
                        int vmod, int ldv, void* dx, float* dgamma, float* dbeta, float* scratch, ctrlv_stream_t stream);
/* ... + add: as ctrlv_groupnorm_bwd_add.  ABI 19. */
int ctrlv_layernorm_bwd_add(const void* x, const void* dy, const void* add, int M, int C, const float* gamma, float eps,
                            const float* V, int vdiv, int vmod, int ldv, void* dx, float* dgamma, float* dbeta, float* scratch,
                            ctrlv_stream_t stream);
/* GEGLU backward.  raw: the projection output [M, 2I] bf16 in the packed (16 value, 16 gate) column-block order, i.e.
 * ctrlv_gemm on the GEGLU-packed weight with geglu = 0; du: [M, I] bf16; draw: [M, 2I] bf16, same layout as raw. */
int ctrlv_geglu_bwd(const void* raw, const void* du, size_t M, int I, void* draw, ctrlv_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * LoRA adapters (ABI 21; csrc/lora.hip): the reference's --enable_lora of the stage-1 UNet step
 * (tools/train_video_diffusion.py:126-136, 205-216: rank-r factors on to_q / to_k / to_v / to_out.0, the UNet frozen).
 * One adapted linear, s = lora_alpha / r:  Y = X . W'^T,  W' = W + s . B . A,  A fp32 [r][Cin], B fp32 [N][r].
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct ctrlv_lora_desc {
  const void* X;      /* [M][ldx] elements: the layer's input rows (16-byte aligned, ldx % 8 == 0) */
  const void* dY;     /* [M][ldy] elements: the gradient of the layer's output (16-byte aligned, ldy % 8 == 0) */
  const float* A;     /* fp32 [g][r][Cin]: the g groups' A factors, contiguous */
  const float* B;     /* fp32 [g][N/g][r] == [N][r]: the g groups' B factors, contiguous */
  float* dA;          /* fp32 [g][r][Cin], WRITTEN (not accumulated) */
  float* dB;          /* fp32 [N][r], WRITTEN */
  int M, Cin, N;      /* N = all g groups' output columns; Cin and N / g multiples of 64, any M >= 1 */
  int g, r;           /* g groups side by side along N (the fused q|k|v projection: 3), rank r % 4 == 0, 4 <= r <= 64,
                         g * r <= 192 */
  int ldx, ldy;
  float scale;        /* s = lora_alpha / r (times the forward's s_acc) */
} ctrlv_lora_desc;
/* The factor gradients without the [N][Cin] weight gradient, for the g groups of one launch (group i owns dY's columns
 * [i N/g, (i+1) N/g) and the factors A_i, B_i):  H_i = X . A_i^T, G_i = dY_i . B_i  ([M][r]),  dA_i = s . G_i^T . X,
 * dB_i = s . dY_i^T . H_i.
 * ROUNDING POINTS (a reference reproduces them): NONE beyond the element rows X and dY themselves.  A, B and the fp32
 * intermediates H and G each enter the matrix pipe as an element pair hi = rne(v), lo = rne(v - hi) (~16 significant bits in
 * bf16; fp16 pairs lose bits for |v| below fp16's normal range) and are multiplied twice: the fp32 reference is
 * dA = s (dY.float() B)^T X.float(), dB = s dY.float()^T (X.float() A^T).  dA and dB are accumulated in fp32, scaled by s last.
 * DETERMINISTIC: row-slab partials (plain stores) added in slab order by a second kernel; the slab partition is a function of
 * (M, Cin, N, g, r) only -- not of the device, its CU count or the environment: the same bits on every MI355X.  No atomics.
 * scratch: ctrlv_lora_grad_scratch_bytes(d) bytes (16-byte aligned; its contents are not kept).  Returns 0 bytes for a
 * descriptor the launch would reject.  Register budget of the csrc/lora.hip kernels: <= 256 VGPRs, no scratch (spill). */
size_t ctrlv_lora_grad_scratch_bytes(const ctrlv_lora_desc* d);
int ctrlv_lora_grad(const ctrlv_lora_desc* d, void* scratch, size_t scratch_bytes, ctrlv_stream_t stream);
/* out = W + scale . B . A in fp32, in the TORCH layout [N][Cin] (ctrlv_pack_weight packs it afterwards); W fp32 / fp16 /
 * bf16 (w_dtype 0 / 1 / 2) [N][Cin]; A fp32 [r][Cin], B fp32 [N][r]; each element is fma(scale, sum_j B[n][j] A[j][c], W)
 * with the r products added in index order.  out may be W itself when W is fp32. */
int ctrlv_lora_merge(const void* W, int w_dtype, const float* A, const float* B, int N, int Cin, int r, float scale,
                     float* out, ctrlv_stream_t stream);

/* ==================================================================================================================
 * Plan-level entry points: one call = one model forward.  (SURVEY.md 8b "what a C-ABI replacement must export".)
 *
 * A plan is the execution plan of ONE model instance -- the reference's `UNetSpatioTemporalConditionModel`
 * (src/ctrlv/models/unet_spatio_temporal_condition.py:13-171) or `ControlNetModel` (src/ctrlv/models/controlnet.py:20-351):
 * its module graph (built from the diffusers-style config), its weights packed once into the kernels' layouts, and the
 * walk over the layer list that issues the kernels above.  A host in any language runs a forward with
 *     ctrlv_plan_create -> ctrlv_plan_load_weights -> ctrlv_plan_workspace_bytes -> ctrlv_{unet,controlnet}_forward.
 * Ownership: packed weights are library-owned device memory (allocated by load_weights, freed by destroy); every
 * input / output / workspace buffer is the caller's; a forward allocates nothing, never synchronises the host and
 * enqueues everything on the caller's stream (HIP-graph capturable).  A plan is re-entrant across plans, not
 * thread-safe on one plan.
 * ================================================================================================================== */
#define CTRLV_MAX_BLOCKS 8
typedef struct ctrlv_model_config {
  int32_t kind;                 /* 0 = UNetSpatioTemporalConditionModel, 1 = ControlNetModel */
  int32_t in_channels;          /* 8 (4 noisy + 4 image latents); ControlNet: control_cond has in_channels / 2 */
  int32_t out_channels;         /* UNet: 4 */
  int32_t n_blocks;             /* len(down_block_types) == len(up_block_types) */
  int32_t block_out_channels[CTRLV_MAX_BLOCKS];
  int32_t down_cross_attn[CTRLV_MAX_BLOCKS]; /* 1: CrossAttnDownBlockSpatioTemporal, 0: DownBlockSpatioTemporal */
  int32_t up_cross_attn[CTRLV_MAX_BLOCKS];   /* 1: CrossAttnUpBlockSpatioTemporal, 0: UpBlockSpatioTemporal (UNet) */
  int32_t layers_per_block[CTRLV_MAX_BLOCKS];
  int32_t num_attention_heads[CTRLV_MAX_BLOCKS];   /* head_dim = channels / heads must be 64 */
  int32_t cross_attention_dim;                     /* 1024 */
  int32_t addition_time_embed_dim;                 /* 256 */
  int32_t projection_class_embeddings_input_dim;   /* 768 */
  int32_t num_frames;                              /* frames the frame-embedding table is prepared for (others work) */
  int32_t time_context_order;   /* 0: "sb" = diffusers 0.27.2 temporal-context ordering quirk, 1: "bs" */
} ctrlv_model_config;

typedef struct ctrlv_tensor_desc {
  const char* name;             /* diffusers state-dict key, e.g. "down_blocks.0.resnets.0.spatial_res_block.conv1.weight" */
  const void* data;             /* contiguous, row-major, in the PyTorch parameter layout */
  int32_t dtype;                /* 0 fp32, 1 fp16, 2 bf16 */
  int32_t on_device;            /* 1: device pointer (of the plan's device), 0: host pointer */
  int64_t numel;
} ctrlv_tensor_desc;

typedef struct ctrlv_plan ctrlv_plan;

int ctrlv_plan_create(const ctrlv_model_config* cfg, int device, ctrlv_plan** out);
/* All parameters of the model by their diffusers key names (extra names are ignored, a missing one is an error).
 * Packs into the kernel layouts: K-contiguous bf16 weights [N32][K64], q|k|v fused, GEGLU rows interleaved in 16-row
 * (value, gate) blocks, every time_emb_proj and every cross-attention to_v concatenated into one GEMM each.
 * May be called again (e.g. after an optimizer step); synchronises the device. */
int ctrlv_plan_load_weights(ctrlv_plan* plan, const ctrlv_tensor_desc* tensors, size_t n);
/* Switch the temporal cross-attention context order of an existing plan (0 "sb" / 1 "bs", see the config). */
int ctrlv_plan_set_time_context_order(ctrlv_plan* plan, int order);
/* Storage of the RESIDUAL TRUNK of the plan's forwards (conv_in output, every block / AlphaBlender output, the skip
 * tensors, the tensors the ControlNet residuals are added into): 0 = one element per value like every other activation
 * (default), 1 = SPLIT into a hi element plane + a one-byte lo plane (see ctrlv_gemm_desc.out_lo: 3 bytes per element, ~15
 * significant bits under fp16 branches; north_star's 1e-3 model-level tolerance).  Mode 1 needs the fp16 element library; the workspace grows
 * (ctrlv_plan_workspace_bytes answers for the current mode).  Model inputs / outputs / residual tensors across the ABI are
 * unchanged. */
int ctrlv_plan_set_trunk_mode(ctrlv_plan* plan, int mode);
/* Precision of the transformer feed-forwards of the plan's forwards: 0 = the element type (default), 1 = e4m3 operands on the
 * block-scaled MFMA (ctrlv_gemm_f8) for every feed-forward whose two projections ctrlv_gemm_f8_serves accepts (K multiples of
 * 128: C = 640 / 1280 of the SVD model; C = 320 keeps ctrlv_ff_fused): LayerNorm + row quantisation in one launch
 * (ctrlv_quant_rows_f8), the GEGLU projection, the row quantisation of its output, the output projection with the layer's
 * epilogue.  A throughput mode with the error class of bf16 storage, opt-in.  The e4m3 weights and their
 * scales are made here (or at the next ctrlv_plan_load_weights) from the packed weights and owned by the plan; the workspace
 * grows (ctrlv_plan_workspace_bytes answers for the current mode).  Does not combine with trunk mode 1: CTRLV_E_BAD_ARG from
 * whichever of the two setters comes second. */
int ctrlv_plan_set_ff_precision(ctrlv_plan* plan, int mode);
/* Bytes of workspace one forward of (B clips, F frames, H x W latent) needs; 0 on error (see ctrlv_last_error). */
size_t ctrlv_plan_workspace_bytes(ctrlv_plan* plan, int B, int F, int H, int W);
/* Number of residual tensors the ControlNet produces / the UNet consumes on the down path (12 for SVD), and the
 * rows / channels of residual i at (B, F, H, W): i in [0, n) = down residuals, i == n = the mid residual. */
int ctrlv_plan_num_down_residuals(ctrlv_plan* plan);
int ctrlv_plan_residual_shape(ctrlv_plan* plan, int i, int B, int F, int H, int W, int64_t* rows, int32_t* channels);

/* UNetSpatioTemporalConditionModel.forward (unet_spatio_temporal_condition.py:31-171).
 *   sample   (B, F, in_channels, H, W) contiguous, dtype 0/1/2       timestep  device fp32 [1] or [B] (n_timestep)
 *   ehs      (B, 1, cross_attention_dim) contiguous, dtype as sample  added_time_ids device fp32 (B, n_ids)
 *   down_res n pointers (or NULL) to channels-last bf16 rows [B*F*h_i*w_i, C_i] -- the layout
 *            ctrlv_controlnet_forward writes; mid_res likewise (both or neither, :61); they are ADDED to the skip
 *            tensors / the mid block output (:119-127,136-137) and not modified.
 *   residual_event: optional hipEvent_t the stream waits on right before it reads the residuals (so a ControlNet
 *            running on another stream overlaps the UNet's down / mid blocks); NULL = none.
 *   out      (B, F, out_channels, H, W) contiguous, dtype as sample. */
int ctrlv_unet_forward(ctrlv_plan* plan, const void* sample, int dtype, const float* timestep, int n_timestep,
                       const void* ehs, const float* added_time_ids, int n_ids, const void* const* down_res,
                       const void* mid_res, void* residual_event, void* out, int B, int F, int H, int W,
                       void* workspace, size_t workspace_bytes, ctrlv_stream_t stream);
/* The down + mid half of the same forward (unet_spatio_temporal_condition.py:64-117,130-135), for the training step of
 * tools/train_video_controlnet.py:451-466: the frozen UNet's encoder has no gradient path (the ControlNet residuals are
 * added to its OUTPUTS, :119-137), so it runs here and hands the n skip tensors and the mid block output back as
 * channels-last bf16 rows (shapes: ctrlv_plan_residual_shape; out_taps[i] / out_mid are caller-owned). */
int ctrlv_unet_encoder_forward(ctrlv_plan* plan, const void* sample, int dtype, const float* timestep, int n_timestep,
                               const void* ehs, const float* added_time_ids, int n_ids, void* const* out_taps,
                               void* out_mid, int B, int F, int H, int W, void* workspace, size_t workspace_bytes,
                               ctrlv_stream_t stream);
/* ControlNetModel.forward (controlnet.py:226-351): control_cond (B, F, in_channels/2, H, W) dtype as sample;
 * writes out_down[i] / out_mid as channels-last bf16 rows (shapes: ctrlv_plan_residual_shape), already multiplied by
 * conditioning_scale (:343-344, folded into the zero-conv epilogue). */
int ctrlv_controlnet_forward(ctrlv_plan* plan, const void* sample, const void* control_cond, int dtype,
                             const float* timestep, int n_timestep, const void* ehs, const float* added_time_ids,
                             int n_ids, float conditioning_scale, void* const* out_down, void* out_mid, int B, int F,
                             int H, int W, void* workspace, size_t workspace_bytes, ctrlv_stream_t stream);
int ctrlv_plan_destroy(ctrlv_plan* plan);

/* Per-launch profile of the plan's OWN launches (measurement aid: bench.py's roofline leg, tools/shape_table.py).  While
 * enabled, every kernel a forward issues is bracketed by HIP events on the launch stream and recorded with its algorithmic
 * FLOPs / bytes (SURVEY.md Appendix B accounting).  Enable OUTSIDE HIP-graph capture and for eager forwards only.
 * ctrlv_plan_profile_read synchronises on the recorded events, writes up to max_records records in launch order, clears
 * the list and returns the number written (max_records == 0: the number pending, nothing cleared); <0 on error. */
enum {
  CTRLV_FAM_GEMM_LINEAR = 0, CTRLV_FAM_GEMM_CONV3X3 = 1, CTRLV_FAM_GEMM_CONV_TEMPORAL = 2, CTRLV_FAM_ATTENTION_SPATIAL = 3,
  CTRLV_FAM_ATTENTION_TEMPORAL = 4, CTRLV_FAM_GROUPNORM = 5, CTRLV_FAM_LAYERNORM = 6, CTRLV_FAM_RESIDUAL_ADD = 7,
  CTRLV_FAM_GEMM_TEMPORAL_BLOCK = 8,    /* ctrlv_temporal_fused: q|k|v projection + attention over the frames + output projection */
  CTRLV_FAM_GEMM_SPATIAL_ENTRY = 9,     /* ctrlv_spatial_entry_fused: GroupNorm apply + proj_in + LayerNorm + q|k|v projection */
};
typedef struct ctrlv_profile_record {
  int32_t family;             /* CTRLV_FAM_* */
  int32_t M, N, K;            /* GEMM: rows, weight rows, taps * Cin; attention: images, tokens, channels; norms: rows, channels */
  int32_t flags;              /* GEMM: bit 0 GEGLU, bits 1-2 residual operands, bits 3-4 vmode, bit 8 fused feed-forward */
  float ms;                   /* elapsed between the launch's two events */
  double flops, bytes;        /* algorithmic work of the launch */
} ctrlv_profile_record;
int ctrlv_plan_profile(ctrlv_plan* plan, int enable);
int ctrlv_plan_profile_read(ctrlv_plan* plan, ctrlv_profile_record* out, int max_records);

/* ==================================================================================================================
 * CLIP vision tower as ONE call (csrc/clip_plan.hip): transformers' CLIPVisionModelWithProjection.forward -- the
 * `image_encoder(pixel_values).image_embeds` of pipeline_video_control.py:220 -- for a host in any language:
 *     ctrlv_clip_plan_create -> ctrlv_clip_plan_load_weights -> ctrlv_clip_plan_workspace_bytes -> ctrlv_clip_forward.
 * Same contract as the plan above: create validates on the host and needs no GPU; packed weights are library-owned; a forward
 * allocates nothing, never synchronises the host and enqueues only on the caller's stream, as ONE chain (HIP-graph capturable,
 * no parallel branch).
 * The walk:  clip_patch_rows -> GEMM -> clip_tokens -> layernorm (pre_layrnorm);  per layer: layernorm -> q|k|v GEMM ->
 * attention_tokens -> out_proj GEMM + residual -> layernorm -> fc1 GEMM with the activation in its epilogue -> fc2 GEMM +
 * residual;  class rows -> layernorm (post_layernorm) -> projection GEMM:  4 + 7 L + 2 kernels (230 for ViT-H), plus one memset
 * node per sliced weight shape (the K-slice counters of ctrlv_gemm_tokens; 2 for ViT-H) and one strided copy node (the class rows).  Which GEMM serves a layer is a
 * table keyed on (N, K) only (csrc/clip_plan.hip): an image has the same bits alone and in any batch.
 * ================================================================================================================== */
typedef struct ctrlv_clip_config {
  int32_t hidden_size, intermediate_size, num_hidden_layers, num_attention_heads;
  int32_t image_size, patch_size, projection_dim;
  int32_t hidden_act;           /* 0 gelu (erf form), 1 quick_gelu */
  float layer_norm_eps;
} ctrlv_clip_config;
typedef struct ctrlv_clip_plan ctrlv_clip_plan;
/* Size rules (clip_vision_hip.supports): hidden and intermediate sizes multiples of 64, hidden <= 2048, projection a multiple
 * of 32, head_dim = hidden / heads a multiple of 16 in [16, 128], image a whole number of patches, at most 4096 tokens. */
int ctrlv_clip_plan_create(const ctrlv_clip_config* cfg, int device, ctrlv_clip_plan** out);
/* transformers' state-dict keys: vision_model.embeddings.{class_embedding, patch_embedding.weight, position_embedding.weight},
 * vision_model.pre_layrnorm.*, vision_model.encoder.layers.N.{layer_norm1, layer_norm2, self_attn.{q,k,v,out}_proj, mlp.fc1,
 * mlp.fc2}.{weight, bias}, vision_model.post_layernorm.*, visual_projection.weight.  Host or device tensors, fp32 or 16-bit;
 * extra names are ignored, a missing one is an error.  q|k|v become one weight.  May be called again; synchronises the device. */
int ctrlv_clip_plan_load_weights(ctrlv_clip_plan* plan, const ctrlv_tensor_desc* tensors, size_t n);
/* Bytes of workspace a forward of n_img images needs; 0 on error ("not loaded" before load_weights: ctrlv_last_error). */
size_t ctrlv_clip_plan_workspace_bytes(ctrlv_clip_plan* plan, int n_img);
/* pixel_values (n_img, 3, image_size, image_size) contiguous, dtype 0 / 1 / 2; image_embeds [n_img, projection_dim] and
 * last_hidden_state [n_img, tokens, hidden_size] (the encoder output before post_layernorm; or NULL) in the element type.
 * workspace 256-byte aligned. */
int ctrlv_clip_forward(ctrlv_clip_plan* plan, const void* pixel_values, int dtype, int n_img, void* image_embeds,
                       void* last_hidden_state, void* workspace, size_t workspace_bytes, ctrlv_stream_t stream);
int ctrlv_clip_plan_destroy(ctrlv_clip_plan* plan);

/* ==================================================================================================================
 * The VAE as ONE call each way (csrc/vae_plan.hip): `vae.encode(x).latent_dist` (the conditioning image and the bbox frames,
 * pipeline_video_control.py:71-101, 235) and `vae.decode(z, num_frames).sample` (:346) of AutoencoderKLTemporalDecoder, for a
 * host in any language:
 *     ctrlv_vae_plan_create -> ctrlv_vae_plan_load_weights -> ctrlv_vae_plan_workspace_bytes -> ctrlv_vae_encode / _decode.
 * With the CLIP plan, the UNet / ControlNet plan and ctrlv_cfg_euler_step, everything a Box2Video clip computes on the GPU is
 * reachable from this header.  Same contract as the plans above: create validates on the host and needs no GPU; packed
 * weights are library-owned; a forward allocates nothing, never synchronises the host and enqueues only on the caller's
 * stream, as ONE chain (HIP-graph capturable; the only non-kernel nodes are the memsets of the zero-padded input channels).
 * The walks are the per-op Python executors' (models/vae_encoder_hip.py with native_down, models/vae_decoder_hip.py), launch
 * for launch and operand for operand:
 *   encode:  nchw_to_rows -> im2col3x3 -> GEMM (conv_in);  per level: res blocks {GroupNorm+SiLU (stats, apply) -> conv1 ->
 *            GroupNorm+SiLU -> [1x1 shortcut] -> conv2 + residual: 6 or 7 kernels}, then the down-sampler as ONE pad_br launch
 *            (3 of the 4 levels);  mid: res, attention, res;  GroupNorm+SiLU -> conv_out -> ctrlv_vae_posterior (quant_conv and
 *            the posterior).  Attention (one head of dim C): GroupNorm -> q, k GEMMs -> per image {scores GEMM (fp32) ->
 *            ctrlv_softmax_rows -> V^T GEMM -> P.V GEMM} -> to_out GEMM + residual: 5 + 4 n kernels.
 *   decode:  per clip of num_frames: conv_in as above;  mid: res, attention, res;  per level: 3 res blocks {the spatial half
 *            as above, per frame range; GroupNorm+SiLU over the clip -> temporal conv1 -> GroupNorm+SiLU -> temporal conv2 with
 *            the AlphaBlender in its epilogue: 12 or 13 kernels}, then the up-sampler conv with the nearest-x2 gather fused
 *            (3 of the 4 levels);  GroupNorm+SiLU -> conv_out -> ctrlv_time_conv_rows_to_nchw.
 *   A conv whose layer shape asks for the K split (ctrlv_gemm_splitk_ws_bytes) runs as two kernels, as in the executors.
 * Two operands are computed at load time: sigmoid(mix_factor) as 1 / (1 + exp(-(double) p)) rounded to float, and the
 * attention's folded output bias b_o + W_o . b_v, in fp64 on the host from the fp32 values, rounded once (the Python
 * executor forms it with a device matvec: the two routes agree bit for bit where to_v.bias is zero, to rounding elsewhere).
 * Element type: the plan runs in the library's element type.  It is exported by libctrlv_hip_f16.so too (same sources) but
 * validated on the bf16 library only: the Python layer routes the VAE there.
 * ================================================================================================================== */
typedef struct ctrlv_vae_config {
  int32_t in_channels, out_channels, latent_channels, layers_per_block, n_blocks;    /* 3, 3, 4, 2, 4 */
  int32_t block_out_channels[CTRLV_MAX_BLOCKS];                                       /* 128, 256, 512, 512 */
  float scaling_factor;         /* 0.18215; informative: ctrlv_vae_encode takes the scale of a call as an argument */
  int64_t offset_limit_bytes;   /* 0 = the kernels' 32-bit limit (2^32 - 2^24); smaller values only shrink the frame
                                   ranges of the per-frame ops: same bits (tests use it) */
} ctrlv_vae_config;
typedef struct ctrlv_vae_plan ctrlv_vae_plan;
/* Size rules (vae_encoder_hip.supports / vae_decoder_hip.supports): four down / up blocks, channel counts multiples of 64,
 * latent_channels <= 8, in_channels <= 8, out_channels <= 4; the mid blocks' attention has one head. */
int ctrlv_vae_plan_create(const ctrlv_vae_config* cfg, int device, ctrlv_vae_plan** out);
/* The diffusers state-dict keys of vae/diffusion_pytorch_model.safetensors (encoder.*, decoder.*, quant_conv.*).  Host or
 * device tensors, fp32 or 16-bit; packed on the device; extra names are ignored, a missing one is an error.  May be called
 * again; synchronises the device. */
int ctrlv_vae_plan_load_weights(ctrlv_vae_plan* plan, const ctrlv_tensor_desc* tensors, size_t n);
/* Bytes of workspace of one call; 0 on error ("not loaded" before load_weights, or a shape the call would refuse:
 * ctrlv_last_error).  what 0: ctrlv_vae_encode of n images of H x W PIXELS (num_frames ignored); what 1: ctrlv_vae_decode of
 * n latent frames of H x W LATENT pixels in clips of num_frames (the workspace is one clip's: it does not grow with n). */
size_t ctrlv_vae_plan_workspace_bytes(ctrlv_vae_plan* plan, int what, int n, int num_frames, int H, int W);
/* pixels (n, in_channels, Hpx, Wpx) in [-1, 1], dtype 0 / 1 / 2.  Outputs, NCHW of out_dtype, either may be NULL:
 * moments (n, 2 L, Hpx/8, Wpx/8) = quant_conv(encoder(pixels)); latents (n, L, Hpx/8, Wpx/8) = scale * (mean + std * noise),
 * noise (n, L, Hpx/8, Wpx/8) fp32 or NULL for latent_dist.mode() (ctrlv_vae_posterior).  Shapes: Hpx, Wpx multiples of 8, latent
 * pixels per image a multiple of 64 and <= 16384, n * Hpx * Wpx * block_out_channels[0] * 2 below the offset limit
 * (CTRLV_E_BAD_SHAPE).  workspace 256-byte aligned; too small: CTRLV_E_WORKSPACE before anything is launched. */
int ctrlv_vae_encode(ctrlv_vae_plan* plan, const void* pixels, int dtype, int n, int Hpx, int Wpx, const float* noise,
                     float scale, void* latents, void* moments, int out_dtype, void* workspace, size_t workspace_bytes,
                     ctrlv_stream_t stream);
/* z (n, L, h, w) latents already divided by the scaling factor, dtype 0 / 1 / 2; frames (n, out_channels, 8 h, 8 w) of
 * out_dtype.  n % num_frames == 0: the clips are decoded one after the other.  Shapes: h * w a multiple of 64 and <= 16384,
 * every whole-clip tensor (num_frames * pixels * channels * 2 bytes per level) below the offset limit (CTRLV_E_BAD_SHAPE). */
int ctrlv_vae_decode(ctrlv_vae_plan* plan, const void* z, int dtype, int n, int num_frames, int h, int w, void* frames,
                     int out_dtype, void* workspace, size_t workspace_bytes, ctrlv_stream_t stream);
int ctrlv_vae_plan_destroy(ctrlv_vae_plan* plan);

/* ==================================================================================================================
 * A whole clip as ONE call (csrc/pipeline.hip, csrc/pipeline_io.hip): what StableVideoControlPipeline.__call__
 * (pipeline_video_control.py:196-350) / VideoDiffusionPipeline.__call__ compute between a uint8 conditioning image (plus the box
 * frames) and uint8 video frames -- prepare_clip -> the denoising loop -> finish_clip of ctrlv_amd/pipelines/pipeline_utils.py --
 * for a host in any language.  Additive entry points: the ABI number does not change.
 * ================================================================================================================== */
/* _resize_with_antialiasing (Gaussian pre-blur, reflect padding; bicubic, align_corners=True, A = -0.75, indices clamped to the
 * image) fused with the affine steps around it.  src: src_u8 = 1: (n, H, W, 3) uint8, read as (v / 255) * 2 - 1; src_u8 = 0:
 * (n, 3, H, W) fp32.  Per axis sigma = max((factor - 1) / 2, 0.001), ks = int(max(4 sigma, 3)) made odd, weights exp(-x^2 / (2
 * sigma^2)) normalised (fp32, formed on the host).  mean / std: host float[3], both or neither: the epilogue ((y + 1) / 2 -
 * mean[c]) / std[c] (CLIP's normalisation).  dst (n, 3, h, w): dst_dtype 0 fp32, or the library's element code: the fp32 value
 * rounded to nearest even.  The blurred rows of an output tile are staged in LDS: the blurred image never reaches memory.
 * CTRLV_E_BAD_SHAPE (host validation): ks / 2 >= H or >= W (reflect padding undefined), a per-axis factor above 8 (more than 15
 * taps), n > 21845. */
int ctrlv_resize_antialias(const void* src, int src_u8, int n, int H, int W, void* dst, int dst_dtype, int h, int w,
                           const float* mean, const float* std, ctrlv_stream_t stream);
/* The VAE encoder's pixel input: image_u8 (n, H, W, 3) uint8, noise fp32 (n, 3, H, W) or NULL -> out (n, 3, H, W) elements =
 * rne(2 * (v / 255) - 1 + strength * noise), every operation rounded in fp32 (VaeImageProcessor.preprocess + the noise
 * augmentation of prepare_clip + the cast to the VAE's dtype). */
int ctrlv_pixels_prepare(const void* image_u8, const float* noise, float strength, int n, int H, int W, void* out,
                         ctrlv_stream_t stream);
/* Decoded frames to display bytes: frames (m, 3, H, W) elements (as ctrlv_vae_decode writes them) -> out_u8 (m, H, W, 3) uint8
 * (4-byte aligned) = rint(clamp(x / 2 + 0.5, 0, 1) * 255), half to even (VaeImageProcessor.postprocess + numpy_to_pil). */
int ctrlv_frames_to_u8(const void* frames, int m, int H, int W, void* out_u8, ctrlv_stream_t stream);

/* One clip request.  The caller MUST clear the struct (memset / calloc / `= {0}` / ctypes) before setting fields, as with
 * ctrlv_gemm_desc.  Device pointers unless said otherwise; h = height / 8, w = width / 8, L = the VAE's latent channels. */
typedef struct ctrlv_clip_request {
  int32_t n_clips, num_frames, height, width;   /* clips, frames per clip (<= 32), pixels (multiples of what the plans need) */
  const void* image_u8;          /* (n, H, W, 3) uint8, already at the working size */
  const void* cond;              /* cond_channels 3: (n, F, 3, H, W) pixels in [-1, 1]; 4: latents (n, F, L, h, w).  NULL only
                                    without a ControlNet */
  int32_t cond_channels;
  int32_t cond_dtype;            /* dtype code of cond (0 fp32, 1 fp16, 2 bf16) */
  const float* aug_noise;        /* fp32 (n, 3, H, W) or NULL: the library draws no random numbers */
  float noise_aug_strength;      /* applied to aug_noise, and the third added time id */
  int32_t num_steps;             /* 1 .. 1024 */
  const float* latents;          /* fp32 (n, F, L, h, w): the initial noise ALREADY multiplied by init_noise_sigma */
  const float* sigmas;           /* HOST float[num_steps + 1], the scheduler's own values, strictly decreasing, sigmas[i] > 0 for
                                    i < num_steps (the host keeps the schedule) */
  const float* timesteps;        /* HOST float[num_steps] */
  int32_t fps, motion_bucket_id; /* added time ids = [fps - 1, motion_bucket_id, noise_aug_strength], each rounded to the element
                                    type as the pipelines' _get_add_time_ids does */
  float min_guidance, max_guidance;   /* per-frame ramp linspace(min, max, F); classifier-free guidance is on iff max > 1 */
  float conditioning_scale;      /* of the ControlNet residuals */
  int32_t decode_chunk;          /* frames per ctrlv_vae_decode call over the n F frames in order (the last chunk may be shorter);
                                    needed when frames are asked for */
  float clip_mean[3], clip_std[3];    /* the feature extractor's image_mean / image_std; all six zero = CLIP's own values */
  float* out_latents;            /* fp32 (n, F, L, h, w), always written (may be `latents` itself) */
  void* out_frames;              /* (n F, 3, H, W) elements in [-1, 1] as decoded, or NULL */
  void* out_frames_u8;           /* (n, F, H, W, 3) uint8, or NULL */
} ctrlv_clip_request;
typedef struct ctrlv_pipeline ctrlv_pipeline;
/* Borrows the four plans (they must outlive the pipeline, be of THIS library and on `device`); controlnet may be NULL (the
 * SVD-only pipeline).  Host-only validation: needs no GPU.  The side stream and the two events of the ControlNet overlap are
 * created by the first ctrlv_pipeline_generate that uses them and released by ctrlv_pipeline_destroy. */
int ctrlv_pipeline_create(ctrlv_plan* unet, ctrlv_plan* controlnet, ctrlv_vae_plan* vae, ctrlv_clip_plan* clip, int device,
                          ctrlv_pipeline** out);
/* on = 1 (default): the ControlNet forward of a step runs on the driver's side stream beside the UNet's down / mid blocks
 * (ctrlv_unet_forward's residual_event); 0: one chain on the caller's stream.  Same bits either way. */
int ctrlv_pipeline_set_overlap(ctrlv_pipeline* p, int on);
/* Bytes of workspace ctrlv_pipeline_generate needs for `r` (pure host arithmetic: the geometry, cond_channels, decode_chunk and
 * which outputs are asked for; never num_steps); 0 on error (a request generate would refuse, or plans without weights:
 * ctrlv_last_error). */
size_t ctrlv_pipeline_workspace_bytes(ctrlv_pipeline* p, const ctrlv_clip_request* r);
/* The clip, enqueued on `stream` (and, with overlap, on the side stream, which is joined to `stream` before the call returns):
 *   1. ctrlv_resize_antialias to the CLIP plan's image_size with the normalisation, ctrlv_clip_forward; ehs = (0 | embeds)
 *   2. ctrlv_pixels_prepare, ctrlv_vae_encode (mode, scale 1) of the image -- repeated over the frames as the conditioning
 *      channels of the model input (0 | latent) -- and of cond when it has 3 channels; control_cond = (0 | cond latents)
 *   3. added time ids, guidance ramp, timesteps: ONE upload in front of the loop (step i passes &t_dev[i])
 *   4. step 0's scaled input = rne(latents * (float) (1 / sqrt(sigma_0^2 + 1))), the reciprocal formed in double
 *      (DenoiseStepper.set_latents: torch's division of a device tensor by a host scalar); per step: the
 *      scaled input into both halves, ctrlv_controlnet_forward, ctrlv_unet_forward, ctrlv_cfg_euler_step.  No host-device copy
 *      and no synchronisation inside the loop
 *   5. z = rne(rne(latents) * (float) (1 / scaling_factor)), ctrlv_vae_decode per chunk;  6. ctrlv_frames_to_u8
 * Every argument and size is validated on the host before the first launch; `ws` (256-byte aligned, caller-owned) smaller than
 * ctrlv_pipeline_workspace_bytes is CTRLV_E_WORKSPACE.  UNet and ControlNet work in disjoint regions; the CLIP, VAE-encode and
 * VAE-decode phases alias them.  No HIP-graph capture inside.  Not thread-safe on one pipeline. */
int ctrlv_pipeline_generate(ctrlv_pipeline* p, const ctrlv_clip_request* r, void* ws, size_t ws_bytes, ctrlv_stream_t stream);
int ctrlv_pipeline_destroy(ctrlv_pipeline* p);

/* ------------------------------------------------------------------------------------------------------------------
 * The box predictor and the boxes-to-video chain (tools/eval_overall.py:74-163 of the reference): stage 1 is an SVD UNet that
 * sees the conditioning image plus the first few and the last bounding-box frames and generates the box frames in between
 * (pipeline_video_diffusion.py:197-206, 297); the frames are cleaned and remapped; stage 2 is ctrlv_pipeline_generate on a
 * pipeline with a ControlNet.  Additive entry points: the ABI number does not change, ctrlv_clip_request keeps its layout.
 * ------------------------------------------------------------------------------------------------------------------ */
/* The box frames of one predict_boxes call.  Clear the struct before setting fields. */
typedef struct ctrlv_box_condition {
  const void* frames;        /* channels 3: (n, F, 3, H, W) pixels in [-1, 1]; channels L: latents (n, F, L, h, w) */
  int32_t channels, dtype;   /* dtype code as cond_dtype (0 fp32, 1 fp16, 2 bf16) */
  int32_t num_cond_frames;   /* K in [0, F]: frames [0, K) and frame F-1 are taken */
  int32_t reserved;          /* must be 0 */
} ctrlv_box_condition;
/* Bytes of workspace ctrlv_pipeline_predict_boxes needs; 0 for a request it would refuse (ctrlv_last_error). */
size_t ctrlv_pipeline_boxes_workspace_bytes(ctrlv_pipeline* p, const ctrlv_clip_request* r, const ctrlv_box_condition* bc);
/* ctrlv_pipeline_generate on a pipeline WITHOUT a ControlNet and a request WITHOUT cond (either is CTRLV_E_BAD_ARG, named, before
 * any launch; the request is otherwise validated as generate validates it), with two differences:
 *   - after the image's latent has been repeated over the frames as the conditioning channels (step 2), those channels of frames
 *     [0, K) and F - 1 of every clip are overwritten in the conditional half: with the VAE mode latents (scale 1) of the 3-channel
 *     box frames, or with the latents as given, rounded to the element type.  With guidance on the unconditional half stays
 *     zero (the reference writes cat[zeros, cond] there).  Only the min(K + 1, F) taken frames are encoded; the encoder treats
 *     every image on its own, so the bits are those of encoding all F;
 *   - out_frames, when asked for, is clamped to [-1, 1].  out_frames_u8 is unchanged by the clamp: ctrlv_frames_to_u8 already
 *     clamps x / 2 + 0.5 to [0, 1], which is the same function of x.
 * CTRLV_E_BAD_ARG: reserved != 0, frames NULL; CTRLV_E_BAD_SHAPE: channels not 3 / L, K outside [0, F]; CTRLV_E_BAD_DTYPE. */
int ctrlv_pipeline_predict_boxes(ctrlv_pipeline* p, const ctrlv_clip_request* r, const ctrlv_box_condition* bc, void* ws,
                                 size_t ws_bytes, ctrlv_stream_t stream);

/* Between the stages (csrc/box_frames.hip; eval_overall.py:96-105, 154 and tensor2vid(..., "pt")).  frames (n F, 3, H, W)
 * elements as decoded; any of the three outputs may be NULL (all three: CTRLV_E_BAD_ARG).  One pass over the frames; every
 * value stays on the device and nothing synchronises with the host, so the call can be captured into a graph.
 *   out_pt   (n F, 3, H, W) elements: y = clamp(x / 2 + 0.5, 0, 1), each operation rounded to the element type
 *   out_cond (n F, 3, H, W) elements: 2 * (y - 0.5), each operation rounded (not the identity on x in fp16)
 *   out_u8   (n, F, 3, H, W) uint8: v = (float) y * 255 in fp32; a pixel whose channel sum (v0 + v1) + v2 is < threshold is
 *            zeroed; an interior frame 1 .. F-2 of a clip whose MINIMUM channel sum over all pixels is > threshold is zeroed
 *            whole (frames 0 and F-1 never are); the rest is truncated to uint8 as numpy's astype does.
 * ws: ctrlv_box_frames_post_ws_bytes(n, F) bytes, 4-byte aligned, needed with out_u8 only: the per-frame minimum (an atomic
 * minimum on the bits of the non-negative sums).  16-byte accesses where H W is a multiple of 16 and the pointers are aligned. */
size_t ctrlv_box_frames_post_ws_bytes(int n, int F);
int ctrlv_box_frames_post(const void* frames, int n, int F, int H, int W, float threshold, void* out_pt, void* out_cond,
                          void* out_u8, void* ws, size_t ws_bytes, ctrlv_stream_t stream);
/* binary_mask_iou's counts (src/ctrlv/metrics/FandJ.py:11-23) of gt_u8 and pred_u8, both (n, F, 3, H, W) uint8: a pixel is in a
 * mask when any of its channels is nonzero.  counts: DEVICE (n, 2, 3) 64-bit -- per clip {gt area, pred area, intersection}
 * over all F frames, then over the frames {0, F-1} (a one-frame clip counts its frame once).  Integers: the metric formed from
 * them on the host is exact. */
int ctrlv_mask_counts(const void* gt_u8, const void* pred_u8, int n, int F, int H, int W, unsigned long long* counts,
                      ctrlv_stream_t stream);

/* The chain as one call.  Clear the struct before setting fields. */
typedef struct ctrlv_two_stage_request {
  ctrlv_clip_request boxes;          /* stage 1 (no cond); out_frames may be NULL: the frames then live in the workspace */
  ctrlv_box_condition box_cond;
  ctrlv_clip_request video;          /* cond must be NULL on entry: the driver supplies stage 1's frames (3 channels, element dtype) */
  void* out_box_frames_u8;           /* cleaned (n, F, 3, H, W), or NULL */
  float clean_threshold;             /* the reference's 50 */
  int32_t reserved;                  /* must be 0 */
} ctrlv_two_stage_request;
/* 0 for a request the call would refuse (ctrlv_last_error). */
size_t ctrlv_pipeline_chain_workspace_bytes(ctrlv_pipeline* boxes, ctrlv_pipeline* video, const ctrlv_two_stage_request* q);
/* In order: ctrlv_pipeline_predict_boxes on `boxes` (no ControlNet), ctrlv_box_frames_post (out_cond -> stage 2's condition,
 * out_u8 -> out_box_frames_u8), ctrlv_pipeline_generate on `video` (with a ControlNet).  Nothing else: the bits are those of the
 * three calls made by hand.  Stage 1's frames and the condition live in `ws`, the stages' own workspaces alias.  Refused by
 * name before any launch: pipelines of another library or on different devices, requests of different geometry, video.cond
 * set, a video pipeline without a ControlNet, and whatever the two stages refuse. */
int ctrlv_pipeline_boxes_to_video(ctrlv_pipeline* boxes, ctrlv_pipeline* video, const ctrlv_two_stage_request* q, void* ws,
                                  size_t ws_bytes, ctrlv_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Seeded clips: what a host without a numerics stack still had to bring to a ctrlv_clip_request -- the two Gaussian draws, the
 * Karras schedule of EulerDiscreteScheduler and PIL's Lanczos resize to the working size (pipeline_utils.py: prepare_latents,
 * prepare_clip; VaeImageProcessor.preprocess) -- as library calls (csrc/pipeline_io.hip, csrc/pipeline.hip).  Pixels of any size
 * plus a 64-bit seed go in, video frames come out.  Additive entry points: the ABI number does not change, the three request
 * structs keep their layouts, ctrlv_pipeline_generate / _predict_boxes / _boxes_to_video are untouched.  The arithmetic stated
 * here is the contract: tests/seeded_ref.py restates it in numpy.
 * ------------------------------------------------------------------------------------------------------------------ */
/* Counter-based Gaussian noise.  out (n_clips, per_clip), out_dtype 0 fp32 or the library's element code.  Element e of clip i is
 * a pure function of (seed, clip0 + i, call, stream_id, e): never of the grid, of n_clips or of the pointer's alignment.
 *   block    j = e / 4 of a clip is Philox4x32-10 (Random123: multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 /
 *            0xBB67AE85, the key bumped before rounds 2 .. 10) of the counter (j, call, stream_id, clip0 + i) under the key
 *            (seed & 0xffffffff, seed >> 32) -> x0 .. x3.  j <= 2^32 - 1: per_clip > 2^34 is CTRLV_E_BAD_SHAPE.
 *            Known answers: counter (0,0,0,0), key (0,0) -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8; all ones -> 408f276d 41c83b0e
 *            a20bc7c6 6d5451fd; (243f6a88, 85a308d3, 13198a2e, 03707344), (a4093822, 299f31d0) -> d16cfe09 94fdcceb 5001e420
 *            24126ea1.
 *   uniform  u_k = the fp32 value nearest to (x_k + 0.5) / 2^32, ties to even, ONE rounding (the integer 2 x_k + 1 converted,
 *            times 2^-33).  u_k lies in [2^-33, 1]: ln u is finite, |z| <= sqrt(66 ln 2) ~ 6.77, never an infinity or a NaN.
 *   normal   Box-Muller in fp32 with the accurate device functions: r = sqrtf(-2 logf(u_a)), (c, s) = sincospif(2 u_b);
 *            elements 4j, 4j+1 = (r c, r s) of (u_0, u_1), elements 4j+2, 4j+3 the same of (u_2, u_3).
 *   output   round_dtype 0: out = scale * z in fp32; round_dtype 1: out = rne_el(rne_el(z) * scale) -- torch's element-typed
 *            randn times a Python scalar (prepare_latents); then stored as out_dtype.
 * One Philox block per thread and iteration, grid-stride; 16-byte stores (8 for 16-bit elements) where a block's four elements
 * are aligned, scalar stores elsewhere and for the tail of a per_clip that is no multiple of 4. */
int ctrlv_randn(uint64_t seed, uint32_t clip0, uint32_t call, uint32_t stream_id, int n_clips, size_t per_clip, float scale,
                int round_dtype, void* out, int out_dtype, ctrlv_stream_t stream);
/* The tables of EulerDiscreteScheduler.set_timesteps (Karras sigmas, "leading" spacing's init_noise_sigma): host arithmetic in
 * double, needs no GPU.  sigma_min = sigma_max = 0: SVD's 0.002 and 700.  With a = pow(max, 1/7.), b = pow(min, 1/7.) and
 * ramp_i = i * (1.0 / (num_steps - 1)) (0 for a single step):
 *   sigmas[i] = (float) pow(a + ramp_i * (b - a), 7.), sigmas[num_steps] = 0;   timesteps[i] = 0.25f * (float) log((double) sigmas[i]);
 *   *init_noise_sigma = sqrt((double) sigmas[0] * sigmas[0] + 1).
 * Against the Python scheduler: the sigmas are bit-equal, a timestep may differ by one fp32 ulp (torch takes the logarithm in
 * fp32).  CTRLV_E_BAD_SHAPE: num_steps outside 1 .. 1024; CTRLV_E_BAD_ARG: bounds not finite, positive and ordered (min < max),
 * NULL outputs (init_noise_sigma may be NULL). */
int ctrlv_euler_schedule(int num_steps, float sigma_min, float sigma_max, float* sigmas, float* timesteps,
                         double* init_noise_sigma);
/* PIL.Image.resize((w, h), resample=LANCZOS) of 8-bit RGB, every byte: src (n, H, W, 3) uint8 -> dst (n, h, w, 3) uint8.
 * Per axis (in -> out), on the host in double: scale = in / out, fs = max(scale, 1), support = 3 fs; per output index x:
 * center = (x + 0.5) scale, xmin = max((int) (center - support + 0.5), 0), xmax = min((int) (center + support + 0.5), in); tap
 * t = 0 .. xmax - xmin - 1 weighs lanczos3((t + xmin - center + 0.5) / fs), lanczos3(v) = sinc(v) sinc(v / 3) for -3 <= v < 3,
 * else 0, sinc(v) = sin(pi v) / (pi v), sinc(0) = 1; the weights are divided by their sum and become 22-bit fixed point:
 * (int) (k 2^22 + 0.5) for k >= 0, (int) (k 2^22 - 0.5) for k < 0.  Two passes, horizontal into a uint8 intermediate (n, H, w, 3)
 * in `ws`, then vertical; each output byte = clip8((2^21 + sum pixel k) >> 22), an arithmetic shift in int32 (255 times the sum
 * of |k| stays below 2^31).  An axis whose size does not change runs its pass too: same bytes as PIL, which skips it.
 * ws: ctrlv_resize_lanczos_ws_bytes bytes, 16-byte aligned: the tables (one upload per call) and the intermediate.  One thread
 * per output pixel (three channels); a workgroup stages its rows of weights in LDS.  CTRLV_E_BAD_SHAPE (host, by name): a zero
 * dimension, a down-scale above 16 per axis, n > 65535; ws_bytes too small: CTRLV_E_WORKSPACE.  The size query is 0 for a
 * shape the call would refuse. */
size_t ctrlv_resize_lanczos_ws_bytes(int n, int H, int W, int h, int w);
int ctrlv_resize_lanczos_u8(const void* src_u8, int n, int H, int W, void* dst_u8, int h, int w, void* ws, size_t ws_bytes,
                            ctrlv_stream_t stream);

/* What ctrlv_pipeline_prepare adds to a clip request.  Clear the struct before setting fields. */
typedef struct ctrlv_seed_request {
  uint64_t seed;
  uint32_t clip_index0;          /* clip i of the request draws as clip clip_index0 + i: the noise of a clip is a function of
                                    (seed, its index), not of the batch or the rank that draws it */
  uint32_t call;                 /* distinguishes the calls of one seed: stage 1 = 0, stage 2 = 1, ... */
  const void* src_image_u8;      /* (n, src_height, src_width, 3) uint8 on the device, or NULL: the request's image_u8 is used */
  int32_t src_height, src_width;
  float sigma_min, sigma_max;    /* both 0: the SVD values */
  float* sigmas_host;            /* caller's HOST arrays of num_steps + 1 and num_steps floats: they outlive the consuming call */
  float* timesteps_host;
  int32_t reserved;              /* must be 0 */
} ctrlv_seed_request;
/* Bytes of prep_ws for (r, s): what of {resized image, aug_noise, latents} the request leaves NULL, plus the resize's own
 * workspace.  Host arithmetic on the plans' configurations (weights need not be loaded); 0 for a pair prepare would refuse. */
size_t ctrlv_pipeline_prepare_bytes(ctrlv_pipeline* p, const ctrlv_clip_request* r, const ctrlv_seed_request* s);
/* *out = *in with the fields `in` leaves NULL filled; a field the caller did set is kept:
 *   sigmas, timesteps  ctrlv_euler_schedule(num_steps, sigma_min, sigma_max) written to sigmas_host / timesteps_host
 *   image_u8           ctrlv_resize_lanczos_u8 of src_image_u8 to (height, width) in prep_ws; the source pointer itself when it
 *                      already has that size (image_u8 and src_image_u8 both set: CTRLV_E_BAD_ARG)
 *   aug_noise          ctrlv_randn(seed, clip_index0, call, stream 0), fp32, scale 1, (n, 3, H, W)
 *   latents            ctrlv_randn(seed, clip_index0, call, stream 1), round_dtype 1, scale (float) init_noise_sigma -- of the
 *                      schedule above, or sqrt(sigmas[0]^2 + 1) of the caller's --, stored as fp32 (n, F, L, h, w)
 * `out` points into prep_ws (256-byte aligned), which stays alive until the consuming call -- ctrlv_pipeline_generate,
 * ctrlv_pipeline_predict_boxes, or a ctrlv_two_stage_request (prepare twice, call = 0 and call = 1) -- has finished on the
 * stream.  The filled request is validated as generate validates it; everything is refused by name on the host before the
 * first launch: reserved != 0, NULL host arrays where the schedule is asked for, a source image without sizes, a resize
 * ctrlv_resize_lanczos_u8 refuses, num_steps outside 1 .. 1024, prep_bytes too small (CTRLV_E_WORKSPACE). */
int ctrlv_pipeline_prepare(ctrlv_pipeline* p, const ctrlv_clip_request* in, const ctrlv_seed_request* s, ctrlv_clip_request* out,
                           void* prep_ws, size_t prep_bytes, ctrlv_stream_t stream);
/* ctrlv_pipeline_prepare_bytes (a multiple of 256) + ctrlv_pipeline_workspace_bytes of the filled request; 0 on refusal. */
size_t ctrlv_pipeline_seeded_workspace_bytes(ctrlv_pipeline* p, const ctrlv_clip_request* r, const ctrlv_seed_request* s);
/* ctrlv_pipeline_prepare into the front of ws, then ctrlv_pipeline_generate on the rest: the bits of the two calls made by hand.
 * sigmas_host / timesteps_host may be NULL here: the pipeline object then keeps the two arrays.  Not thread-safe on one
 * pipeline. */
int ctrlv_pipeline_generate_seeded(ctrlv_pipeline* p, const ctrlv_clip_request* r, const ctrlv_seed_request* s, void* ws,
                                   size_t ws_bytes, ctrlv_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Box evaluation around the chain (csrc/box_eval.hip, csrc/pipeline.hip): the reference's best-of-N loop over stage-1 guidance
 * ramps (tools/eval_overall.py:83-114, tools/draw_teaser.py:160-175) and its boundary F-measure (src/ctrlv/metrics/FandJ.py:
 * 94-156, tools/eval_video_bbox_prediction.py:85-95), with no host synchronisation between the stages.  Additive entry points:
 * the ABI number does not change, the existing structs keep their layouts, the existing entry points their bits.
 * ------------------------------------------------------------------------------------------------------------------ */
/* Per clip, the candidate whose all-frames mask IoU is largest.  counts: DEVICE (C, n, 2, 3) 64-bit, candidate c's block exactly
 * what one ctrlv_mask_counts call writes; winner: DEVICE int32 (n).  Over {gt, pred, inter} of all frames: union = gt + pred -
 * inter, iou = union > 0 ? (double) inter / (double) union : 1.0, compared in fp64 as numpy compares; a tie goes to the HIGHEST c
 * (the reference's `best_score = max(best_score, miou); if best_score == miou:` lets a later equal score replace an earlier
 * one).  Two ratios that round to the same double tie, as they do there.  One thread per clip, no atomics, no host sync: the call
 * can be captured into a graph.  CTRLV_E_BAD_ARG: NULL pointers, counts not 8-byte / winner not 4-byte aligned;
 * CTRLV_E_BAD_SHAPE: C outside 1 .. 8, n <= 0. */
int ctrlv_best_candidate(const unsigned long long* counts, int n, int C, int32_t* winner, ctrlv_stream_t stream);
/* dst[i] = src[winner[i]][i]: src (C, n, bytes_per_clip), dst (n, bytes_per_clip), winner DEVICE int32 (n), read on the device.
 * A winner outside [0, C) is clamped into the range, so a bad index never reads out of bounds.  A clip whose source and
 * destination share their offset from a 16-byte boundary is copied with 16-byte accesses between a head and a tail of single
 * bytes (bytes_per_clip a multiple of 16 and both pointers aligned: no head, no tail); any other clip byte by byte.
 * CTRLV_E_BAD_ARG: NULL pointers, winner not 4-byte aligned; CTRLV_E_BAD_SHAPE: C outside 1 .. 8, n <= 0, bytes_per_clip 0. */
int ctrlv_gather_clips(const void* src, const int32_t* winner, int n, int C, size_t bytes_per_clip, void* dst,
                       ctrlv_stream_t stream);

/* Best of C stage-1 candidates.  Clear the struct before setting fields. */
typedef struct ctrlv_best_boxes_request {
  int32_t n_candidates;                  /* C in 1 .. 8 */
  int32_t reserved;                      /* must be 0 */
  const ctrlv_clip_request* candidates;  /* HOST array of C stage-1 requests: one geometry (n_clips, num_frames, height, width);
                                            latents, aug_noise, guidance, schedule and steps may differ.  out_frames and
                                            out_frames_u8 must be NULL (the frames live in the workspace), out_latents as
                                            ctrlv_pipeline_generate wants it */
  ctrlv_box_condition box_cond;          /* one condition, shared by all candidates */
  const void* gt_u8;                     /* (n, F, 3, H, W) uint8 ground-truth box frames */
  float clean_threshold;                 /* the reference's 50 */
  int32_t reserved2;                     /* must be 0 */
  void* out_pt;                          /* (n F, 3, H, W) elements: the winner's [0, 1] frames, or NULL */
  void* out_cond;                        /* (n F, 3, H, W) elements: the winner's 2 (y - 0.5), or NULL */
  void* out_u8;                          /* (n, F, 3, H, W) uint8: the winner's cleaned frames, or NULL */
  unsigned long long* out_counts;        /* DEVICE (C, n, 2, 3), or NULL (then kept in the workspace) */
  int32_t* out_winner;                   /* DEVICE (n), or NULL (then kept in the workspace) */
} ctrlv_best_boxes_request;
/* 0 for a request the call would refuse (ctrlv_last_error). */
size_t ctrlv_pipeline_best_boxes_workspace_bytes(ctrlv_pipeline* p, const ctrlv_best_boxes_request* q);
/* In order, on `stream`: for c = 0 .. C-1 { the clip of candidate c as ctrlv_pipeline_predict_boxes runs it, its decoded
 * (clamped) frames into workspace slot c; ctrlv_box_frames_post of slot c with out_u8 only, into one scratch buffer all
 * candidates share; ctrlv_mask_counts(gt_u8, scratch) into block c of the counts }; one ctrlv_best_candidate; one
 * ctrlv_gather_clips of the frame slots -- the selection is PER CLIP: two clips of one call may take different candidates --; one
 * ctrlv_box_frames_post of the gathered frames into out_pt / out_cond / out_u8 (all three NULL: the last two calls are skipped).
 * Nothing else: the bits are those of these calls made by hand.  The candidates' own workspaces alias one region, as the stages
 * of ctrlv_pipeline_boxes_to_video do; nothing synchronises with the host.  Refused by name on the host before any launch:
 * C outside 1 .. 8 (CTRLV_E_BAD_SHAPE), a NULL candidates array or gt_u8, a nonzero reserved field, a threshold that is not
 * finite, a candidate with out_frames or out_frames_u8 set, out_counts / out_winner misaligned (CTRLV_E_BAD_ARG), candidates
 * of different geometry (CTRLV_E_BAD_SHAPE), whatever ctrlv_pipeline_predict_boxes refuses, ws too small (CTRLV_E_WORKSPACE). */
int ctrlv_pipeline_best_boxes(ctrlv_pipeline* p, const ctrlv_best_boxes_request* q, void* ws, size_t ws_bytes,
                              ctrlv_stream_t stream);

/* Best-of-C boxes, then the video.  Clear the struct before setting fields. */
typedef struct ctrlv_best_chain_request {
  ctrlv_best_boxes_request boxes;        /* out_cond NULL: the condition lives in the workspace */
  ctrlv_clip_request video;              /* cond must be NULL on entry: the driver supplies the winner's frames */
  int32_t reserved;                      /* must be 0 */
} ctrlv_best_chain_request;
/* 0 for a request the call would refuse (ctrlv_last_error). */
size_t ctrlv_pipeline_best_chain_workspace_bytes(ctrlv_pipeline* boxes, ctrlv_pipeline* video, const ctrlv_best_chain_request* q);
/* ctrlv_pipeline_best_boxes on `boxes`, its out_cond (the caller's, or a buffer in ws) becoming the condition of
 * ctrlv_pipeline_generate on `video`; the two pipelines' workspaces alias.  With C = 1: the bits of
 * ctrlv_pipeline_boxes_to_video.  Refused by name before any launch: what ctrlv_pipeline_best_boxes and
 * ctrlv_pipeline_boxes_to_video refuse (pipelines of another library or on different devices, a video pipeline without a
 * ControlNet, video.cond set, a video request of another geometry). */
int ctrlv_pipeline_best_boxes_to_video(ctrlv_pipeline* boxes, ctrlv_pipeline* video, const ctrlv_best_chain_request* q, void* ws,
                                       size_t ws_bytes, ctrlv_stream_t stream);

/* The pixel radius of f_measure's boundary tolerance (host arithmetic, needs no GPU): bound_th itself when bound_th >= 1 (an
 * integer), else ceil(bound_th * sqrt((double) (H^2 + W^2))) in double -- the square root of the integer, not hypot: at 75 x 100
 * the product with 0.008 is exactly 1.  576 x 1024 -> 10, 320 x 512 -> 5.  < 0 on refusal (ctrlv_last_error): sizes not
 * positive, bound_th not finite, negative, or >= 1 and not an integer. */
int ctrlv_boundary_radius(int H, int W, double bound_th);
/* The four counts of f_measure per frame.  gt_u8, pred_u8 (n, F, 3, H, W) uint8 as for ctrlv_mask_counts; counts: DEVICE
 * (n, F, 4) 64-bit, 8-byte aligned, zeroed by the call: {n_fg, n_gt, fg_match, gt_match}.  With G and P the masks of a frame:
 *   mask      mask_mode 0: any channel nonzero (binary_mask_iou's mask); mask_mode 1: (19595 R + 38470 G + 7471 B + 0x8000) >> 16
 *             != 0, PIL's convert('L') (eval_video_bbox_prediction.py:89-92) -- not mode 0: (1, 0, 0) is outside the mask
 *   b(S)      the one-pixel boundary map: for y < H-1, x < W-1: S[y,x] != S[y,x+1] | S[y,x] != S[y+1,x] | S[y,x] != S[y+1,x+1];
 *             last row, x < W-1: S[y,x] != S[y,x+1]; last column, y < H-1: S[y,x] != S[y+1,x]; the bottom-right corner: 0
 *   D(b)      dilation by a disk: D(b)[y,x] = OR of b[y+dy, x+dx] over dx^2 + dy^2 <= radius^2 inside the image (outside
 *             contributes nothing)
 *   counts    n_fg = |b(P)|, n_gt = |b(G)|, fg_match = |b(P) & D(b(G))|, gt_match = |b(G) & D(b(P))|
 * Integers: precision = fg_match / n_fg, recall = gt_match / n_gt and F are formed from them on the host.  One workgroup per
 * frame and band of rows: the mask bits of the band, `radius` rows of halo and one row below go into LDS as 64-bit words
 * (16-byte loads where W is a multiple of 16 and the pointers are aligned, single bytes and a ballot otherwise), the boundary
 * words by shift and xor, the dilation per dy as a horizontal OR-spread by floor(sqrt(radius^2 - dy^2)); the dilated image
 * never reaches memory.  Refused by name on the host before any launch: NULL pointers, counts misaligned (CTRLV_E_BAD_ARG),
 * radius outside 1 .. 32, mask_mode outside {0, 1}, sizes not positive, a width whose rows of words do not fit the LDS layout
 * at this radius (1856 at radius 32, more at smaller radii), more than 2^31 - 1 workgroups (CTRLV_E_BAD_SHAPE). */
int ctrlv_boundary_counts(const void* gt_u8, const void* pred_u8, int n, int F, int H, int W, int mask_mode, int radius,
                          unsigned long long* counts, ctrlv_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Per-frame SSIM and PSNR of generated clips (csrc/frame_quality.hip, csrc/pipeline_io.hip): the ssim_score_image and
 * psnr_score_image numbers of the reference's evaluate_vids (src/ctrlv/metrics/fvd.py:187-289), which resizes every frame with
 * PIL, maps both clips to v / 127.5 - 1 in fp32 and calls scikit-image per frame with data_range = the joint value range of the
 * two frames.  Here the frames stay on the device as bytes; n F doubles and 3 n F integers come back.  Additive entry points: the
 * ABI number does not change.  All validation on the host, by name, before any launch; no host synchronisation (the calls can
 * be captured into a graph); outputs are set by the call, the caller zeroes nothing.  tests/frame_quality_ref.py restates the
 * arithmetic in numpy.
 * ------------------------------------------------------------------------------------------------------------------ */
/* gt_u8, gen_u8 (n, F, 3, H, W) uint8 as for ctrlv_mask_counts; stats: DEVICE (n, F, 3) 64-bit, 8-byte aligned: per frame {min
 * byte, max byte, sum of (gt - gen)^2} over all three channels of BOTH frames.  Integer reductions only (wave reductions, then
 * integer atomics): exact and independent of order.  PSNR = 10 log10((max - min)^2 3 H W / sum) is formed from them on the host in
 * double.  16-byte loads where 3 H W is a multiple of 16 and both pointers are 16-byte aligned, single bytes otherwise.
 * CTRLV_E_BAD_ARG: NULL pointers, stats misaligned; CTRLV_E_BAD_SHAPE: sizes not positive, more than 2^31 - 1 frames. */
int ctrlv_frame_stats(const void* gt_u8, const void* gen_u8, int n, int F, int H, int W, long long* stats, ctrlv_stream_t stream);
/* ssim: DEVICE (n, F) double = structural_similarity(gt, gen, channel_axis=0, data_range=R, gaussian_weights=True, sigma=1.5) of
 * every frame; stats: what ctrlv_frame_stats wrote for the same frames, read on the device.  With x = gt - 127.5 and
 * y = gen - 127.5 in byte units (SSIM is scale-invariant once R is in the same units) and R = max - min:
 *   g[i]  = exp(-i^2 / 4.5) / sum, i = -5 .. 5, formed on the host in double;   u. = (g (x) g) * .   (the 11 x 11 window)
 *   v_x   = (121 / 120) (u_xx - u_x^2), likewise v_y and v_xy = (121 / 120) (u_xy - u_x u_y);   C1 = (0.01 R)^2, C2 = (0.03 R)^2
 *   S     = (2 u_x u_y + C1) (2 v_xy + C2) / ((u_x^2 + u_y^2 + C1) (v_x + v_y + C2))
 *   ssim  = the mean of S over 5 <= row < H - 5, 5 <= col < W - 5 and the three channels: structural_similarity's crop, so no
 *           window touches a border and its `reflect` padding is never evaluated.
 * The kernel takes the moments about m = (min + max) / 2: it filters x' = gt - m and y' = gen - m (exact in fp32), forms the
 * v from those (they are shift-invariant) and adds m - 127.5 to the two means.  Every term then scales with R^2 as C1 and C2 do;
 * about 127.5, fp32 loses u_xx - u_x^2 to cancellation on low-contrast frames (a 12 x 75 frame of 250 with one pixel at 247 is
 * off by 1e-3).  fp32 inside a pixel, each compared product rounded by its own operation (gen == gt gives exactly 1); S is
 * summed in double.  One workgroup per (frame, channel, 16 x 64 tile of outputs): the tile and 5 pixels of halo of both frames
 * in LDS, a horizontal pass into LDS, the vertical pass from there -- the filtered images never reach memory.  A workgroup adds
 * its S in a fixed order (per thread in pixel order, wave shuffles, the four waves in order) into its own slot of ws; a second
 * launch adds a frame's slots (one wave per frame: lane l the slots l, l + 64, ... in index order, then a shuffle tree) and
 * divides.  No floating-point atomics: a frame's value is bit-identical run to run and independent of n, of the other frames
 * and of pointer alignment.  R = 0 (both frames one constant): NaN, the reference's 0 / 0; other frames are not disturbed.
 * ws: ctrlv_frame_ssim_ws_bytes bytes (0 for a shape the call would refuse), 8-byte aligned.  CTRLV_E_BAD_SHAPE: H or W below 11
 * (scikit-image raises there too), sizes not positive, more than 2^31 - 1 workgroups; CTRLV_E_BAD_ARG: NULL pointers, stats /
 * ssim / ws not 8-byte aligned; CTRLV_E_WORKSPACE: ws_bytes too small. */
size_t ctrlv_frame_ssim_ws_bytes(int n, int F, int H, int W);
int ctrlv_frame_ssim(const void* gt_u8, const void* gen_u8, int n, int F, int H, int W, const long long* stats, double* ssim,
                     void* ws, size_t ws_bytes, ctrlv_stream_t stream);
/* PIL.Image.resize((w, h), resample=filter) of 8-bit planes, every byte: src (planes, H, W) uint8 -> dst (planes, h, w) uint8,
 * planes = n F 3 for a batch of clips.  PIL filters the bands of an RGB image independently with the same coefficients, so the
 * planar result equals PIL's on the stacked RGB image.  filter takes PIL's codes: 1 LANCZOS (support 3, as
 * ctrlv_resize_lanczos_u8), 2 BILINEAR (support 1, 1 - |v|), 3 BICUBIC (support 2, a = -0.5: ((a + 2) |v| - (a + 3)) v^2 + 1 for
 * |v| < 1, (((|v| - 5) |v| + 8) |v| - 4) a for |v| < 2); anything else is CTRLV_E_BAD_ARG (NEAREST is another code path in PIL and
 * is not built).  Everything else is as stated for ctrlv_resize_lanczos_u8 with `support` for its 3: ksize = 2 ceil(support fs) +
 * 1, 22-bit fixed-point weights, two passes through a uint8 intermediate (planes, H, w) in ws.  ws:
 * ctrlv_resize_frames_ws_bytes bytes (0 for a request the call would refuse), 16-byte aligned.  CTRLV_E_BAD_SHAPE: a zero
 * dimension, a down-scale above 16 per axis, more than 262140 rows; CTRLV_E_WORKSPACE: ws_bytes too small. */
size_t ctrlv_resize_frames_ws_bytes(int planes, int H, int W, int h, int w, int filter);
int ctrlv_resize_frames_u8(const void* src_u8, int planes, int H, int W, void* dst_u8, int h, int w, int filter, void* ws,
                           size_t ws_bytes, ctrlv_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * LPIPS of generated frames (csrc/lpips.hip): `lpips.LPIPS(net='alex')(gt, gen)` of evaluate_vids (src/ctrlv/metrics/fvd.py:
 * 241-248) per frame -- the scaling layer, AlexNet's five convolutions and two max-pools, the channel normalisation of the five
 * ReLU outputs, the five bias-free 1x1 "lin" layers and the spatial mean -- on frames in [-1, 1].  Additive entry points: the ABI
 * number does not change and no existing struct or kernel does.
 *
 * The metric subtracts two normalised feature maps, so 16-bit activations lose it where the frames are close (17 % on frames one
 * grey level apart).  Every convolution therefore runs on SPLIT operands through ctrlv_gemm with fp32 output:
 *     x = hi + lo,  hi = rne_el(x),  lo = rne_el(x - hi)  (x - hi is exact in fp32), the weight w split the same way,
 *     y = b + lo whi + hi wlo + hi whi   as ONE ctrlv_gemm launch: A rows [lo | hi | hi] against W rows [whi | wlo | whi].
 * The launch walks K in order, so the two small products are summed first and the fp32 chain that carries the full-size sum is
 * one block long, not three.
 * In the fp16 library hi SATURATES at +-65504 (lo then carries what is left, itself saturated): real AlexNet activations stay
 * far below.  Activations between layers are fp32 channels-last rows [m H W, C] holding the convolution output BEFORE ReLU;
 * every consumer (the next im2col, the pool, the distance kernel) applies max(v, 0) when it reads.
 * ------------------------------------------------------------------------------------------------------------------ */
/* The A operand of one convolution: element rows [M, 3 Kp], column blocks lo | hi | hi, Kp = k k C rounded up to a multiple of
 * 64, columns [k k C, Kp) of each block zero, taps outside the image zero.  rows dense, 16-byte aligned, M Kp 3 < 2^31.
 *   form 0 (first layer): src planar frames (m, 3, H, W), src_dtype 3 = uint8, 0 = fp32 in [-1, 1].  In fp32, each operation
 *     rounded: v = u8 / 127.5f - 1.0f (skipped for fp32), then (v - shift[c]) / scale[c], shift = (-.030, -.088, -.188), scale =
 *     (.458, .448, .450).  k = 11, stride 4, padding 2: M = m Ho Wo, Ho = (H - 7) / 4 + 1; columns in (c, ky, kx) order.  C = 3;
 *     ld is ignored.
 *   form 1 (rows): src fp32 rows [m H W, ld] of C channels (C a multiple of 8, ld a multiple of 4 and >= C), read as max(v, 0);
 *     k = 3 or 5, stride 1, padding (k - 1) / 2: M = m H W; columns tap-major (ky, kx, c). */
int ctrlv_lpips_im2col_split(const void* src, int form, int src_dtype, int m, int H, int W, int C, int ld, int k, void* rows,
                             ctrlv_stream_t stream);
/* A convolution's parameter [N][C][k][k] (dtype_code 0 / 1 / 2) -> element rows [N][3 Kp] = whi | wlo | whi in the column order
 * of the matching im2col: order 0 (c, ky, kx), order 1 (ky, kx, c); padding columns zero.  dst dense, 16-byte aligned. */
int ctrlv_lpips_pack_weight(const void* w, int dtype_code, int N, int C, int k, int order, void* dst, ctrlv_stream_t stream);
/* max_pool2d(relu(x), 3, stride 2) in floor mode without padding on fp32 rows: x [m H W, ldx] of C channels (C, ldx, ldo
 * multiples of 4) -> out [m Ho Wo, ldo], Ho = (H - 3) / 2 + 1.  One value per output is selected: exact.  H, W >= 3. */
int ctrlv_relu_maxpool_rows(const float* x, int m, int H, int W, int C, int ldx, float* out, int ldo, ctrlv_stream_t stream);
/* One layer's distance: gt, gen fp32 rows [frames pix, ld] of C channels (the same pixels of both), read as max(v, 0); lin fp32
 * [C].  Per pixel in fp32: n = x / (sqrt(sum_c x^2) + 1e-10) for both, d = sum_c lin[c] (n_gt - n_gen)^2 -- the channel sums
 * per lane in channel order, then a fixed shuffle tree.  The d of a frame are added in fp64: a workgroup owns 64 consecutive
 * pixels of one frame (a wave 16, in order; the four waves in order) and writes its sum to partials[frame][block], block <
 * ctrlv_lpips_distance_blocks(pix) = ceil(pix / 64).  No atomics: a frame's partials do not depend on the other frames.  C a
 * multiple of 4, at most 512; ld a multiple of 4. */
int ctrlv_lpips_distance_blocks(int pix);
int ctrlv_lpips_layer_distance(const float* gt, const float* gen, int ld, const float* lin, int frames, int pix, int C,
                               double* partials, ctrlv_stream_t stream);
/* out[frame] = sum over the layers, in order, of (the layer's partials of the frame summed in block order) / pix[layer].
 * partials: the layers' [frames][blocks] arrays one behind the other; pix: n_layers (at most 8) pixel counts, a HOST array. */
int ctrlv_lpips_finish(const double* partials, int frames, int n_layers, const int* pix, double* out, ctrlv_stream_t stream);

/* The metric as one call: ctrlv_lpips_plan_create -> ctrlv_lpips_plan_load_weights -> ctrlv_lpips_ws_bytes ->
 * ctrlv_lpips_frames.  Weights (host or device tensors, fp32 or 16-bit; extra names are ignored, a missing one is an error that
 * names it): torchvision's alexnet `features.{0,3,6,8,10}.{weight,bias}` and lpips' `lin{0..4}.model.1.weight`.  The plan owns
 * the packed split weights; load_weights may be called again and synchronises the device. */
typedef struct ctrlv_lpips_plan ctrlv_lpips_plan;
int ctrlv_lpips_plan_create(int device, ctrlv_lpips_plan** out);
int ctrlv_lpips_plan_load_weights(ctrlv_lpips_plan* plan, const ctrlv_tensor_desc* tensors, size_t n);
/* Bytes of workspace for frames of H x W taken frames_per_chunk at a time; 0 on error (ctrlv_last_error). */
size_t ctrlv_lpips_ws_bytes(ctrlv_lpips_plan* plan, int H, int W, int frames_per_chunk);
/* gt, gen: planar frames (n, F, 3, H, W), src_dtype 3 = uint8 or 0 = fp32 in [-1, 1]; out: n F doubles, the LPIPS of every frame
 * pair (evaluate_vids averages them).  The frames are taken in chunks; a chunk's gt and gen frames are stacked as 2 chunk images:
 *     im2col -> ctrlv_gemm (mode 0, taps 1, Cin = 3 Kp, fp32 output, bias, the 128 x 128 tile named per layer) for conv1;
 *     distance, pool, conv2;  distance, pool, conv3;  distance, conv4;  distance, conv5;  distance, finish.
 * The chunk is the largest the workspace holds (every im2col buffer below 2^31 elements); a frame's bits do not depend on n, F,
 * the chunk or the workspace size.  No host synchronisation, nothing read back: capturable into a HIP graph.  Everything is
 * checked before the first launch.  CTRLV_E_BAD_SHAPE: H or W below 31 (the second pool has no output), n or F not positive;
 * CTRLV_E_WORKSPACE: ws (256-byte aligned) smaller than ctrlv_lpips_ws_bytes(plan, H, W, 1). */
int ctrlv_lpips_frames(ctrlv_lpips_plan* plan, const void* gt, const void* gen, int src_dtype, int n, int F, int H, int W,
                       double* out, void* ws, size_t ws_bytes, ctrlv_stream_t stream);
int ctrlv_lpips_plan_destroy(ctrlv_lpips_plan* plan);

/* ------------------------------------------------------------------------------------------------------------------
 * Training batches: what the reference's training loops do between a data-loader batch and their model call
 * (tools/train_video_controlnet.py:366-449, tools/train_video_diffusion.py:428-514) -- the clamped CLIP prologue, the VAE
 * posterior samples, the per-clip draws into the scheduler's tables, the noising, the conditioning dropout, the box predictor's
 * frame layout and the channel concat -- as library calls (csrc/train_batch.hip, csrc/train_batch_plan.hip).  Pixels plus
 * (seed, step, clip index) go in, what train_step reads comes out.  Additive entry points: the ABI number does not change, the
 * existing structs keep their layouts, the existing entry points their bits.  The arithmetic stated here is the contract:
 * tests/train_batch_ref.py restates it in numpy on top of tests/seeded_ref.py.
 * ------------------------------------------------------------------------------------------------------------------ */
/* ctrlv_resize_antialias with encode_video_image's clamp (utils/util.py:97-125) in the normalising epilogue:
 * (min(max((y + 1) * 0.5, 0), 1) - mean[c]) / std[c]; a NaN stays a NaN, as with torch.clamp.  The same kernel: the clamp is one
 * runtime branch, and where nothing clamps the bits are ctrlv_resize_antialias'.  mean / std are required here
 * (CTRLV_E_BAD_ARG). */
int ctrlv_resize_antialias_clamped(const void* src, int src_u8, int n, int H, int W, void* dst, int dst_dtype, int h, int w,
                                   const float* mean, const float* std, ctrlv_stream_t stream);
/* The per-clip draws of a training step.  One Philox4x32-10 block per clip (the key and rounds of ctrlv_randn): counter
 * (0, call, 2, clip0 + i) under the key (seed & 0xffffffff, seed >> 32) -> x0 .. x3.  sigma_table / timestep_table: DEVICE fp32
 * [T], 1 <= T <= 65536 (EulerDiscreteScheduler().sigmas[:T] and .timesteps as __init__ builds them: the lookup is then the
 * reference's get_sigmas).  Outputs, DEVICE arrays of n_clips entries, any of them may be NULL:
 *   indices[i]     (int32) = (uint64(x0) * T) >> 32: in [0, T), the multiply-shift form of randint
 *   sigmas[i]      = sigma_table[indices[i]];  timesteps[i] = timestep_table[indices[i]]
 *   random_p[i]    = ctrlv_randn's uniform rule applied to x1 (in [2^-33, 1])
 *   prompt_keep[i] = !(p < t2);  image_mask[i] = 1 - (p >= t1) * (p < t3)        (fp32: 0 or 1)
 * with t1 = (float) dropout_prob, t2 = (float) (2.0 * dropout_prob), t3 = (float) (3.0 * dropout_prob): the products formed in
 * double and rounded once, torch's rule for an fp32 tensor compared with a Python scalar.  dropout_prob < 0 switches both masks
 * off (all ones: conditioning_dropout_prob=None).  One thread per clip, no atomics: clip i's values depend on (seed, clip0 + i,
 * call) only.  CTRLV_E_BAD_ARG: a NULL table, a dropout_prob that is not finite; CTRLV_E_BAD_SHAPE: T or n_clips (1 .. 65536)
 * out of range. */
int ctrlv_train_draws(uint64_t seed, uint32_t clip0, uint32_t call, int n_clips, const float* sigma_table,
                      const float* timestep_table, int T, double dropout_prob, int32_t* indices, float* sigmas, float* timesteps,
                      float* random_p, float* prompt_keep, float* image_mask, ctrlv_stream_t stream);
/* One pass over the latents of a batch: the noising, the model input and the conditioning channels.  All tensors DEVICE,
 * contiguous; plane = L h w, per_clip = F plane.
 *   target      fp32 (n, F, L, h, w): the clean latents, already scaled.  L <= 8, F <= 32
 *   noise       fp32 of the same shape, or NULL: the noise is then drawn in the kernel by ctrlv_randn's contract -- (seed,
 *               clip0 + i, call), stream_id 3, scale 1, round_dtype 0, per_clip as above -- and the outputs have the bits of
 *               ctrlv_randn followed by this call with that noise.  seed / clip0 / call are ignored when noise is given
 *   sigmas      fp32 (n);  image_mask fp32 (n) or NULL (all ones)
 *   cond_image  fp32 (n, L, h, w);  cond_frames fp32 (n, F, L, h, w), required for layout 1 and ignored for layout 0
 *   layout      0 (Box2Video, plain stage 1): c = cond_image for every frame;  1 (box predictor, train_video_diffusion.py:457-458):
 *               c = cond_frames for f < K or f == F - 1, cond_image otherwise.  0 <= K <= F
 *   noisy       fp32 (n, F, L, h, w) = target + noise * sigma
 *   sample      (n, F, 2 L, h, w), sample_dtype 0 fp32 or the library's element code:
 *               sample[:, :, :L] = rne(noisy / sqrtf(sigma * sigma + 1)),  sample[:, :, L:] = rne(image_mask * c)
 *   noise_out   fp32 (n, F, L, h, w) or NULL: the noise that was used
 * Every operation is rounded on its own in fp32 (no contraction), division and square root correctly rounded: the bits of the
 * eager torch expressions of ctrlv_amd.training._noised_inputs.  One thread per four consecutive elements of a clip (one Philox
 * block): 16-byte accesses (8 for a 16-bit sample) when plane is a multiple of 4 and every pointer is 16-byte aligned, element by
 * element otherwise and in the tail of a per_clip that is no multiple of 4.  No atomics; a clip's bits depend neither on the
 * batch, nor on the grid, nor on which of the two paths ran.  noisy / sample / noise_out must not overlap the inputs. */
int ctrlv_train_assemble(const float* target, const float* noise, const float* sigmas, const float* image_mask,
                         const float* cond_frames, const float* cond_image, int layout, int K, int n, int F, int L, int h, int w,
                         uint64_t seed, uint32_t clip0, uint32_t call, float* noisy, void* sample, int sample_dtype,
                         float* noise_out, ctrlv_stream_t stream);

/* One training batch.  Clear the struct before setting fields.  Device pointers; h = height / 8, w = width / 8, L = the VAE's
 * latent channels, D = the CLIP plan's projection_dim. */
typedef struct ctrlv_train_batch_request {
  int32_t n_clips, num_frames, height, width;   /* clips (<= 4096), frames per clip (<= 32), pixels (what the VAE plan takes) */
  const void* clips;             /* (n, F, 3, H, W) pixels in [-1, 1] */
  const void* box_frames;        /* the same shape: required for modes 0 and 2, NULL for mode 1 */
  int32_t clips_dtype, box_dtype;      /* dtype codes (0 fp32, 1 fp16, 2 bf16) */
  int32_t mode;                  /* 0 ControlNet step, 1 stage-1 UNet step, 2 box-predictor step */
  int32_t num_cond_frames;       /* K of mode 2, 0 <= K <= F (the other modes ignore it) */
  double dropout_prob;           /* conditioning_dropout_prob; negative: none */
  uint64_t seed;
  uint32_t clip_index0;          /* clip i draws as clip clip_index0 + i */
  uint32_t call;                 /* the optimisation step */
  const float* sigma_table;      /* DEVICE fp32 [table_size] */
  const float* timestep_table;
  int32_t table_size;            /* T, 1 .. 65536 */
  float scaling_factor;          /* of the target latents; 0: the VAE plan's */
  float clip_mean[3], clip_std[3];     /* all six zero = CLIP's own values */
  int32_t sample_dtype;          /* 0 fp32, or the library's element code */
  int32_t reserved;              /* must be 0 */
  float* target_latents;         /* fp32 (n, F, L, h, w) */
  float* noisy_latents;          /* fp32 (n, F, L, h, w) */
  void* sample;                  /* (n, F, 2 L, h, w) of sample_dtype */
  float* control_cond;           /* fp32 (n, F, L, h, w): mode 0 only (required there, NULL elsewhere) */
  void* encoder_hidden_states;   /* (n, 1, D) elements */
  float* sigmas;                 /* fp32 (n) */
  float* timesteps;              /* fp32 (n) */
  int32_t* indices;              /* int32 (n) */
  float* random_p;               /* fp32 (n) */
  float* noise;                  /* fp32 (n, F, L, h, w), or NULL */
} ctrlv_train_batch_request;
/* Bytes of workspace ctrlv_train_batch_prepare needs for `r`; 0 for a request the call would refuse, or plans without weights
 * (ctrlv_last_error). */
size_t ctrlv_train_batch_workspace_bytes(ctrlv_vae_plan* vae, ctrlv_clip_plan* clip, const ctrlv_train_batch_request* r);
/* The batch, enqueued on `stream` in this order (img = clips[:, 0] as fp32 (n, 3, H, W), one gather kernel in front):
 *   1. ctrlv_resize_antialias_clamped of img to the CLIP plan's image_size in the element type, ctrlv_clip_forward
 *   2. ctrlv_train_draws(seed, clip_index0, call) into indices / sigmas / timesteps / random_p
 *   3. encoder_hidden_states = rne_el(prompt_keep * embeds)
 *   4. / 5. per encoded tensor, ctrlv_randn(seed, clip_index0, call, stream_id, n, per_clip = its latents per clip, scale 1,
 *      round_dtype 0, fp32) as the `noise` of one ctrlv_vae_encode with fp32 latents out:
 *        mode 0: target = clips (stream 4, scale scaling_factor), image = img (5, scale 1), control_cond = box_frames (6, scale 1)
 *        mode 1: target and image as in mode 0
 *        mode 2: cond_frames = box_frames (stream 4, scale 1) -- encoded once, as the reference reuses one sample
 *                (train_video_diffusion.py:442-460) --, target = cond_frames * scaling_factor (one fp32 multiply), image as above
 *   6. ctrlv_train_assemble with in-kernel noise (stream 3): layout 0, or for mode 2 layout 1 with K = num_cond_frames
 * No host synchronisation and no host-device copy after the first launch.  Every field and size is refused by name on the host
 * before the first launch: reserved != 0, a mode outside 0 .. 2, NULL tables or table_size outside 1 .. 65536, num_cond_frames
 * outside [0, F], box_frames missing (modes 0, 2) or set (mode 1), control_cond missing (mode 0) or set, NULL outputs, dtype codes,
 * a geometry the VAE or the resize refuses, plans on two devices or with other than 3 image channels; `ws` (256-byte aligned, caller-owned) too small:
 * CTRLV_E_WORKSPACE -- against the driver's own buffers first (host arithmetic on the plans' configurations), then against
 * ctrlv_train_batch_workspace_bytes (plans with weights).  The bits are those of the calls made by hand.  The CLIP phase and the
 * VAE phase alias one region of the workspace.  The plans are borrowed; not thread-safe on one pair of plans. */
int ctrlv_train_batch_prepare(ctrlv_vae_plan* vae, ctrlv_clip_plan* clip, const ctrlv_train_batch_request* r, void* ws,
                              size_t ws_bytes, ctrlv_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Optimiser pass of the training steps (csrc/optim.hip): replaces torch.optim.AdamW's per-tensor launches
 * (tools/train_video_diffusion.py:196-201) and diffusers' EMAModel.step (:550) for parameters kept in ONE flat fp32 buffer.
 *
 * ctrlv_adamw_step: torch.optim.AdamW with amsgrad=False, maximize=False over n elements, in torch's operation order:
 *     g *= grad_scale (in registers);  p *= 1 - lr*weight_decay;  m = beta1*m + (1-beta1)*g;  v = beta2*v + (1-beta2)*g*g;
 *     p -= (lr/bias1) * m / (sqrt(v)/sqrt(bias2) + eps)
 * each operation rounded as torch's single-tensor path rounds it on the device (m as lerp(m, g, 1 - beta1), v as
 * fma(1 - beta2, g*g, beta2*v), the division by sqrt(bias2) as a product with its fp32 reciprocal, the last line as one fma).
 * bias1 = 1 - beta1^t and bias2 = 1 - beta2^t are computed by the host in double; they arrive as fp32, so the entry point
 * recovers t from them and recomputes both in double (a value not of that form is used as given).  With ema != NULL the same pass then does
 * ema -= (1 - ema_decay) * (ema - p) on the new p (diffusers' form, applied after optimizer.step()); the result equals
 * ctrlv_adamw_step(ema = NULL) followed by ctrlv_ema_step bit for bit.  All buffers are fp32, contiguous and 16-byte aligned;
 * nothing at or past element n is read or written; an all-zero element (alignment padding of a flat layout) stays all-zero.
 * One pass, no atomics: the same bits in every run.  Buffers above 2^30 elements are split into launches of 2^30.
 * Refused on the host (CTRLV_E_BAD_ARG; n == 0: CTRLV_E_BAD_SHAPE): NULL p / g / m / v, a misaligned base, a non-finite lr,
 * weight_decay or grad_scale, a beta outside [0, 1), eps <= 0, bias1 / bias2 outside (0, 1], with ema an ema_decay outside [0, 1].
 * The code is the same in both element libraries.  Additive: the ABI number does not move. */
int ctrlv_adamw_step(float* p, const float* g, float* m, float* v, float* ema, size_t n, float lr, float beta1, float beta2,
                     float eps, float weight_decay, float bias1, float bias2, float grad_scale, float ema_decay,
                     ctrlv_stream_t stream);
/* ema -= (1 - decay) * (ema - p) over n fp32 elements: the last line of ctrlv_adamw_step alone (same refusals). */
int ctrlv_ema_step(float* ema, const float* p, size_t n, float decay, ctrlv_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Global gradient-norm clipping on the device, fused into the AdamW pass (csrc/optim.hip): what
 * `accelerator.clip_grad_norm_(params, max_grad_norm)` in front of `optimizer.step()` does, without a second pass over the
 * gradients and without a host read.  Three stages on one stream; the record stays on the device.
 *
 * The device record.  16 bytes, 16-byte aligned, zero-initialised by the caller once (skipped_total is a running count). */
typedef struct ctrlv_grad_state {
  float norm;            /* fp32(|grad_scale| * sqrt(S)), S the fp64 sum of squares: rounded ONCE, from double */
  float coef;            /* clamp(max_norm / (norm + 1e-6f), max = 1), torch's clip_grad_norm_ formula with the add and ONE
                          * correctly rounded divide in fp32: what fp32 tensors give on the device (with max_norm as a Python
                          * scalar torch divides as reciprocal() * max_norm, which can differ in the last bit).  A NaN norm
                          * gives NaN, as there; 1 when max_norm is +inf */
  int32_t skip;          /* 1 when norm is not finite (a NaN or inf element, or S beyond fp32 after the scale), else 0 */
  int32_t skipped_total; /* += skip on every ctrlv_grad_finish */
} ctrlv_grad_state;

/* Stage 1.  Slots of `partials` that ctrlv_grad_sumsq fills for n elements: one per block of 4096 elements,
 * ceil(n / 4096).  A function of n alone -- not of the device, its CU count or the environment: the same partition, and so the same
 * bits, everywhere. */
size_t ctrlv_grad_sumsq_partials(size_t n);
/* partials[slot0 + b] = sum of (double)g[i] * (double)g[i] (each product exact) over block b = [4096 b, min(n, 4096 (b + 1))),
 * added in fp64 in a fixed order (per lane in element order, then a fixed tree over the workgroup).  No atomics: the same bits in
 * every run.  g (fp32, 16-byte aligned) is read once, with 16-byte loads and a scalar tail for n % 4, and never written;
 * nothing at or past element n is read; exactly the slots [slot0, slot0 + ctrlv_grad_sumsq_partials(n)) are written, so the runs
 * of several parameter groups fill one array.  Refused on the host (CTRLV_E_BAD_ARG; n == 0: CTRLV_E_BAD_SHAPE): NULL or
 * misaligned g, NULL or 8-byte-misaligned partials, a slot range that ends beyond partials_len. */
int ctrlv_grad_sumsq(const float* g, size_t n, double* partials, size_t partials_len, size_t slot0, ctrlv_stream_t stream);
/* Stage 2, one workgroup.  S = partials[0] + ... + partials[count - 1] in fp64 in a fixed order (lane l of 1024 adds slots
 * l, l + 1024, ... in index order, then a fixed tree), then the record as its fields say.  grad_scale is the multiplier the
 * step applies to the gradients (the norm is that of the scaled gradients); max_norm = +inf asks for the norm and the skip flag
 * without clipping.  Refused on the host: NULL / misaligned pointers, count == 0 (CTRLV_E_BAD_SHAPE), max_norm that is not
 * positive or is NaN, a grad_scale that is not finite. */
int ctrlv_grad_finish(const double* partials, size_t count, float grad_scale, float max_norm, ctrlv_grad_state* state,
                      ctrlv_stream_t stream);
/* Stage 3.  ctrlv_adamw_step with the gradient taken as (g * grad_scale) * state->coef -- two fp32 multiplications in that order,
 * as an unscale followed by torch's mul_(clip_coef) -- and every constant derived on the host exactly as there.  state->skip
 * set: nothing is written to p, m or v (g, m and v are not even read); with ema != NULL the shadow is still updated against the
 * UNCHANGED p, bit for bit what ctrlv_ema_step gives (`ema.step()` after a skipped `optimizer.step()`).  With coef = 1 and
 * skip = 0 the result equals ctrlv_adamw_step's bit for bit.  coef and skip are read from device memory by the kernel: no host
 * synchronisation.  Same refusals as ctrlv_adamw_step, plus a NULL or misaligned state. */
int ctrlv_adamw_step_dev(float* p, const float* g, float* m, float* v, float* ema, size_t n, float lr, float beta1, float beta2,
                         float eps, float weight_decay, float bias1, float bias2, float grad_scale, float ema_decay,
                         const ctrlv_grad_state* state, ctrlv_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Dynamic loss scaling on the device (csrc/optim.hip): what accelerate's GradScaler does around the backward of a step under
 * --mixed_precision fp16 -- unscale, found-inf check, skipped step, scale update (torch's _amp_update_scale_) -- inside the
 * three stages above, without a host read.  The scale lives in a second device record that updates itself.
 *
 * The record.  32 bytes, 16-byte aligned, initialised by the host once (scale, growth_interval, the two factors; the rest 0). */
typedef struct ctrlv_loss_scale_state {
  float scale;            /* multiplier of the NEXT backward's loss */
  float unscale;          /* what THIS step multiplies gradients by: fp32(host grad_scale * fp32(1.0 / (double)scale)),
                             scale taken before the update -- torch: _scale.double().reciprocal().float() */
  int32_t growth_tracker; /* consecutive unskipped steps since the last change of scale */
  int32_t growth_interval;
  float growth_factor, backoff_factor; /* fp32: torch keeps Python doubles; 2 and 0.5 (any fp32 number) behave identically */
  int32_t reserved[2];
} ctrlv_loss_scale_state;

/* Stage 2 under a loss scale: ctrlv_grad_finish with the multiplier formed ON THE DEVICE, unscale = grad_scale * fp32(1 / (double)
 * ls->scale) (one fp32 product; grad_scale is the host's multiplier, e.g. 1 / accumulation steps).  Writes ls->unscale, then norm,
 * coef, skip and skipped_total of `state` exactly as ctrlv_grad_finish does with grad_scale = unscale: one workgroup, the same
 * summation order, so the norm is bit-identical given the same multiplier.  The same thread then applies torch's
 * _amp_update_scale_: on skip scale *= backoff_factor and growth_tracker = 0; otherwise, when growth_tracker + 1 == growth_interval,
 * scale *= growth_factor if that product is finite, and growth_tracker = 0; otherwise growth_tracker += 1.  The record is validated
 * on the device: a scale that is not positive and finite sets skip (unscale, and so norm, are NaN) and leaves scale and
 * growth_tracker alone.  Refused on the host: what ctrlv_grad_finish refuses, plus a NULL or misaligned ls. */
int ctrlv_grad_finish_scaled(const double* partials, size_t count, float grad_scale, float max_norm, ctrlv_loss_scale_state* ls,
                             ctrlv_grad_state* state, ctrlv_stream_t stream);
/* Stage 3 under a loss scale: ctrlv_adamw_step_dev with the gradient taken as (g * ls->unscale) * state->coef, two fp32
 * multiplications in that order; ls->unscale == grad_scale gives ctrlv_adamw_step_dev's bits.  Skip and EMA-on-skip as there.
 * g is NEVER written: the gradient buffer keeps the SCALED gradients (unlike after torch's unscale_).  Same refusals as
 * ctrlv_adamw_step (without grad_scale), plus a NULL or misaligned ls or state. */
int ctrlv_adamw_step_scaled(float* p, const float* g, float* m, float* v, float* ema, size_t n, float lr, float beta1, float beta2,
                            float eps, float weight_decay, float bias1, float bias2, float ema_decay,
                            const ctrlv_loss_scale_state* ls, const ctrlv_grad_state* state, ctrlv_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Box and trajectory frames from coordinates (csrc/box_render.hip, csrc/pipeline.hip): what the reference draws on the host with
 * OpenCV (src/ctrlv/utils/plotting.py:33-124 plot_3d_bbox / plot_trajectory, called from datasets/kitti_abstract.py:220-241)
 * and then takes through Resize -> ToTensor -> Normalize(0.5, 0.5) (kitti_abstract.py:92-96).  A device table of box records goes
 * in, the conditioning frames come out.  Additive entry points: the ABI number does not change, no existing struct changes its
 * layout, no existing entry point its bits.
 *
 * THE CONTRACT IS THE INTEGER GEOMETRY STATED HERE, NOT OpenCV'S BYTES.  It follows what OpenCV's drawing does as far as that can
 * be stated without running it (an inclusive fill, a thickness-2 line as a radius-1 capsule, a saturating round-half-even
 * write-out of the 0.75 / 0.25 blend); that agreement is UNVERIFIED, and cv2's exact line rasters are out of scope.  The
 * reference's own frames are not reproducible either: its track colours come from an unseeded np.random (plotting.py:29).
 * tests/box_render_ref.py restates this section in numpy.
 *
 * The records.  Clear before setting; little-endian; both tables live on the DEVICE. */
typedef struct ctrlv_box_object { /* 64 bytes */
  int32_t x1, y1, x2, y2;         /* the 2-D box in source pixels, already truncated toward zero (the reference's int(...));
                                     either corner order */
  uint8_t fill_rgb[3], pad0;      /* the track colour, written to channels 0, 1, 2 as it stands */
  uint8_t line_rgb[3], pad1;      /* the class colour, same rule */
  int16_t corner[8][2];           /* the projected 3-D corners (x, y) in the reference's loop order (i in 1, -1; j in 1, -1; k in
                                     0, 1).  On a trajectory frame corner[0] is the centre of the discs */
  uint32_t flags;                 /* CTRLV_BOX_FILL | CTRLV_BOX_OUTLINE | CTRLV_BOX_WIRE; the kernel tests only these bits */
  int32_t reserved;               /* must be 0 */
} ctrlv_box_object;
enum { CTRLV_BOX_FILL = 1, CTRLV_BOX_OUTLINE = 2, CTRLV_BOX_WIRE = 4 };
typedef struct ctrlv_box_frame { /* 16 bytes */
  int32_t first, count;           /* frame j draws objects first .. first + count - 1 in that order */
  int32_t kind;                   /* 0: a box frame; 1: a trajectory frame (any other value is drawn as a box frame) */
  int32_t reserved;               /* must be 0 */
} ctrlv_box_frame;
/* The kernel is safe for ANY table content: no content makes a lane read outside the two tables or write outside its frame.
 *   - first outside [0, n_objects): the frame's count becomes 0.  Otherwise count becomes min(count, n_objects - first, 1024), and
 *     0 when it is negative.
 *   - every coordinate (x1 .. y2, corner) is clamped to [-8191, 8191] before use; source sizes are at most 4096 per axis.  With
 *     these limits every product below fits in int64 (the worst case is 4 (2 * 12287 * 16382)^2 < 2^63).
 *
 * The picture, in integers only, per pixel q = (x, y) and channel c.
 *   capsule(P0, P1, R4): with d = P1 - P0, e = q - P0, L = d.d, t = d.e the pixel is covered iff
 *       L == 0 or t <= 0:  4 e.e <= R4;      t >= L:  4 |q - P1|^2 <= R4;      otherwise:  4 (d x e)^2 <= R4 L.
 *     R4 = 4 is a radius-1 capsule (the "thickness 2" lines), R4 = 1 radius 1/2 ("thickness 1").  The bounds are closed.
 *   With xa = min(x1, x2), xb = max(x1, x2), ya, yb likewise:
 *     rect(o)  xa <= x <= xb and ya <= y <= yb, both corners inclusive.
 *     ring(o)  the union of the radius-1 capsules of the box's four edges: a 3-pixel band around the box without its four outermost
 *              corner pixels.
 *     wire(o)  the radius-1 capsules of corner[2i] - corner[2i+1], i = 0 .. 3, and of corner[i] - corner[(i+2) % 8], i = 0 .. 7,
 *              and the radius-1/2 capsules of corner[2] - corner[5] and corner[3] - corner[4].
 *   Box frame (kind 0).  Three layers U, T, W start at zero.  The objects are visited in order; a later object overwrites an earlier
 *   one, and all three channels are written, zeros included:
 *       OUTLINE and q in ring: U = line_rgb;      FILL and q in rect: T = fill_rgb;      WIRE and q in wire: W = line_rgb.
 *   Then per channel, as the reference's per-element masks do (plotting.py:120-123):
 *       out[c] = W[c] != 0 ? W[c] : (T[c] != 0 ? rhe((3 T[c] + U[c]) / 4) : U[c]),
 *   rhe = round-half-to-even of the exact quarter (the 0.75 / 0.25 addWeighted and its saturating write-out).
 *   Trajectory frame (kind 1).  The objects are visited in order and write directly, no blend: the closed disc
 *   |q - corner[0]|^2 <= 400 in fill_rgb, then the closed disc <= 100 in line_rgb.
 *
 * out_u8 (n_frames, 3, Hs, Ws) uint8, planar: the layout ctrlv_resize_frames_u8 takes with planes = 3 n_frames.  One workgroup
 * per 128 x 32 tile of a frame: it culls the frame's objects against the tile, compacts the survivors into LDS in table order
 * (wave ballots plus a prefix over the waves, 256 objects per round) and its lanes walk only that list, each lane owning 4
 * consecutive x of a row: per channel one 32-bit store where the address is aligned, two 16-bit or four single stores elsewhere
 * and at the right edge.  No atomics; the bytes do not depend on the grid, the tile, the pointer's
 * alignment or on how many frames share a launch.  CTRLV_E_BAD_ARG: NULL tables or output, n_objects < 0; CTRLV_E_BAD_SHAPE:
 * n_frames < 1, Hs or Ws outside [1, 4096], more than 2^31 - 1 tiles. */
int ctrlv_render_box_frames(const ctrlv_box_object* objects, int n_objects, const ctrlv_box_frame* frames, int n_frames, int Hs,
                            int Ws, void* out_u8, ctrlv_stream_t stream);
/* The conditioning frames at the working size, in order:
 *   1. ctrlv_render_box_frames at (Hs, Ws) -- into out_u8 (n_frames, 3, Hs, Ws) when it is given, else into ws;
 *   2. ctrlv_resize_frames_u8 with filter 2 (BILINEAR: what transforms.Resize does to a PIL image) to (H, W); skipped when
 *      (Hs, Ws) == (H, W) -- PIL returns a copy there;
 *   3. out = rne_el(((float) v / 255.0f - 0.5f) / 0.5f), each operation rounded in fp32 (ToTensor, then Normalize).
 * out (n_frames, 3, H, W), 16-byte aligned, out_dtype 0 (fp32, no last rounding) or the library's element code.  ws:
 * ctrlv_box_frames_cond_ws_bytes bytes, 16-byte aligned (the query is 0 for sizes the call would refuse).  Refused by name on the
 * host before any launch: what ctrlv_render_box_frames and ctrlv_resize_frames_u8 refuse, a NULL or misaligned out
 * (CTRLV_E_BAD_ARG), another out_dtype (CTRLV_E_BAD_DTYPE), ws_bytes too small (CTRLV_E_WORKSPACE). */
size_t ctrlv_box_frames_cond_ws_bytes(int n_frames, int Hs, int Ws, int H, int W);
int ctrlv_box_frames_cond(const ctrlv_box_object* objects, int n_objects, const ctrlv_box_frame* frames, int n_frames, int Hs,
                          int Ws, int H, int W, void* out, int out_dtype, void* out_u8, void* ws, size_t ws_bytes,
                          ctrlv_stream_t stream);
/* Host-only helpers for filling the tables (no GPU needed).
 * The reference's eleven-entry class palette (plotting.py:30 TYPE_LOOKUP) in its order, the three numbers of an entry as they
 * stand there.  An id outside [0, 11) is CTRLV_E_BAD_ARG. */
int ctrlv_box_class_color(int id, uint8_t* rgb);
/* A track's colour as a function of (seed, track_id): one Philox4x32-10 block under ctrlv_randn's key rule, counter
 * ((uint32) track_id, (uint32) (track_id >> 32), 7, 0) -> x0 .. x3; rgb[c] = 50 + (uint8) (((uint64) x_c * 205) >> 32), the
 * reference's range [50, 254] -- and the same colour for the same track in every frame and run, which the reference does not give. */
int ctrlv_box_track_color(uint64_t seed, int64_t track_id, uint8_t* rgb);
/* The eight projected corners of a 3-D box, in double as plotting.py:81-95 computes them.  cam_to_img: row-major (3, cols), cols 3
 * or 4; location (x, y, z); dimensions (h, w, l); for (i in 1, -1) (j in 1, -1) (k in 0, 1):
 *     px = x + i w / 2 cos(-rot_y + pi / 2) + (j i) l / 2 cos(-rot_y);  pz = z + i w / 2 sin(-rot_y + pi / 2) + (j i) l / 2 sin(-rot_y);
 *     py = y - k h;   v = cam_to_img . (px, py, pz[, 1]);   (u0, u1) = (v0, v1) / (|v2| > 1e-4 ? v2 : 1e-4),
 * each product and sum in the order written there.  corners[8][2] = (u0, u1) truncated toward zero, then clamped to
 * [-8191, 8191] (a NaN becomes 0).  CTRLV_E_BAD_ARG: NULL pointers; CTRLV_E_BAD_SHAPE: cols not 3 or 4. */
int ctrlv_box_project_corners(const double* cam_to_img, int cols, const double* location, const double* dimensions, double rot_y,
                              int16_t* corners);
/* The tables of one ctrlv_pipeline_generate_from_boxes call.  Clear the struct before setting fields. */
typedef struct ctrlv_box_render_request {
  const ctrlv_box_object* objects;  /* DEVICE, n_objects records */
  const ctrlv_box_frame* frames;    /* DEVICE, n_frames records: frame f of clip i is record i * num_frames + f */
  int32_t n_objects, n_frames;      /* n_frames must equal n_clips * num_frames of the clip request */
  int32_t src_height, src_width;    /* (Hs, Ws) */
  int32_t reserved[2];              /* must be 0 */
} ctrlv_box_render_request;
/* 0 for a request the call would refuse (ctrlv_last_error). */
size_t ctrlv_pipeline_from_boxes_workspace_bytes(ctrlv_pipeline* p, const ctrlv_clip_request* r, const ctrlv_box_render_request* b);
/* ctrlv_box_frames_cond of `b` to (height, width) of `r` in the element type, into the workspace; then exactly
 * ctrlv_pipeline_generate on `r` with that buffer as cond, cond_channels = 3: the bits of the two calls made by hand.  Refused by
 * name before any launch: r->cond set (CTRLV_E_BAD_ARG: the driver supplies it), a pipeline without a ControlNet, reserved != 0,
 * n_frames != n_clips * num_frames (CTRLV_E_BAD_SHAPE), and whatever the two calls refuse.  A trajectory frame is a record with
 * kind = 1 (the reference's if_last_frame_trajectory at inference: frame num_frames - 1). */
int ctrlv_pipeline_generate_from_boxes(ctrlv_pipeline* p, const ctrlv_clip_request* r, const ctrlv_box_render_request* b, void* ws,
                                       size_t ws_bytes, ctrlv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CTRLV_HIP_H */
