// Internal launchers of csrc/pipeline_io.hip that only the clip driver (csrc/pipeline.hip) calls: the classifier-free-guidance
// assembly and the two fp32 -> element conversions around the loop.  Not part of the C ABI.
#pragma once
#include "common.h"

// dst [(cfg ? 2 : 1) B][per] elements: the conditional half (the second one with cfg) = src [B][per] of dtype 0 / 1 / 2 rounded
// to the element type, the unconditional half (first) = exact zeros -- torch.cat([zeros_like(x), x]).
int ctrlv_pio_cfg_double(const void* src, int src_dtype, void* dst, int B, long per, int cfg, hipStream_t s);
// The conditioning channels [c_lat, 2 c_lat) of the model input lmi [(cfg ? 2 : 1) B][F][2 c_lat][hw]: first [B][c_lat][hw]
// (elements) repeated over the F frames in the conditional half, zeros in the unconditional one.
int ctrlv_pio_lmi_cond(const void* first, void* lmi, int B, int F, int c_lat, int hw, int cfg, hipStream_t s);
// The box predictor's overwrite (pipeline_video_diffusion.py:200-206), after ctrlv_pio_lmi_cond: in the conditional half of lmi
// the conditioning channels of frames [0, K) and F - 1 of every clip = src rounded to the element type.  src (dtype 0 / 1 / 2)
// holds src_frames frames of [c_lat][hw] per clip: all F of them (compact = 0), or only the min(K + 1, F) taken ones in order
// (compact = 1).  The unconditional half is not touched: it stays zero.
int ctrlv_pio_lmi_boxes(const void* src, int src_dtype, int src_frames, int compact, void* lmi, int B, int F, int K, int c_lat,
                        int hw, int cfg, hipStream_t s);
// x [n] elements = clamp(x, -1, 1) in place: torch.clamp(frames, -1, 1) of pipeline_video_diffusion.py:297.
int ctrlv_pio_clamp_frames(void* x, long n, hipStream_t s);
// Channels [0, c_lat) of both halves of lmi = scaled [B][F][c_lat][hw] (elements): DenoiseStepper.step's two slice copies.
int ctrlv_pio_lmi_scatter(const void* scaled, void* lmi, int B, int F, int c_lat, int hw, int cfg, hipStream_t s);
// out [n] = x [n] (fp32 copy; skipped when out == x) and scaled [n] = rne_el(x [n] * inv): DenoiseStepper.set_latents.
int ctrlv_pio_scale_latents(const float* x, float* out, void* scaled, long n, float inv, hipStream_t s);
// z [n] = rne_el(rne_el(x [n]) * inv): `1 / scaling_factor * latents.to(vae.dtype)` of decode_latents.
int ctrlv_pio_decode_input(const float* x, void* z, long n, float inv, hipStream_t s);
// Host-side validation of one ctrlv_resize_antialias call (the driver refuses a request before its first launch).
int ctrlv_resize_check(int n, int H, int W, int h, int w);
// Host-side validation of one ctrlv_resize_lanczos_u8 call (ctrlv_pipeline_prepare refuses a request before its first launch).
int ctrlv_resize_lanczos_check(int n, int H, int W, int h, int w);
