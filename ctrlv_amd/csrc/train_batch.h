// Internal launchers of csrc/train_batch.hip that only the batch driver (csrc/train_batch_plan.hip) calls.  Not part of the C ABI.
#pragma once
#include "common.h"

// dst fp32 (n, per) = frame 0 of every clip of src (n, F, per) of dtype 0 / 1 / 2: `clips[:, 0].float()`.
int ctrlv_tb_first_frames(const void* src, int dtype, int n, int F, long per, float* dst, hipStream_t s);
// out (n, D) elements = rne_el(keep[i] * emb[i, d]): the prompt half of the conditioning dropout.
int ctrlv_tb_keep_rows(const void* emb, const float* keep, int n, int D, void* out, hipStream_t s);
// out [count] = x [count] * scale, one fp32 multiply (the box predictor's target from its unscaled sample).
int ctrlv_tb_scale(const float* x, float scale, long count, float* out, hipStream_t s);
// Host-side validation of one ctrlv_train_assemble geometry (the driver refuses a request before its first launch).
int ctrlv_train_assemble_check(int layout, int K, int n, int F, int L, int h, int w);
