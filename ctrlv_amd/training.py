"""cfg5: one training step of the ControlNet on the HIP kernels (reference: tools/train_video_controlnet.py:366-488).
Stage 1 of Ctrl-V (fine-tuning the UNet itself, tools/train_video_diffusion.py:459-541) is `unet_train_step` below: the
same blocks with the UNet's encoder, mid block and tail trainable as well.  The third script, the VAE decoder fine-tuning
(tools/train_vae_finetuning.py:303-320), is `vae_train_step` at the end of this file.

    ControlNet forward (trainable, fp32 master parameters, bf16 compute)
    -> frozen UNet forward: encoder + mid on the inference executor (no gradients flow there: the residuals join the skip
       tensors AFTER the down path, unet_spatio_temporal_condition.py:119-137), decoder in training mode (dgrad only)
    -> EDM-preconditioned MSE (train_video_controlnet.py:468-478) -> backward -> AdamW (torch.optim on the fp32 masters).
The compute type is bf16 unless a step is called with compute_dtype=torch.float16 (the reference's --mixed_precision fp16), then
usually with a `ctrlv_amd.optim.LossScaler`, whose scale is read and updated on the device inside the optimiser's launches.

Everything activation-sized runs in the kernels of libctrlv_hip.so through ctrlv_amd.autograd; the per-clip vectors (time
and added-id embeddings, time_emb_proj, the one-key cross-attention vectors, the frame positional embedding MLP) are
plain fp32 torch ops on [B, 1280]-sized tensors.  Multi-GPU: `GradientBuckets` all-reduces flat fp32 buckets (25 MB, the
reference's DDP default) over torch.distributed WHILE the backward pass runs (hooks fire as gradients complete);
`allreduce_gradients` is the simple reduce-after-backward form (RCCL on the GPU box, gloo in the CPU tests).
"""
import contextlib
import math

import torch
import torch.distributed as dist
import torch.nn.functional as Fn

from . import ops
from . import optim as _optim
from .autograd import (GroupNormSiLU, TimeConvOut, f32, gemm, gradient_checkpointing, prefetch_mix_factors,
                       res_block_train_forward, sinusoid, transformer_train_forward, vae_attention_train_forward,
                       vae_res_block_train_forward, zero_conv_train_forward)
from .models.blocks import TransformerSpatioTemporalModel  # noqa: F401  (documentation anchor)


# ------------------------------------------------------------------------------------------------- embeddings
def clip_embeddings(model, timestep, added_time_ids, B, device):
    """silu(time_embedding(t) + add_embedding(ids)) -> fp32 [B, 1280] (controlnet.py:262-286); torch autograd."""
    boc0 = model.conv_in.weight.shape[0]
    t = timestep if torch.is_tensor(timestep) else torch.tensor(float(timestep))
    t = t.to(device=device, dtype=torch.float32).reshape(-1)
    if t.numel() == 1:
        t = t.expand(B)

    def mlp(e, x):
        return Fn.linear(Fn.silu(Fn.linear(x, f32(e.linear_1.weight), f32(e.linear_1.bias))),
                         f32(e.linear_2.weight), f32(e.linear_2.bias))

    emb = mlp(model.time_embedding, sinusoid(t, boc0))
    ids = added_time_ids.to(device=device, dtype=torch.float32)
    add_dim = model.config.addition_time_embed_dim
    aug = mlp(model.add_embedding, sinusoid(ids.reshape(-1), add_dim).reshape(B, -1))
    return Fn.silu(emb + aug)


def _temb_tables(block, emb_s):
    return [Fn.linear(emb_s, f32(m.time_emb_proj.weight), f32(m.time_emb_proj.bias)).contiguous()
            for m in (block.spatial_res_block, block.temporal_res_block)]


# ------------------------------------------------------------------------------------------------- blocks
def _res(block, x, emb_s, B, F, H, W):
    return res_block_train_forward(block, x, _temb_tables(block, emb_s), B, F, H, W)


def _conv(conv, x, H, W, Ho, Wo, stride, up):
    return gemm(x, conv.weight, conv.bias, mode=1, conv=(H, W, Ho, Wo, stride, up))


def down_block_train(blk, x, emb_s, ehs, B, F, H, W, order):
    taps = []
    attns = getattr(blk, "attentions", None)
    for i, resnet in enumerate(blk.resnets):
        x = _res(resnet, x, emb_s, B, F, H, W)
        if attns is not None:
            x = transformer_train_forward(attns[i], x, ehs, B, F, H, W, order)
        taps.append((x, H, W))
    if blk.downsamplers is not None:
        Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
        x = _conv(blk.downsamplers[0].conv, x, H, W, Ho, Wo, 2, 0)
        H, W = Ho, Wo
        taps.append((x, H, W))
    return x, H, W, taps


def mid_block_train(blk, x, emb_s, ehs, B, F, H, W, order):
    x = _res(blk.resnets[0], x, emb_s, B, F, H, W)
    for attn, resnet in zip(blk.attentions, blk.resnets[1:]):
        x = transformer_train_forward(attn, x, ehs, B, F, H, W, order)
        x = _res(resnet, x, emb_s, B, F, H, W)
    return x


def up_block_train(blk, x, emb_s, ehs, B, F, H, W, skips, order):
    attns = getattr(blk, "attentions", None)
    for i, resnet in enumerate(blk.resnets):
        x = torch.cat([x, skips.pop()], dim=1)               # unet_3d_blocks: torch.cat([hidden, skip], dim=1)
        x = _res(resnet, x, emb_s, B, F, H, W)
        if attns is not None:
            x = transformer_train_forward(attns[i], x, ehs, B, F, H, W, order)
    if blk.upsamplers is not None:
        x = _conv(blk.upsamplers[0].conv, x, H, W, 2 * H, 2 * W, 1, 1)
        H, W = 2 * H, 2 * W
    return x, H, W


# ------------------------------------------------------------------------------------------------- models
def _element_dtype(compute_dtype):
    """The element type of a step's activations: None is torch.bfloat16 (the default route), else bf16 or fp16."""
    if compute_dtype is None:
        return torch.bfloat16
    if compute_dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f"compute_dtype must be torch.bfloat16 or torch.float16 (None: bfloat16), not {compute_dtype}")
    return compute_dtype


def _input_cols(planes, N, h, w, cp, kp, device):
    """NCHW planes -> channels-last rows [M, cp] -> im2col [M, kp] (the tiny-channel input convs run as ONE GEMM), in the
    element type of the planes (fp32 planes: bf16)."""
    M = N * h * w
    el = planes[0].dtype if planes[0].dtype in (torch.bfloat16, torch.float16) else torch.bfloat16
    x16 = torch.zeros(M, cp, dtype=el, device=device)
    off = 0
    for p in planes:
        ops.nchw_to_rows(p.contiguous(), x16, off)
        off += p.shape[1]
    col = torch.empty(M, kp, dtype=el, device=device)
    ops.im2col3x3(x16, N, h, w, col)
    return col


def _input_conv_weight(convs, cp, kp):
    """[N, kp] im2col weight of conv_in (+ control_conv_in) built with differentiable torch ops (packing.pack_conv_in)."""
    n = convs[0].weight.shape[0]
    w = torch.cat([c.weight for c in convs], dim=1)                                   # [N, sum C, 3, 3]
    w = Fn.pad(w.permute(0, 2, 3, 1), (0, cp - w.shape[1]))                           # [N, 3, 3, cp]
    w = Fn.pad(w.reshape(n, 9 * cp), (0, kp - 9 * cp))
    b = sum(c.bias for c in convs)
    return w, b


def _encoder_train(model, planes, timestep, encoder_hidden_states, added_time_ids, B, F):
    """The encoder side the ControlNet and the trainable UNet share: NCHW input planes -> im2col -> the input conv(s) as ONE
    GEMM -> down blocks -> mid block, GEGLU feed-forwards checkpointed if the model asks for it
    (`enable_gradient_checkpointing()`, tools/train_video_controlnet.py:185-186).  Returns (mid rows, H, W, taps, emb_s,
    ehs); taps: (rows [N*H*W, C] bf16, H, W) in the order of `down_block_res_samples`."""
    N, (h, w), dev = B * F, planes[0].shape[2:], planes[0].device
    order = model.time_context_order
    emb_s = clip_embeddings(model, timestep, added_time_ids, B, dev)
    ehs = encoder_hidden_states.reshape(B, -1).float()
    convs = [model.conv_in] + model._extra_input_convs()
    cp = (sum(c.weight.shape[1] for c in convs) + 7) // 8 * 8
    kp = (9 * cp + 63) // 64 * 64
    col = _input_cols(planes, N, h, w, cp, kp, dev)
    wi, bi = _input_conv_weight(convs, cp, kp)
    x = gemm(col, wi, bi)
    taps, H, W = [(x, h, w)], h, w
    with gradient_checkpointing(getattr(model, "gradient_checkpointing", False)):
        for blk in model.down_blocks:
            x, H, W, t = down_block_train(blk, x, emb_s, ehs, B, F, H, W, order)
            taps += t
        x = mid_block_train(model.mid_block, x, emb_s, ehs, B, F, H, W, order)
    return x, H, W, taps, emb_s, ehs


def _unet_tail(unet, x, N, H, W):
    """conv_norm_out + SiLU + conv_out -> the prediction as channels-last rows [N*H*W, out_channels] (bf16)."""
    xn = GroupNormSiLU.apply(x, unet.conv_norm_out.weight, unet.conv_norm_out.bias, N, H * W, 1, 1e-5, True)
    return gemm(xn, unet.conv_out.weight, unet.conv_out.bias, mode=1, conv=(H, W, H, W, 1, 0))


def controlnet_train_forward(model, sample, timestep, encoder_hidden_states, added_time_ids, control_cond,
                             conditioning_scale=1.0):
    """`ControlNetModel.forward` (controlnet.py:226-351) with gradients.  Returns (down, mid): lists of
    (rows [N*H*W, C] bf16, H, W) in the order of `down_block_res_samples`, and the mid tuple."""
    B, F, Cin, h, w = sample.shape
    planes = [sample.reshape(B * F, Cin, h, w), control_cond.reshape(B * F, -1, h, w).to(sample.device)]
    x, H, W, taps, _, _ = _encoder_train(model, planes, timestep, encoder_hidden_states, added_time_ids, B, F)
    down = [(zero_conv_train_forward(zc, r, conditioning_scale), hh, ww)
            for (r, hh, ww), zc in zip(taps, model.controlnet_down_blocks)]
    mid = (zero_conv_train_forward(model.controlnet_mid_block, x, conditioning_scale), H, W)
    return down, mid


@contextlib.contextmanager
def _element_feed_forwards(model):
    """A training walk does not use the FP8 feed-forward mode (ff_dtype "f8" is an inference mode): the frozen encoder of a
    training step runs its feed-forwards in the element type whatever the attribute says."""
    had = "ff_dtype" in model.__dict__
    prev = model.__dict__.get("ff_dtype")
    model.__dict__["ff_dtype"] = "same"
    try:
        yield
    finally:
        if had:
            model.__dict__["ff_dtype"] = prev
        else:
            del model.__dict__["ff_dtype"]


def unet_train_forward(unet, sample, timestep, encoder_hidden_states, added_time_ids, down_res, mid_res):
    """Frozen-UNet forward that is differentiable w.r.t. the ControlNet residuals.  Encoder + mid run on the inference
    executor under no_grad (no gradient path: the residuals are added to its OUTPUTS); the decoder runs in training
    mode.  Returns the model prediction as channels-last rows [B*F*h*w, out_channels] (bf16)."""
    B, F, Cin, h, w = sample.shape
    N, dev = B * F, sample.device
    order = unet.time_context_order
    with torch.no_grad(), _element_feed_forwards(unet):
        if unet._use_plan():
            # the library-owned C++ plan walks the frozen encoder (ctrlv_unet_encoder_forward): one host call
            plan = unet._ensure_plan(sample)
            t32, ehs_p, ids32 = unet._plan_inputs(sample, timestep, encoder_hidden_states, added_time_ids)
            shapes = [plan.residual_shape(i, B, F, h, w) for i in range(plan.n_down + 1)]
            rows = [torch.empty(M, C, dtype=sample.dtype, device=dev) for M, C in shapes]
            plan.unet_encoder_forward(sample.contiguous(), t32, ehs_p, ids32, rows[:-1], rows[-1])
            hw = [(h, w)]
            for M, _ in shapes[1:]:
                hh, ww = hw[-1]
                while hh * ww * N != M:
                    hh, ww = (hh + 2 - 3) // 2 + 1, (ww + 2 - 3) // 2 + 1
                hw.append((hh, ww))
            taps = [(r, a, b) for r, (a, b) in zip(rows[:-1], hw[:-1])]
            x, (H, W) = rows[-1], hw[-1]
        else:                        # per-op executor (profiling / tracing modes)
            ws = unet._ensure_ready(sample)
            ctx = unet._context(ws, sample, timestep, encoder_hidden_states, added_time_ids)
            x = unet._input_rows(ws, [sample.reshape(N, Cin, h, w)], N, h, w)
            x, H, W, taps = unet._run_down_mid(ctx, x, h, w)
        emb_s = clip_embeddings(unet, timestep, added_time_ids, B, dev)
    ehs = encoder_hidden_states.reshape(B, -1).float()
    if len(down_res) != len(taps):
        raise ValueError(f"expected {len(taps)} down_block_additional_residuals, got {len(down_res)}")
    skips = [s + r for (s, _, _), (r, _, _) in zip(taps, down_res)]            # :119-127 (out of place: s is arena memory)
    x = x + mid_res[0]                                                         # :136-137
    with gradient_checkpointing(getattr(unet, "gradient_checkpointing", False)):
        for blk in unet.up_blocks:
            x, H, W = up_block_train(blk, x, emb_s, ehs, B, F, H, W, skips, order)
    return _unet_tail(unet, x, N, H, W)


def unet_full_train_forward(unet, sample, timestep, encoder_hidden_states, added_time_ids):
    """`UNetSpatioTemporalConditionModel.forward` (no ControlNet residuals) with gradients for every parameter that
    requires them: the stage-1 forward of tools/train_video_diffusion.py:519-531.  The encoder and mid block run the
    ControlNet's trainable blocks (the ControlNet is a copy of this encoder), their taps feed the decoder's skip concat --
    autograd adds the two gradients of each tap.  Returns the prediction as channels-last rows [B*F*h*w, out_channels]."""
    B, F, Cin, h, w = sample.shape
    x, H, W, taps, emb_s, ehs = _encoder_train(unet, [sample.reshape(B * F, Cin, h, w)], timestep, encoder_hidden_states,
                                               added_time_ids, B, F)
    skips = [t[0] for t in taps]
    with gradient_checkpointing(getattr(unet, "gradient_checkpointing", False)):
        for blk in unet.up_blocks:
            x, H, W = up_block_train(blk, x, emb_s, ehs, B, F, H, W, skips, unet.time_context_order)
    return _unet_tail(unet, x, B * F, H, W)


# ------------------------------------------------------------------------------------------------- loss / step
def rows_of(x5):
    """(B, F, C, h, w) -> channels-last rows [B*F*h*w, C] (torch permute: tiny latent tensors)."""
    B, F, C, h, w = x5.shape
    return x5.permute(0, 1, 3, 4, 2).reshape(B * F * h * w, C)


def edm_loss(pred_rows, noisy_latents, target_latents, sigmas):
    """train_video_controlnet.py:468-478: denoised = c_out * pred + c_skip * noisy, weighting (1 + s^2) / s^2, mean over
    everything but the batch, then over the batch.  latents (B, F, 4, h, w) fp32; sigmas [B]."""
    B = noisy_latents.shape[0]
    per = noisy_latents[0].numel()
    s = sigmas.float().reshape(B, 1).repeat_interleave(per // noisy_latents.shape[2], 0)          # one per row
    c_out, c_skip = -s / (s * s + 1) ** 0.5, 1.0 / (s * s + 1)
    den = pred_rows.float() * c_out + c_skip * rows_of(noisy_latents).float()
    wgt = (1 + s * s) / (s * s)
    err = wgt * (den - rows_of(target_latents).float()) ** 2
    return err.reshape(B, -1).mean(dim=1).mean()


def train_step(controlnet, unet, batch, optimizer=None, conditioning_scale=1.0, world_size=1, buckets=None,
               accumulate=False, loss_scale=1.0, max_grad_norm=None, compute_dtype=None, scaler=None):
    """One optimisation step.  compute_dtype: the element type of the activations and activation gradients, torch.bfloat16
    (None, the default) or torch.float16 -- the reference's --mixed_precision fp16; master parameters, parameter gradients, loss and
    optimiser stay fp32 either way.  The frozen UNet must hold its parameters in that type (`unet.half()` for fp16).  scaler: a
    `ctrlv_amd.optim.LossScaler` -- the loss is multiplied by `scaler.scale(...)` before the backward and the step is
    `optimizer.step(scaler=..., max_grad_norm=...)` (unscale, finite check, skipped step and scale update on the device; the
    optimiser must be a `ctrlv_amd.optim.AdamW`; `loss_scale` stays the accumulation factor).  max_grad_norm: clip the gradients to that global norm in front of the optimiser step (the
    reference's --max_grad_norm; see `_backward_and_step`; None: no clipping).  Data parallel: pass `buckets=GradientBuckets(params)` (all-reduce overlapped with the
    backward pass), or only `world_size > 1` for the simple reduce-after-backward path.
    Gradient accumulation (`accelerator.accumulate`, gradient_accumulation_steps of train_video_controlnet.py:376): call
    with accumulate=True and loss_scale=1/steps for every micro-batch but the last -- gradients add up locally, nothing is
    all-reduced and the optimizer does not step; the last micro-batch (accumulate=False) reduces the sums and steps.  batch: dict(latents (B,F,4,h,w) clean, noise, sigmas [B], image_latents (B,F,4,h,w)
    (conditioning frame repeated), control_cond (B,F,4,h,w), encoder_hidden_states (B,1,D), added_time_ids (B,3)).
    Returns the loss as a device tensor; the one host read of the step is the batched mix-factor fetch at its start."""
    prefetch_mix_factors(controlnet, unet)          # the step's only device-to-host read (about 60 scalars, one copy)
    el = _element_dtype(compute_dtype)
    _check_scaler(scaler, optimizer)
    udt = next(unet.parameters()).dtype
    if udt != el and udt != torch.float32:
        raise ValueError(f"train_step: compute_dtype {el} with a frozen UNet held in {udt}: cast it first (unet.to({el}))")
    lat, sig, noisy, timesteps, sample = _noised_inputs(batch, el)
    down, mid = controlnet_train_forward(controlnet, sample, timesteps, batch["encoder_hidden_states"],
                                         batch["added_time_ids"], batch["control_cond"].to(el),
                                         conditioning_scale)
    pred = unet_train_forward(unet, sample, timesteps, batch["encoder_hidden_states"], batch["added_time_ids"], down, mid)
    loss = edm_loss(pred, noisy, lat, sig)
    return _backward_and_step(controlnet, loss, optimizer, world_size, buckets, accumulate, loss_scale, max_grad_norm, scaler)


def unet_train_step(unet, batch, optimizer=None, world_size=1, buckets=None, accumulate=False, loss_scale=1.0, max_grad_norm=None,
                    compute_dtype=None, scaler=None):
    """One stage-1 optimisation step: the whole UNet fine-tuned (tools/train_video_diffusion.py:515-541; UNet forward,
    EDM loss, backward, optimizer step).  Which parameters train is the caller's choice through `unet.enable_grad(...)`
    (all=True: the demo scripts; temporal_transformer_block=True: temporal-only mode) -- frozen parameters get no gradient,
    and switching modes between steps needs nothing else (packed forms are cached only for frozen parameters, keyed on
    their version).  batch: `train_step`'s keys without control_cond; image_latents (B,F,4,h,w) per frame (the
    predict-bbox layout passes unchanged), encoder_hidden_states with the caller's conditioning dropout already applied.
    Data parallel / gradient accumulation / max_grad_norm / compute_dtype / scaler / zero gradients for parameters without a
    gradient path: as in `train_step`.  Returns the detached loss."""
    el = _element_dtype(compute_dtype)
    _check_scaler(scaler, optimizer)
    prefetch_mix_factors(unet)
    lat, sig, noisy, timesteps, sample = _noised_inputs(batch, el)
    pred = unet_full_train_forward(unet, sample, timesteps, batch["encoder_hidden_states"], batch["added_time_ids"])
    loss = edm_loss(pred, noisy, lat, sig)
    return _backward_and_step(unet, loss, optimizer, world_size, buckets, accumulate, loss_scale, max_grad_norm, scaler)


def _check_scaler(scaler, optimizer):
    """A loss scaler works with the project's optimiser only (the scale is read and updated on the device): refused before any
    device work.  A disabled scaler is no scaler."""
    if scaler is not None and not isinstance(scaler, _optim.LossScaler):
        raise TypeError(f"scaler must be a ctrlv_amd.optim.LossScaler, not {type(scaler).__name__}")
    if scaler is not None and scaler.is_enabled() and optimizer is not None and not isinstance(optimizer, _optim.AdamW):
        raise TypeError(f"a LossScaler steps a ctrlv_amd.optim.AdamW only, not {type(optimizer).__name__}")


def _noised_inputs(batch, el=torch.bfloat16):
    """EDM noising of a batch (train_video_controlnet.py:404-410, train_video_diffusion.py:519-527): (clean latents,
    sigmas, noisy latents, continuous timesteps 0.25 ln sigma, model input = [scaled noisy | image latents] in the element type `el`).  A batch
    from `prepare_batch` carries noisy_latents / sample / timesteps already (ctrlv_train_assemble wrote them, the timesteps
    are the scheduler's table entries): they are used as they are."""
    if "noisy_latents" in batch and "sample" in batch and "timesteps" in batch:
        return (batch["latents"].float(), batch["sigmas"].float(), batch["noisy_latents"].float(), batch["timesteps"].float(),
                batch["sample"].to(el))
    lat, noise, sig = batch["latents"].float(), batch["noise"].float(), batch["sigmas"].float()
    B = lat.shape[0]
    s5 = sig.reshape(B, 1, 1, 1, 1)
    noisy = lat + noise * s5                                                    # EulerDiscreteScheduler.add_noise
    inp = noisy / (s5 * s5 + 1) ** 0.5                                          # :410
    timesteps = 0.25 * torch.log(sig)                                           # continuous timestep of sigma
    sample = torch.cat([inp, batch["image_latents"].float()], dim=2).to(el)
    return lat, sig, noisy, timesteps, sample


def prepare_batch(plan, clips, box_frames=None, *, mode, seed, step, num_cond_frames=0, dropout_prob=None, fps=7,
                  motion_bucket_id=127, noise_aug_strength=0.02, return_noise=False, boxes=None, source_size=None):
    """A data-loader batch -> the dict `train_step` (mode "controlnet") / `unet_train_step` (modes "unet" and "boxes") take,
    in one library call (plan: a `ctrlv_amd.plan.TrainBatchPlan`; tools/train_video_controlnet.py:366-449,
    tools/train_video_diffusion.py:428-514): CLIP on the clamped first frame, the VAE posterior samples, the draws into the
    scheduler's tables, the noising, both conditioning-dropout masks, the frame layout and the channel concat, all keyed on
    (seed: a `DeviceSeed`, step, clip index).  clips / box_frames: (n, F, 3, H, W) pixels in [-1, 1] on the plan's device.  The
    dict carries noisy_latents / sample / timesteps, which `_noised_inputs` then takes as they are; added_time_ids is
    [fps - 1, motion_bucket_id, noise_aug_strength] per clip, as the reference's get_add_time_ids (the one upload of the call; nothing is read back).
    boxes= (a `ctrlv_amd.boxes.BoxTable`) with source_size= instead of box_frames: the frames are rendered from the table."""
    out = plan.prepare(clips, box_frames, mode=mode, seed=seed, step=step, num_cond_frames=num_cond_frames,
                       dropout_prob=dropout_prob, return_noise=return_noise, boxes=boxes, source_size=source_size)
    n = clips.shape[0]
    batch = {"latents": out["target_latents"], "sigmas": out["sigmas"], "noisy_latents": out["noisy_latents"],
             "sample": out["sample"], "timesteps": out["timesteps"], "encoder_hidden_states": out["encoder_hidden_states"],
             "added_time_ids": torch.tensor([[float(fps - 1), float(motion_bucket_id), float(noise_aug_strength)]],
                                            dtype=torch.float32).repeat(n, 1).to(clips.device, non_blocking=True),
             "indices": out["indices"], "random_p": out["random_p"]}
    for k in ("control_cond", "noise"):
        if k in out:
            batch[k] = out[k]
    return batch


def _backward_and_step(model, loss, optimizer, world_size, buckets, accumulate, loss_scale, max_grad_norm=None, scaler=None):
    """backward, gradient reduction and optimizer step of `train_step` / `unet_train_step` (model: the trained one).
    max_grad_norm: the gradients are clipped to that global L2 norm in front of the step (the reference's --max_grad_norm,
    `accelerator.clip_grad_norm_`): a `ctrlv_amd.optim.AdamW` does it inside its own pass on the device
    (`step(max_grad_norm=...)`), any other optimiser gets `torch.nn.utils.clip_grad_norm_` over its parameters.  Either way the
    norm is taken AFTER the gradient reduction: every rank computes the same bits from the same gradients, no collective is added.
    scaler (a `ctrlv_amd.optim.LossScaler`): the backward starts from loss * scale, and the optimiser -- a `ctrlv_amd.optim.AdamW`,
    anything else raises -- unscales, checks and steps or skips on the device (`step(scaler=...)`); the found-inf decision is taken
    from that same post-reduction norm, so it needs no collective either.  loss_scale stays the accumulation factor."""
    _check_scaler(scaler, optimizer)
    if scaler is not None and not scaler.is_enabled():
        scaler = None
    if buckets is not None:
        buckets.enabled = not accumulate
    scaled = loss * loss_scale if loss_scale != 1.0 else loss
    (scaler.scale(scaled) if scaler is not None else scaled).backward()
    if accumulate:
        return loss.detach()
    if buckets is not None:
        buckets.finish()
    elif world_size > 1:
        allreduce_gradients([p for p in model.parameters() if p.requires_grad])
    # parameters without a gradient path get ZERO gradients (what the reference's autograd gives them: weight decay then
    # applies), whatever the world size -- the data-parallel paths write zeros for them, so does the single-GPU one
    for p in model.parameters():
        if p.requires_grad and p.grad is None:
            p.grad = torch.zeros_like(p)
    if optimizer is not None:
        if scaler is not None:
            optimizer.step(scaler=scaler, max_grad_norm=max_grad_norm)
        elif max_grad_norm is None:
            optimizer.step()
        elif isinstance(optimizer, _optim.AdamW):
            optimizer.step(max_grad_norm=max_grad_norm)
        else:
            torch.nn.utils.clip_grad_norm_([p for g in optimizer.param_groups for p in g["params"] if p.grad is not None],
                                           max_grad_norm)
            optimizer.step()
        optimizer.zero_grad(set_to_none=True)
    return loss.detach()


# ------------------------------------------------------------------------------------------------- data parallel
class GradientBuckets:
    """DDP-style overlap of the gradient all-reduce with the backward pass (reference: torch DDP under `accelerate`,
    train_video_controlnet.py:225,485).  Parameters are grouped into flat fp32 buckets of `bucket_bytes` in REVERSE
    registration order (the order in which autograd finishes them); a post-accumulate-grad hook on every parameter counts
    its bucket down and launches the bucket's asynchronous all-reduce (RCCL: on its own stream) the moment the last
    gradient of the bucket exists, while the backward pass keeps running.  `finish()` -- after `loss.backward()` --
    flushes buckets whose parameters got no gradient (zeros: every rank issues identical collectives), waits, divides by
    the world size and writes the averaged gradients back.  One instance per model; re-armed by `finish()`.

    Collective ORDER is fixed: bucket i is launched only after buckets 0 .. i-1 (the expected completion order), whatever
    the order in which the hooks fire -- ranks whose graphs differ (a branch that is taken on one rank only) still issue
    the same sequence of all-reduces.  A parameter learnt as "unused" that receives a gradient after all, after its
    bucket has gone out, marks the bucket DIRTY: `finish()` agrees on the dirty set across ranks (one MAX all-reduce of a
    byte mask) and reduces those buckets again with the gradient in place, so no gradient is ever dropped."""

    def __init__(self, params, bucket_bytes=25 * 1024 * 1024, group=None):
        self.group = group
        self.active = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
        self.world = dist.get_world_size(group) if self.active else 1
        self.buckets = _bucketed(reversed([p for p in params if p.requires_grad]), bucket_bytes)
        self.bucket_of = {id(p): i for i, b in enumerate(self.buckets) for p in b}
        self.enabled = True               # False = accumulate locally (accelerate's no_sync micro-batches): no collective
        self.launch_order = []
        self.unused = set()               # ids of parameters without a gradient path, learnt in the first step
        self._arm()
        self.handles = [p.register_post_accumulate_grad_hook(self._hook) for b in self.buckets for p in b] if self.active else []

    def _arm(self):
        # parameters that received no gradient in the previous step (the one-key cross-attentions' to_q / to_k / norm2:
        # softmax over one key is constant) never fire their hook: they are not waited for, so their buckets are
        # all-reduced DURING the backward pass like every other one (their slots carry zeros)
        self.pending = [len(b) - sum(1 for p in b if id(p) in self.unused) for b in self.buckets]
        self.inflight = [None] * len(self.buckets)
        self.launch_order = []
        self.fired = set()
        self.next = 0                     # buckets [0, next) have been launched: the collective order is the bucket order
        self.dirty = set()                # buckets that went out before a (formerly unused) parameter's gradient arrived

    def _launch(self, i):
        self.inflight[i] = _launch_bucket(self.buckets[i], self.group)
        self.launch_order.append(i)

    def _hook(self, p):
        if not self.enabled:
            return
        i = self.bucket_of[id(p)]
        self.fired.add(id(p))
        if id(p) in self.unused:          # it has a gradient after all: count it again from the next step on, and
            self.unused.discard(id(p))    # reduce its bucket again if that has already gone out without this gradient
            if self.inflight[i] is not None:
                self.dirty.add(i)
            return
        self.pending[i] -= 1
        while self.next < len(self.buckets) and self.pending[self.next] <= 0:
            self._launch(self.next)
            self.next += 1

    def finish(self):
        if not self.active or not self.enabled:
            return 0
        while self.next < len(self.buckets):
            self._launch(self.next)
            self.next += 1
        # late gradients: every rank must re-reduce the same buckets, in the same order
        mask = torch.zeros(len(self.buckets), dtype=torch.uint8, device=self.inflight[0][0].device)
        for i in self.dirty:
            mask[i] = 1
        dist.all_reduce(mask, op=dist.ReduceOp.MAX, group=self.group)
        redo = [i for i, v in enumerate(mask.tolist()) if v]
        for i in redo:
            self.inflight[i][1].wait()
            self._launch(i)
        for b, inflight in zip(self.buckets, self.inflight):
            _write_back(b, *inflight, self.world)
        n = len(self.buckets)
        self.unused = {id(p) for b in self.buckets for p in b if id(p) not in self.fired}
        self._arm()
        return n

    def remove(self):
        for h in self.handles:
            h.remove()
        self.handles = []


def _bucketed(params, bucket_bytes):
    """params in order, grouped into buckets of at most `bucket_bytes` of fp32 (a larger parameter gets its own)"""
    buckets, cur, size = [], [], 0
    for p in params:
        nbytes = p.numel() * 4
        if cur and size + nbytes > bucket_bytes:
            buckets.append(cur)
            cur, size = [], 0
        cur.append(p)
        size += nbytes
    if cur:
        buckets.append(cur)
    return buckets


def _launch_bucket(bucket, group):
    """(flat fp32 gradients of the bucket -- zeros where there is none: every rank must issue identical collectives --,
    the handle of their asynchronous SUM all-reduce)"""
    flat = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).float().reshape(-1) for p in bucket])
    return flat, dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group, async_op=True)


def _write_back(bucket, flat, work, world):
    """waits for the bucket's all-reduce and writes the average into the parameters' .grad"""
    work.wait()
    flat.div_(world)
    off = 0
    for p in bucket:
        n = p.numel()
        g = flat[off:off + n].reshape(p.shape).to(p.dtype)
        if p.grad is None:
            p.grad = g
        else:
            p.grad.copy_(g)
        off += n


def allreduce_gradients(params, bucket_bytes=25 * 1024 * 1024, group=None):
    """Average the gradients over the process group in flat fp32 buckets (reference: DDP's 25 MB default under
    `accelerate`, train_video_controlnet.py:225,485).  All buckets are launched asynchronously before the first wait, so
    the transfers queue back to back on the collective stream; parameters without a gradient contribute zeros."""
    if not dist.is_available() or not dist.is_initialized() or dist.get_world_size(group) == 1:
        return 0
    buckets = _bucketed(params, bucket_bytes)
    pending = [_launch_bucket(b, group) for b in buckets]
    for b, inflight in zip(buckets, pending):
        _write_back(b, *inflight, dist.get_world_size(group))
    return len(buckets)


# ------------------------------------------------------------------------------------------------- VAE decoder fine-tuning
def _vae_train_supported(decoder, z, num_frames):
    """Shapes the training walk takes: what the inference executor takes (vae_decoder_hip.supports) and, since all clips run
    in ONE walk, every activation of the whole batch below the kernels' 32-bit byte-offset limit."""
    from .models import vae_decoder_hip as vh
    if z.dim() != 4 or z.shape[0] % num_frames or not vh.supports(z, num_frames, decoder):
        return False
    n, _, h, w = z.shape
    wide = [max(blk.resnets[0].spatial_res_block.conv1.weight.shape[:2]) for blk in decoder.up_blocks]
    return all(n * h * w * 4 ** i * c * 2 < vh._LIMIT for i, c in enumerate(wide))


def vae_decoder_train_forward(decoder, z, num_frames):
    """`TemporalDecoder.forward` of the SVD VAE with gradients for every decoder parameter that requires them (the decoder of
    tools/train_vae_finetuning.py:303-320): conv_in as the im2col GEMM, the mid block (res block, head-dim-512 attention, res
    block), the up blocks with nearest-x2 fused into the upsampler convs, conv_norm_out + SiLU, conv_out and time_conv_out.
    The launches are those of models/vae_decoder_hip.decode (same bits forward; all clips of the batch in one walk).
    z: (n, 4, h, w) latents, n a multiple of num_frames (frames per clip).  Returns (n, 3, 8h, 8w) fp32."""
    if z.dim() != 4 or z.shape[0] % num_frames:
        raise ValueError(f"vae_decoder_train_forward: latents {tuple(z.shape)} are not whole clips of num_frames={num_frames}")
    if not _vae_train_supported(decoder, z, num_frames):
        raise ValueError(f"vae_decoder_train_forward: {tuple(z.shape)} latents in clips of {num_frames} are not served by the HIP "
                         "decoder (CUDA latents, h*w a multiple of 64 and <= 16384, every activation below 4 GiB)")
    n, cz, H, W = z.shape
    n_clips, F = n // num_frames, num_frames
    cp = (cz + 7) // 8 * 8
    kp = (9 * cp + 63) // 64 * 64
    col = _input_cols([z.detach()], n, H, W, cp, kp, z.device)
    wi, bi = _input_conv_weight([decoder.conv_in], cp, kp)
    x = gemm(col, wi, bi)
    mid = decoder.mid_block
    x = vae_res_block_train_forward(mid.resnets[0], x, n_clips, F, H, W)
    for attn, resnet in zip(mid.attentions, mid.resnets[1:]):
        x = vae_attention_train_forward(attn, x, n, H, W)
        x = vae_res_block_train_forward(resnet, x, n_clips, F, H, W)
    for blk in decoder.up_blocks:
        for resnet in blk.resnets:
            x = vae_res_block_train_forward(resnet, x, n_clips, F, H, W)
        if blk.upsamplers is not None:
            x = _conv(blk.upsamplers[0].conv, x, H, W, 2 * H, 2 * W, 1, 1)
            H, W = 2 * H, 2 * W
    gno = decoder.conv_norm_out
    xn = GroupNormSiLU.apply(x, gno.weight, gno.bias, n, H * W, 1, gno.eps, True)
    # conv_out has 3 output channels: its rows are stored 4 wide (zero weight row and bias: differentiable torch pads on the
    # [3, 128, 3, 3] parameter), the width time_conv_out's kernel reads; the GEMM backward pads N further as for the UNet's 4
    co = decoder.conv_out.weight.shape[0]
    pad = (co + 3) // 4 * 4 - co
    y = gemm(xn, Fn.pad(decoder.conv_out.weight, (0, 0, 0, 0, 0, 0, 0, pad)), Fn.pad(decoder.conv_out.bias, (0, pad)),
             mode=1, conv=(H, W, H, W, 1, 0))
    return TimeConvOut.apply(y, decoder.time_conv_out.weight, decoder.time_conv_out.bias, n_clips, F, H, W)


def vae_train_step(vae, batch, optimizer=None, num_frames=1, sample_posterior=True, generator=None, world_size=1, buckets=None,
                   accumulate=False, loss_scale=1.0):
    """One step of the VAE decoder fine-tuning (tools/train_vae_finetuning.py:303-320: `vae(images, sample_posterior=True)`
    with num_frames=1, clamp(-1, 1), MSE, AdamW on the `decoder.*` parameters).  batch["pixel_values"]: (B, 3, H, W) in
    [-1, 1], B whole clips of num_frames.  The frozen side -- encoder, quant_conv, the posterior sample -- runs under
    no_grad on the HIP encoder path; the decoder runs `vae_decoder_train_forward`; clamp and MSE are plain torch on the
    image-sized fp32 prediction.  Which decoder parameters train is the caller's choice through requires_grad (the
    reference: all of them); encoder and quant_conv are never touched.  Data parallel / gradient accumulation: as in
    `train_step` (the reduced model is the decoder).  Gradient clipping: this step's argument list is pinned by its tests, so the
    norm is set on the optimiser -- `ctrlv_amd.optim.AdamW(...).clip_grad_norm(max_norm)` clips in every later `step()`.
    Returns the detached loss."""
    px = batch["pixel_values"]
    if px.dim() != 4 or px.shape[1] != vae.config.in_channels:
        raise ValueError(f"vae_train_step: pixel_values must be (B, {vae.config.in_channels}, H, W), got {tuple(px.shape)}")
    B, _, Hp, Wp = px.shape
    if B % num_frames:
        raise ValueError(f"vae_train_step: a batch of {B} images is not whole clips of num_frames={num_frames}")
    probe = torch.empty(B, vae.config.latent_channels, Hp // 8, Wp // 8, dtype=torch.bfloat16, device=px.device)
    if Hp % 8 or Wp % 8 or not _vae_train_supported(vae.decoder, probe, num_frames):
        raise ValueError(f"vae_train_step: {B} images of {Hp}x{Wp} in clips of {num_frames} are not served by the HIP decoder "
                         "(CUDA tensors, H and W multiples of 8, H*W/64 a multiple of 64 and <= 16384, activations below 4 GiB)")
    with torch.no_grad():
        dist = vae.encode(px).latent_dist
        z = dist.sample(generator) if sample_posterior else dist.mode()
    prefetch_mix_factors(vae.decoder, host_sigmoid=True)       # the step's only device-to-host read
    pred = vae_decoder_train_forward(vae.decoder, z, num_frames)
    loss = Fn.mse_loss(pred.clamp(-1.0, 1.0), px.float())
    return _backward_and_step(vae.decoder, loss, optimizer, world_size, buckets, accumulate, loss_scale)
