#!/usr/bin/env python
"""Stage 1 on one MI355X: the UNet fine-tuning step (tools/train_video_diffusion.py:515-541; B = 1, full SVD width) through
ctrlv_amd.training.unet_train_step.  Prints ONE JSON line: ms per optimisation step, its split (forward / backward /
optimizer, HIP events), peak device memory, the mode (`all`: every parameter, the demo scripts; `temporal`: the temporal
transformer blocks only), gradient checkpointing, and the analytic work of the step -- counted from the layer list (torch's
FLOP counter over the oracle UNet's forward and backward on the meta device: GEMMs, convs and attention; checkpoint
recomputes are not counted).  Synthetic data, random-init weights (there are no checkpoints in this image).
Default size: the stage-1 training size 320 x 512 (src/ctrlv/datasets/kitti_abstract.py:86-90); --height 576 --width 1024
for the full frame.
usage: python tools/train_unet_bench.py [--steps 3] [--warmup 1] [--frames 25] [--height 320] [--width 512]
       [--mode all|temporal|lora] [--rank 4] [--gradient-checkpointing 0|1] [--gpus N] [--optimizer torch|hip] [--ema 0|1]
--optimizer hip: ctrlv_amd.optim.AdamW (flat buffers, one ctrlv_adamw_step launch) instead of torch.optim.AdamW; --ema 1: an EMA of
the trained parameters inside optimizer_ms -- fused into the AdamW pass with --optimizer hip, torch's foreach ops on per-tensor
shadows with --optimizer torch (a stand-in for diffusers' per-tensor Python loop, and a conservative one: fewer launches).
Data parallel: --gpus N as in tools/train_bench.py (one rank process per GPU, its own clip per rank, the fp32 gradients
all-reduced in 25 MB buckets while the backward runs); the time is the MAX over ranks."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def analytic_tflop(frames, h, w, mode="all", config=None, rank=4):
    """(forward, backward) TFLOP of one stage-1 step at B = 1 and an h x w latent, from the layer list of the oracle UNet
    (SVD configuration unless `config`), counted on the meta device: no memory, no arithmetic.  mode "lora": the UNet frozen,
    rank-`rank` factors on every to_q / to_k / to_v / to_out.0 (the branch base(x) + s B(A(x)) around the oracle's
    nn.Linear): dgrad everywhere plus the LoRA products, no weight gradient of the base."""
    from torch.utils.flop_counter import FlopCounterMode
    if os.path.join(ROOT, "oracle") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ctrlv_ref as R
    cfg = dict(config or R.SVD_CONFIG, num_frames=frames)
    with torch.device("meta"):
        ou = R.UNetSpatioTemporalConditionModel(**cfg)
    ou = ou.to("meta")                 # (a few parameters are built with the legacy constructor, on the CPU)
    for n, p in ou.named_parameters():
        p.requires_grad_(mode == "all" or (mode == "temporal" and "temporal_transformer_block" in n))
    if mode == "lora":
        import torch.nn.functional as Fn
        for n, m in ou.named_modules():
            if isinstance(m, torch.nn.Linear) and (n.rsplit(".", 1)[-1] in ("to_q", "to_k", "to_v") or n.endswith("to_out.0")):
                a = torch.empty(rank, m.in_features, device="meta", requires_grad=True)
                b = torch.empty(m.out_features, rank, device="meta", requires_grad=True)
                m.register_forward_hook(lambda _m, inp, out, a=a, b=b: out + Fn.linear(Fn.linear(inp[0], a), b))
    dc = cfg["cross_attention_dim"]
    dc = dc if isinstance(dc, int) else dc[0]
    x = torch.empty(1, frames, cfg["in_channels"], h, w, device="meta")
    with FlopCounterMode(display=False) as fwd:
        out = ou(x, torch.tensor(1.0, device="meta"), torch.empty(1, 1, dc, device="meta"),
                 torch.empty(1, 3, device="meta"))[0]
    with FlopCounterMode(display=False) as bwd:
        out.float().sum().backward()
    return fwd.get_total_flops() / 1e12, bwd.get_total_flops() / 1e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=25)
    ap.add_argument("--height", type=int, default=320)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--mode", choices=("all", "temporal", "lora"), default="all",
                    help="all: unet.enable_grad(all=True) (the demo scripts); temporal: temporal_transformer_block only; "
                         "lora: unet.add_adapter(rank --rank on to_q / to_k / to_v / to_out.0), the UNet frozen")
    ap.add_argument("--rank", type=int, default=4, help="LoRA rank of --mode lora (lora_alpha = rank, as the reference)")
    ap.add_argument("--lr", type=float, default=1e-5)
    ap.add_argument("--fused-adamw", type=int, default=1, help="torch.optim.AdamW(fused=...)")
    ap.add_argument("--optimizer", choices=("torch", "hip"), default="torch",
                    help="torch: torch.optim.AdamW; hip: ctrlv_amd.optim.AdamW (flat buffers, csrc/optim.hip)")
    ap.add_argument("--ema", type=int, default=0, help="1: EMA of the trained parameters (ctrlv_amd.optim.EMAModel), timed in optimizer_ms")
    ap.add_argument("--max-grad-norm", type=float, default=None,
                    help="clip the gradients to this global norm, timed in optimizer_ms (the reference's --max_grad_norm, default 1.0 "
                         "there): inside the AdamW pass with --optimizer hip, torch.nn.utils.clip_grad_norm_ with torch")
    ap.add_argument("--gradient-checkpointing", type=int, default=0,
                    help="1: unet.enable_gradient_checkpointing() (the GEGLU feed-forward intermediates are recomputed in "
                         "the backward)")
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16", help="element type of activations and activation gradients")
    ap.add_argument("--loss-scale", default="none",
                    help="none | dynamic (ctrlv_amd.optim.LossScaler, torch's defaults) | a number (a fixed scale: no growth, no "
                         "backoff); needs --optimizer hip: the scale is read and updated on the device")
    ap.add_argument("--gpus", type=int, default=0,
                    help="N > 1 without a torchrun environment: start N rank processes (one per GPU) from this GPU-free parent")
    args = ap.parse_args()
    if args.loss_scale != "none" and args.optimizer != "hip":
        raise SystemExit("train_unet_bench.py: --loss-scale needs --optimizer hip")
    if args.gpus > 1 and "RANK" not in os.environ:
        from ctrlv_amd.distributed import launch_local_ranks
        launch_local_ranks(__file__, sys.argv[1:], args.gpus)
        return
    world, rank, local = (int(os.environ.get(k, d)) for k, d in (("WORLD_SIZE", 1), ("RANK", 0), ("LOCAL_RANK", 0)))
    if args.gpus and args.gpus != world:
        raise SystemExit(f"train_unet_bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    dev = torch.device(f"cuda:{local}")
    torch.cuda.set_device(dev)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    import __graft_entry__ as ge
    if rank == 0:
        ge.build()
    if world > 1:
        dist.barrier()
    from ctrlv_amd import training
    from ctrlv_amd.autograd import prefetch_mix_factors
    from ctrlv_amd.models import UNetSpatioTemporalConditionModel
    from ctrlv_amd.utils import build_on_device, random_init_
    unet = build_on_device(UNetSpatioTemporalConditionModel, dev, dtype=torch.float32, num_frames=args.frames)  # fp32 masters
    random_init_(unet, seed=0)
    if args.mode == "all":
        unet.enable_grad(all=True)
    elif args.mode == "lora":                                    # tools/train_video_diffusion.py:126-136
        unet.add_adapter(dict(r=args.rank, lora_alpha=args.rank, init_lora_weights="gaussian", lora_dropout=0.0,
                              target_modules=["to_k", "to_q", "to_v", "to_out.0"]))
    else:
        unet.enable_grad(temporal_transformer_block=True)
    if args.gradient_checkpointing:
        unet.enable_gradient_checkpointing()
    params = unet.get_parameters_with_grad()
    from ctrlv_amd import optim
    ema = optim.EMAModel(params) if args.ema else None
    if args.optimizer == "hip":
        opt = optim.AdamW(params, lr=args.lr, weight_decay=1e-2).attach_ema(ema)      # the shadow update rides in the AdamW pass
    else:
        opt = torch.optim.AdamW(params, lr=args.lr, weight_decay=1e-2, fused=bool(args.fused_adamw))
    el = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    scaler = optim.loss_scaler_from_option(args.loss_scale)
    buckets = training.GradientBuckets(params) if world > 1 else None
    B, F, h, w = 1, args.frames, args.height // 8, args.width // 8
    g = torch.Generator(device=dev).manual_seed(1234 + rank)             # every rank: its own clip
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)      # noqa: E731
    batch = dict(latents=rn(B, F, 4, h, w), noise=rn(B, F, 4, h, w), sigmas=torch.tensor([1.5], device=dev),
                 image_latents=rn(B, 1, 4, h, w).repeat(1, F, 1, 1, 1), encoder_hidden_states=rn(B, 1, 1024),
                 added_time_ids=torch.tensor([[6.0, 127.0, 0.02]], device=dev))
    ev = lambda: torch.cuda.Event(enable_timing=True)             # noqa: E731
    times, losses = [], []
    for i in range(args.warmup + args.steps):
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        t0 = time.time()
        e = [ev() for _ in range(4)]
        e[0].record()
        # unet_train_step, cut at its phase boundaries
        prefetch_mix_factors(unet)
        lat, sig, noisy, ts, sample = training._noised_inputs(batch, el)
        pred = training.unet_full_train_forward(unet, sample, ts, batch["encoder_hidden_states"], batch["added_time_ids"])
        loss = training.edm_loss(pred, noisy, lat, sig)
        e[1].record()
        training._backward_and_step(unet, loss, None, world, buckets, False, 1.0, None, scaler)
        e[2].record()
        if scaler is not None:
            scaler.step(opt, max_grad_norm=args.max_grad_norm)    # unscale, finite check, skip and scale update on the device
            scaler.update()
        elif args.max_grad_norm is None:
            opt.step()
        elif args.optimizer == "hip":
            opt.step(max_grad_norm=args.max_grad_norm)            # norm, coefficient and skip flag on the device, inside the pass
        else:
            torch.nn.utils.clip_grad_norm_(params, args.max_grad_norm)
            opt.step()
        if ema is not None and args.optimizer != "hip":
            ema.step(params)
        opt.zero_grad(set_to_none=True)
        e[3].record()
        torch.cuda.synchronize()
        wall = (time.time() - t0) * 1e3
        if world > 1:                                             # slowest rank defines the step
            wt = torch.tensor([wall], device=dev)
            dist.all_reduce(wt, op=dist.ReduceOp.MAX)
            wall = float(wt)
        if i >= args.warmup:
            times.append((wall, e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2]), e[2].elapsed_time(e[3])))
        losses.append(float(loss.detach()))
        del pred, loss
    if rank != 0:
        return
    n = len(times)
    avg = [sum(t[k] for t in times) / n for k in range(4)]
    tf_f, tf_b = analytic_tflop(F, h, w, args.mode, rank=args.rank)
    print(json.dumps({"metric": "stage-1 UNet training step (B=1 per GPU, no CFG)", "n_gpus": world, "mode": args.mode,
                      "samples_per_s": round(world * 1e3 / avg[0], 3), "scaling": "weak", "ms_per_step": round(avg[0], 1),
                      "forward_ms": round(avg[1], 1), "backward_ms": round(avg[2], 1), "optimizer_ms": round(avg[3], 1),
                      "steps": n, "warmup": args.warmup, "frames": F, "latent": [h, w],
                      "analytic_tflop_per_step": round(tf_f + tf_b, 1), "analytic_tflop_forward": round(tf_f, 1),
                      "analytic_tflop_backward": round(tf_b, 1), "tflops": round((tf_f + tf_b) / avg[0] * 1e3, 1),
                      "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2**30, 1),
                      "trainable_params_m": round(sum(p.numel() for p in params) / 1e6, 1),
                      "losses": [round(v, 5) for v in losses],
                      "gradient_checkpointing": bool(args.gradient_checkpointing), "optimizer": args.optimizer, "ema": bool(args.ema),
                      **({"rank": args.rank} if args.mode == "lora" else {}),
                      **({"max_grad_norm": args.max_grad_norm} if args.max_grad_norm is not None else {}),
                      **({"loss_scale": args.loss_scale, "final_scale": scaler.get_scale(),
                          "skipped_steps": int(opt.grad_state()["skipped_total"])} if scaler is not None else {}),
                      "dtype": f"{args.dtype} compute, fp32 master parameters + AdamW", "data": "synthetic, random-init weights"}))


if __name__ == "__main__":
    main()
