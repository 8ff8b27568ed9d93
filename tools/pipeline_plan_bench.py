"""A whole clip: the one-call driver (ctrlv_pipeline_generate, CTRLV_PIPELINE=plan) against the Python pipeline with its HIP graph.

One StableVideoControlPipeline at cfg3 size (Box2Video: ControlNet + UNet at full SVD widths, CFG batch 2, 25 frames, 576 x 1024;
random weights, the default AutoencoderKLTemporalDecoder, a ViT-H-sized CLIP tower), one PIL image at the working size, fp32 box
frames.  The two routes are ALTERNATED on the same device, `--rounds` times each after one warm call each, both under
CTRLV_VAE_HIP=plan and CTRLV_CLIP_HIP=plan, so the only difference is who issues the calls: the driver launches every step
eagerly from C; the Python loop runs its first step eagerly, captures the second into a HIP graph and replays it (a new call is a
new capture).  Wall time of a call (host clock around a synchronised call, output_type="pil"), at `--steps` and at `--steps-lo`
denoising steps: per clip = the `--steps` call, per denoising step = the difference of the two divided by the difference of
the step counts (what a step adds, without the per-clip work around the loop).  One JSON line appended to `--out`.  Run the whole
tool under one `timeout`.

    timeout -k 10 900 python tools/pipeline_plan_bench.py [--steps 25 --steps-lo 5 --rounds 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
VIT_H = dict(hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=16, image_size=224, patch_size=14,
             projection_dim=1024, hidden_act="gelu", layer_norm_eps=1e-5)


def build_pipe(frames, clip_layers):
    from PIL import Image  # noqa: F401  (the route needs PIL)
    from ctrlv_amd.models import (AutoencoderKLTemporalDecoder, CLIPVisionModelWithProjection, ControlNetModel,
                                  UNetSpatioTemporalConditionModel)
    from ctrlv_amd.pipelines import StableVideoControlPipeline
    from ctrlv_amd.pipelines.pipeline_utils import MinimalCLIPImageProcessor
    from ctrlv_amd.schedulers import EulerDiscreteScheduler
    from ctrlv_amd.utils import build_on_device, random_init_
    bf = torch.bfloat16
    unet = build_on_device(UNetSpatioTemporalConditionModel, DEV, num_frames=frames)
    random_init_(unet, seed=0)
    ctrl = build_on_device(ControlNetModel, DEV, num_frames=frames)
    random_init_(ctrl, seed=1, zero_conv_std=0.02)
    torch.manual_seed(0)
    vae = AutoencoderKLTemporalDecoder().eval().to(DEV, bf).requires_grad_(False)
    with torch.device(DEV):
        clip = CLIPVisionModelWithProjection(**dict(VIT_H, num_hidden_layers=clip_layers))
    with torch.no_grad():
        for p in clip.parameters():
            if p.dim() > 1:
                p.normal_(0.0, 0.02)
    clip = clip.to(bf).eval().requires_grad_(False)
    pipe = StableVideoControlPipeline(vae, clip, unet.eval(), ctrl.eval(), EulerDiscreteScheduler(), MinimalCLIPImageProcessor())
    pipe.set_progress_bar_config(disable=True)
    return pipe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pipeline_plan_bench.jsonl"))
    ap.add_argument("--height", type=int, default=576)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=25)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--steps-lo", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--clip-layers", type=int, default=32)
    args = ap.parse_args()
    if not 2 <= args.steps_lo < args.steps:
        ap.error("2 <= --steps-lo < --steps (the Python loop captures its graph in the second step)")
    import __graft_entry__ as g
    g.build()
    from PIL import Image
    from ctrlv_amd import plan as plan_mod
    os.environ["CTRLV_VAE_HIP"] = "plan"
    os.environ["CTRLV_CLIP_HIP"] = "plan"
    H, W, F = args.height, args.width, args.frames
    pipe = build_pipe(F, args.clip_layers)
    gen = torch.Generator().manual_seed(3)
    image = Image.fromarray(torch.randint(0, 256, (H, W, 3), generator=gen, dtype=torch.uint8).numpy())
    cond = (torch.rand(1, F, 3, H, W, generator=gen) * 2 - 1).to(DEV)
    entered = [0]
    real = plan_mod.PipelinePlan.generate

    def counting(self, *a, **k):
        entered[0] += 1
        return real(self, *a, **k)
    plan_mod.PipelinePlan.generate = counting

    def call(route, steps):
        if route == "plan":
            os.environ["CTRLV_PIPELINE"] = "plan"
        else:
            os.environ.pop("CTRLV_PIPELINE", None)
        before = entered[0]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        frames = pipe(image, cond_images=cond, height=H, width=W, num_frames=F, num_inference_steps=steps, decode_chunk_size=F,
                      generator=torch.Generator().manual_seed(7), output_type="pil").frames
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert (entered[0] - before) == (1 if route == "plan" else 0), "the call did not take the route it was asked for"
        return dt, frames

    with torch.no_grad():
        ref = {}
        for route in ("python", "plan"):                                  # warm: weights packed, plans loaded, workspaces sized
            ref[route] = np.asarray(call(route, args.steps_lo)[1][0][F // 2]).astype(np.float32)
        diff = float(np.abs(ref["plan"] - ref["python"]).mean())
        times = {(r, s): [] for r in ("python", "plan") for s in (args.steps_lo, args.steps)}
        for _ in range(args.rounds):
            for steps in (args.steps_lo, args.steps):
                for route in ("python", "plan"):
                    times[(route, steps)].append(call(route, steps)[0])
    med = {k: statistics.median(v) for k, v in times.items()}
    span = args.steps - args.steps_lo
    rec = dict(tool="pipeline_plan_bench", size=f"{H}x{W}", frames=F, steps=args.steps, steps_lo=args.steps_lo, rounds=args.rounds,
               clip_layers=args.clip_layers, device=torch.cuda.get_device_name(0),
               mean_abs_byte_difference_mid_frame=round(diff, 3))
    for route in ("python", "plan"):
        rec[route] = dict(clip_s=round(med[(route, args.steps)], 4), clip_lo_s=round(med[(route, args.steps_lo)], 4),
                          step_ms=round(1e3 * (med[(route, args.steps)] - med[(route, args.steps_lo)]) / span, 3),
                          all_clip_s=[round(v, 4) for v in times[(route, args.steps)]])
    rec["plan_over_python_clip"] = round(rec["plan"]["clip_s"] / rec["python"]["clip_s"], 4)
    rec["plan_over_python_step"] = round(rec["plan"]["step_ms"] / rec["python"]["step_ms"], 4)
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
