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

`--boxes` times the two-stage chain instead (boxes_main below): image + first / last box frames -> video as ONE C call against
the two Python pipeline calls with host numpy in between; the record goes to profiles/box_chain_bench.jsonl.

    timeout -k 10 900 python tools/pipeline_plan_bench.py --boxes [--height 320 --width 512 --steps 25 --rounds 3]

`--seeded` times what precedes a seeded clip instead (seeded_main below): the prepare phase as ONE C call
(ctrlv_pipeline_prepare: Lanczos resize, the two Gaussian draws, the sigma schedule) against the same work on the host route
(PIL's resize, two torch.randn, set_timesteps, the uploads), for 375 x 1242 -> 320 x 512 and 720 x 1280 -> 576 x 1024 at 25
frames.  Needs no weights: prepare reads the plans' configurations only.

    timeout -k 10 300 python tools/pipeline_plan_bench.py --seeded [--rounds 10]

`--best-of C` times the best-of-C loop over stage-1 candidates instead (best_main below): ONE C call (ctrlv_pipeline_best_boxes)
against C predict_boxes calls with the clean-up and the counts on the device, the counts copied to the host per candidate and the
argmax there; the record goes to profiles/box_eval_bench.jsonl.

    timeout -k 10 900 python tools/pipeline_plan_bench.py --best-of 5 --height 320 --width 512 [--steps 25 --rounds 3]
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


def host_between(bbox_im, threshold):
    """What a Python host does between the two pipeline calls (the reference's eval_overall.py:96-105, 154): the [0, 1] box
    frames (F, 3, H, W) come to the host, dark pixels and box-less interior frames are zeroed in numpy and the result is
    truncated to bytes; the condition of stage 2 is formed on the device."""
    v = bbox_im.detach().float().cpu().numpy() * 255
    total = v.sum(axis=1)
    v[np.repeat((total < threshold)[:, None], 3, axis=1)] = 0
    for f in range(1, v.shape[0] - 1):
        if v[f].sum(axis=0).min() > threshold:
            v[f] = 0
    return v.astype(np.uint8), 2 * (bbox_im - 0.5).unsqueeze(0)


def boxes_main(args):
    """--boxes: image + first / last box frames -> video.  `chain`: ONE C call (plan.boxes_to_video: box predictor, the
    kernels between the stages, Box2Video) against `python`: VideoDiffusionPipeline, host numpy, StableVideoControlPipeline --
    two Python pipeline calls with their HIP graphs.  Same device, one process, alternated `--rounds` times after one warm
    call each; host clock around synchronised calls that end with the video's and the cleaned box frames' bytes on the host."""
    import __graft_entry__ as g
    g.build()
    from PIL import Image
    from ctrlv_amd import plan as plan_mod
    from ctrlv_amd.models import UNetSpatioTemporalConditionModel
    from ctrlv_amd.pipelines import VideoDiffusionPipeline
    from ctrlv_amd.pipelines.pipeline_utils import randn_tensor
    from ctrlv_amd.utils import build_on_device, random_init_
    os.environ["CTRLV_VAE_HIP"] = "plan"
    os.environ["CTRLV_CLIP_HIP"] = "plan"
    os.environ.pop("CTRLV_PIPELINE", None)
    H, W, F, K, steps, thr = args.height, args.width, args.frames, args.cond_frames, args.steps, 50.0
    video = build_pipe(F, args.clip_layers)
    box_unet = build_on_device(UNetSpatioTemporalConditionModel, DEV, num_frames=F)
    random_init_(box_unet, seed=2)
    boxes_pipe = VideoDiffusionPipeline(video.vae, video.image_encoder, box_unet.eval(), video.scheduler, video.feature_extractor)
    boxes_pipe.set_progress_bar_config(disable=True)
    gen = torch.Generator().manual_seed(3)
    image = Image.fromarray(torch.randint(0, 256, (H, W, 3), generator=gen, dtype=torch.uint8).numpy())
    bbox = (torch.rand(1, F, 3, H, W, generator=gen) * 2 - 1).to(DEV)
    common = dict(height=H, width=W, num_frames=F, num_inference_steps=steps, decode_chunk_size=F)

    def python_route():
        bbox_im = boxes_pipe(image, bbox_images=bbox, generator=torch.Generator().manual_seed(7), output_type="pt",
                             num_cond_bbox_frames=K, **common).frames[0]
        clean, cond = host_between(bbox_im, thr)
        frames = video(image, cond_images=cond, generator=torch.Generator().manual_seed(8), output_type="pil", **common).frames
        return np.stack([np.asarray(im) for im in frames[0]]), clean

    def chain_route():
        pb, pv = boxes_pipe._pipeline_plan(), video._pipeline_plan()
        assert pb is not None and pv is not None, "the plans do not serve these pipelines"
        image_u8 = torch.from_numpy(np.array(image)[None]).to(DEV)
        sched = video.scheduler
        sched.set_timesteps(steps, device=DEV)
        schedule = (list(sched._sigmas_host), list(sched._timesteps_host))
        draws = []
        for pipe, seed in ((boxes_pipe, 7), (video, 8)):          # the pipelines' own two draws, in their order
            gn = torch.Generator().manual_seed(seed)
            aug = randn_tensor((1, 3, H, W), generator=gn, device=DEV, dtype=torch.float32)
            draws.append((aug, pipe.prepare_latents(1, F, 8, H, W, pb.dtype, DEV, gn, None).float()))
        kw = dict(noise_aug_strength=0.02, fps=7, motion_bucket_id=127, min_guidance=1.0, max_guidance=3.0, decode_chunk=F)
        out = plan_mod.boxes_to_video(pb, pv, image_u8, draws[0][1], draws[1][1], schedule, schedule, bbox, K,
                                      box_aug_noise=draws[0][0], video_aug_noise=draws[1][0], clean_threshold=thr, box_kw=kw,
                                      video_kw=dict(kw, conditioning_scale=1.0), frames=False)
        return out[2][0].cpu().numpy(), out[3][0].cpu().numpy()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    routes = {"python": python_route, "chain": chain_route}
    with torch.no_grad():
        ref = {name: timed(fn)[1] for name, fn in routes.items()}                     # warm
        times = {name: [] for name in routes}
        for _ in range(args.rounds):
            for name, fn in routes.items():
                times[name].append(timed(fn)[0])
    diff = float(np.abs(ref["chain"][0].astype(np.float32) - ref["python"][0].astype(np.float32)).mean())
    clean_diff = float((ref["chain"][1] != ref["python"][1]).mean())
    rec = dict(tool="pipeline_plan_bench --boxes", size=f"{H}x{W}", frames=F, steps=steps, cond_frames=K, rounds=args.rounds,
               clip_layers=args.clip_layers, device=torch.cuda.get_device_name(0), mean_abs_byte_difference_video=round(diff, 3),
               cleaned_box_bytes_that_differ=round(clean_diff, 5))
    for name in routes:
        rec[name] = dict(chain_s=round(statistics.median(times[name]), 4), all_chain_s=[round(v, 4) for v in times[name]])
    rec["chain_over_python"] = round(rec["chain"]["chain_s"] / rec["python"]["chain_s"], 4)
    print(json.dumps(rec), flush=True)
    out_path = args.out or os.path.join(ROOT, "profiles", "box_chain_bench.jsonl")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "a") as f:
        f.write(json.dumps(rec) + "\n")


RAMPS = ((1, 2), (1, 3), (2, 4), (2, 5), (3, 5), (1, 4), (2, 3), (3, 4))      # the reference's five, then three more


def best_main(args):
    """--best-of C: image + first / last box frames + ground-truth box frames -> the best candidate's frames.  `one_call`:
    PipelinePlan.best_boxes (every candidate, the scores, the choice and the winner's post-processing enqueued by one C call;
    the host waits once, at the end).  `by_hand`: what a host of the plan route did before -- per candidate predict_boxes,
    ops.box_frames_post, ops.mask_counts and the counts' .cpu() (one synchronisation per candidate), metrics.best_of on the
    host, then ops.box_frames_post of the winner.  Same plans, same inputs, same device, alternated `--rounds` times after one
    warm call each; host clock around synchronised calls.  The kernels are the same: what differs is the synchronisations."""
    import __graft_entry__ as g
    g.build()
    from ctrlv_amd import metrics, ops
    from ctrlv_amd.models import AutoencoderKLTemporalDecoder, CLIPVisionModelWithProjection, UNetSpatioTemporalConditionModel
    from ctrlv_amd.pipelines import VideoDiffusionPipeline
    from ctrlv_amd.pipelines.pipeline_utils import MinimalCLIPImageProcessor
    from ctrlv_amd.schedulers import EulerDiscreteScheduler
    from ctrlv_amd.utils import build_on_device, random_init_
    os.environ["CTRLV_VAE_HIP"] = "plan"
    os.environ["CTRLV_CLIP_HIP"] = "plan"
    H, W, F, K, steps, C, thr = args.height, args.width, args.frames, args.cond_frames, args.steps, args.best_of, 50.0
    bf = torch.bfloat16
    box_unet = build_on_device(UNetSpatioTemporalConditionModel, DEV, num_frames=F)
    random_init_(box_unet, seed=2)
    torch.manual_seed(0)
    vae = AutoencoderKLTemporalDecoder().eval().to(DEV, bf).requires_grad_(False)
    with torch.device(DEV):
        clip = CLIPVisionModelWithProjection(**dict(VIT_H, num_hidden_layers=args.clip_layers))
    with torch.no_grad():
        for p in clip.parameters():
            if p.dim() > 1:
                p.normal_(0.0, 0.02)
    clip = clip.to(bf).eval().requires_grad_(False)
    sched = EulerDiscreteScheduler()
    boxes_pipe = VideoDiffusionPipeline(vae, clip, box_unet.eval(), sched, MinimalCLIPImageProcessor())
    pb = boxes_pipe._pipeline_plan()
    assert pb is not None, "the plan does not serve this pipeline"
    gen = torch.Generator().manual_seed(3)
    image_u8 = torch.randint(0, 256, (1, H, W, 3), generator=gen, dtype=torch.uint8).to(DEV)
    bbox = (torch.rand(1, F, 3, H, W, generator=gen) * 2 - 1).to(DEV)
    gt = (torch.rand(1, F, 3, H, W, generator=gen) < 0.3).to(torch.uint8).mul(255).to(DEV)
    sched.set_timesteps(steps, device=DEV)
    schedule = (list(sched._sigmas_host), list(sched._timesteps_host))
    lats = [(torch.randn(1, F, 4, H // 8, W // 8, generator=gen) * sched.init_noise_sigma).to(DEV) for _ in range(C)]
    augs = [torch.randn(1, 3, H, W, generator=gen).to(DEV) for _ in range(C)]
    ramps = RAMPS[:C]
    kw = dict(noise_aug_strength=0.02, fps=7, motion_bucket_id=127, decode_chunk=F)

    def one_call():
        pt, cond, u8, winner, counts = pb.best_boxes(image_u8, bbox, gt, ramps, K, latents=lats, aug_noise=augs, schedule=schedule,
                                                     clean_threshold=thr, **kw)
        return u8.cpu().numpy(), winner.cpu().tolist(), counts.cpu()

    def by_hand():
        frames, counts = [], []
        for c, (lo, hi) in enumerate(ramps):
            _, fr, _ = pb.predict_boxes(image_u8, lats[c], *schedule, bbox, K, aug_noise=augs[c], frames_u8=False, min_guidance=lo,
                                        max_guidance=hi, **kw)
            clean = ops.box_frames_post(fr, F, thr, pt=False, cond=False)[2]
            frames.append(fr.clone())                                   # (the next call's frames land in a fresh tensor anyway)
            counts.append(ops.mask_counts(gt, clean).cpu())             # the score of this candidate, on the host
        winner = metrics.best_of(torch.stack(counts))
        pt, cond, u8 = ops.box_frames_post(frames[winner[0]], F, thr)
        return u8.cpu().numpy(), winner, torch.stack(counts)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    routes = {"by_hand": by_hand, "one_call": one_call}
    with torch.no_grad():
        ref = {name: timed(fn)[1] for name, fn in routes.items()}                     # warm
        times = {name: [] for name in routes}
        for _ in range(args.rounds):
            for name, fn in routes.items():
                times[name].append(timed(fn)[0])
    rec = dict(tool="pipeline_plan_bench --best-of", candidates=C, size=f"{H}x{W}", frames=F, steps=steps, cond_frames=K,
               rounds=args.rounds, clip_layers=args.clip_layers, device=torch.cuda.get_device_name(0),
               same_winner=ref["by_hand"][1] == ref["one_call"][1], same_counts=bool(torch.equal(ref["by_hand"][2], ref["one_call"][2])),
               same_cleaned_bytes=bool((ref["by_hand"][0] == ref["one_call"][0]).all()))
    for name in routes:
        rec[name] = dict(call_s=round(statistics.median(times[name]), 4), all_call_s=[round(v, 4) for v in times[name]])
    rec["one_call_over_by_hand"] = round(rec["one_call"]["call_s"] / rec["by_hand"]["call_s"], 4)
    print(json.dumps(rec), flush=True)
    out_path = args.out or os.path.join(ROOT, "profiles", "box_eval_bench.jsonl")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "a") as f:
        f.write(json.dumps(rec) + "\n")


SVD = dict(in_channels=8, out_channels=4, block_out_channels=(320, 640, 1280, 1280), layers_per_block=2,
           down_block_types=("CrossAttnDownBlockSpatioTemporal",) * 3 + ("DownBlockSpatioTemporal",),
           up_block_types=("UpBlockSpatioTemporal",) + ("CrossAttnUpBlockSpatioTemporal",) * 3,
           num_attention_heads=(5, 10, 20, 20), cross_attention_dim=1024, addition_time_embed_dim=256,
           projection_class_embeddings_input_dim=768, num_frames=25)
VAE = dict(in_channels=3, out_channels=3, latent_channels=4, layers_per_block=2, block_out_channels=(128, 256, 512, 512),
           scaling_factor=0.18215)
SEEDED_SIZES = (((375, 1242), (320, 512)), ((720, 1280), (576, 1024)))


def seeded_main(args):
    """--seeded: what fills a clip request before the loop, per clip.  `prepare`: the source image's bytes go up and
    ctrlv_pipeline_prepare resizes, draws and tabulates (PipelinePlan._stage_request + prepare).  `host`: what the pipelines'
    plan route does today -- PIL's Lanczos resize, the upload, randn_tensor twice with a CPU generator (augmentation noise
    fp32, latents in bf16 times init_noise_sigma, widened), EulerDiscreteScheduler.set_timesteps.  Alternated `--rounds` times
    after one warm call each; host clock around synchronised phases."""
    import __graft_entry__ as g
    g.build()
    from PIL import Image
    from ctrlv_amd.pipelines.pipeline_utils import randn_tensor
    from ctrlv_amd.plan import ClipPlan, PipelinePlan, Plan, VaePlan
    from ctrlv_amd.schedulers import EulerDiscreteScheduler
    F, steps = args.frames, args.steps
    pipe = PipelinePlan(Plan("unet", SVD, DEV), None, VaePlan(VAE, DEV), ClipPlan(VIT_H, DEV))      # configurations only
    sched = EulerDiscreteScheduler()
    for (SH, SW), (H, W) in SEEDED_SIZES:
        src = torch.randint(0, 256, (SH, SW, 3), generator=torch.Generator().manual_seed(3), dtype=torch.uint8).numpy()
        image = Image.fromarray(src)

        def prepare_route():
            image_u8 = torch.from_numpy(src[None]).to(DEV)
            st = pipe._stage_request("bench", image_u8, seed=7, num_steps=steps, num_frames=F, height=H, width=W, frames=False,
                                     frames_u8=False)
            return pipe.prepare(st.request, st.seed_request), st

        def host_route():
            gen = torch.Generator().manual_seed(7)
            image_u8 = torch.from_numpy(np.asarray(image.resize((W, H), resample=Image.LANCZOS))[None].copy()).to(DEV)
            sched.set_timesteps(steps, device=DEV)
            aug = randn_tensor((1, 3, H, W), generator=gen, device=torch.device(DEV), dtype=torch.float32)
            lat = randn_tensor((1, F, 4, H // 8, W // 8), generator=gen, device=torch.device(DEV), dtype=torch.bfloat16)
            return image_u8, aug, (lat * sched.init_noise_sigma).float(), list(sched._sigmas_host), list(sched._timesteps_host)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        routes = {"host": host_route, "prepare": prepare_route}
        for fn in routes.values():
            timed(fn)                                                                     # warm
        times = {name: [] for name in routes}
        for _ in range(args.rounds):
            for name, fn in routes.items():
                times[name].append(timed(fn)[0])
        rec = dict(tool="pipeline_plan_bench --seeded", source=f"{SH}x{SW}", size=f"{H}x{W}", frames=F, steps=steps,
                   rounds=args.rounds, device=torch.cuda.get_device_name(0))
        for name in routes:
            rec[name] = dict(clip_ms=round(1e3 * statistics.median(times[name]), 3),
                             all_clip_ms=[round(1e3 * v, 3) for v in times[name]])
        rec["prepare_over_host"] = round(rec["prepare"]["clip_ms"] / rec["host"]["clip_ms"], 4)
        print(json.dumps(rec), flush=True)
        out_path = args.out or os.path.join(ROOT, "profiles", "pipeline_plan_bench.jsonl")
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeded", action="store_true", help="time the prepare phase (appends to profiles/pipeline_plan_bench.jsonl)")
    ap.add_argument("--boxes", action="store_true", help="time the boxes-to-video chain (appends to profiles/box_chain_bench.jsonl)")
    ap.add_argument("--best-of", type=int, default=0, metavar="C", help="time the best-of-C candidate loop, C in 1 .. 8 (appends to "
                    "profiles/box_eval_bench.jsonl)")
    ap.add_argument("--cond-frames", type=int, default=3, help="--boxes / --best-of: num_cond_bbox_frames")
    ap.add_argument("--out", default=None)
    ap.add_argument("--height", type=int, default=576)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=25)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--steps-lo", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--clip-layers", type=int, default=32)
    args = ap.parse_args()
    if args.best_of:
        if not 1 <= args.best_of <= len(RAMPS):
            ap.error("--best-of takes 1 to 8 candidates")
        return best_main(args)
    if args.boxes:
        return boxes_main(args)
    if args.seeded:
        return seeded_main(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "pipeline_plan_bench.jsonl")
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
