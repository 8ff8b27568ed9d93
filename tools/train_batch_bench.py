"""Batch preparation of one training step (plan.TrainBatchPlan.prepare: ctrlv_train_batch_prepare; csrc/train_batch_plan.hip)
against the Python route on the same plans: B clips of 25 x 320 x 512, the full-size VAE and CLIP ViT-H/14 with random
weights, bf16 elements, the ControlNet step's batch (mode 0: 2 F + 1 VAE encodes and one CLIP call per clip).

The Python route is what a user of the package wrote before, after the reference's loop (tools/train_video_controlnet.py:
366-449): the torch restatement of encode_video_image in front of the CLIP plan, three `vae.encode(...).latent_dist.sample()`
calls (the encoder runs on the same VAE plan), torch randn / randint into the scheduler's tables, the two dropout masks as
torch expressions and `_noised_inputs`.  Both routes end with everything `train_step` reads on the device.

After a warm call of each, `--rounds` rounds alternate the two routes; wall time of a whole call between two device
synchronisations, medians.  Nothing is gated: no earlier measurement of batch preparation exists.  One JSON line appended to
`--out`.  Run the whole tool under one `timeout`.

    timeout -k 10 600 python tools/train_batch_bench.py [--batch 1 --rounds 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
F, H, W = 25, 320, 512
MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
DROPOUT = 0.1


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def python_route(vae, clip, sched_sigmas, sched_timesteps, clips, boxes, generator):
    """The batch dict of `train_step`, built op by op."""
    from ctrlv_amd.models import clip_vision_hip
    from ctrlv_amd.pipelines.pipeline_utils import _resize_with_antialiasing
    from ctrlv_amd.training import _noised_inputs
    B = clips.shape[0]
    el = next(vae.parameters()).dtype
    first = clips[:, 0]
    px = torch.clamp((_resize_with_antialiasing(first.float(), (224, 224)) + 1.0) * 0.5, min=0.0, max=1.0)
    mean = torch.tensor(MEAN, device=clips.device).view(1, 3, 1, 1)
    std = torch.tensor(STD, device=clips.device).view(1, 3, 1, 1)
    ehs = clip_vision_hip.encode_plan(clip, ((px - mean) / std).to(el)).unsqueeze(1)
    sf = vae.config.scaling_factor
    image = vae.encode(first.to(el)).latent_dist.sample().float()
    control = vae.encode(boxes.flatten(0, 1).to(el)).latent_dist.sample().float().unflatten(0, (B, F))
    latents = vae.encode(clips.flatten(0, 1).to(el)).latent_dist.sample().float().unflatten(0, (B, F)) * sf
    noise = torch.randn(latents.shape, generator=generator, device=clips.device)
    indices = torch.randint(0, sched_sigmas.numel(), (B,), generator=generator, device=clips.device)
    sigmas = sched_sigmas[indices]
    random_p = torch.rand(B, generator=generator, device=clips.device)
    prompt_mask = (random_p < 2 * DROPOUT).reshape(B, 1, 1)
    ehs = torch.where(prompt_mask, torch.zeros_like(ehs), ehs)
    image_mask = 1 - ((random_p >= DROPOUT).float() * (random_p < 3 * DROPOUT).float())
    image = image_mask.reshape(B, 1, 1, 1) * image
    batch = {"latents": latents, "noise": noise, "sigmas": sigmas, "image_latents": image.unsqueeze(1).repeat(1, F, 1, 1, 1),
             "control_cond": control, "encoder_hidden_states": ehs, "timesteps": sched_timesteps[indices]}
    _, _, batch["noisy_latents"], _, batch["sample"] = _noised_inputs(batch)
    return batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_batch_bench.jsonl"))
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    os.environ.setdefault("CTRLV_VAE_HIP", "plan")           # vae.encode on the VaePlan the one call borrows (one C call per encode)
    import __graft_entry__ as g
    g.build()
    from ctrlv_amd import DeviceSeed
    from ctrlv_amd.models import AutoencoderKLTemporalDecoder, clip_vision_hip
    from ctrlv_amd.plan import TrainBatchPlan, vae_plan
    from tools.clip_bench import build_vit_h
    el, B = torch.bfloat16, args.batch
    torch.manual_seed(0)
    vae = AutoencoderKLTemporalDecoder().eval().requires_grad_(False).to(DEV, el)
    clip = build_vit_h(el, DEV)
    plan = TrainBatchPlan(vae_plan(vae, dtype=el), clip_vision_hip._plan(clip))
    gen = torch.Generator().manual_seed(1)
    clips = (torch.rand(B, F, 3, H, W, generator=gen) * 2 - 1).to(DEV)
    boxes = (torch.rand(B, F, 3, H, W, generator=gen) * 2 - 1).to(DEV)
    dgen = torch.Generator(device=DEV).manual_seed(2)
    step = [0]

    def one_call():
        step[0] += 1
        return plan.prepare(clips, boxes, mode="controlnet", seed=DeviceSeed(3), step=step[0], dropout_prob=DROPOUT)

    def by_hand():
        with torch.no_grad():
            return python_route(vae, clip, plan.sigma_table, plan.timestep_table, clips, boxes, dgen)

    _, a = wall_ms(one_call)                                 # a warm call each
    _, b = wall_ms(by_hand)
    assert a["sample"].shape == b["sample"].shape and bool(torch.isfinite(a["sample"].float()).all())
    call_t, hand_t = [], []
    for _ in range(args.rounds):                             # alternated rounds
        call_t.append(wall_ms(one_call)[0])
        hand_t.append(wall_ms(by_hand)[0])
    rec = dict(tool="train_batch_bench", size=f"{F}x{H}x{W}", batch=B, mode="controlnet", dtype="bfloat16", rounds=args.rounds,
               device=torch.cuda.get_device_name(0), vae_encodes_per_clip=2 * F + 1,
               one_call_ms=round(statistics.median(call_t), 2), all_one_call_ms=[round(v, 2) for v in call_t],
               python_route_ms=round(statistics.median(hand_t), 2), all_python_route_ms=[round(v, 2) for v in hand_t],
               workspace_mbytes=round(plan._ws.numel() / 1e6, 1))
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
