#!/usr/bin/env python
"""Time of one CLIP ViT-H/14 image encode -- `image_encoder(pixel_values).image_embeds`, the call that opens every pipeline call
and every step of the reference's video training loops -- on the HIP kernels, per op (models/clip_vision_hip.encode) and as one C
call (encode_plan: ctrlv_clip_forward), against the SAME module's torch forward.  Random-init weights on the device (1280 / 5120 / 32 layers / 16 heads / 224 / projection 1024),
batches 1 and 8, bf16 and fp16 elements.

The three paths ALTERNATE in one process after a warm-up (weights packed, code objects loaded, torch's GEMM choices made); every
call ends in a device synchronise and the iteration count gives each path a window of at least `--seconds`.  Reported per
case: ms per call of each (mean and median), the launch count and per-family kernel times of the HIP path (one profiled call,
HIP events around every launch, outside the timed window), the agreement of the two results, and the algorithmic FLOPs and
weight bytes.  One JSON line per case is printed and appended to profiles/clip_encode_bench.jsonl (--out)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VIT_H = dict(hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=16, image_size=224,
             patch_size=14, projection_dim=1024, hidden_act="gelu", layer_norm_eps=1e-5)


def algorithmic(cfg, n):
    """(FLOPs of one encode of n images, bytes of the weights in a 16-bit type)."""
    C, I, L = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"]
    P = (cfg["image_size"] // cfg["patch_size"]) ** 2
    S, k = P + 1, 3 * cfg["patch_size"] ** 2
    per_layer = 2.0 * S * C * 3 * C + 4.0 * S * S * C + 2.0 * S * C * C + 4.0 * S * C * I
    flops = n * (2.0 * P * k * C + L * per_layer) + n * 2.0 * C * cfg["projection_dim"]
    params = k * C + (S + 1) * C + L * (4 * C * C + 2 * C * I + 9 * C + I) + 4 * C + C * cfg["projection_dim"]
    return flops, 2.0 * params


def timed(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def run_case(m, n, seconds, warmup):
    from ctrlv_amd import profiler
    from ctrlv_amd.models import clip_vision_hip as H
    px = torch.randn(n, 3, 224, 224, generator=torch.Generator().manual_seed(n)).to(m.device, m.dtype)
    assert H.supports(m, px)
    hip = lambda: H.encode(m, px)                          # noqa: E731
    tor = lambda: m.torch_forward(px).image_embeds         # noqa: E731
    pln = lambda: H.encode_plan(m, px)                     # noqa: E731
    with torch.no_grad():
        for _ in range(warmup):
            hip(), tor(), pln()
        torch.cuda.synchronize()
        probe = max(timed(hip), timed(tor), timed(pln))
        iters = max(10, int(seconds * 1e3 / max(min(timed(hip), timed(tor), timed(pln)), 1e-3)) + 1)
        t_hip, t_tor, t_pln = [], [], []
        for _ in range(iters):                              # alternate: all see the same clock / machine state
            t_hip.append(timed(hip))
            t_tor.append(timed(tor))
            t_pln.append(timed(pln))
        with profiler.KernelTimer() as kt:
            a = hip()
        torch.cuda.synchronize()
        b = tor()
        c = pln()
    fam = {k: dict(calls=v["calls"], ms=round(v["ms"], 4)) for k, v in kt.summary().items()}
    rel = ((a.float() - b.float()).norm() / b.float().norm()).item()
    rel_plan = ((c.float() - b.float()).norm() / b.float().norm()).item()
    flops, wbytes = algorithmic(VIT_H, n)
    return {"metric": "CLIP ViT-H/14 image encode, ms per call", "batch": n, "dtype": str(m.dtype)[6:], "iters": iters,
            "hip_ms_mean": round(statistics.mean(t_hip), 4), "hip_ms_median": round(statistics.median(t_hip), 4),
            "torch_ms_mean": round(statistics.mean(t_tor), 4), "torch_ms_median": round(statistics.median(t_tor), 4),
            "plan_ms_mean": round(statistics.mean(t_pln), 4), "plan_ms_median": round(statistics.median(t_pln), 4),
            "window_s": {"hip": round(sum(t_hip) / 1e3, 3), "torch": round(sum(t_tor) / 1e3, 3), "plan": round(sum(t_pln) / 1e3, 3)},
            "first_probe_ms": round(probe, 3), "plan_launches": H.plan_launches(VIT_H["num_hidden_layers"]),
            "plan_vs_torch_rel_l2": float(f"{rel_plan:.3e}"),
            "hip_launches": len(kt.records), "hip_launches_expected": H.launches(VIT_H["num_hidden_layers"]),
            "hip_family_ms_profiled_call": fam, "hip_vs_torch_rel_l2": float(f"{rel:.3e}"),
            "algorithmic_gflop": round(flops / 1e9, 2), "weight_mbytes": round(wbytes / 1e6, 1),
            "hip_tflops": round(flops / statistics.median(t_hip) / 1e9, 2),
            "plan_tflops": round(flops / statistics.median(t_pln) / 1e9, 2), "device": torch.cuda.get_device_name(0)}


def build_vit_h(dtype, device="cuda:0"):
    """Random-init ViT-H/14 of ctrlv_amd's own class on the device, frozen."""
    from ctrlv_amd.models import CLIPVisionModelWithProjection
    from ctrlv_amd.utils import build_on_device, random_init_
    m = build_on_device(CLIPVisionModelWithProjection, device, dtype, **VIT_H).requires_grad_(False)
    random_init_(m, seed=0)                                 # Linear / Conv2d / LayerNorm; the two embeddings below
    with torch.no_grad():
        m.vision_model.embeddings.class_embedding.normal_(0.0, 0.02)
        m.vision_model.embeddings.position_embedding.weight.normal_(0.0, 0.02)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="timed window per path and case")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_encode_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_bench.py measures on the GPU; no device found")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for dtype in (torch.bfloat16, torch.float16):
        torch.manual_seed(0)
        m = build_vit_h(dtype)
        for n in a.batches:
            rec = run_case(m, n, a.seconds, a.warmup)
            line = json.dumps(rec)
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
