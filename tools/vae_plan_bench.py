"""VAE encode / decode: the per-op executors against the one-call plan (csrc/vae_plan.hip).

Cases: encode of 26 images (the conditioning image + 25 bbox frames) and decode of 25 frames, at 576x1024 and at 320x512.
Routes: "per_op" (the default route: down-samplers as stride-1 conv + strided copy, quant_conv / posterior in torch),
"native_down" (the per-op twin with the pad_br down-samplers and ctrlv_vae_posterior; encode only) and "plan".
Per case and route: device time per call (HIP events around `--iters` calls after `--warmup`), the per-op call's
torch.cuda.max_memory_allocated delta beside the plan's workspace_bytes, and the number of C entry-point calls (a GroupNorm
is two; torch ops of the per-op routes -- zero fill, strided copy, quant_conv, posterior -- are not counted).
One process, one JSON line per case into profiles/vae_plan_bench.jsonl.  Run the whole tool under one `timeout`.

    timeout -k 10 900 python tools/vae_plan_bench.py [--out profiles/vae_plan_bench.jsonl]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def peak_delta(fn):
    """max_memory_allocated of one call above what was allocated before it (inputs, weights, persistent scratch)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    del out
    return peak - base


def c_calls(fn):
    """Status-checked C calls of one per-op call (every entry point of the executors goes through ops.check)."""
    from ctrlv_amd import ops
    n = [0]
    real = ops.check

    def counting(rc, what, lib=None):
        n[0] += 1
        return real(rc, what, lib) if lib is not None else real(rc, what)
    ops.check = counting
    try:
        fn()
    finally:
        ops.check = real
    torch.cuda.synchronize()
    return n[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vae_plan_bench.jsonl"))
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--sizes", default="576x1024,320x512")
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from ctrlv_amd import ops
    from ctrlv_amd.models import AutoencoderKLTemporalDecoder
    from ctrlv_amd.models import vae_decoder_hip as vh
    from ctrlv_amd.models import vae_encoder_hip as ve
    from ctrlv_amd.plan import vae_plan
    torch.manual_seed(0)
    vae = AutoencoderKLTemporalDecoder().eval().to(DEV, torch.bfloat16)
    for p in vae.parameters():
        p.requires_grad_(False)
    plan = vae_plan(vae)
    sf = vae.config.scaling_factor
    qw = vae.quant_conv.weight.detach().float().reshape(8, 8).contiguous()
    qb = vae.quant_conv.bias.detach().float().contiguous()
    lines = []
    with torch.no_grad():
        for size in args.sizes.split(","):
            H, W = (int(v) for v in size.split("x"))
            x = (torch.rand(26, 3, H, W, device=DEV) * 2 - 1).to(torch.bfloat16)
            z = torch.randn(25, 4, H // 8, W // 8, device=DEV).to(torch.bfloat16)

            def enc_per_op():
                return vae.quant_conv(ve.encode(vae.encoder, x))[:, :4] * sf          # latent_dist.mode() * scaling_factor

            def enc_native_down():       # the per-op twin of the plan: pad_br down-samplers, then ctrlv_vae_posterior
                rows = ve.encode(vae.encoder, x, native_down=True, rows=True)
                lat = torch.empty(26, 4, H // 8, W // 8, dtype=x.dtype, device=DEV)
                return ops.vae_posterior(rows, 26, 4, (H // 8) * (W // 8), qw, qb, None, sf, None, lat)[1]

            enc = {"per_op": enc_per_op,
                   "native_down": enc_native_down,
                   "plan": lambda: ve.encode_plan(vae, x, scale=sf, moments=False)[0]}
            dec = {"per_op": lambda: vh.decode(vae.decoder, z, 25),
                   "plan": lambda: vh.decode_plan(vae, z, 25)}
            for what, routes, ws in (("encode", enc, plan.workspace_bytes("encode", 26, 1, H, W)),
                                     ("decode", dec, plan.workspace_bytes("decode", 25, 25, H // 8, W // 8))):
                ms = {k: round(timed(f, args.warmup, args.iters), 3) for k, f in routes.items()}
                rec = dict(case=what, size=size, n=26 if what == "encode" else 25, ms=ms,
                           per_op_peak_bytes=peak_delta(routes["per_op"]), plan_workspace_bytes=ws,
                           c_calls={k: c_calls(f) for k, f in routes.items() if k != "plan"}, plan_c_calls=1,
                           device=torch.cuda.get_device_name(0), iters=args.iters)
                rec["workspace_over_per_op_peak"] = round(ws / rec["per_op_peak_bytes"], 4)
                print(json.dumps(rec), flush=True)
                lines.append(json.dumps(rec))
            del x, z
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
