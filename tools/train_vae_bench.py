#!/usr/bin/env python
"""Time of one VAE decoder fine-tuning step (tools/train_vae_finetuning.py:303-320: frozen encoder, posterior sample,
decoder forward, clamp, MSE, backward, AdamW on `decoder.*`) on the HIP kernels -- ctrlv_amd.training.vae_train_step -- and,
in the same process on the same device, of the same step through the torch modules (the path the reference takes on
PyTorch-ROCm: MIOpen convolutions, SDPA).  Random-init SVD VAE, fp32 master parameters.  Prints one JSON line per mode:
ms per step and the peak device memory; the second line carries the ratio."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--height", type=int, default=320)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--num-frames", type=int, default=1, help="frames per clip (the reference trains with 1)")
    ap.add_argument("--steps", type=int, default=5, help="timed steps per mode")
    ap.add_argument("--warmup", type=int, default=2, help="untimed steps per mode (MIOpen searches on first use)")
    ap.add_argument("--modes", default="hip,torch", help="comma-separated: hip, torch")
    return ap.parse_args(argv)


def torch_module_step(vae, batch, optimizer, num_frames, generator):
    """The same step through the torch modules (autograd through `TemporalDecoder.forward`); the frozen side as in
    vae_train_step."""
    import torch
    import torch.nn.functional as F
    px = batch["pixel_values"]
    with torch.no_grad():
        z = vae.encode(px).latent_dist.sample(generator)
    loss = F.mse_loss(vae.decoder(z, num_frames).clamp(-1.0, 1.0).float(), px.float())
    loss.backward()
    optimizer.step()
    optimizer.zero_grad(set_to_none=True)
    return loss.detach()


def main(argv=None):
    a = parse(argv)
    import torch
    from ctrlv_amd.models import AutoencoderKLTemporalDecoder
    from ctrlv_amd.training import vae_train_step
    dev = "cuda:0"
    torch.manual_seed(0)
    px = (torch.rand(a.batch, 3, a.height, a.width, device=dev) * 2 - 1)
    batch = {"pixel_values": px}
    results = {}
    for mode in a.modes.split(","):
        torch.manual_seed(1)
        vae = AutoencoderKLTemporalDecoder().to(dev).eval()
        for n, p in vae.named_parameters():
            p.requires_grad_(n.startswith("decoder."))
        opt = torch.optim.AdamW(vae.decoder.parameters(), lr=1e-5, weight_decay=1e-2)
        gen = torch.Generator(device=dev).manual_seed(2)

        def step():
            if mode == "hip":
                return vae_train_step(vae, batch, opt, num_frames=a.num_frames, generator=gen)
            return torch_module_step(vae, batch, opt, a.num_frames, gen)

        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            loss = step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        results[mode] = ms
        rec = dict(tool="train_vae_bench", mode=mode, height=a.height, width=a.width, batch=a.batch, num_frames=a.num_frames,
                   steps=a.steps, warmup=a.warmup, ms_per_step=round(ms, 2), loss=round(float(loss), 6),
                   peak_mem_gib=round(torch.cuda.max_memory_allocated() / 2**30, 2), device=torch.cuda.get_device_name(0))
        if mode == "torch" and "hip" in results:
            rec["torch_over_hip"] = round(ms / results["hip"], 2)
        print(json.dumps(rec), flush=True)
        del vae, opt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
