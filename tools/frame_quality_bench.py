"""Per-frame SSIM / PSNR of one clip (metrics.frame_quality; csrc/frame_quality.hip, csrc/pipeline_io.hip) against the host route
on the same frames: 25 frames of 320 x 512 and of 576 x 1024, each with size=(256, 410) -- the evaluation's own resize -- and
without.  The host route is what a user of the package did before: .cpu(), PIL's bicubic resize of every frame, and the numpy
restatement of tests/frame_quality_ref.py (scipy's Gaussian filter in its place where scipy is importable).

After a warm call of each, `--rounds` rounds alternate the two routes; wall time of a whole call (it ends in the copy of the
results to the host, which synchronises), medians.  The first launch after a long host-only phase can take milliseconds by
itself, whatever it launches, so the device call is also timed `--rounds` times back to back.  Nothing is gated: no earlier
device path exists and the metric is once-per-clip work.  Beside it, device time of the SSIM and statistics kernels alone from HIP events around `--iters` back-to-back calls, the
input bytes (both clips) over that time, and the rate of a device-to-device copy of the same bytes measured the same way.  One
JSON line per case appended to `--out`.  Run the whole tool under one `timeout`.

    timeout -k 10 900 python tools/frame_quality_bench.py [--rounds 5 --iters 20]
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
SIZES = ((25, 320, 512), (25, 576, 1024))
EVAL_SIZE = (256, 410)


def clip_pair(F, H, W, seed):
    """A smooth seeded scene with noise, and a noisier copy of it: (1, F, 3, H, W) uint8 each."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    scene = torch.stack([(yy + xx) % 256, (3 * yy + xx // 2) % 256, ((yy // 16 + xx // 16) % 2) * 200 + 20])
    gt = (scene[None, None] + torch.randint(-20, 21, (1, F, 3, H, W), generator=g)).clamp(0, 255).to(torch.uint8)
    gen = (gt.long() + torch.randint(-12, 13, gt.shape, generator=g)).clamp(0, 255).to(torch.uint8)
    return gt.to(DEV), gen.to(DEV)


def host_route(gt, gen, size):
    """(ssim, psnr) float64 (F) of one clip the way the host did it."""
    from PIL import Image
    from tests import frame_quality_ref as Q
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    a, b = gt[0].cpu().numpy(), gen[0].cpu().numpy()
    if size is not None:
        h, w = size

        def pil(clip):
            return np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(f.transpose(1, 2, 0))).resize((w, h), resample=Image.BICUBIC))
                             .transpose(2, 0, 1) for f in clip])
        a, b = pil(a), pil(b)
    ssim, psnr = [], []
    for x, y in zip(a, b):
        lo, hi, sse = Q.stats(x, y)
        psnr.append(Q.psnr_from_stats(lo, hi, sse, x.size))
        if ndimage is None:
            ssim.append(Q.ssim_u8(x, y))
            continue
        f = lambda v: ndimage.gaussian_filter(v, (0, 1.5, 1.5), mode="reflect", truncate=3.5)[:, 5:-5, 5:-5]
        p, q, R = x.astype(np.float64) - 127.5, y.astype(np.float64) - 127.5, float(hi - lo)
        ux, uy, uxx, uyy, uxy = f(p), f(q), f(p * p), f(q * q), f(p * q)
        cov, C1, C2 = 121 / 120, (0.01 * R) ** 2, (0.03 * R) ** 2
        vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
        ssim.append(float((((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))).mean()))
    return np.array(ssim), np.array(psnr)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def device_ms(fn, warmup, iters, rounds):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / iters)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_quality_bench.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from ctrlv_amd import _lib, metrics, ops
    for F, H, W in SIZES:
        gt, gen = clip_pair(F, H, W, H)
        for size in (EVAL_SIZE, None):
            dev_fn, host_fn = (lambda: metrics.frame_quality(gt, gen, size=size)), (lambda: host_route(gt, gen, size))
            _, q = wall_ms(dev_fn)                       # a warm call each
            _, (hs, hp) = wall_ms(host_fn)
            dev_t, host_t = [], []
            for _ in range(args.rounds):                 # alternated rounds
                dev_t.append(wall_ms(dev_fn)[0])
                host_t.append(wall_ms(host_fn)[0])
            b2b = [wall_ms(dev_fn)[0] for _ in range(args.rounds)]          # ... and the device call back to back
            # the kernels alone, at the size they run at
            a, b = (gt, gen) if size is None else (ops.resize_frames_u8(gt, *size), ops.resize_frames_u8(gen, *size))
            h, w = a.shape[-2:]
            stats = torch.empty(1, F, 3, dtype=torch.int64, device=DEV)
            ssim = torch.empty(1, F, dtype=torch.float64, device=DEV)
            ws = torch.empty(_lib.load().ctrlv_frame_ssim_ws_bytes(1, F, h, w), dtype=torch.uint8, device=DEV)
            stats_ms = device_ms(lambda: ops.frame_stats(a, b, out=stats), args.warmup, args.iters, args.rounds)
            ssim_ms = device_ms(lambda: ops.frame_ssim(a, b, stats, out=ssim, workspace=ws), args.warmup, args.iters, args.rounds)
            nbytes = a.numel() + b.numel()
            src, dst = torch.cat([a.flatten(), b.flatten()]), torch.empty(nbytes, dtype=torch.uint8, device=DEV)
            copy_ms = device_ms(lambda: dst.copy_(src), args.warmup, args.iters, args.rounds)
            resize_ms = None
            if size is not None:
                rws = torch.empty(_lib.load().ctrlv_resize_frames_ws_bytes(F * 3, H, W, h, w, 3), dtype=torch.uint8, device=DEV)
                resize_ms = device_ms(lambda: ops.resize_frames_u8(gt, h, w, out=a, workspace=rws), args.warmup, args.iters, args.rounds)
            rec = dict(tool="frame_quality_bench", size=f"{F}x{H}x{W}", scored_at=f"{h}x{w}", resized=size is not None,
                       host_filter="scipy" if "scipy" in sys.modules else "numpy", rounds=args.rounds, iters=args.iters,
                       device=torch.cuda.get_device_name(0),
                       device_call_ms=round(statistics.median(dev_t), 3), all_device_call_ms=[round(v, 3) for v in dev_t],
                       device_call_back_to_back_ms=round(statistics.median(b2b), 3),
                       host_call_ms=round(statistics.median(host_t), 1), all_host_call_ms=[round(v, 1) for v in host_t],
                       stats_kernel_ms=round(stats_ms, 4), ssim_kernels_ms=round(ssim_ms, 4),
                       resize_one_clip_ms=None if resize_ms is None else round(resize_ms, 4),
                       input_bytes=nbytes, ssim_input_gb_per_s=round(nbytes / ssim_ms / 1e6, 1),
                       stats_input_gb_per_s=round(nbytes / stats_ms / 1e6, 1), copy_ms=round(copy_ms, 4),
                       copy_read_gb_per_s=round(nbytes / copy_ms / 1e6, 1),
                       mean_ssim=round(float(q["ssim"].mean()), 6), mean_psnr=round(float(q["psnr"].mean()), 4),
                       worst_ssim_vs_host=float(np.abs(q["ssim"][0] - hs).max()), worst_psnr_vs_host=float(np.abs(q["psnr"][0] - hp).max()))
            print(json.dumps(rec), flush=True)
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
