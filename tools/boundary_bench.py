"""The boundary F-measure's kernel (ctrlv_boundary_counts, csrc/box_eval.hip) at the two working sizes: 25 frames of 576 x 1024
at radius 10 and of 320 x 512 at radius 5, luma masks of seeded box-like frames.  Device time per call from HIP events around
`--iters` back-to-back calls after `--warmup` warm ones (the median of `--rounds` such measurements), the input bytes (ground truth
+ prediction) over that time, and beside it the rate of a device-to-device copy of the same number of bytes measured the same way.
One JSON line per size appended to `--out`.  Run the whole tool under one `timeout`.

    timeout -k 10 300 python tools/boundary_bench.py [--rounds 5 --iters 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
SIZES = ((25, 576, 1024), (25, 320, 512))


def box_frames(F, H, W, seed):
    """Frames of a few filled rectangles on black, as cleaned box frames are."""
    g = torch.Generator().manual_seed(seed)
    out = torch.zeros(1, F, 3, H, W, dtype=torch.uint8)
    for f in range(F):
        for _ in range(6):
            y0, x0 = int(torch.randint(0, H - 8, (1,), generator=g)), int(torch.randint(0, W - 8, (1,), generator=g))
            h, w = int(torch.randint(8, H // 3, (1,), generator=g)), int(torch.randint(8, W // 3, (1,), generator=g))
            out[0, f, :, y0:y0 + h, x0:x0 + w] = torch.randint(60, 256, (3, 1, 1), generator=g, dtype=torch.uint8)
    return out.to(DEV)


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
    return statistics.median(times), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_eval_bench.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from ctrlv_amd import metrics, ops
    for F, H, W in SIZES:
        gt, pred = box_frames(F, H, W, 1), box_frames(F, H, W, 2)
        r = metrics.boundary_radius(H, W)
        out = torch.empty(1, F, 4, dtype=torch.int64, device=DEV)
        ms, all_ms = device_ms(lambda: ops.boundary_counts(gt, pred, r, 1, out=out), args.warmup, args.iters, args.rounds)
        nbytes = gt.numel() + pred.numel()
        src, dst = torch.cat([gt.flatten(), pred.flatten()]), torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        copy_ms, _ = device_ms(lambda: dst.copy_(src), args.warmup, args.iters, args.rounds)
        f = metrics.boundary_f_measure(gt, pred)
        rec = dict(tool="boundary_bench", size=f"{F}x{H}x{W}", radius=r, mask="luma", iters=args.iters, rounds=args.rounds,
                   device=torch.cuda.get_device_name(0), kernel_ms=round(ms, 4), all_kernel_ms=[round(v, 4) for v in all_ms],
                   input_bytes=nbytes, input_gb_per_s=round(nbytes / ms / 1e6, 1), copy_ms=round(copy_ms, 4),
                   copy_read_gb_per_s=round(nbytes / copy_ms / 1e6, 1), mean_f=round(float(f.mean()), 6))
        print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
