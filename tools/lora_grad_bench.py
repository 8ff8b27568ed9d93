#!/usr/bin/env python
"""ctrlv_lora_grad (csrc/lora.hip) against the naive merged-weight chain, for every (M, Cin, N, g) of the stage-1 LoRA step
(B = 1, 25 frames; the q|k|v call with g = 3 and the to_out call with g = 1 of the spatial and the temporal attn1 of every
transformer) at 320 x 512 and 576 x 1024.  The naive chain treats W' as a leaf: dW' = ctrlv_gemm_wgrad (deterministic form),
then dA_i = s B_i^T dW'_i and dB_i = s dW'_i A_i^T.  The two are timed in the same process, alternating call by call (HIP
events, median of --reps).  TB/s = the bytes of X and dY (the minimum either must read) / time.  The last lines weight every
shape by its count per step.
usage: python tools/lora_grad_bench.py [--rank 4] [--reps 20]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# transformers of the SVD UNet per (channels, latent downscale): down blocks 0-2 (2 each), mid (1), up blocks 1-3 (3 each)
LEVELS = ((320, 1, 5), (640, 2, 5), (1280, 4, 5), (1280, 8, 1))


def shapes(h, w, frames=25):
    """[(tag, M, Cin, N, g, calls per step)]: per transformer the spatial and the temporal attn1 -> 2 calls of each kind"""
    out = []
    for c, d, n_tr in LEVELS:
        M = frames * (h // d) * (w // d)
        out.append((f"{c} qkv  {h // d}x{w // d}", M, c, 3 * c, 3, 2 * n_tr))
        out.append((f"{c} out  {h // d}x{w // d}", M, c, c, 1, 2 * n_tr))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from ctrlv_amd import ops
    dev = torch.device("cuda:0")
    r, s = args.rank, 1.0
    ev = lambda: torch.cuda.Event(enable_timing=True)     # noqa: E731
    print(f"ctrlv_lora_grad vs naive chain (ctrlv_gemm_wgrad + dA / dB from dW'), rank {r}, bf16, median of {args.reps}")
    print(f"{'size':>9} {'shape':<20} {'M':>7} {'Cin':>5} {'N':>5} {'g':>2} {'calls':>5} {'lora ms':>8} {'TB/s':>6} "
          f"{'naive ms':>9} {'TB/s':>6} {'naive/lora':>10}")
    for (H, W) in ((40, 64), (72, 128)):
        tot_l = tot_n = 0.0
        for tag, M, cin, N, g, calls in shapes(H, W):
            gen = torch.Generator(device=dev).manual_seed(M + N)
            X = torch.randn(M, cin, device=dev, generator=gen).to(torch.bfloat16)
            dY = torch.randn(M, N, device=dev, generator=gen).to(torch.bfloat16)
            A = torch.randn(g * r, cin, device=dev, generator=gen) / r
            B = torch.randn(N, r, device=dev, generator=gen) * 0.01
            dW = torch.empty(N, cin, device=dev)
            ng = N // g

            def lora():
                ops.lora_grad(X, dY, A, B, g, s)

            def naive():
                ops.gemm_wgrad(X, dY, dW, N=N, cin=cin, torch_layout=True, assign=True)
                for i in range(g):
                    wi = dW[i * ng:(i + 1) * ng]
                    (s * B[i * ng:(i + 1) * ng].t()) @ wi
                    (s * wi) @ A[i * r:(i + 1) * r].t()

            for f in (lora, naive, lora, naive):         # warm-up (scratch allocation, first launches)
                f()
            tl, tn = [], []
            for _ in range(args.reps):
                for f, acc in ((lora, tl), (naive, tn)):
                    e0, e1 = ev(), ev()
                    e0.record()
                    f()
                    e1.record()
                    e1.synchronize()
                    acc.append(e0.elapsed_time(e1))
            ml, mn = sorted(tl)[len(tl) // 2], sorted(tn)[len(tn) // 2]
            gb = (X.numel() + dY.numel()) * 2 / 1e9
            tot_l += calls * ml
            tot_n += calls * mn
            print(f"{H * 8}x{W * 8:<5} {tag:<20} {M:>7} {cin:>5} {N:>5} {g:>2} {calls:>5} {ml:>8.3f} {gb / ml:>6.2f} "
                  f"{mn:>9.3f} {gb / mn:>6.2f} {mn / ml:>10.2f}")
            del X, dY, dW
        print(f"{H * 8}x{W * 8}: all LoRA factor gradients of one step: ctrlv_lora_grad {tot_l:.2f} ms, naive chain "
              f"{tot_n:.2f} ms (ratio {tot_l / tot_n:.2f})")


if __name__ == "__main__":
    main()
