#!/usr/bin/env python
"""ctrlv_gemm_tokens against ctrlv_gemm on the five GEMM shapes of a CLIP ViT-H/14 layer walk -- patch embedding 640 -> 1280,
q|k|v 1280 -> 3840, out_proj 1280 -> 1280, fc1 1280 -> 5120 (with erf-GELU: the ctrlv_gemm arm is followed by ctrlv_act_rows),
fc2 5120 -> 1280 -- at M = 257 (one image) and M = 2056 (eight), bf16 and fp16 elements.

The two kernels ALTERNATE in one process after a warm-up.  Each arm's `--batch` back-to-back launches are captured ONCE in a HIP
graph and timed by device events around a replay, so that the figure is the device's time per launch (kernel + the gap to the
next one) and not the rate at which Python can issue launches (~15 us each, above several of these kernels); replays are
repeated until each arm has a window of at least `--seconds`.  `--no-graph` times eager launches instead.  One JSON line per (dtype, shape, M) is printed
and appended to profiles/gemm_tokens_bench.jsonl (--out).  The routing table of csrc/clip_plan.hip (use_tokens) is read off
this file."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("patch", 1280, 640, None, False), ("qkv", 3840, 1280, None, False), ("out_proj", 1280, 1280, None, True),
          ("fc1", 5120, 1280, "gelu", False), ("fc2", 1280, 5120, None, True)]       # name, N, K, activation, residual


def captured(fn, batch):
    """`batch` launches of fn as one graph; returns its replay."""
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(batch):
            fn()
    return graph.replay


def window(fn, batch):
    """ms per launch; fn issues `batch` launches."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / batch


def run_case(ops, dtype, name, N, K, act, res, M, seconds, batch, graph):
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(N + K + M)
    A = torch.randn(M, K, generator=gen).to(dtype).to(dev)
    W = (torch.randn(N, K, generator=gen) / K ** 0.5).to(dtype).to(dev)
    bias = torch.randn(N, generator=gen).to(dev)
    R1 = torch.randn(M, N, generator=gen).to(dtype).to(dev) if res else None
    o_tok, o_gemm = torch.empty(M, N, dtype=dtype, device=dev), torch.empty(M, N, dtype=dtype, device=dev)

    # the tokens arm runs as the CLIP plan runs it: its own workspace, the counter words cleared once (every launch leaves them
    # zero), no memset per launch
    need = ops._L(A).ctrlv_gemm_tokens_ws_bytes(M, N, K)
    ws = torch.zeros(max(need, 256), dtype=torch.uint8, device=dev)

    def tok():
        ops.gemm_tokens(A, W, o_tok, N=N, K=K, bias=bias, R1=R1, act=act, workspace=ws, ws_zeroed=True)

    def gemm():
        ops.gemm(A, W, o_gemm, N=N, cin=K, bias=bias, R1=R1)
        if act is not None:
            ops.act_rows(o_gemm, act)

    for _ in range(3):
        tok(), gemm()
    torch.cuda.synchronize()
    rel = ((o_tok.float() - o_gemm.float()).norm() / o_gemm.float().norm()).item()
    if graph:
        run_tok, run_gemm = captured(tok, batch), captured(gemm, batch)
    else:
        run_tok, run_gemm = (lambda: [tok() for _ in range(batch)]), (lambda: [gemm() for _ in range(batch)])
    run_tok(), run_gemm()
    torch.cuda.synchronize()
    t_tok, t_gemm = [], []
    while sum(t_tok) * batch < seconds * 1e3 or sum(t_gemm) * batch < seconds * 1e3:
        t_tok.append(window(run_tok, batch))
        t_gemm.append(window(run_gemm, batch))
    bn, slices = ops.gemm_tokens_plan(N, K, dtype)
    return {"metric": "us per launch, device events around " + ("a HIP-graph replay of" if graph else "eager") + " back-to-back launches", "shape": name, "M": M, "N": N, "K": K,
            "act": act, "residual": res, "dtype": str(dtype)[6:], "tokens_bn": bn, "tokens_slices": slices,
            "tokens_us_median": round(statistics.median(t_tok) * 1e3, 2), "tokens_us_mean": round(statistics.mean(t_tok) * 1e3, 2),
            "gemm_us_median": round(statistics.median(t_gemm) * 1e3, 2), "gemm_us_mean": round(statistics.mean(t_gemm) * 1e3, 2),
            "gemm_arm_launches": 2 if act else 1, "windows": len(t_tok), "batch": batch,
            "window_s": {"tokens": round(sum(t_tok) * batch / 1e3, 3), "gemm": round(sum(t_gemm) * batch / 1e3, 3)},
            "tokens_vs_gemm_rel_l2": float(f"{rel:.3e}"), "weight_mbytes": round(N * K * 2 / 1e6, 2),
            "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="timed window per arm and case")
    ap.add_argument("--batch", type=int, default=50, help="launches between one pair of events")
    ap.add_argument("--no-graph", action="store_true", help="eager launches (host issue rate included)")
    ap.add_argument("--rows", type=int, nargs="+", default=[257, 2056])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gemm_tokens_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gemm_tokens_bench.py measures on the GPU; no device found")
    from ctrlv_amd import ops
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for dtype in (torch.bfloat16, torch.float16):
        for name, N, K, act, res in SHAPES:
            for M in a.rows:
                rows = M - M // 257 if name == "patch" else M              # the patch GEMM has 256 rows per image
                line = json.dumps(run_case(ops, dtype, name, N, K, act, res, rows, a.seconds, a.batch, not a.no_graph))
                print(line, flush=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
