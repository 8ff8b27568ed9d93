#!/usr/bin/env python
"""ctrlv_adamw_step / ctrlv_ema_step alone on one MI355X (csrc/optim.hip): ms per launch and achieved bytes per second against the
traffic floor of the pass -- 28 bytes per element for AdamW (p, m, v read and written, g read), 36 with the fused EMA shadow, 12 for
the EMA update alone.  Prints one JSON line per (kernel, n).  HIP events around `--iters` back-to-back launches after `--warmup`;
the buffers are far larger than the 256 MiB Infinity Cache at the default sizes.
usage: python tools/optim_bench.py [--n 268435456,1073741825] [--iters 20] [--warmup 3]"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="268435456,1073741825", help="comma-separated element counts (2^30 + 1: two launches and a tail)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from ctrlv_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                 # noqa: E731
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731
    for n in (int(x) for x in args.n.split(",")):
        p, g = torch.randn(n, device=dev), torch.randn(n, device=dev)
        m, v, e = torch.zeros(n, device=dev), torch.zeros(n, device=dev), p.clone()

        def adamw(ema):
            _lib.check(lib.ctrlv_adamw_step(ptr(p), ptr(g), ptr(m), ptr(v), ptr(e) if ema else None, n, 1e-5, 0.9, 0.999, 1e-8, 1e-2,
                                            0.1, 0.001, 1.0, 0.999, stream()), "ctrlv_adamw_step", lib)

        def ema_only():
            _lib.check(lib.ctrlv_ema_step(ptr(e), ptr(p), n, 0.999, stream()), "ctrlv_ema_step", lib)

        for name, fn, nbytes in (("adamw", lambda: adamw(False), 28), ("adamw+ema", lambda: adamw(True), 36), ("ema", ema_only, 12)):
            for _ in range(args.warmup):
                fn()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.iters):
                fn()
            t1.record()
            torch.cuda.synchronize()
            ms = t0.elapsed_time(t1) / args.iters
            print(json.dumps({"kernel": name, "n": n, "ms": round(ms, 4), "bytes_per_element": nbytes,
                              "tb_per_s": round(n * nbytes / ms / 1e9, 3), "iters": args.iters}), flush=True)
        del p, g, m, v, e
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
