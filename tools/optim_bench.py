#!/usr/bin/env python
"""ctrlv_adamw_step / ctrlv_ema_step alone on one MI355X (csrc/optim.hip): ms per launch and achieved bytes per second against the
traffic floor of the pass -- 28 bytes per element for AdamW (p, m, v read and written, g read), 36 with the fused EMA shadow, 12 for
the EMA update alone.  Prints one JSON line per (kernel, n).  HIP events around `--iters` back-to-back launches after `--warmup`;
the buffers are far larger than the 256 MiB Infinity Cache at the default sizes.

--max-grad-norm X adds the clipped step of `AdamW.step(max_grad_norm=X)` -- ctrlv_grad_sumsq, ctrlv_grad_finish, ctrlv_adamw_step_dev:
32 / 40 bytes per element, one more read of g -- its two small stages alone, and what a user has without it:
torch.nn.utils.clip_grad_norm_ followed by the plain step (at its best here: ONE flat gradient tensor, where a model has hundreds;
a norm pass, a read-modify-write of g, then the step: 40 / 48 bytes per element).  The variants of one n are timed `--repeats` times
in turn, so that a drift of the machine shows as a spread of every row and not as a difference between rows.
--loss-scale {dynamic,<number>} adds the loss-scaled step of `AdamW.step(scaler=...)` -- ctrlv_grad_sumsq, ctrlv_grad_finish_scaled,
ctrlv_adamw_step_scaled: the same 32 / 40 bytes per element as the clipped step, with --max-grad-norm as its max_norm (+inf without).
usage: python tools/optim_bench.py [--n 268435456,1073741825] [--iters 20] [--warmup 3] [--max-grad-norm 1.0] [--loss-scale dynamic]
                                   [--repeats 3]"""
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
    ap.add_argument("--max-grad-norm", type=float, default=None, help="also time the clipped step and its alternatives")
    ap.add_argument("--loss-scale", default="none", help="none | dynamic | a number: also time the loss-scaled three-stage step")
    ap.add_argument("--repeats", type=int, default=1, help="time every variant of an n this many times, in turn")
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from ctrlv_amd import _lib, optim
    lib = _lib.load()
    dev = torch.device("cuda:0")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                 # noqa: E731
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731
    for n in (int(x) for x in args.n.split(",")):
        p, g = torch.randn(n, device=dev), torch.randn(n, device=dev)
        m, v, e = torch.zeros(n, device=dev), torch.zeros(n, device=dev), p.clone()
        hyper = (1e-5, 0.9, 0.999, 1e-8, 1e-2, 0.1, 0.001, 1.0, 0.999)

        def adamw(ema):
            _lib.check(lib.ctrlv_adamw_step(ptr(p), ptr(g), ptr(m), ptr(v), ptr(e) if ema else None, n, *hyper, stream()),
                       "ctrlv_adamw_step", lib)

        def ema_only():
            _lib.check(lib.ctrlv_ema_step(ptr(e), ptr(p), n, 0.999, stream()), "ctrlv_ema_step", lib)

        variants = [("adamw", lambda: adamw(False), 28), ("adamw+ema", lambda: adamw(True), 36), ("ema", ema_only, 12)]
        if args.max_grad_norm is not None:
            slots = lib.ctrlv_grad_sumsq_partials(n)
            partials = torch.zeros(slots, dtype=torch.float64, device=dev)
            state = torch.zeros(4, dtype=torch.int32, device=dev)
            param = torch.nn.Parameter(p.detach(), requires_grad=True)        # (shares p's memory: only its .grad is used)
            param.grad = g

            def sumsq():
                _lib.check(lib.ctrlv_grad_sumsq(ptr(g), n, ptr(partials), slots, 0, stream()), "ctrlv_grad_sumsq", lib)

            def finish():
                _lib.check(lib.ctrlv_grad_finish(ptr(partials), slots, 1.0, args.max_grad_norm, ptr(state), stream()),
                           "ctrlv_grad_finish", lib)

            def clipped(ema):
                sumsq()
                finish()
                _lib.check(lib.ctrlv_adamw_step_dev(ptr(p), ptr(g), ptr(m), ptr(v), ptr(e) if ema else None, n, *hyper, ptr(state),
                                                    stream()), "ctrlv_adamw_step_dev", lib)

            def torch_clip(ema):
                torch.nn.utils.clip_grad_norm_([param], args.max_grad_norm)
                adamw(ema)

            variants += [("grad_sumsq", sumsq, 4), ("grad_finish", finish, 8.0 * slots / n),
                         ("clip+adamw", lambda: clipped(False), 32), ("clip+adamw+ema", lambda: clipped(True), 40),
                         ("torch_clip_grad_norm+adamw", lambda: torch_clip(False), 40),
                         ("torch_clip_grad_norm+adamw+ema", lambda: torch_clip(True), 48)]
        scaler = optim.loss_scaler_from_option(args.loss_scale)
        if scaler is not None:
            ls = scaler._record_on(dev)
            ls_slots = lib.ctrlv_grad_sumsq_partials(n)
            ls_partials = torch.zeros(ls_slots, dtype=torch.float64, device=dev)
            ls_state = torch.zeros(4, dtype=torch.int32, device=dev)
            ls_norm = float("inf") if args.max_grad_norm is None else args.max_grad_norm

            def scaled(ema):
                _lib.check(lib.ctrlv_grad_sumsq(ptr(g), n, ptr(ls_partials), ls_slots, 0, stream()), "ctrlv_grad_sumsq", lib)
                _lib.check(lib.ctrlv_grad_finish_scaled(ptr(ls_partials), ls_slots, 1.0, ls_norm, ptr(ls), ptr(ls_state), stream()),
                           "ctrlv_grad_finish_scaled", lib)
                _lib.check(lib.ctrlv_adamw_step_scaled(ptr(p), ptr(g), ptr(m), ptr(v), ptr(e) if ema else None, n, *hyper[:7], hyper[8],
                                                       ptr(ls), ptr(ls_state), stream()), "ctrlv_adamw_step_scaled", lib)

            variants += [("scaled+adamw", lambda: scaled(False), 32), ("scaled+adamw+ema", lambda: scaled(True), 40)]
        for rep in range(args.repeats):
            for name, fn, nbytes in variants:
                for _ in range(args.warmup):
                    fn()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.iters):
                    fn()
                t1.record()
                torch.cuda.synchronize()
                ms = t0.elapsed_time(t1) / args.iters
                row = {"kernel": name, "n": n, "ms": round(ms, 4), "bytes_per_element": round(nbytes, 6),
                       "tb_per_s": round(n * nbytes / ms / 1e9, 3), "iters": args.iters}
                if args.repeats > 1:
                    row["repeat"] = rep
                if args.max_grad_norm is not None:
                    row["max_grad_norm"] = args.max_grad_norm
                if scaler is not None:
                    row["loss_scale"] = args.loss_scale
                print(json.dumps(row), flush=True)
                if args.max_grad_norm is not None:
                    g.normal_()                 # torch's clip scales g in place: every variant starts from gradients of the same size
        del p, g, m, v, e, variants
        if args.max_grad_norm is not None:
            del param, partials, state
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
