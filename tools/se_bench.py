#!/usr/bin/env python
"""Times the fused entry of the spatial transformer block at C = 320 (csrc/spatial_entry_fused.hip) against the four launches
it replaces -- GroupNorm apply, proj_in, LayerNorm, q|k|v -- at M = 50 x 9216 rows with buffer sets in rotation, after >= 2 s
of warm launches on random data (developer tool).  The statistics pass is common to both routes and timed on its own line.
Prints one JSON line per measurement."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ctrlv_amd import ops, packing  # noqa: E402

DEV = "cuda:0"
N, S, C = 50, int(os.environ.get("SE_S", 9216)), 320
M = N * S
g = torch.Generator(device=DEV).manual_seed(0)
r = lambda *s: torch.randn(*s, generator=g, device=DEV)      # noqa: E731
win, b_in = packing.pack_linear(r(C, C) / C ** 0.5), r(C)
wqkv = packing.pack_qkv(r(C, C) / C ** 0.5, r(C, C) / C ** 0.5, r(C, C) / C ** 0.5)
wf = ops.spatial_entry_fused_pack(win, wqkv)
gn, ln = (r(C), r(C)), (r(C), r(C), 1e-5)
NSET = 3
bf = torch.bfloat16
sets = [dict(x=(r(M, C) * 1.5 + 3).to(bf), tt=torch.empty(M, C, dtype=bf, device=DEV), h0=torch.empty(M, C, dtype=bf, device=DEV),
             qkv=torch.empty(M, 3 * C, dtype=bf, device=DEV),
             part=torch.empty(ops.groupnorm_scratch_floats(N, S, C, 1), dtype=torch.float32, device=DEV)) for _ in range(NSET)]
for b in sets:
    b["stats"] = ops.groupnorm_stats(b["x"], N, S, C, 1, 1e-6, b["part"])


def stats_only(b):
    ops.groupnorm_stats(b["x"], N, S, C, 1, 1e-6, b["part"])


def four(b):
    ops.groupnorm_apply(b["x"], N, S, C, 1, gn[0], gn[1], False, b["tt"], b["part"])
    ops.gemm(b["tt"], win, b["h0"], N=C, cin=C, bias=b_in)
    ops.layernorm(b["h0"], ln[0], ln[1], 1e-5, b["tt"])
    ops.gemm(b["tt"], wqkv, b["qkv"], N=3 * C, cin=C, n_scale2=C, s_acc2=ops.Q_PRESCALE)


def fused(b):
    ops.spatial_entry_fused(b["x"], wf, b["stats"], gn, ln, b["h0"], b["qkv"], N, S, bias_in=b_in)


def timeit(name, fn, reps=8):
    t0 = time.time()
    while time.time() - t0 < 2.0:                     # warm launches
        for b in sets:
            fn(b)
        torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        for b in sets:
            fn(b)
    e.record(); torch.cuda.synchronize()
    ms = s.elapsed_time(e) / (reps * NSET)
    print(json.dumps({"tool": "se_bench", "what": name, "M": M, "us": round(ms * 1e3, 1),
                      "tflops": round(2.0 * M * C * 4 * C / ms / 1e9, 1)}), flush=True)


for name, fn in (("statistics pass (both routes)", stats_only), ("four launches", four), ("fused", fused)) * 2:
    timeit(name, fn)
