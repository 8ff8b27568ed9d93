#!/usr/bin/env python
"""Kernel time and gaps of ONE batch-1 CLIP ViT-H/14 encode on a HIP route, from a kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/clip_trace.py run --route ops|plan [--dtype bf16|fp16]
    python tools/clip_trace.py summarise OUT --route ops|plan --dtype bf16 [--out profiles/clip_trace_summary.jsonl]

`run` builds the random-init ViT-H of tools/clip_bench.py, warms the route up and encodes `--calls` times, a device synchronise
after each.  `summarise` reads the *kernel_trace.csv under OUT, cuts the trace at every clip_patch_rows launch (the first kernel
of an encode; the fill kernels right before it -- the plan's counter memsets -- go with it), drops the warm-up calls and reports per call (median over the calls): launches, the sum of the kernels' own
durations, the span from the first kernel's start to the last one's end, the gaps between kernels (span - kernel time), and
the kernel time per kernel family."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP = 3


def run(a):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from clip_bench import build_vit_h
    from ctrlv_amd.models import clip_vision_hip as H
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    m = build_vit_h(dtype)
    px = torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(1)).to(m.device, dtype)
    fn = H.encode_plan if a.route == "plan" else H.encode
    with torch.no_grad():
        for _ in range(WARMUP + a.calls):
            fn(m, px)
            torch.cuda.synchronize()
    print(f"{a.route} {a.dtype}: {WARMUP} + {a.calls} encodes done")


FAMILIES = (("gemm_tokens", "gemm_tokens"), ("attn_tokens", "attention_tokens"), ("act_rows", "act_rows"), ("ln_", "layernorm"),
            ("layernorm", "layernorm"), ("clip_patch_rows", "clip_patch_rows"), ("clip_tokens", "clip_tokens"), ("gemm", "gemm"),
            ("fill", "memset"), ("copy", "copy"))


def family(name):
    low = name.lower()
    for key, fam in FAMILIES:
        if key in low:
            return fam
    return "other"


def summarise(a):
    files = glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {a.dir}")
    rows = []
    for f in files:
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    starts = []
    for i, r in enumerate(rows):
        if "clip_patch_rows" in r[2]:
            while i > 0 and family(rows[i - 1][2]) == "memset" and i - 1 not in starts:
                i -= 1                    # the plan's counter memsets open its forward: they belong to THIS call
            starts.append(i)
    if len(starts) <= WARMUP:
        raise SystemExit(f"{len(starts)} encodes in the trace, more than {WARMUP} needed")
    calls = []
    for j, i0 in enumerate(starts):
        i1 = starts[j + 1] if j + 1 < len(starts) else len(rows)
        calls.append(rows[i0:i1])         # (nothing follows the last call's projection GEMM in `run`)
    calls = calls[WARMUP:]
    med = lambda xs: statistics.median(xs)      # noqa: E731
    fams = {}
    for seg in calls:
        per = {}
        for s, e, n in seg:
            per.setdefault(family(n), [0, 0.0])
            per[family(n)][0] += 1
            per[family(n)][1] += (e - s) / 1e3
        for k, (c, us) in per.items():
            fams.setdefault(k, []).append((c, us))
    rec = {"metric": "one CLIP ViT-H/14 encode, batch 1, from rocprofv3 --kernel-trace (microseconds, median over calls)",
           "route": a.route, "dtype": a.dtype, "calls": len(calls),
           "launches": med([len(seg) for seg in calls]),
           "kernel_us": round(med([sum(e - s for s, e, _ in seg) / 1e3 for seg in calls]), 1),
           "span_us": round(med([(max(e for _, e, _ in seg) - seg[0][0]) / 1e3 for seg in calls]), 1),
           "families": {k: {"launches": med([c for c, _ in v]), "kernel_us": round(med([u for _, u in v]), 1)}
                        for k, v in sorted(fams.items())}}
    rec["gaps_us"] = round(rec["span_us"] - rec["kernel_us"], 1)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--route", choices=["ops", "plan"], required=True)
    r.add_argument("--dtype", choices=["bf16", "fp16"], default="bf16")
    r.add_argument("--calls", type=int, default=10)
    s = sub.add_parser("summarise")
    s.add_argument("dir")
    s.add_argument("--route", required=True)
    s.add_argument("--dtype", default="bf16")
    s.add_argument("--out", default=None)
    a = ap.parse_args()
    run(a) if a.cmd == "run" else summarise(a)


if __name__ == "__main__":
    main()
