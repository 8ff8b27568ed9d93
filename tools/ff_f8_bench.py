#!/usr/bin/env python
"""Measures the FP8 feed-forward mode (ff_dtype "f8") against what it replaces, on one device and one build.

    python tools/ff_f8_bench.py                 everything: the shapes for both element types, then bench.py with and without
                                                CTRLV_FF=f8 for both element types; results -> profiles/ff_f8_bench.jsonl
    python tools/ff_f8_bench.py --shapes bf16   (child step) the per-shape measurement for one element type

Per feed-forward shape of cfg3 (C = 640 at M = 115 200; C = 1280 at M = 28 800 and M = 7 200) the four launches of the f8
route -- quantise (+ LayerNorm), GEGLU GEMM, quantise u, output GEMM -- against the three launches they replace (layernorm and
the two ctrlv_gemm), every launch timed on its own with device events over rotating buffer sets, A and B alternated.  The
parent process never touches the GPU: every step that does is a child process under its own `timeout`, and the first step that
fails, faults or runs out of time ends the run.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(640, 115200), (1280, 28800), (1280, 7200)]      # (C, M) of cfg3's served feed-forwards
ROUNDS = 3                                                  # A / B alternations


def shapes(dtype_name, out_path):
    import torch
    from ctrlv_amd import ops, packing
    el = torch.float16 if dtype_name == "fp16" else torch.bfloat16
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g, device=dev)      # noqa: E731
    recs = []
    for C, M in SHAPES:
        I = 4 * C
        with packing.element_dtype(el):
            w1p, b1 = packing.pack_geglu(r(2 * I, C) / C ** 0.5, r(2 * I))
            w2p = packing.pack_linear(r(C, I) / I ** 0.5)
        b2, gamma, beta = r(C), 1 + 0.1 * r(C), 0.1 * r(C)
        (q1w, s1w), (q2w, s2w) = ops.quant_rows_f8(w1p), ops.quant_rows_f8(w2p)
        per_set = M * (C * 2 * 4 + I * 2 + I + 4)
        nset = max(2, min(6, int(1.5e9 // per_set)))             # rotate through more bytes than the 256 MB Infinity Cache
        sets = [dict(x=(2 * r(M, C) + 0.3).to(el), r1=r(M, C).to(el), t=torch.empty(M, C, dtype=el, device=dev),
                     u=torch.empty(M, I, dtype=el, device=dev), out=torch.empty(M, C, dtype=el, device=dev),
                     q=torch.empty(M * I, dtype=torch.uint8, device=dev), qs=torch.empty(M, device=dev)) for _ in range(nset)]
        qa = lambda b: b["q"][:M * C].view(M, C)                 # noqa: E731
        qu = lambda b: b["q"].view(M, I)                         # noqa: E731
        launches = {
            "same": [("layernorm", lambda b: ops.layernorm(b["x"], gamma, beta, 1e-5, b["t"])),
                     ("gemm_geglu", lambda b: ops.gemm(b["t"], w1p, b["u"], N=2 * I, cin=C, bias=b1, geglu=1)),
                     ("gemm_out", lambda b: ops.gemm(b["u"], w2p, b["out"], N=C, cin=I, bias=b2, R1=b["r1"]))],
            "f8": [("quant_ln", lambda b: ops.quant_rows_f8(b["x"], qa(b), b["qs"], ln=(gamma, beta, 1e-5))),
                   ("gemm_f8_geglu", lambda b: ops.gemm_f8(qa(b), b["qs"], q1w, s1w, b["u"], N=2 * I, cin=C, bias=b1, geglu=1)),
                   ("quant_u", lambda b: ops.quant_rows_f8(b["u"], qu(b), b["qs"])),
                   ("gemm_f8_out", lambda b: ops.gemm_f8(qu(b), b["qs"], q2w, s2w, b["out"], N=C, cin=I, bias=b2, R1=b["r1"]))],
        }
        times = {k: {n: [] for n, _ in v} for k, v in launches.items()}
        for rnd in range(ROUNDS + 1):                            # round 0 warms every launch up
            for route in ("same", "f8"):
                for name, fn in launches[route]:
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    for _ in range(2):
                        for b in sets:
                            fn(b)
                    e.record()
                    torch.cuda.synchronize()
                    if rnd:
                        times[route][name].append(s.elapsed_time(e) * 1e3 / (2 * nset))
        med = lambda v: sorted(v)[len(v) // 2]                   # noqa: E731
        rec = dict(kind="ff_shape", dtype=dtype_name, C=C, M=M, rounds=ROUNDS, buffer_sets=nset, device=torch.cuda.get_device_name(0),
                   us={k: {n: round(med(v), 1) for n, v in t.items()} for k, t in times.items()},
                   us_all={k: {n: [round(x, 1) for x in v] for n, v in t.items()} for k, t in times.items()})
        rec["us_total"] = {k: round(sum(rec["us"][k].values()), 1) for k in rec["us"]}
        flop = 2.0 * M * C * (2 * I + I)
        rec["tflops_gemms"] = {"same": round(flop / (rec["us"]["same"]["gemm_geglu"] + rec["us"]["same"]["gemm_out"]) / 1e6, 1),
                               "f8": round(flop / (rec["us"]["f8"]["gemm_f8_geglu"] + rec["us"]["f8"]["gemm_f8_out"]) / 1e6, 1)}
        rec["speedup"] = round(rec["us_total"]["same"] / rec["us_total"]["f8"], 3)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
        del sets
        torch.cuda.empty_cache()
    with open(out_path, "a") as f:
        for rec in recs:
            f.write(json.dumps(rec) + "\n")


def child(cmd, limit, env=None):
    """one GPU step: its own process under its own time limit; (exit status, stdout)"""
    full = ["timeout", "-k", "10", str(limit)] + cmd
    print("+", " ".join(full), flush=True)
    p = subprocess.run(full, cwd=ROOT, env=env, stdout=subprocess.PIPE, text=True)
    sys.stdout.write(p.stdout[-4000:])
    sys.stdout.flush()
    return p.returncode, p.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", choices=["bf16", "fp16"], help="child step: measure the shapes for one element type")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ff_f8_bench.jsonl"))
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-bench", action="store_true", help="the shapes only")
    ap.add_argument("--bench-rounds", type=int, default=2, help="same / f8 alternations of bench.py per element type")
    a = ap.parse_args()
    if a.shapes:
        shapes(a.shapes, a.out)
        return 0
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").close()
    for dt in ("bf16", "fp16"):
        rc, _ = child([sys.executable, os.path.abspath(__file__), "--shapes", dt, "--out", a.out], 300)
        if rc != 0:
            print(f"shapes {dt}: exit status {rc}; stopping", flush=True)
            return rc
    if a.no_bench:
        return 0
    for dt in ("bf16", "fp16"):
        for _ in range(a.bench_rounds):
            for mode in ("same", "f8"):
                env = dict(os.environ, CTRLV_FF=mode)
                rc, out = child([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(a.steps), "--warmup",
                                 str(a.warmup), "--dtype", dt], 420, env)
                if rc != 0:
                    print(f"bench {dt} CTRLV_FF={mode}: exit status {rc}; stopping", flush=True)
                    return rc
                line = [ln for ln in out.splitlines() if ln.startswith("{")][-1]
                res = json.loads(line)
                rec = dict(kind="bench", dtype=dt, ff=mode, steps=a.steps, warmup=a.warmup, ms_per_step=res.get("ms_per_step"),
                           value=res.get("value"), unit=res.get("unit"), finite=res.get("finite"), time=time.strftime("%Y-%m-%d %H:%M:%S"))
                with open(a.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
