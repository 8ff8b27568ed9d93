"""LPIPS of generated clips on the device (plan.LpipsPlan; csrc/lpips.hip): 8 clips x 25 frames at 256 x 410 -- the evaluation's
size -- with seeded random weights, through both libraries (bf16 and fp16 elements).

Per library: device time of the whole ctrlv_lpips_frames call from HIP events around `--iters` back-to-back calls (median of
`--rounds`), the same per stage on one chunk of 25 frame pairs through the ops-level chain (im2col, GEMM, pool, distance per
layer), the bytes the im2col rows cost per frame pair, and the accuracy table of DESIGN 3.14 re-measured: relative error against
the fp64 CPU forward (tests/lpips_ref.py) on pairs that are identical, one grey level apart and 40 levels apart, for the device,
for the emulation of its arithmetic and for a plain 16-bit forward.  Then, on the same device, the plain fp32 torch-ROCm forward
of the same network: its time for the same 200 frame pairs and its error on the same pairs -- the comparison line.  One JSON line
per run appended to `--out`.  Run the whole tool under one `timeout`.

    timeout -k 10 600 python tools/lpips_bench.py [--rounds 5 --iters 3]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
CLIPS, FRAMES, H, W = 8, 25, 256, 410
ERR_SIZES = ((37, 50, 6), (64, 96, 4))


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


def clips(seed):
    """gt in [40, 215] and gen = gt + U[-12, 12]: (CLIPS, FRAMES, 3, H, W) uint8 on the device."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.randint(40, 216, (CLIPS, FRAMES, 3, H, W), generator=g, dtype=torch.int16)
    gen = gt + torch.randint(-12, 13, gt.shape, generator=g, dtype=torch.int16)
    return gt.to(torch.uint8).to(DEV), gen.to(torch.uint8).to(DEV)


def stage_times(weights, el, gt, gen, args):
    """Device ms per stage of one chunk of FRAMES frame pairs (2 FRAMES images) through the ops-level chain."""
    from ctrlv_amd import ops
    from ctrlv_amd.models.lpips_alex import CONVS
    t = {}
    m = 2 * FRAMES
    frames = torch.cat([gt[0], gen[0]])
    h, w = (H - 7) // 4 + 1, (W - 7) // 4 + 1
    x, hw = None, None
    for l, (_, cin, cout, k, _, _) in enumerate(CONVS):
        wt, b = weights.conv(l)
        Wp, bias, lin = ops.lpips_pack_weight(wt.to(DEV), 0 if l == 0 else 1, dtype=el), b.to(DEV), weights.lin(l).to(DEV)
        if l == 0:
            A = ops.lpips_im2col_split(frames, dtype=el)
            t["im2col1"] = device_ms(lambda: ops.lpips_im2col_split(frames, dtype=el, out=A), args.warmup, args.iters, args.rounds)
        else:
            if l <= 2:
                pooled = ops.relu_maxpool_rows(x, (m, h, w))
                t[f"pool{l}"] = device_ms(lambda: ops.relu_maxpool_rows(x, (m, h, w), out=pooled), args.warmup, args.iters, args.rounds)
                x, h, w = pooled, (h - 3) // 2 + 1, (w - 3) // 2 + 1
            A = ops.lpips_im2col_split(x, k=k, hw=(m, h, w), dtype=el)
            src = x
            t[f"im2col{l + 1}"] = device_ms(lambda: ops.lpips_im2col_split(src, k=k, hw=(m, h, w), dtype=el, out=A), args.warmup,
                                            args.iters, args.rounds)
        y = torch.empty(A.shape[0], cout, dtype=torch.float32, device=DEV)
        gemm = lambda: ops.gemm(A, Wp, y, N=cout, cin=A.shape[1], bias=bias, out_f32=True, tile=1, splitk=False)     # noqa: E731
        t[f"gemm{l + 1}"] = device_ms(gemm, args.warmup, args.iters, args.rounds)
        half = y.shape[0] // 2
        t[f"distance{l + 1}"] = device_ms(lambda: ops.lpips_layer_distance(y[:half], y[half:], lin, FRAMES), args.warmup, args.iters,
                                          args.rounds)
        t[f"rows{l + 1}"] = (A.shape[0] // m, A.shape[1])
        x = y
    return t


def torch_features(weights, frames_u8, dtype):
    """The plain torch forward of the same network on the device in `dtype` (activations and weights): per-pair scores."""
    from ctrlv_amd.models.lpips_alex import CONVS, SCALE, SHIFT
    shift = torch.tensor(SHIFT, device=DEV).reshape(1, 3, 1, 1)
    scale = torch.tensor(SCALE, device=DEV).reshape(1, 3, 1, 1)
    x = ((frames_u8.float() / 127.5 - 1.0 - shift) / scale).to(dtype)
    outs = []
    for l, (_, _, _, _, stride, pad) in enumerate(CONVS):
        wt, b = weights.conv(l)
        x = torch.relu(F.conv2d(x, wt.to(DEV, dtype), b.to(DEV, dtype), stride, pad))
        outs.append(x)
        if l < 2:
            x = F.max_pool2d(x, 3, 2)
    return outs


def torch_scores(weights, gt_u8, gen_u8, dtype=torch.float32):
    n = gt_u8.shape[0]
    feats = torch_features(weights, torch.cat([gt_u8, gen_u8]), dtype)
    total = torch.zeros(n, dtype=torch.float64, device=DEV)
    for l, f in enumerate(feats):
        f = f.float()
        nrm = f / (f.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        d = (weights.lin(l).to(DEV).reshape(1, -1, 1, 1) * (nrm[:n] - nrm[n:]) ** 2).sum(1)
        total += d.double().mean(dim=(1, 2))
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_bench.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from ctrlv_amd.models.lpips_alex import LpipsAlexWeights
    from ctrlv_amd.plan import LpipsPlan
    from tests import lpips_ref as R
    weights = LpipsAlexWeights.random(0)
    gt, gen = clips(1)
    err_cases = []
    for (h, w, pairs) in ERR_SIZES:
        a, b = R.make_pairs(h, w, pairs, seed=h)
        err_cases.append((h, w, a, b, R.forward(weights, a, b)))

    def emit(rec):
        print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(json.dumps(rec) + "\n")

    def errors(score_fn):
        """{size: (error on the +-1 pair, worst error on the +-40 pairs, value on the identical pair)} against fp64."""
        out = {}
        for h, w, a, b, ref in err_cases:
            v = torch.as_tensor(score_fn(a, b), dtype=torch.float64).cpu()
            rel = ((v - ref).abs() / ref.abs())[1:]
            out[f"{h}x{w}"] = dict(pm1=float(rel[0]), pm40=float(rel[1:].max()), identical=float(v[0]))
        return out

    for el in (torch.bfloat16, torch.float16):
        plan = LpipsPlan(weights, DEV, dtype=el)
        ws = torch.empty(plan.workspace_bytes(H, W, FRAMES), dtype=torch.uint8, device=DEV)
        call_ms = device_ms(lambda: plan.frames(gt, gen, workspace=ws), args.warmup, args.iters, args.rounds)
        score = plan.frames(gt, gen, workspace=ws)
        st = stage_times(weights, el, gt, gen, args)
        rows = {k: v for k, v in st.items() if k.startswith("rows")}
        im2col_bytes = sum(2 * r * c * 2 for r, c in rows.values())                   # both frames of a pair, two bytes an element
        emit(dict(tool="lpips_bench", elements=str(el).replace("torch.", ""), clips=CLIPS, frames=FRAMES, size=f"{H}x{W}",
                  device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters,
                  call_ms=round(call_ms, 3), ms_per_frame_pair=round(call_ms / (CLIPS * FRAMES), 5), chunk_frames=FRAMES,
                  workspace_mib=round(ws.numel() / 2 ** 20, 1),
                  stage_ms_per_chunk={k: round(v, 4) for k, v in st.items() if not k.startswith("rows")},
                  stages_sum_ms_per_call=round(sum(v for k, v in st.items() if not k.startswith("rows")) * CLIPS, 3),
                  im2col_rows_per_image={k: list(v) for k, v in rows.items()},
                  im2col_mib_per_frame_pair=round(im2col_bytes / 2 ** 20, 2), mean_lpips=float(score.mean()),
                  rel_err_vs_fp64=dict(device=errors(lambda a, b: plan.frames(a[None].to(DEV), b[None].to(DEV))[0]),
                                       emulation=errors(lambda a, b: R.forward_split(weights, a, b, el)),
                                       plain_16bit_cpu=errors(lambda a, b: R.forward_plain16(weights, a, b, el)),
                                       fp32_cpu=errors(lambda a, b: R.forward(weights, a, b, torch.float32)))))
        del plan, ws
    # the comparison line: the plain fp32 torch-ROCm forward of the same network, a clip (25 frame pairs) at a time
    def torch_call():
        return torch.stack([torch_scores(weights, gt[c], gen[c]) for c in range(CLIPS)])
    t_ms = device_ms(torch_call, args.warmup, args.iters, args.rounds)
    emit(dict(tool="lpips_bench", elements="torch_fp32", clips=CLIPS, frames=FRAMES, size=f"{H}x{W}",
              device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters, call_ms=round(t_ms, 3),
              ms_per_frame_pair=round(t_ms / (CLIPS * FRAMES), 5), mean_lpips=float(torch_call().mean()),
              rel_err_vs_fp64=dict(device=errors(lambda a, b: torch_scores(weights, a.to(DEV), b.to(DEV))),
                                   torch_bf16_device=errors(lambda a, b: torch_scores(weights, a.to(DEV), b.to(DEV), torch.bfloat16)),
                                   torch_fp16_device=errors(lambda a, b: torch_scores(weights, a.to(DEV), b.to(DEV), torch.float16)))))


if __name__ == "__main__":
    main()
