"""Box frames from coordinates: what the rendering costs, and whether it matters in the chain (csrc/box_render.hip).

Cases: 25 frames at 1280x720 and at 1242x375 with 8 and with 64 objects per frame (filled 2-D boxes plus the projected 3-D
wire: the KITTI path, 15 primitives per object), rendered at the source size and taken to 576x1024 in the element type
(ctrlv_box_frames_cond).  Per case, medians over `--rounds` timed rounds of `--iters` calls after a warm-up, HIP events around each
round, the arms alternating inside one process:
  render_ms          ctrlv_render_box_frames, binned (the product)
  render_nobin_ms    the same kernel with CTRLV_BOX_CULL=0: every tile walks every object of its frame
  cond_ms            ctrlv_box_frames_cond: render + BILINEAR resize + normalisation
  write_floor_ms     the render's output bytes at the 5.3 TB/s device copy rate; render_over_floor = render_ms / that
  vae_encode_ms      ctrlv_vae_encode of the same 25 frames at 576x1024, the step that follows in the chain
One JSON line per case, with the library's build id, into profiles/box_render_bench.jsonl.  No threshold: nothing was measured before.

    timeout -k 10 600 python tools/box_render_bench.py [--out profiles/box_render_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
COPY_RATE = 5.3e12           # bytes / s, DESIGN 3.6


def round_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def table(n_frames, per_frame, Hs, Ws, seed):
    """Random KITTI-like objects: a 2-D box of 20 .. 300 pixels and eight corners around it (two offset rectangles)."""
    from ctrlv_amd.boxes import FRAME_DTYPE, OBJECT_DTYPE, BoxTable
    from ctrlv_amd._lib import BOX_FILL, BOX_WIRE
    rng = np.random.RandomState(seed)
    n = n_frames * per_frame
    o = np.zeros(n, dtype=OBJECT_DTYPE)
    w, h = rng.randint(20, 300, n), rng.randint(20, 200, n)
    x1, y1 = rng.randint(-50, Ws - 20, n), rng.randint(-30, Hs - 20, n)
    o["x1"], o["y1"], o["x2"], o["y2"] = x1, y1, x1 + w, y1 + h
    o["fill_rgb"][:, :3] = rng.randint(50, 255, (n, 3))
    o["line_rgb"][:, :3] = rng.randint(0, 256, (n, 3))
    dx, dy = w // 4, h // 5
    # the reference's corner order: (front / back) x (left / right) x (bottom / top)
    xs = np.stack([x1 + w, x1 + w, x1 + w - dx, x1 + w - dx, x1 + dx, x1 + dx, x1, x1], axis=1)
    ys = np.stack([y1 + h, y1 + dy, y1 + h - dy, y1, y1 + h - dy, y1, y1 + h, y1 + dy], axis=1)
    o["corner"][:, :, 0], o["corner"][:, :, 1] = np.clip(xs, -8191, 8191), np.clip(ys, -8191, 8191)
    o["flags"] = BOX_FILL | BOX_WIRE
    f = np.zeros(n_frames, dtype=FRAME_DTYPE)
    f["first"], f["count"] = np.arange(n_frames) * per_frame, per_frame
    return BoxTable.from_records(o, f, 1, n_frames).to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_render_bench.jsonl"))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=25)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from ctrlv_amd import _lib, ops
    from ctrlv_amd.models import AutoencoderKLTemporalDecoder
    from ctrlv_amd.models import vae_encoder_hip as ve
    el = torch.bfloat16
    H, W, F = 576, 1024, args.frames
    torch.manual_seed(0)
    vae = AutoencoderKLTemporalDecoder().eval().to(DEV, el)
    for p in vae.parameters():
        p.requires_grad_(False)
    lines = []
    with torch.no_grad():
        for Hs, Ws in ((720, 1280), (375, 1242)):
            for per_frame in (8, 64):
                t = table(F, per_frame, Hs, Ws, seed=per_frame)
                u8 = torch.empty(1, F, 3, Hs, Ws, dtype=torch.uint8, device=DEV)
                cond = torch.empty(1, F, 3, H, W, dtype=el, device=DEV)
                ws = torch.empty(_lib.load(el).ctrlv_box_frames_cond_ws_bytes(F, Hs, Ws, H, W), dtype=torch.uint8, device=DEV)

                def render():
                    ops.render_box_frames(t, (Hs, Ws), out=u8)

                def render_nobin():
                    os.environ["CTRLV_BOX_CULL"] = "0"
                    try:
                        ops.render_box_frames(t, (Hs, Ws), out=u8)
                    finally:
                        del os.environ["CTRLV_BOX_CULL"]

                def full():
                    ops.box_frames_cond(t, (Hs, Ws), (H, W), dtype=el, out=cond, workspace=ws)

                def encode():
                    return ve.encode_plan(vae, cond.view(F, 3, H, W), scale=1.0, moments=False)[0]

                # the two arms give the same bytes
                render()
                want = u8.clone()
                render_nobin()
                torch.cuda.synchronize()
                assert torch.equal(u8, want) and bool(want.any())
                arms = {"render_ms": render, "render_nobin_ms": render_nobin, "cond_ms": full, "vae_encode_ms": encode}
                for fn in arms.values():
                    for _ in range(args.warmup if fn is not encode else 1):
                        fn()
                torch.cuda.synchronize()
                ms = {k: [] for k in arms}
                for _ in range(args.rounds):                      # the arms alternate: one round each, in turn
                    for k, fn in arms.items():
                        ms[k].append(round_ms(fn, args.iters if fn is not encode else 1))
                rec = dict(case=f"{F}x{Ws}x{Hs}", objects_per_frame=per_frame, to=f"{W}x{H}", elem="bf16")
                for k, v in ms.items():
                    rec[k] = round(statistics.median(v), 4)
                    rec[k.replace("_ms", "_min_ms")] = round(min(v), 4)
                out_bytes = F * 3 * Hs * Ws
                rec["write_floor_ms"] = round(out_bytes / COPY_RATE * 1e3, 4)
                rec["render_over_floor"] = round(rec["render_ms"] / rec["write_floor_ms"], 2)
                rec["nobin_over_binned"] = round(rec["render_nobin_ms"] / rec["render_ms"], 2)
                rec["cond_over_vae_encode"] = round(rec["cond_ms"] / rec["vae_encode_ms"], 5)
                rec.update(rounds=args.rounds, iters=args.iters, device=torch.cuda.get_device_name(0), build_id=_lib.build_id())
                print(json.dumps(rec), flush=True)
                lines.append(json.dumps(rec))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
