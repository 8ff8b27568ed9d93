#!/usr/bin/env python
"""Golden vectors for the kernels between the box predictor and Box2Video, produced BY THE REFERENCE'S OWN CODE (build container
only: reads /root/reference, which does not exist on the GPU box).  As tests/golden/make_ref_helpers.py does, this script takes

  * the clean-up statements of tools/eval_overall.py:96-105 (the predicted box frames times 255, dark pixels zeroed, box-less
    interior frames zeroed, truncated to uint8), and
  * `binary_mask_iou` of src/ctrlv/metrics/FandJ.py:11-23

out of the reference files with `ast` (no reference text is written into this repository), executes them here on seeded inputs
and stores inputs + outputs in tests/golden/box_chain_vectors.npz.  The inputs are built so that every branch of the clean-up
occurs, and the script asserts that on the reference's own output.
usage: python tests/golden/make_box_chain_golden.py"""
import ast
import os

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
THRESHOLD = 50.0


def _targets(stmt):
    if isinstance(stmt, ast.Assign):
        return [t.id if isinstance(t, ast.Name) else (t.value.id if isinstance(t, ast.Subscript) and
                                                      isinstance(t.value, ast.Name) else None) for t in stmt.targets]
    return []


def cleanup_statements(path):
    """The statements between `bbox_im = bbox_pipeline(...)` and `bbox_frames = bbox_frames.astype(np.uint8)` (inclusive) of
    the loop that holds them, as the reference wrote them."""
    tree = ast.parse(open(path).read())
    for node in ast.walk(tree):
        if not isinstance(node, ast.For):
            continue
        firsts = [(_targets(s) or [None])[0] for s in node.body]
        if "bbox_im" in firsts and "bbox_frames" in firsts:
            i0 = firsts.index("bbox_im") + 1
            i1 = max(i for i, s in enumerate(node.body) if isinstance(s, ast.Assign) and "astype" in ast.unparse(s))
            body = node.body[i0:i1 + 1]
            text = "\n".join(ast.unparse(s) for s in body)
            assert "< 50" in text and "> 50" in text and "astype" in text, text
            return body
    raise AssertionError("the clean-up statements were not found")


def function(path, name):
    tree = ast.parse(open(path).read())
    ns = {"np": np}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name == name:
            exec(compile(ast.Module([node], []), path, "exec"), ns)
    return ns[name]


def clean(body, path, y):
    ns = {"np": np, "bbox_im": torch.from_numpy(y.copy())}
    exec(compile(ast.Module(body, []), path, "exec"), ns)
    out = ns["bbox_frames"]
    assert out.dtype == np.uint8 and out.shape == y.shape
    return out


def sums(y):
    """Per-pixel channel sums of y * 255 as numpy forms them (fp32, (v0 + v1) + v2)."""
    return (y * np.float32(255)).sum(axis=1)


def grid(rng, shape, lo=40):
    return (rng.integers(lo, 257, size=shape) / 256.0).astype(np.float32)


def exact_fifty():
    """An fp32 triple whose fp32 channel sum is exactly the threshold."""
    y0 = y1 = np.float32(0.0625)
    y2 = np.float32(18.125 / 255.0)
    for _ in range(64):
        for cand in (y2, np.nextafter(y2, np.float32(0)), np.nextafter(y2, np.float32(1))):
            t = np.array([y0, y1, cand], dtype=np.float32)[None, :, None, None]
            if float(sums(t)[0, 0, 0]) == THRESHOLD:
                return t[0, :, 0, 0]
        y2 = np.nextafter(y2, np.float32(1))
    raise AssertionError("no exact-threshold triple found")


def main():
    path = os.path.join(REF, "tools/eval_overall.py")
    body = cleanup_statements(path)
    iou = function(os.path.join(REF, "src/ctrlv/metrics/FandJ.py"), "binary_mask_iou")
    rng = np.random.default_rng(20240607)
    out = {"threshold": np.float32(THRESHOLD)}

    # ---- grid (5, 3, 16, 24): every value k / 256, exact in bf16 and fp16 and through x = 2 y - 1
    y = grid(rng, (5, 3, 16, 24))
    y[2, :, 5, 7] = np.array([3, 4, 5], dtype=np.float32) / 256                       # the single dark pixel of frame 2
    dark = rng.random((16, 24)) < 0.3
    y[3][:, dark] = (rng.integers(0, 17, size=(3, int(dark.sum()))) / 256.0).astype(np.float32)
    # ---- odd (4, 3, 7, 13): arbitrary fp32 values, odd tails, the pixel at exactly the threshold
    z = (rng.random((4, 3, 7, 13)) * 0.9 + 0.1).astype(np.float32)
    z[0][:, rng.random((7, 13)) < 0.25] = np.float32(0.01)
    z[1, :, 3, 11] = exact_fifty()                                                     # frame 1's minimum: exactly 50
    # ---- pair (2, 3, 8, 8): no interior frame
    p = grid(rng, (2, 3, 8, 8))
    p[0][:, rng.random((8, 8)) < 0.2] = np.float32(2 / 256)
    cases = {"grid": y, "grid_rolled": y[[1, 2, 3, 4, 0]].copy(), "odd": z, "pair": p}
    for name, v in cases.items():
        out[name + "_y"], out[name + "_u8"] = v, clean(body, path, v)

    # ---- every branch occurs, on the reference's own output
    s, u = sums(y), out["grid_u8"]
    assert (s[0] >= THRESHOLD).all() and u[0].any() and (s[4] >= THRESHOLD).all() and u[4].any()      # first / last: kept
    assert s[1].min() > THRESHOLD and not u[1].any()                                                  # box-less interior: blanked
    assert int((s[2] < THRESHOLD).sum()) == 1 and u[2].any() and not u[2, :, 5, 7].any()               # single dark pixel: kept
    assert (s[3] < THRESHOLD).sum() > 10 and not u[3][:, s[3] < THRESHOLD].any() and u[3][:, s[3] >= THRESHOLD].all()
    v = y * np.float32(255)
    frac = (v != np.floor(v)) & (np.repeat(s[:, None] >= THRESHOLD, 3, axis=1))
    frac[1] = False
    assert frac.any() and (u[frac] == np.floor(v[frac])).all()                                        # truncation, not rounding
    r = out["grid_rolled_u8"]
    assert r[0].any() and r[4].any() and not r[3].any() and r[1].any() and r[2].any()                  # the rule is positional
    s, u = sums(z), out["odd_u8"]
    assert float(s[1, 3, 11]) == THRESHOLD and s[1].min() == THRESHOLD and u[1, :, 3, 11].any() and u[1].any()
    assert s[2].min() > THRESHOLD and not u[2].any() and (s[0] < THRESHOLD).any() and u[3].any()
    u = out["pair_u8"]
    assert u[0].any() and u[1].all() and not u[0][:, sums(p)[0] < THRESHOLD].any()

    # ---- binary_mask_iou: (gt, pred) pairs, over all frames and over the first and last one
    def boxes(shape, k):
        g = np.zeros(shape, dtype=np.uint8)
        F, _, H, W = shape
        for f in range(F):
            for _ in range(k):
                y0, x0 = int(rng.integers(0, H - 2)), int(rng.integers(0, W - 2))
                y1, x1 = int(rng.integers(y0 + 1, H + 1)), int(rng.integers(x0 + 1, W + 1))
                g[f, int(rng.integers(0, 3)), y0:y1, x0:x1] = int(rng.integers(1, 256))
        return g

    gt_grid = boxes((5, 3, 16, 24), 2)
    pairs = {
        "grid": (gt_grid, out["grid_u8"]),
        "grid_rolled": (gt_grid, out["grid_rolled_u8"]),
        "odd": (boxes((4, 3, 7, 13), 1), out["odd_u8"]),
        "pair": (boxes((2, 3, 8, 8), 1), out["pair_u8"]),
        "both_empty": (np.zeros((2, 3, 8, 8), np.uint8), np.zeros((2, 3, 8, 8), np.uint8)),
        "gt_empty": (np.zeros((2, 3, 8, 8), np.uint8), out["pair_u8"]),
        "pred_empty": (boxes((2, 3, 8, 8), 1), np.zeros((2, 3, 8, 8), np.uint8)),
    }
    for name, (gt, pred) in pairs.items():
        F = gt.shape[0]
        out[f"iou_{name}_gt"], out[f"iou_{name}_pred"] = gt, pred
        out[f"iou_{name}_all"] = np.array(iou(gt, pred), dtype=np.float64)
        out[f"iou_{name}_first_last"] = np.array(iou(gt[[0, F - 1]], pred[[0, -1]]), dtype=np.float64)
        cnt = []
        for a, b in ((gt, pred), (gt[[0, F - 1]], pred[[0, -1]])):
            ma, mb = a.astype(np.int64).sum(axis=1) > 0, b.astype(np.int64).sum(axis=1) > 0
            cnt.append([int(ma.sum()), int(mb.sum()), int((ma & mb).sum())])
        out[f"iou_{name}_counts"] = np.array(cnt, dtype=np.int64)
    assert tuple(out["iou_both_empty_all"]) == (1.0, 1.0, 1.0)
    assert out["iou_gt_empty_all"][0] == 0 and out["iou_gt_empty_all"][2] == 1 and out["iou_pred_empty_all"][1] == 1
    assert 0 < out["iou_grid_all"][0] < 1
    dst = os.path.join(HERE, "box_chain_vectors.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
