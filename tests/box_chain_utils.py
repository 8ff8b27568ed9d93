"""Shared by tests/test_box_chain_cpu.py and tests/test_box_frames_gpu.py (a helper module, not a conftest): the golden vectors
of tests/golden/box_chain_vectors.npz (made by tests/golden/make_box_chain_golden.py from the reference's own statements) and a
numpy restatement of the clean-up they record.

The restatement exists because the kernel computes y = clamp(x / 2 + 0.5, 0, 1) itself, in the element type: a golden input y
reaches it unchanged only where x = 2 y - 1 and the way back are exact in that type.  Where they are not, the expectation is the
restatement applied to the y the kernel does see -- and the restatement is pinned, bit for bit, to the reference's recorded output
on every golden input (test_the_restated_cleanup_is_the_references)."""
import os

import numpy as np

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "box_chain_vectors.npz"))
THRESHOLD = float(G["threshold"])
CLEAN_CASES = ("grid", "grid_rolled", "odd", "pair")
IOU_CASES = ("grid", "grid_rolled", "odd", "pair", "both_empty", "gt_empty", "pred_empty")


def cleanup_numpy(y, threshold=THRESHOLD):
    """y fp32 (F, 3, H, W) in [0, 1] -> uint8, the recipe of include/ctrlv_hip.h (ctrlv_box_frames_post, out_u8) in numpy fp32."""
    v = y.astype(np.float32) * np.float32(255)
    s = (v[:, 0] + v[:, 1]) + v[:, 2]
    v = np.where((s < np.float32(threshold))[:, None], np.float32(0), v)
    for f in range(1, y.shape[0] - 1):
        if s[f].min() > np.float32(threshold):
            v[f] = 0
    return v.astype(np.uint8)
