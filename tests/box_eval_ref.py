"""Shared by tests/test_box_eval_cpu.py, tests/test_boundary_gpu.py and tests/test_best_boxes_gpu.py (a helper module, not a
conftest): a numpy restatement of the boundary F-measure's counts as include/ctrlv_hip.h states them (ctrlv_boundary_counts), the
masks the tests feed it, and the crafted counts of the best-of-N rule.  The dilation is an OR of shifted copies in plain numpy:
scipy may be absent where the GPU tests run.  Pinned to known answers by tests/test_box_eval_cpu.py."""
import math

import numpy as np

H0, W0 = 37, 70
RECTS = {"A": ((5, 20, 8, 40), (7, 23, 10, 45)), "B": ((20, 37, 50, 70), (22, 37, 47, 70))}        # G, P as [y0, y1) x [x0, x1)
# (case, radius) -> (n_fg, n_gt, fg_match, gt_match)
KNOWN = {("A", 1): (102, 94, 6, 6), ("A", 2): (102, 94, 48, 53), ("A", 3): (102, 94, 80, 85), ("A", 10): (102, 94, 102, 94),
         ("B", 1): (39, 38, 3, 3), ("B", 3): (39, 38, 39, 38)}
KNOWN_F = {("A", 1): 0.06122448979591836, ("A", 2): 0.513006654567453, ("A", 3): 0.840024706609018, ("A", 10): 1.0}


def rect(y0, y1, x0, x1, H=H0, W=W0):
    m = np.zeros((H, W), bool)
    m[y0:y1, x0:x1] = True
    return m


def mask_of(u8, mode):
    """u8 (..., 3, H, W) uint8 -> bool (..., H, W).  mode 0: any channel nonzero; mode 1: PIL's convert('L') != 0."""
    c = u8.astype(np.int64)
    if mode == 0:
        return (c[..., 0, :, :] | c[..., 1, :, :] | c[..., 2, :, :]) != 0
    return ((19595 * c[..., 0, :, :] + 38470 * c[..., 1, :, :] + 7471 * c[..., 2, :, :] + 0x8000) >> 16) != 0


def boundary_map(S):
    """The one-pixel boundary map of a bool (H, W) mask."""
    H, W = S.shape
    b = np.zeros((H, W), bool)
    b[:, :W - 1] |= S[:, :W - 1] != S[:, 1:]                       # the right neighbour, every row
    b[:H - 1, :] |= S[:H - 1, :] != S[1:, :]                       # the lower neighbour, every column
    b[:H - 1, :W - 1] |= S[:H - 1, :W - 1] != S[1:, 1:]            # the diagonal one
    return b


def radius(H, W, bound_th=0.008):
    return int(bound_th) if bound_th >= 1 else int(math.ceil(bound_th * math.sqrt(float(H * H + W * W))))


def dilate(b, r):
    """OR of b[y + dy, x + dx] over dx^2 + dy^2 <= r^2, nothing from outside the image."""
    H, W = b.shape
    out = np.zeros((H, W), bool)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dx * dx + dy * dy > r * r:
                continue
            ys, ye = max(0, -dy), min(H, H - dy)                     # output rows whose source row y + dy is inside
            xs, xe = max(0, -dx), min(W, W - dx)
            if ys < ye and xs < xe:
                out[ys:ye, xs:xe] |= b[ys + dy:ye + dy, xs + dx:xe + dx]
    return out


def frame_counts(G, P, r):
    bg, bp = boundary_map(G), boundary_map(P)
    return int(bp.sum()), int(bg.sum()), int((bp & dilate(bg, r)).sum()), int((bg & dilate(bp, r)).sum())


def boundary_counts(gt_u8, pred_u8, mode, r):
    """(n, F, 3, H, W) uint8 twice -> int64 (n, F, 4)."""
    G, P = mask_of(gt_u8, mode), mask_of(pred_u8, mode)
    n, F = G.shape[:2]
    return np.array([[frame_counts(G[i, f], P[i, f], r) for f in range(F)] for i in range(n)], dtype=np.int64)


def blocky_u8(seed, n, F, H, W):
    """Seeded frames whose masks are unions of rectangles, with channel values that separate the two mask rules: (1, 0, 0) and
    (0, 0, 4) are in the any-channel mask and outside the luma one."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, F, 3, H, W), np.uint8)
    colours = np.array([(255, 255, 255), (1, 0, 0), (0, 0, 4), (0, 2, 0), (200, 0, 30), (3, 0, 0)], np.uint8)
    for i in range(n):
        for f in range(F):
            for _ in range(int(rng.integers(1, 5))):
                y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
                y1, x1 = y0 + 1 + int(rng.integers(0, max(1, H // 2))), x0 + 1 + int(rng.integers(0, max(1, W // 2)))
                out[i, f, :, y0:y1, x0:x1] = colours[int(rng.integers(0, len(colours)))][:, None, None]
    return out


def as_u8(mask):
    """bool (H, W) -> (3, H, W) uint8, white inside."""
    return np.repeat(mask[None].astype(np.uint8) * 255, 3, 0)


# ---- the best-of-N rule: counts (C, n, 2, 3) and the winners.  Only the all-frames triple {gt, pred, inter} decides.
def _triples(*rows):
    return [[[list(t), [0, 0, 0]]] for t in rows]           # C candidates x one clip


BEST_CASES = {
    "middle": (_triples((10, 10, 2), (10, 10, 9), (10, 10, 5)), [1]),
    "tie_later_wins": (_triples((10, 10, 5), (8, 12, 5), (10, 10, 1)), [1]),             # 5 / 15 twice
    "all_unions_zero": (_triples((0, 0, 0), (0, 0, 0), (0, 0, 0)), [2]),
    "one_third_twice": (_triples((2, 2, 1), (4, 4, 2), (9, 9, 0)), [1]),                 # 1 / 3 and 2 / 6
}


def _same_double_case():
    """Two 44-bit pairs inter / union whose ratios differ as rationals and round to one double: n / (2 n + 1) against
    (n - 1) / (2 n - 1) differ by 1 / ((2 n + 1) (2 n - 1)) ~ 2^-88, far below half an ulp (2^-55) of a value near 0.5.  As
    rationals the FIRST is the larger one: a comparison by cross-multiplied integers would take candidate 0."""
    n = 2 ** 42 + 12345
    i1, u1, i2, u2 = n, 2 * n + 1, n - 1, 2 * n - 1
    assert i1 * u2 != i2 * u1 and i1 * u2 > i2 * u1 and i1 / u1 == i2 / u2 and 2 ** 43 < u2 < u1 < 2 ** 44
    # union = gt + pred - inter with pred = inter: gt = union
    return _triples((u1, i1, i1), (u2, i2, i2)), [1]


BEST_CASES["same_double"] = _same_double_case()
