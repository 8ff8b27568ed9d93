"""numpy restatement, in float64, of the per-frame SSIM / PSNR arithmetic include/ctrlv_hip.h states for ctrlv_frame_stats and
ctrlv_frame_ssim -- in its PLAIN form: about 127.5, no pilot, so that the tests prove the kernel's shifted moments equivalent
instead of assuming it.  A helper module, not a conftest.  tests/test_frame_quality_cpu.py pins it to scipy's filter, to closed
forms and to the reference's own fp32 preparation before the GPU tests compare anything with it."""
import math

import numpy as np

SHAPES = [(1, 1, 11, 11), (1, 2, 12, 75), (2, 3, 37, 70), (1, 1, 64, 64), (1, 2, 96, 129), (1, 1, 150, 200)]
KINDS = ("noise", "noise3", "ramp1", "flat250", "dark", "blocks", "same")
WELL_CONDITIONED = ("noise", "noise3", "ramp1", "blocks")
BOUND = 2e-5          # |device ssim - restatement|: 10 x the 2.0e-6 the pilot arithmetic reaches in numpy fp32 on these cases


def window():
    """g[i] = exp(-i^2 / 4.5) / sum, i = -5 .. 5 (sigma = 1.5 truncated at 3.5 sigma)."""
    g = np.exp(-np.arange(-5, 6, dtype=np.float64) ** 2 / 4.5)
    return g / g.sum()


def filt(a):
    """(..., H, W) -> (..., H - 10, W - 10): the separable 11 x 11 window at every position where it fits the image."""
    g = window()
    H, W = a.shape[-2:]
    rows = sum(g[t] * a[..., :, t:t + W - 10] for t in range(11))
    return sum(g[t] * rows[..., t:t + H - 10, :] for t in range(11))


def ssim_values(x, y, R):
    """x, y (3, H, W) float64 in any one unit, R the data range in that unit -> the mean of S over the crop and the channels."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if R == 0:             # both frames one constant: every variance and C2 are exactly 0, S is 0 / 0 (about 127.5 float64 leaves
        return math.nan    # rounding noise in u_xx - u_x^2 instead of the 0 the exact arithmetic has)
    ux, uy, uxx, uyy, uxy = filt(x), filt(y), filt(x * x), filt(y * y), filt(x * y)
    cov = 121.0 / 120.0
    vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
    C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return float(S.mean(dtype=np.float64))


def stats(gt, gen):
    """(3, H, W) uint8 pair -> (min byte, max byte, sum of squared differences) as Python ints."""
    d = gt.astype(np.int64) - gen.astype(np.int64)
    return int(min(gt.min(), gen.min())), int(max(gt.max(), gen.max())), int((d * d).sum())


def stats_clip(gt, gen):
    """(n, F, 3, H, W) -> int64 (n, F, 3)."""
    n, F = gt.shape[:2]
    return np.array([[stats(gt[i, f], gen[i, f]) for f in range(F)] for i in range(n)], dtype=np.int64)


def ssim_u8(gt, gen):
    """(3, H, W) uint8 pair -> SSIM in byte units about 127.5 with R = max - min (NaN for R = 0)."""
    lo, hi, _ = stats(gt, gen)
    return ssim_values(gt.astype(np.float64) - 127.5, gen.astype(np.float64) - 127.5, float(hi - lo))


def ssim_clip(gt, gen):
    n, F = gt.shape[:2]
    return np.array([[ssim_u8(gt[i, f], gen[i, f]) for f in range(F)] for i in range(n)], dtype=np.float64)


def psnr_from_stats(lo, hi, sse, count):
    r = hi - lo
    if r == 0:
        return math.nan
    if sse == 0:
        return math.inf
    return 10.0 * math.log10(r * r * count / sse)


def psnr_clip(gt, gen):
    n, F = gt.shape[:2]
    count = gt[0, 0].size
    return np.array([[psnr_from_stats(*stats(gt[i, f], gen[i, f]), count) for f in range(F)] for i in range(n)], dtype=np.float64)


def prepared(a):
    """The reference's preparation (fvd.py:229-234): float32 v / 127.5 - 1."""
    return a.astype(np.float32) / np.float32(127.5) - np.float32(1.0)


def reference_route(gt, gen):
    """(ssim, psnr) of one frame pair the way evaluate_vids feeds scikit-image: prepared fp32 values, data_range from those
    floats; SSIM by the restatement in float64 on them, PSNR with skimage's mean of fp32 squared differences in float64."""
    a, b = prepared(gt), prepared(gen)
    R = max(a.max(), b.max()) - min(a.min(), b.min())              # a float32, as in the reference
    s = ssim_values(a.astype(np.float64), b.astype(np.float64), float(R))
    mse = np.mean((a - b) ** 2, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = float(10 * np.log10(np.float64(R) ** 2 / mse))
    return s, p


def pair(kind, H, W, seed):
    """One (gt, gen) pair of (3, H, W) uint8 frames of the named kind."""
    rng = np.random.default_rng(seed)
    noise = rng.integers(0, 256, size=(3, H, W), dtype=np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "noise":
        gt, gen = noise, rng.integers(0, 256, size=(3, H, W))
    elif kind == "noise3":
        gt, gen = noise, noise + rng.integers(-3, 4, size=(3, H, W))
    elif kind == "ramp1":
        gt = np.stack([(yy + xx) * 255 // (H + W - 2), (yy + 2 * xx) * 255 // (H + 2 * W - 3), (2 * yy + xx) * 255 // (2 * H + W - 3)])
        gen = gt + rng.integers(-1, 2, size=(3, H, W))
    elif kind == "flat250":
        gt = np.full((3, H, W), 250)
        gen = gt.copy()
        gen[:, H // 2, W // 2] = 247
    elif kind == "dark":
        gt, gen = rng.integers(0, 4, size=(3, H, W)), rng.integers(0, 4, size=(3, H, W))
    elif kind == "blocks":
        gt = np.broadcast_to(((yy // 8 + xx // 8) % 2) * 255, (3, H, W)).copy()
        gen = np.roll(gt, 2, axis=-1)
    elif kind == "same":
        gt, gen = noise, noise.copy()
    else:
        raise ValueError(kind)
    return np.clip(gt, 0, 255).astype(np.uint8), np.clip(gen, 0, 255).astype(np.uint8)


def clip_kinds(shape, start=0):
    """The kind of every frame of a shape: the kinds cycled over the frames in (clip, frame) order from KINDS[start]."""
    n, F = shape[:2]
    return [[KINDS[(start + i * F + f) % len(KINDS)] for f in range(F)] for i in range(n)]


def clips(shape, start=0):
    """(gt, gen) uint8 (n, F, 3, H, W) of a shape, seeded by the shape."""
    n, F, H, W = shape
    kinds = clip_kinds(shape, start)
    pairs = [[pair(kinds[i][f], H, W, 1000 * H + 10 * W + i * F + f + 97 * start) for f in range(F)] for i in range(n)]
    gt = np.stack([np.stack([p[0] for p in row]) for row in pairs])
    gen = np.stack([np.stack([p[1] for p in row]) for row in pairs])
    return gt, gen


def quality_summary(ssim, psnr):
    """evaluate_vids' two expressions (fvd.py:275-276, 281-284) written out."""
    ssim_score_image, psnr_score_image = np.asarray(ssim), np.asarray(psnr)
    ssim_score_image_error = np.sqrt(((ssim_score_image - ssim_score_image.mean()) ** 2).sum() / 200)
    psnr_score_image_error = np.sqrt(((psnr_score_image - psnr_score_image.mean()) ** 2).sum() / 200)
    return ssim_score_image.mean(), ssim_score_image_error, psnr_score_image.mean(), psnr_score_image_error
