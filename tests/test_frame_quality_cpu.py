"""Pins tests/frame_quality_ref.py -- the float64 restatement of the per-frame SSIM / PSNR arithmetic of include/ctrlv_hip.h --
before the GPU tests compare the kernels with it: against scipy's Gaussian filter with scikit-image's formula, against closed
forms, and against the reference's own preparation (fp32 v / 127.5 - 1, data_range from those floats), which is what licenses
working in byte units.  Also metrics.psnr_from_stats and metrics.quality_summary, which need no device."""
import math

import numpy as np
import pytest

from tests import frame_quality_ref as Q

CASES = [(kind, H, W) for (_, _, H, W) in Q.SHAPES for kind in Q.KINDS]


def _skimage_ssim(x, y, R):
    """structural_similarity(channel_axis=0, data_range=R, gaussian_weights=True, sigma=1.5) restated on scipy's filter."""
    ndi = pytest.importorskip("scipy.ndimage")
    f = lambda a: ndi.gaussian_filter(a, 1.5, mode="reflect", truncate=3.5)
    out = []
    for c in range(3):
        a, b = x[c].astype(np.float64), y[c].astype(np.float64)
        ux, uy, uxx, uyy, uxy = f(a), f(b), f(a * a), f(b * b), f(a * b)
        cov = 121 / 120
        vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
        C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
        with np.errstate(invalid="ignore", divide="ignore"):
            S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
        out.append(S[5:-5, 5:-5].mean(dtype=np.float64))
    return float(np.mean(out))


def test_the_restatement_is_scipys_filter_and_skimages_formula():
    pytest.importorskip("scipy")
    worst = 0.0
    for kind, H, W in CASES:
        gt, gen = Q.pair(kind, H, W, 3 * H + W)
        lo, hi, _ = Q.stats(gt, gen)
        want = _skimage_ssim(gt.astype(np.float64) - 127.5, gen.astype(np.float64) - 127.5, float(hi - lo))
        got = Q.ssim_u8(gt, gen)
        worst = max(worst, abs(got - want))
        assert abs(got - want) <= 1e-9, (kind, H, W, got, want)
    print("restatement against scipy: worst", worst)


def test_known_answers():
    # identical non-constant frames: exactly 1
    for H, W in ((11, 11), (12, 75), (37, 70)):
        gt, gen = Q.pair("same", H, W, 5)
        assert Q.ssim_u8(gt, gen) == 1.0
        assert Q.psnr_from_stats(*Q.stats(gt, gen), gt.size) == math.inf
    # two constant frames a != b: the variances vanish, the luminance term is left
    for a, b in ((250, 247), (0, 255), (100, 101)):
        gt, gen = np.full((3, 12, 75), a, np.uint8), np.full((3, 12, 75), b, np.uint8)
        p, q, R = a - 127.5, b - 127.5, abs(a - b)
        C1 = (0.01 * R) ** 2
        assert Q.ssim_u8(gt, gen) == pytest.approx((2 * p * q + C1) / (p * p + q * q + C1), rel=0, abs=1e-9)
    # PSNR of one pixel differing by d in a frame of byte range R
    H, W, d = 12, 75, 3
    gt = np.random.default_rng(1).integers(10, 201, size=(3, H, W)).astype(np.uint8)
    gt[0, 0, 0], gt[0, 0, 1] = 10, 200
    gen = gt.copy()
    gen[1, 6, 40] = gt[1, 6, 40] - d if gt[1, 6, 40] >= 10 + d else gt[1, 6, 40] + d
    lo, hi, sse = Q.stats(gt, gen)
    assert (lo, hi, sse) == (10, 200, d * d)
    assert Q.psnr_from_stats(lo, hi, sse, gt.size) == pytest.approx(10 * math.log10(190 ** 2 * 3 * H * W / d ** 2), rel=1e-15)
    # R = 0
    c = np.full((3, 11, 11), 9, np.uint8)
    assert math.isnan(Q.ssim_u8(c, c)) and math.isnan(Q.psnr_from_stats(*Q.stats(c, c), c.size))


def test_byte_units_are_the_references_preparation():
    worst_s, worst_p = 0.0, 0.0
    for kind, H, W in CASES:
        gt, gen = Q.pair(kind, H, W, 7 * H + W)
        s_ref, p_ref = Q.reference_route(gt, gen)
        p = Q.psnr_from_stats(*Q.stats(gt, gen), gt.size)
        if math.isfinite(p):
            worst_p = max(worst_p, abs(p - p_ref))
            assert abs(p - p_ref) <= 1e-3, (kind, H, W, p, p_ref)
        else:
            assert p == p_ref == math.inf
        if kind in Q.WELL_CONDITIONED:
            s = Q.ssim_u8(gt, gen)
            worst_s = max(worst_s, abs(s - s_ref))
            assert abs(s - s_ref) <= 5e-6, (kind, H, W, s, s_ref)
    print("byte units against the prepared fp32 values: ssim", worst_s, "psnr dB", worst_p)


def test_metrics_psnr_from_stats_and_quality_summary():
    from ctrlv_amd import metrics
    for args in ((10, 200, 9, 2700), (0, 255, 123456, 3 * 256 * 410), (3, 250, 1, 363)):
        assert metrics.psnr_from_stats(*args) == Q.psnr_from_stats(*args)
        r = args[1] - args[0]
        assert metrics.psnr_from_stats(*args) == pytest.approx(10 * math.log10(r * r * args[3] / args[2]), rel=1e-15)
    assert metrics.psnr_from_stats(0, 255, 0, 363) == math.inf
    assert math.isnan(metrics.psnr_from_stats(7, 7, 0, 363))
    rng = np.random.default_rng(4)
    ssim, psnr = rng.random((6, 25)), 20 + 10 * rng.random((6, 25))
    got = metrics.quality_summary(ssim, psnr)
    want = Q.quality_summary(ssim, psnr)
    assert (got["ssim_score_image"], got["ssim_score_image_error"], got["psnr_score_image"], got["psnr_score_image_error"]) \
        == pytest.approx(want, rel=1e-15)
    half = metrics.quality_summary(ssim, psnr, denominator=50)
    assert half["ssim_score_image_error"] == pytest.approx(2 * got["ssim_score_image_error"], rel=1e-14)
