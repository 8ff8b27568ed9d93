"""The metrics the boxes-to-video chain and its evaluation use, formed on the host from integers counted on the device.

- `binary_mask_iou` (src/ctrlv/metrics/FandJ.py:11-23; tools/eval_overall.py:106,112): the mask IoU of predicted against
  ground-truth box frames.  ops.mask_counts counts the pixels; only the six counts of a clip come to the host.
- `best_of` / `candidate_scores`: the reference's best-of-N rule over stage-1 candidates (eval_overall.py:83-114) restated on
  Python ints and floats -- what ctrlv_best_candidate decides on the device -- and the triples that loop logs.
- `boundary_f_measure` (FandJ.py:94-156; tools/eval_video_bbox_prediction.py:85-95): the boundary F-measure of the box
  predictor.  ops.boundary_counts gives four integers per frame; precision, recall and F are formed here in double.

- `frame_quality` / `psnr_from_stats` / `quality_summary` (src/ctrlv/metrics/fvd.py:251-286): the per-frame SSIM and PSNR of a
  generated clip against its ground truth, as evaluate_vids computes them with PIL and scikit-image -- the ssim_score_image
  and psnr_score_image numbers and their error terms.  The resize, the three integers of PSNR and SSIM itself run on the
  device (ops.resize_frames_u8, ops.frame_stats, ops.frame_ssim); n F doubles and 3 n F integers come to the host.
- `lpips_frames` (fvd.py:241-248): `lpips.LPIPS(net='alex')` of every frame pair, the third number evaluate_vids prints, through
  a `plan.LpipsPlan` -- AlexNet on split 16-bit operands with fp32 maps between the layers; n F doubles
  come to the host.  The weights are the caller's (models.lpips_alex: the two published files, or a seeded network).

FVD (a TorchScript I3D fetched from a URL) and the per-video 3-D SSIM / PSNR the reference computes but no longer prints stay
out of scope."""
import math

import numpy as np
import torch

from . import _lib, ops


def iou_from_counts(gt_area, pred_area, intersection):
    """(iou, precision, recall) with the reference's conventions: a zero denominator gives 1."""
    gt_area, pred_area, intersection = int(gt_area), int(pred_area), int(intersection)
    union = gt_area + pred_area - intersection
    iou = intersection / union if union > 0 else 1
    recall = intersection / gt_area if gt_area > 0 else 1
    precision = intersection / pred_area if pred_area > 0 else 1
    return iou, precision, recall


def binary_mask_iou(gt_u8, pred_u8, first_last=False):
    """gt_u8, pred_u8: (F, 3, H, W) or (n, F, 3, H, W) uint8 box frames on a HIP device; a pixel is in a mask when any channel
    is nonzero.  first_last: over the frames {0, F - 1} only (eval_overall.py:112).  Returns (iou, precision, recall) for one
    clip, a list of such triples for a batch of clips."""
    single = gt_u8.dim() == 4
    if single:
        gt_u8, pred_u8 = gt_u8[None], pred_u8[None]
    counts = ops.mask_counts(gt_u8.contiguous(), pred_u8.contiguous()).cpu()
    out = [iou_from_counts(*counts[b, 1 if first_last else 0].tolist()) for b in range(counts.shape[0])]
    return out[0] if single else out


def _count_rows(counts):
    """counts (C, n, 2, 3) -- a tensor, an array or nested lists -- as nested lists of Python ints."""
    if isinstance(counts, torch.Tensor):
        counts = counts.cpu()
    rows = counts.tolist() if hasattr(counts, "tolist") else counts
    return [[[[int(v) for v in t] for t in clip] for clip in cand] for cand in rows]


def best_of(counts):
    """counts (C, n, 2, 3): candidate c's block as ops.mask_counts gives it.  Returns the winner per clip, a list of n ints:
    the largest all-frames IoU, and a tie goes to the highest c -- the reference keeps `best_score = max(best_score, miou)` and
    takes the candidate `if best_score == miou`, so a later equal score replaces an earlier one.  The IoU is the Python float
    inter / union (1.0 for an empty union): two ratios that round to the same double tie, as they do in numpy."""
    rows = _count_rows(counts)
    winners = []
    for i in range(len(rows[0])):
        best, w = -1.0, 0
        for c in range(len(rows)):
            gt, pred, inter = rows[c][i][0]
            union = gt + pred - inter
            iou = inter / union if union > 0 else 1.0
            if iou >= best:
                best, w = iou, c
        winners.append(w)
    return winners


def candidate_scores(counts):
    """counts (C, n, 2, 3) -> [c][i] = ((iou, precision, recall) over all frames, the same over the frames {0, F - 1}): what
    eval_overall.py:106-112 logs per candidate."""
    return [[(iou_from_counts(*clip[0]), iou_from_counts(*clip[1])) for clip in cand] for cand in _count_rows(counts)]


def f_from_counts(n_fg, n_gt, fg_match, gt_match):
    """(F, precision, recall) of f_measure from its four integers, in double: precision = fg_match / n_fg, recall = gt_match /
    n_gt; no predicted boundary but a true one: (1, 0); a predicted but no true one: (0, 1); neither: (1, 1); F = 0 when
    precision + recall = 0, else 2 p r / (p + r)."""
    n_fg, n_gt, fg_match, gt_match = int(n_fg), int(n_gt), int(fg_match), int(gt_match)
    if n_fg == 0 and n_gt > 0:
        precision, recall = 1.0, 0.0
    elif n_fg > 0 and n_gt == 0:
        precision, recall = 0.0, 1.0
    elif n_fg == 0 and n_gt == 0:
        precision, recall = 1.0, 1.0
    else:
        precision, recall = fg_match / n_fg, gt_match / n_gt
    f = 0.0 if precision + recall == 0 else 2 * precision * recall / (precision + recall)
    return f, precision, recall


def boundary_radius(H, W, bound_th=0.008):
    """The tolerance of f_measure in pixels (ctrlv_boundary_radius): bound_th when it is >= 1, else
    ceil(bound_th * sqrt(H^2 + W^2))."""
    lib = _lib.load()
    r = lib.ctrlv_boundary_radius(int(H), int(W), float(bound_th))
    if r < 0:
        _lib.check(r, "ctrlv_boundary_radius", lib=lib)
    return r


def pt_frames_to_u8(frames):
    """The preparation eval_video_bbox_prediction.py applies to "pt" frames in [0, 1] before the metric: values under 5 / 255
    become 0, the rest is scaled by 255 and truncated to uint8, in the tensor's dtype."""
    return torch.where(frames < 5 / 255, 0, frames).mul(255).byte()


def boundary_f_measure(gt_u8, pred_u8, mask="luma", bound_th=0.008):
    """gt_u8, pred_u8: (F, 3, H, W) or (n, F, 3, H, W) uint8 frames on a HIP device -> float64 array (F) or (n, F): f_measure of
    every frame.  mask: "luma" (PIL's convert('L') != 0, what the evaluation script feeds the metric) or "any" (any channel
    nonzero, binary_mask_iou's mask).  The mean over F is the clip score the script prints."""
    modes = {"any": 0, "luma": 1}
    if mask not in modes:
        raise ValueError(f"boundary_f_measure: mask {mask!r} must be 'luma' or 'any'")
    single = gt_u8.dim() == 4
    if single:
        gt_u8, pred_u8 = gt_u8[None], pred_u8[None]
    H, W = gt_u8.shape[-2:]
    counts = ops.boundary_counts(gt_u8.contiguous(), pred_u8.contiguous(), boundary_radius(H, W, bound_th), modes[mask]).cpu()
    out = np.array([[f_from_counts(*row)[0] for row in clip] for clip in counts.tolist()], dtype=np.float64)
    return out[0] if single else out


def psnr_from_stats(min_byte, max_byte, sse, count):
    """peak_signal_noise_ratio(gt, gen, data_range=R) from the integers of ops.frame_stats, in double: R = max - min, count the
    number of compared values (3 H W): 10 log10(R^2 count / sse).  inf for sse = 0 with R > 0 (skimage's division by a zero
    error), NaN for R = 0 (both frames one constant: the reference's log10(0 / 0))."""
    r, sse, count = int(max_byte) - int(min_byte), int(sse), int(count)
    if r == 0:
        return math.nan
    if sse == 0:
        return math.inf
    return 10.0 * math.log10((r * r * count) / sse)


def _clip_pair(gt_u8, gen_u8, size, resample):
    """The two clips as contiguous (n, F, 3, h, w) uint8 after the optional PIL-exact resize, and whether a clip axis was added."""
    single = gt_u8.dim() == 4
    if single:
        gt_u8, gen_u8 = gt_u8[None], gen_u8[None]
    gt_u8, gen_u8 = gt_u8.contiguous(), gen_u8.contiguous()
    if size is not None:
        h, w = (int(v) for v in size)
        gt_u8 = ops.resize_frames_u8(gt_u8, h, w, resample)
        gen_u8 = ops.resize_frames_u8(gen_u8, h, w, resample)
    return gt_u8, gen_u8, single


def lpips_frames(gt_u8, gen_u8, plan, size=None, resample="bicubic"):
    """gt_u8, gen_u8: (F, 3, H, W) or (n, F, 3, H, W) uint8 frames on a HIP device, plan: a `plan.LpipsPlan` -> float64 array (F)
    or (n, F): lpips.LPIPS(net='alex') of every frame pair on frames scaled to [-1, 1] (u8 / 127.5 - 1), as evaluate_vids feeds
    it.  size / resample: as `frame_quality`.  The mean over everything is its lpips_score (`quality_summary`)."""
    gt_u8, gen_u8, single = _clip_pair(gt_u8, gen_u8, size, resample)
    out = plan.frames(gt_u8, gen_u8).cpu().numpy()
    return out[0] if single else out


def frame_quality(gt_u8, gen_u8, size=None, resample="bicubic", lpips=None):
    """gt_u8, gen_u8: (F, 3, H, W) or (n, F, 3, H, W) uint8 frames on a HIP device -> {"ssim": float64 (F) or (n, F), "psnr":
    the same}: per frame, scikit-image's structural_similarity(channel_axis=0, data_range=R, gaussian_weights=True, sigma=1.5)
    and peak_signal_noise_ratio(data_range=R) with R the joint value range of the two frames -- evaluate_vids'
    ssim_score_image / psnr_score_image.  size=(h, w): both clips are first resized on the device as PIL resizes them
    (evaluate_vids: size=(256, 410), PIL's default bicubic).  A frame pair of one constant value is NaN in both.
    lpips: a `plan.LpipsPlan`; the result then also has "lpips", the array `lpips_frames` gives for the same (resized) frames."""
    gt_u8, gen_u8, single = _clip_pair(gt_u8, gen_u8, size, resample)
    stats = ops.frame_stats(gt_u8, gen_u8)
    ssim = ops.frame_ssim(gt_u8, gen_u8, stats).cpu().numpy()
    count = 3 * gt_u8.shape[-2] * gt_u8.shape[-1]
    psnr = np.array([[psnr_from_stats(*row, count) for row in clip] for clip in stats.cpu().tolist()], dtype=np.float64)
    out = {"ssim": ssim, "psnr": psnr}
    if lpips is not None:
        out["lpips"] = lpips.frames(gt_u8, gen_u8).cpu().numpy()
    return {k: v[0] for k, v in out.items()} if single else out


def quality_summary(ssim, psnr, denominator=200, lpips=None):
    """The four numbers evaluate_vids prints from its (samples, frames) arrays: ssim_score_image and psnr_score_image (the
    means) and their error terms sqrt(sum((v - mean)^2) / denominator).  The reference divides by a literal 200 whatever the
    sample count (fvd.py:275-276): that is the default here.  lpips: the per-frame array of `lpips_frames`; adds lpips_score, its
    plain mean (fvd.py:245-248 averages the frames of a clip, then the clips: clips of one length, so the same number)."""
    out = {}
    for name, v in (("ssim", ssim), ("psnr", psnr)):
        v = np.asarray(v, dtype=np.float64)
        out[f"{name}_score_image"] = float(v.mean())
        out[f"{name}_score_image_error"] = float(np.sqrt(((v - v.mean()) ** 2).sum() / denominator))
    if lpips is not None:
        out["lpips_score"] = float(np.asarray(lpips, dtype=np.float64).mean())
    return out


__all__ = ["binary_mask_iou", "iou_from_counts", "best_of", "candidate_scores", "f_from_counts", "boundary_radius",
           "pt_frames_to_u8", "boundary_f_measure", "psnr_from_stats", "frame_quality", "quality_summary", "lpips_frames"]
