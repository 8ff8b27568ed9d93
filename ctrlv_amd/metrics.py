"""The metrics the boxes-to-video chain and its evaluation use, formed on the host from integers counted on the device.

- `binary_mask_iou` (src/ctrlv/metrics/FandJ.py:11-23; tools/eval_overall.py:106,112): the mask IoU of predicted against
  ground-truth box frames.  ops.mask_counts counts the pixels; only the six counts of a clip come to the host.
- `best_of` / `candidate_scores`: the reference's best-of-N rule over stage-1 candidates (eval_overall.py:83-114) restated on
  Python ints and floats -- what ctrlv_best_candidate decides on the device -- and the triples that loop logs.
- `boundary_f_measure` (FandJ.py:94-156; tools/eval_video_bbox_prediction.py:85-95): the boundary F-measure of the box
  predictor.  ops.boundary_counts gives four integers per frame; precision, recall and F are formed here in double.

FVD and the other evaluation metrics stay out of scope."""
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


__all__ = ["binary_mask_iou", "iou_from_counts", "best_of", "candidate_scores", "f_from_counts", "boundary_radius",
           "pt_frames_to_u8", "boundary_f_measure"]
