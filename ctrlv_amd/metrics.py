"""The one metric the boxes-to-video chain itself uses (the reference's tools/eval_overall.py:106,112): the mask IoU of
predicted against ground-truth box frames, `binary_mask_iou` of src/ctrlv/metrics/FandJ.py:11-23.  The pixels are counted on
the device (ops.mask_counts: exact integers); only the six counts of a clip come to the host.  F-measure, FVD and the other
evaluation metrics stay out of scope."""
from . import ops


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


__all__ = ["binary_mask_iou", "iou_from_counts"]
