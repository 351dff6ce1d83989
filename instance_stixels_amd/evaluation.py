"""Scores of the dense result maps that Stixels.RenderBatch / is_render_sections accumulate on the device.

The reference scores stixels through per-pixel images (tools/run_cityscapes.py:585-640: each setting of its
hyper-parameter search is scored as semantic_score + 1.5 * instance_score): the label images go to
cityscapesscripts for the mean IoU, the disparity images to tools/evaluation/disparity.py.  This module holds
the host half of that scoring, on the confusion matrix and the deviation sums the device leaves.

cityscapes_iou restates cityscapesscripts' evalPixelLevelSemanticLabeling.getIouScoreForLabel and its average
over the evaluated classes.  That package is not a dependency of this project, so the restatement is not pinned
against it by any test here: it follows the published source, and the hand-worked cases of
tests/test_render_cpu.py check the restatement itself.
"""
import numpy as np

# trainId -> labelId of the 19 Cityscapes training classes (cityscapesscripts labels.py, trainId2label[c].id):
# the default class -> label table of is_render_sections
CITYSCAPES_TRAINID_TO_LABELID = np.array([7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33],
                                         np.uint8)
# the labelIds with ignoreInEval == False, in labelId order
CITYSCAPES_EVAL_LABELIDS = tuple(int(x) for x in CITYSCAPES_TRAINID_TO_LABELID)
# labelIds 0 .. 33: the confusion matrix of the Cityscapes evaluation is 34 x 34 (the default n_labels)
CITYSCAPES_N_LABELS = 34


def cityscapes_iou(conf, eval_labels=CITYSCAPES_EVAL_LABELIDS):
    """(per-class IoU [len(eval_labels)], mean IoU) of a confusion matrix conf[gt][pred].

    For an evaluated label l: tp = conf[l, l]; fn = (row sum of l) - tp, so every prediction counts, ignored
    labels and background included; fp = the sum of conf[k, l] over the OTHER evaluated labels k, so pixels
    whose ground truth is an ignored label never count as false positives.  IoU = tp / (tp + fp + fn), NaN when
    the denominator is 0 (or l lies outside the matrix); the mean is taken over the classes that are not NaN
    (NaN when all are)."""
    conf = np.asarray(conf)
    if conf.ndim != 2 or conf.shape[0] != conf.shape[1]:
        raise ValueError("conf must be a square [gt][pred] matrix")
    n = conf.shape[0]
    c = conf.astype(np.int64)
    iou = np.full(len(eval_labels), np.nan)
    for i, l in enumerate(eval_labels):
        if not 0 <= l < n:
            continue
        tp = int(c[l, l])
        fn = int(c[l, :].sum()) - tp
        others = [k for k in eval_labels if k != l and 0 <= k < n]
        fp = int(c[others, l].sum()) if others else 0
        denom = tp + fp + fn
        if denom > 0:
            iou[i] = tp / denom
    valid = ~np.isnan(iou)
    mean = float(iou[valid].mean()) if valid.any() else float("nan")
    return iou, mean


def mean_disparity_deviation(disp_abs_sum, disp_count):
    """Per frame, the mean absolute deviation of tools/evaluation/disparity.py:56-62 (the mean of
    |stixel - gt| over pixels where both are non-zero) from RenderBatch's sums and counts; NaN for a frame
    without such pixels.  Both images must be in the same units: the reference compares its stixel disparity
    tiff (x 256) with the ground-truth files."""
    s = np.asarray(disp_abs_sum, np.float64)
    n = np.asarray(disp_count, np.int64)
    out = np.full(s.shape, np.nan)
    np.divide(s, n, out=out, where=n > 0)
    return out
