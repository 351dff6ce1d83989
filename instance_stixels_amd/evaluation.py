"""Scores of the dense result maps that Stixels.RenderBatch / is_render_sections accumulate on the device.

The reference scores stixels through per-pixel images (tools/run_cityscapes.py:585-640: each setting of its
hyper-parameter search is scored as semantic_score + 1.5 * instance_score): the label images go to
cityscapesscripts for the mean IoU, the disparity images to tools/evaluation/disparity.py.  This module holds
the host half of that scoring, on the confusion matrix and the deviation sums the device leaves, and on the
per-frame overlap tables of Stixels.InstanceOverlapBatch for the instance AP (CityscapesInstanceEval).

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


# ---- instance segmentation: Cityscapes AP from the per-frame overlap tables of InstanceOverlapBatch ----------
# labelIds of the 8 Cityscapes classes with instances (person .. bicycle), in labelId order
CITYSCAPES_INSTANCE_LABELIDS = (24, 25, 26, 27, 28, 31, 32, 33)
# labelIds with ignoreInEval == True (cityscapesscripts labels.py); -1 is 'license plate', which no uint16
# instanceIds file holds but an int32 gt can
CITYSCAPES_VOID_LABELIDS = (-1, 0, 1, 2, 3, 4, 5, 6, 9, 10, 14, 15, 16, 18, 29, 30)
CITYSCAPES_OVERLAPS = np.arange(0.5, 1.0, 0.05)
CITYSCAPES_MIN_REGION_SIZE = 100


class CityscapesInstanceEval:
    """Cityscapes instance-level AP ("average" and 50 % lines) from the sparse tables H_f(pred, gt) that
    Stixels.InstanceOverlapBatch / is_instance_overlap leave per frame.

    It restates cityscapesscripts' evalInstanceLevelSemanticLabeling (assignGt2Preds + evaluateMatches, without
    the distance variants) on the tables.  That package is not a dependency of this project, so the restatement
    follows the published source and is NOT pinned against it by any test here; tests/test_instance_eval_cpu.py
    checks it with hand-worked cases and against a literal per-mask restatement.  The contract:

    - predictions are the distinct non-zero pred ids of a frame; the label of pred p is
      CITYSCAPES_TRAINID_TO_LABELID[p // 1000] (others, and ids outside that table, are skipped); only the 8
      instance labels are scored.  Confidence: 1.0 unless given (the reference writes 1.0 for every mask).
      Pred area = sum over g of H(p, g).
    - gt instances of a label are the distinct g with label(g) equal to it, label(g) = g // 1000 for g >= 1000,
      else g; gt area = sum over p of H(p, g).  Groups (g < 1000) and gts under minRegionSize (100) px take part
      in matching but are not counted; an unmatched counted gt is a hard false negative.
    - thresholds np.arange(0.5, 1.0, 0.05), compared as iou > th in float64, iou = i / (gt + pred - i).  A second
      prediction over an already matched gt is a false positive at the lower score.
    - an unmatched prediction is a false positive unless its ignored share (void intersection + intersection with
      groups + intersection with small gts, a small group counted twice as in the published code) / area is above
      the threshold.  Void: the raw gt value is a labelId with ignoreInEval (CITYSCAPES_VOID_LABELIDS).
    - the precision/recall curve with its artificial (r = 0, p = 1) point and the step integration of
      evaluateMatches; with one constant confidence AP = r (p + 1) / 2.  AP is NaN for a class without gt over
      all added frames, 0 for a class with gt but no prediction.

    add(tables, confidences=None) per batch: tables, a sequence of per-frame record arrays (fields pred, gt,
    count); confidences, None or per frame a mapping {pred id: confidence}.  result() gives the per-class x
    per-threshold AP, AP (nanmean over classes of the mean over thresholds) and AP50."""

    def __init__(self, overlaps=CITYSCAPES_OVERLAPS, min_region_size=CITYSCAPES_MIN_REGION_SIZE):
        self.overlaps = np.asarray(overlaps, np.float64)
        self.min_region_size = int(min_region_size)
        self._images = []

    def add(self, tables, confidences=None):
        for i, t in enumerate(tables):
            conf = None if confidences is None else confidences[i]
            self._images.append(self._matches(t, conf))

    def _matches(self, table, conf):
        t = np.asarray(table)
        p = t["pred"].astype(np.int64)
        g = t["gt"].astype(np.int64)
        c = t["count"].astype(np.int64)
        parea, garea, pvoid = {}, {}, {}
        void = np.isin(g, CITYSCAPES_VOID_LABELIDS)
        for pi, gi, ci, vi in zip(p.tolist(), g.tolist(), c.tolist(), void.tolist()):
            parea[pi] = parea.get(pi, 0) + ci
            garea[gi] = garea.get(gi, 0) + ci
            if vi:
                pvoid[pi] = pvoid.get(pi, 0) + ci
        table_ids = CITYSCAPES_TRAINID_TO_LABELID

        def plabel(x):
            k = x // 1000
            return int(table_ids[k]) if x > 0 and k < table_ids.size else None

        out = {}
        for lab in CITYSCAPES_INSTANCE_LABELIDS:
            gts = [gi for gi in sorted(garea) if (gi // 1000 if gi >= 1000 else gi) == lab]
            preds = [pi for pi in sorted(parea) if plabel(pi) == lab]
            gidx = {gi: k for k, gi in enumerate(gts)}
            pidx = {pi: k for k, pi in enumerate(preds)}
            gt_list = [dict(id=gi, area=garea[gi], matched=[]) for gi in gts]
            pred_list = [dict(area=parea[pi], void=pvoid.get(pi, 0),
                              conf=1.0 if conf is None else float(conf.get(pi, 1.0)), matched=[]) for pi in preds]
            for pi, gi, ci in zip(p.tolist(), g.tolist(), c.tolist()):
                if pi in pidx and gi in gidx and ci > 0:
                    pr, gr = pred_list[pidx[pi]], gt_list[gidx[gi]]
                    pr["matched"].append((gr["id"], gr["area"], ci))
                    gr["matched"].append((pr["area"], ci, pr["conf"]))
            out[lab] = (gt_list, pred_list)
        return out

    def _ap(self, lab, th):
        y_true, y_score = [], []
        hard_fns = 0
        have_gt = have_pred = False
        mrs = self.min_region_size
        for img in self._images:
            gts, preds = img[lab]
            counted = [gt for gt in gts if gt["id"] >= 1000 and gt["area"] >= mrs]
            have_gt |= bool(counted)
            have_pred |= bool(preds)
            cur_true = [1.0] * len(counted)
            cur_score = [-np.inf] * len(counted)
            cur_match = [False] * len(counted)
            for k, gt in enumerate(counted):
                found = False
                for parea, inter, conf in gt["matched"]:
                    if float(inter) / (gt["area"] + parea - inter) > th:
                        if cur_match[k]:
                            cur_score[k], low = max(cur_score[k], conf), min(cur_score[k], conf)
                            cur_true.append(0.0)
                            cur_score.append(low)
                            cur_match.append(True)
                        else:
                            found = True
                            cur_match[k] = True
                            cur_score[k] = conf
                if not found:
                    hard_fns += 1
            y_true += [t for t, m in zip(cur_true, cur_match) if m]
            y_score += [s for s, m in zip(cur_score, cur_match) if m]
            for pr in preds:
                if any(float(inter) / (garea + pr["area"] - inter) > th for _, garea, inter in pr["matched"]):
                    continue
                ignored = pr["void"]
                for gid, garea, inter in pr["matched"]:
                    if gid < 1000:
                        ignored += inter
                    if garea < mrs:
                        ignored += inter
                if float(ignored) / pr["area"] <= th:
                    y_true.append(0.0)
                    y_score.append(pr["conf"])
        if not have_gt:
            return float("nan")
        if not have_pred:
            return 0.0
        y_true, y_score = np.asarray(y_true, np.float64), np.asarray(y_score, np.float64)
        order = np.argsort(y_score, kind="stable")
        ys, yt = y_score[order], y_true[order]
        cum = np.cumsum(yt)
        _, uniq = np.unique(ys, return_index=True)
        n_ex, n_true = len(ys), cum[-1]
        cum = np.append(cum, 0)
        prec, rec = np.zeros(len(uniq) + 1), np.zeros(len(uniq) + 1)
        for r, i in enumerate(uniq):
            cs = cum[i - 1]
            tp = n_true - cs
            fp = n_ex - i - tp
            fn = cs + hard_fns
            prec[r] = tp / (tp + fp)
            rec[r] = tp / (tp + fn)
        prec[-1], rec[-1] = 1.0, 0.0
        conv = np.concatenate([[rec[0]], rec, [0.0]])
        steps = np.convolve(conv, [-0.5, 0, 0.5], "valid")
        return float(np.dot(prec, steps))

    def result(self):
        """dict: ap [8 classes][thresholds] (NaN rows: no gt), labels, overlaps, class_ap [8] (mean over
        thresholds), AP (nanmean of class_ap: the "average" line), AP50 (nanmean at the 0.5 threshold)."""
        labs = CITYSCAPES_INSTANCE_LABELIDS
        ap = np.array([[self._ap(lab, th) for th in self.overlaps] for lab in labs], np.float64).reshape(
            len(labs), len(self.overlaps))
        class_ap = ap.mean(axis=1)
        o50 = np.where(np.isclose(self.overlaps, 0.5))[0]
        with np.errstate(all="ignore"):
            valid = ~np.isnan(class_ap)
            AP = float(class_ap[valid].mean()) if valid.any() else float("nan")
            a50 = ap[:, o50].ravel()
            AP50 = float(a50[~np.isnan(a50)].mean()) if (~np.isnan(a50)).any() else float("nan")
        return dict(ap=ap, labels=labs, overlaps=self.overlaps.copy(), class_ap=class_ap, AP=AP, AP50=AP50)


# ---- parameter sweeps: the reference's search objective without a re-initialisation per sample ----------------
def sweep_scores(st, sets, gt_label, gt_instance, n_labels=CITYSCAPES_N_LABELS, stream=0):
    """The raw scores of every set of the last st.SweepBatch(..., sets) of `st` (a host.Stixels), on the device: per
    set SelectSweepSet, RenderBatch metrics-only (no image is written) against gt_label (device uint8
    [frames][rows][cols], a pointer as int) and InstanceOverlapBatch against gt_instance (device int32, or None: a
    sweep without instances).  `sets` are the sets that call was given: ValueError when their number is not the
    number of sets the object holds.  Returns one dict per set: confusion ([n_labels][n_labels] uint64, gt x pred,
    summed over the frames), stixel_count ([frames] int32) and overlaps (the per-frame tables, None without
    gt_instance) -- what cityscapes_iou and CityscapesInstanceEval take.  tools/run_cityscapes.py:585-640 scores a
    sample as mean IoU + 1.5 * AP."""
    import torch
    if len(sets) != st.SweepSets():
        raise ValueError(f"sweep_scores: {len(sets)} sets given, the last SweepBatch of the object holds {st.SweepSets()}")
    frames = st.LastFrames()
    dev = torch.device("cuda", st.GetActiveDevice())
    out = []
    for k in range(len(sets)):
        st.SelectSweepSet(k)
        conf = torch.zeros((n_labels, n_labels), dtype=torch.int64, device=dev)
        _, _, count = st.RenderBatch(frames, gt_label=gt_label, n_labels=n_labels, confusion=conf.data_ptr(),
                                     stream=stream)
        overlaps = None if gt_instance is None else st.InstanceOverlapBatch(frames, gt_instance, stream=stream)
        out.append(dict(confusion=conf.cpu().numpy().astype(np.uint64), stixel_count=count, overlaps=overlaps))
    return out


def instance_disparity_scores(st, gt_instance, disparity_u8, eps, min_pts, size_filter, evaluator=None, stream=0):
    """The instance AP of the last compute call of `st` (a host.Stixels; or of its selected sweep set) with the
    instance ids of the reference's --use-disparity from_gt clustering, without a per-frame loop:
    ClusterInstanceDisparityBatch over (instance_mean_x, instance_mean_y, instance disparity), then
    InstanceOverlapBatch against the same ground truth, then CityscapesInstanceEval.  gt_instance: device int32
    [frames][rows][cols] (a pointer as int); disparity_u8: device uint8 of the same shape.  evaluator: a
    CityscapesInstanceEval to add the frames to (one is made otherwise).  Returns dict(overlaps = the per-frame tables,
    result = evaluator.result()); the labels stay on the device for RenderBatch / WorldBatch / InstanceObjectsBatch."""
    frames = st.LastFrames()
    st.ClusterInstanceDisparityBatch(frames, gt_instance, disparity_u8, eps, min_pts, size_filter, with_mapping=False,
                                     stream=stream)
    overlaps = st.InstanceOverlapBatch(frames, gt_instance, stream=stream)
    ev = evaluator if evaluator is not None else CityscapesInstanceEval()
    ev.add(overlaps)
    return dict(overlaps=overlaps, result=ev.result())


def gt_offset_scores(st, pairwise, d_disparity_big, d_segmentation, road, gt_instance, evaluator=None, stream=0):
    """The instance AP of a resident batch with the CNN's two offset channels replaced by the ground truth, the
    reference's --usegtoffsets row, without a per-frame loop: GroundTruthOffsetsBatch rewrites channels 19 and 20 of
    d_segmentation (device int32 [frames][cols / 8][21][P2S], a pointer as int; it is CHANGED), then ComputeBatch on
    d_disparity_big and that tensor with `road` (one tuple per frame), InstanceOverlapBatch against the same ground
    truth, then CityscapesInstanceEval.  gt_instance: device int32 [frames][rows][cols] (a pointer as int).
    evaluator: a CityscapesInstanceEval to add the frames to (one is made otherwise).  Returns dict(stixels = the
    frames' StixelsData, overlaps = the per-frame tables, result = evaluator.result())."""
    frames = len(road)
    st.GroundTruthOffsetsBatch(frames, gt_instance, d_segmentation, stream=stream)
    stixels, _ = st.ComputeBatch(pairwise, d_disparity_big, d_segmentation, road, with_instances=True, stream=stream)
    overlaps = st.InstanceOverlapBatch(frames, gt_instance, stream=stream)
    ev = evaluator if evaluator is not None else CityscapesInstanceEval()
    ev.add(overlaps)
    return dict(stixels=stixels, overlaps=overlaps, result=ev.result())


# ---- the CNN alone: the second semantic row of the reference's evaluation --------------------------------------------
def cnn_scores(cnn_out, gt_label, n_classes=19, mode="nearest", confusion=None):
    """The IoU of the CNN's own label image, the row the reference prints beside the stixels'
    (tools/run_cityscapes.py:353-365, 551) and selects models by (tools/CNN_training/train.py:559-605), on the device:
    core.cnn_label_maps without a label image (is_cnn_label_maps, metrics only) adds the batch to the confusion
    table, and cityscapes_iou scores the table.

    cnn_out     device float32 [n][channels >= n_classes][rows8][cols8], the float output of core.segmentation_head
    gt_label    device uint8 [n][8 * rows8][cols >= 8 * cols8] of Cityscapes labelIds
    mode        "nearest" (the downsampled models) or "deconv" (the full-resolution ones)
    confusion   the "confusion" of an earlier call (a device int64 tensor [34][34]): this batch is added to it, so a
                validation loop passes it back in batch after batch; None: a new table

    Returns dict(confusion = the table on the device, iou = per-class IoU [19], mean_iou); reading the table back is
    the call's one synchronisation.  With cnn_out None nothing is launched and `confusion` (a tensor or an array) is
    scored as it is."""
    if cnn_out is not None:
        from . import core
        confusion = core.cnn_label_maps(cnn_out, n_classes, mode=mode, cols=int(gt_label.shape[-1]), gt_label=gt_label,
                                        n_labels=CITYSCAPES_N_LABELS, confusion=confusion,
                                        want_label=False)["confusion"]
    elif confusion is None:
        raise ValueError("cnn_scores: neither a network output nor a table")
    host = confusion.cpu().numpy() if hasattr(confusion, "cpu") else np.asarray(confusion)
    iou, mean = cityscapes_iou(host)
    return dict(confusion=confusion, iou=iou, mean_iou=mean)
