"""numpy restatement of is_instance_overlap / Stixels::InstanceOverlapBatch (f6) and a literal per-mask
restatement of cityscapesscripts' assignGt2Preds + evaluateMatches, for the tests -- not a test itself.

joint_histogram(inst, gt): the sorted sparse table {pred, gt, count} of one frame (render_reference.render's
instance image against the gt instanceIds), every pixel counted, pred 0 included.
masks_ap(frames): the published evaluation on boolean masks (np.count_nonzero of logical ands), one mask per
non-zero pred id, written as the published loops are, so that the table-based evaluator of
instance_stixels_amd.evaluation can be checked against an independent statement of the same rules.
"""
import numpy as np

from instance_stixels_amd.core import OVERLAP_DTYPE
from instance_stixels_amd.evaluation import (CITYSCAPES_INSTANCE_LABELIDS, CITYSCAPES_OVERLAPS,
                                             CITYSCAPES_TRAINID_TO_LABELID, CITYSCAPES_VOID_LABELIDS)


def joint_histogram(inst, gt):
    """inst, gt: int32 [rows][cols] -> OVERLAP_DTYPE records ascending by (pred, gt) as signed int32."""
    p = (np.asarray(inst, np.int32).ravel().astype(np.int64) + 2**31).astype(np.uint64)
    g = (np.asarray(gt, np.int32).ravel().astype(np.int64) + 2**31).astype(np.uint64)
    u, cnt = np.unique((p << np.uint64(32)) | g, return_counts=True)
    out = np.zeros(u.size, OVERLAP_DTYPE)
    out["pred"] = ((u >> np.uint64(32)).astype(np.int64) - 2**31).astype(np.int32)
    out["gt"] = ((u & np.uint64(0xffffffff)).astype(np.int64) - 2**31).astype(np.int32)
    out["count"] = cnt
    return out


def _assign(inst, gt, conf):
    """assignGt2Preds on one frame: (gt instances, pred instances) per instance labelId."""
    gt = np.asarray(gt, np.int64)
    inst = np.asarray(inst, np.int64)
    void = np.isin(gt, CITYSCAPES_VOID_LABELIDS)
    gts = {lab: [] for lab in CITYSCAPES_INSTANCE_LABELIDS}
    for gid in np.unique(gt):
        lab = gid // 1000 if gid >= 1000 else gid
        if lab in gts:
            gts[lab].append(dict(instID=int(gid), pixelCount=int(np.count_nonzero(gt == gid)), matchedPred=[]))
    preds = {lab: [] for lab in CITYSCAPES_INSTANCE_LABELIDS}
    for pid in np.unique(inst):
        if pid <= 0 or pid // 1000 >= CITYSCAPES_TRAINID_TO_LABELID.size:
            continue
        lab = int(CITYSCAPES_TRAINID_TO_LABELID[pid // 1000])
        if lab not in preds:
            continue
        mask = inst == pid
        n = int(np.count_nonzero(mask))
        if not n:
            continue
        pred = dict(pixelCount=n, confidence=conf.get(int(pid), 1.0) if conf else 1.0,
                    voidIntersection=int(np.count_nonzero(np.logical_and(void, mask))))
        matched = []
        for g in gts[lab]:
            inter = int(np.count_nonzero(np.logical_and(gt == g["instID"], mask)))
            if inter > 0:
                matched.append(dict(g, intersection=inter))
                g["matchedPred"].append(dict(pred, intersection=inter))
        pred["matchedGt"] = matched
        preds[lab].append(pred)
    return gts, preds


def masks_ap(frames, confidences=None, overlaps=CITYSCAPES_OVERLAPS, min_region_size=100):
    """frames: [(instance image, gt instanceIds)]; returns ap [8][len(overlaps)] as evaluateMatches."""
    matches = [_assign(i, g, None if confidences is None else confidences[k]) for k, (i, g) in enumerate(frames)]
    ap = np.zeros((len(CITYSCAPES_INSTANCE_LABELIDS), len(overlaps)))
    for oI, th in enumerate(overlaps):
        for lI, lab in enumerate(CITYSCAPES_INSTANCE_LABELIDS):
            y_true, y_score = np.empty(0), np.empty(0)
            hard_fns = 0
            have_gt = have_pred = False
            for gts_all, preds_all in matches:
                pred_instances = preds_all[lab]
                gt_instances = [g for g in gts_all[lab] if g["instID"] >= 1000 and g["pixelCount"] >= min_region_size]
                if gt_instances:
                    have_gt = True
                if pred_instances:
                    have_pred = True
                cur_true = np.ones(len(gt_instances))
                cur_score = np.ones(len(gt_instances)) * (-float("inf"))
                cur_match = np.zeros(len(gt_instances), dtype=bool)
                for gI, g in enumerate(gt_instances):
                    found = False
                    for pred in g["matchedPred"]:
                        overlap = float(pred["intersection"]) / (g["pixelCount"] + pred["pixelCount"]
                                                                 - pred["intersection"])
                        if overlap > th:
                            confidence = pred["confidence"]
                            if cur_match[gI]:
                                max_s, min_s = max(cur_score[gI], confidence), min(cur_score[gI], confidence)
                                cur_score[gI] = max_s
                                cur_true = np.append(cur_true, 0)
                                cur_score = np.append(cur_score, min_s)
                                cur_match = np.append(cur_match, True)
                            else:
                                found = True
                                cur_match[gI] = True
                                cur_score[gI] = confidence
                    if not found:
                        hard_fns += 1
                cur_true = cur_true[cur_match]
                cur_score = cur_score[cur_match]
                for pred in pred_instances:
                    found_gt = False
                    for g in pred["matchedGt"]:
                        overlap = float(g["intersection"]) / (g["pixelCount"] + pred["pixelCount"] - g["intersection"])
                        if overlap > th:
                            found_gt = True
                            break
                    if not found_gt:
                        ignore = pred["voidIntersection"]
                        for g in pred["matchedGt"]:
                            if g["instID"] < 1000:
                                ignore += g["intersection"]
                            if g["pixelCount"] < min_region_size:
                                ignore += g["intersection"]
                        if float(ignore) / pred["pixelCount"] <= th:
                            cur_true = np.append(cur_true, 0)
                            cur_score = np.append(cur_score, pred["confidence"])
                y_true = np.append(y_true, cur_true)
                y_score = np.append(y_score, cur_score)
            if have_gt and have_pred:
                order = np.argsort(y_score)
                ys, yt = y_score[order], y_true[order]
                cum = np.cumsum(yt)
                _, uniq = np.unique(ys, return_index=True)
                n_pr = len(uniq) + 1
                n_ex, n_true = len(ys), cum[-1]
                precision, recall = np.zeros(n_pr), np.zeros(n_pr)
                cum = np.append(cum, 0)
                for r, i in enumerate(uniq):
                    cs = cum[i - 1]
                    tp = n_true - cs
                    fp = n_ex - i - tp
                    fn = cs + hard_fns
                    precision[r] = float(tp) / (tp + fp)
                    recall[r] = float(tp) / (tp + fn)
                precision[-1], recall[-1] = 1.0, 0.0
                rc = np.append(np.append(recall[0], recall), 0.0)
                steps = np.convolve(rc, [-0.5, 0, 0.5], "valid")
                ap[lI, oI] = np.dot(precision, steps)
            elif have_gt:
                ap[lI, oI] = 0.0
            else:
                ap[lI, oI] = float("nan")
    return ap


def synth_gt(inst, seed):
    """A Cityscapes-like gt instanceIds image from a rendered instance image: each predicted instance becomes a
    gt instance that is shifted, sometimes split in two or merged with its neighbour, sometimes a group (the bare
    labelId); the background is a mix of stuff labelIds and void; a few caravan (29xxx) blobs and hostile values
    (negative, >= 34000) are sprinkled in."""
    rng = np.random.default_rng(seed)
    inst = np.asarray(inst, np.int32)
    n, rows, cols = inst.shape
    gt = np.empty_like(inst)
    stuff = np.array([7, 8, 11, 17, 21, 23, 0, 1, 4, 6], np.int32)
    for f in range(n):
        band = rng.integers(0, stuff.size, (rows // 16 + 1, cols // 16 + 1))
        g = stuff[band].repeat(16, 0).repeat(16, 1)[:rows, :cols].copy()
        dy, dx = int(rng.integers(-3, 4)), int(rng.integers(-3, 4))
        src = np.roll(inst[f], (dy, dx), axis=(0, 1))
        ids = np.unique(src[src > 0])
        serial = {}
        for pid in ids.tolist():
            k = pid // 1000
            if k >= CITYSCAPES_TRAINID_TO_LABELID.size:
                continue
            lab = int(CITYSCAPES_TRAINID_TO_LABELID[k])
            m = src == pid
            r = rng.random()
            if lab not in CITYSCAPES_INSTANCE_LABELIDS:
                g[m] = lab
                continue
            serial[lab] = serial.get(lab, 0) + 1
            if r < 0.15:
                g[m] = lab                                            # a group
            elif r < 0.3:                                             # split in two by columns
                xs = np.nonzero(m.any(0))[0]
                cut = xs[len(xs) // 2]
                left = m.copy(); left[:, cut:] = False
                g[left] = lab * 1000 + serial[lab]
                serial[lab] += 1
                g[m & ~left] = lab * 1000 + serial[lab]
            elif r < 0.4 and lab in serial and serial[lab] > 1:       # merged with the previous one of the label
                g[m] = lab * 1000 + serial[lab] - 1
            else:
                g[m] = lab * 1000 + serial[lab]
        for _ in range(3):                                            # caravans
            y, x = int(rng.integers(0, rows)), int(rng.integers(0, cols))
            g[y:y + 12, x:x + 20] = 29000 + int(rng.integers(0, 5))
        hostile = rng.random((rows, cols)) < 0.002
        g[hostile] = rng.choice(np.array([-1, -7, -2**31, 34000, 2**31 - 1, 99999], np.int32), int(hostile.sum()))
        gt[f] = g
    return gt
