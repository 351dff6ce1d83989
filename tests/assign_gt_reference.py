"""numpy restatement of is_assign_instances_gt / Stixels::AssignInstancesGTBatch (f8), for the tests -- not a test
itself.  Written from the rules of the entry point (instance_stixels_core.h), which restate the reference tooling's
assign_instances_gt over load_instance_mask:

- every section in front of its column's terminator has a class c, whatever its type; w = cols // realcols;
- only c in 11..18 takes part; class c owns labelId L = label_ids[c - 11] (c itself for trainId ground truth);
- the rectangle is image rows rows-1-vT .. rows-1-vB, image columns column*w .. column*w + w-1, clipped to the frame;
  an empty rectangle gives -1 and no vote;
- a pixel v votes for k = v - L*1000 if v > 1000 and L*1000 <= v < (L+1)*1000, else for background;
- the most frequent value wins, background competes, ties go to background and then to the smaller k;
- the winner's count must NOT be < (min_fraction * w) * (vT - vB) in binary64, in that operand order;
- label = k when a non-background value won and passed, else -1; votes = the winner's pixel count (0: no vote);
- slots at and behind the terminator: label -1, votes 0.
"""
import numpy as np

CITYSCAPES_LABEL_IDS = (24, 25, 26, 27, 28, 31, 32, 33)


def column_count(col):
    t = np.nonzero(col["type"] == -1)[0]
    return int(t[0]) if t.size else len(col)


def vote(pixels, L, min_fraction, w, vB, vT):
    """(label, votes) of one non-empty rectangle of ground-truth pixels for a class that owns labelId L."""
    v = np.asarray(pixels, np.int64).ravel()
    k = v - L * 1000
    inst = (v > 1000) & (k >= 0) & (k < 1000)
    counts = np.bincount(np.where(inst, k + 1, 0), minlength=1001)   # bin 0: background, bin 1 + k: instance k
    win = int(counts.argmax())                                       # the smaller bin on a tie
    n = int(counts[win])
    few = float(n) < (float(min_fraction) * float(w)) * float(int(vT) - int(vB))
    return (win - 1 if win > 0 and not few else -1), n


def assign(sections, gt, min_fraction=0.1, label_ids=CITYSCAPES_LABEL_IDS, gt_is_train_ids=False):
    """sections [n][realcols][max_sections] SECTION_DTYPE, gt [n][rows][cols] int32 ->
    (labels, votes), each int32 [n][realcols][max_sections]."""
    sections = np.asarray(sections)
    gt = np.asarray(gt, np.int32)
    n, C, S = sections.shape
    _, rows, cols = gt.shape
    w = cols // C
    labels = np.full((n, C, S), -1, np.int32)
    votes = np.zeros((n, C, S), np.int32)
    for f in range(n):
        for c in range(C):
            col = sections[f, c]
            for i in range(column_count(col)):
                cls = int(col[i]["semantic_class"])
                if not 11 <= cls <= 18:
                    continue
                vB, vT = int(col[i]["vB"]), int(col[i]["vT"])
                top, bot = max(rows - 1 - vT, 0), min(rows - 1 - vB, rows - 1)
                if top > bot:
                    continue
                L = cls if gt_is_train_ids else int(label_ids[cls - 11])
                labels[f, c, i], votes[f, c, i] = vote(gt[f, top:bot + 1, c * w:c * w + w], L, min_fraction, w, vB, vT)
    return labels, votes


def mappings(labels):
    """Per frame {(column, section): label} of the labelled sections: what the consumers' references take."""
    out = []
    for lab in labels:
        cs, ss = np.nonzero(lab >= 0)
        out.append({(int(c), int(s)): int(lab[c, s]) for c, s in zip(cs, ss)})
    return out
