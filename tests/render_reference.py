"""numpy restatement of is_render_sections / Stixels::RenderBatch (f5), for the tests -- not a test itself.

It follows the reference tooling that draws and scores stixel result images on the host
(tools/visualization/clustering_visualization.py, tools/evaluation/disparity.py of the reference):
- stixel width w = cols // len(stixels) (draw_stixels :186), NOT column_step;
- section (c, i) is the filled rectangle x in [c*w, c*w + w-1], y in [rows-1-vT, rows-1-vB] (:214-217), clipped
  to the frame as cv2.rectangle clips; sections are drawn in index order, so the last one wins where hand-built
  sections overlap;
- label image: trainId2label[class].id (:396-402), i.e. class_to_label[class], 0 for a class outside the table;
- disparity image: the section's disparity for every section type (:403-409, "TODO: Handle ground stixels");
- instance image: class*1000 + l for a section with cluster label 0 <= l < 1000, else 0 (read_stixel_file
  :108-114; draw_instance_masks :118-142 draws the mask of id k where this image equals k);
- pixels no section covers stay 0 (the zero-initialised images of :1166-1176);
- disparity deviation over pixels where stixel != 0 and gt != 0 (disparity.py:56-62);
- stixel count: the sections in front of the terminators (run_cityscapes.py:611, avg_no_stixels).
"""
import numpy as np

CITYSCAPES = np.array([7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33], np.uint8)


def column_count(col):
    """Sections in front of the terminator (type == -1) of one column."""
    t = np.nonzero(col["type"] == -1)[0]
    return int(t[0]) if t.size else len(col)


def render(sections, rows, cols, instances=None, class_to_label=CITYSCAPES):
    """sections [n][realcols][max_sections] SECTION_DTYPE; instances: None, or per frame a mapping
    {(column, section): cluster label} (Stixels.ComputeBatch / GetInstanceStixels).
    Returns label uint8, disparity float32, instance int32, each [n][rows][cols], and stixel counts int32 [n]."""
    sections = np.asarray(sections)
    n, C, S = sections.shape
    w = cols // C
    table = np.asarray(class_to_label, np.uint8)
    label = np.zeros((n, rows, cols), np.uint8)
    disp = np.zeros((n, rows, cols), np.float32)
    inst = np.zeros((n, rows, cols), np.int32)
    counts = np.zeros(n, np.int32)
    for f in range(n):
        m = instances[f] if instances is not None else {}
        for c in range(C):
            col = sections[f, c]
            k = column_count(col)
            counts[f] += k
            for i in range(k):
                s = col[i]
                top, bot = rows - 1 - int(s["vT"]), rows - 1 - int(s["vB"])
                top, bot = max(top, 0), min(bot, rows - 1)
                if top > bot:
                    continue
                cls = int(s["semantic_class"])
                lab = table[cls] if 0 <= cls < table.size else 0
                l = m.get((c, i), -1)
                iv = np.int64(cls) * 1000 + l if 0 <= l < 1000 else 0
                iv = np.array(iv & 0xffffffff, np.uint32).view(np.int32)   # (int32 arithmetic, wrapping)
                label[f, top:bot + 1, c * w:c * w + w] = lab
                disp[f, top:bot + 1, c * w:c * w + w] = s["disparity"]
                inst[f, top:bot + 1, c * w:c * w + w] = iv
    return label, disp, inst, counts


def confusion(label, gt, n_labels):
    """conf[gt][pred] over all pixels with gt < n_labels and pred < n_labels, uint64 [n_labels][n_labels]."""
    p = np.asarray(label).astype(np.int64).ravel()
    g = np.asarray(gt).astype(np.int64).ravel()
    keep = (p < n_labels) & (g < n_labels)
    return np.bincount(g[keep] * n_labels + p[keep], minlength=n_labels * n_labels).astype(np.uint64).reshape(
        n_labels, n_labels)


def deviation(disp, gt_disp):
    """Per frame: (sum of |stixel - gt| -- each term fp32, summed in fp64 --, count) over pixels where both are
    non-zero."""
    disp = np.asarray(disp, np.float32)
    gt_disp = np.asarray(gt_disp, np.float32)
    sums, counts = [], []
    for d, g in zip(disp, gt_disp):
        mask = (d != 0) & (g != 0)
        sums.append(float(np.abs(d[mask] - g[mask]).astype(np.float64).sum()))
        counts.append(int(mask.sum()))
    return np.array(sums, np.float64), np.array(counts, np.int64)
