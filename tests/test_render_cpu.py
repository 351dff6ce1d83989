"""CPU tests of f5 (stixels to dense result maps, scored on the device): the C-ABI and host entry points are
declared, exported and bound and refuse bad arguments before they touch a device; the numpy restatement
(tests/render_reference.py) and the Cityscapes IoU give hand-worked answers."""
import ctypes
import os
import re

import numpy as np
import pytest

import render_reference as rr
from instance_stixels_amd import core, evaluation, host
from instance_stixels_amd.config import SECTION_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RENDER_CORE = ["is_section_instance_labels", "is_render_sections"]
RENDER_HOST = ["ish_render_batch"]
FAKE = 1 << 20   # an aligned, never dereferenced "device" address: every call below fails its checks first


def test_render_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "instance_stixels_core.h")).read()
    declared = set(re.findall(r"\b(is_[a-z0-9_]+)\s*\(", text))
    L, H = core.lib(), host.lib()
    for name in RENDER_CORE:
        assert name in declared, f"{name} is not declared in instance_stixels_core.h"
        assert name in core.EXPORTS
        assert hasattr(L, name), f"libis_core.so does not export {name}"
    for name in RENDER_HOST:
        assert name in host.EXPORTS
        assert hasattr(H, name), f"libInstanceStixels.so does not export {name}"
    assert int(re.search(r"#define IS_RENDER_MAX_LABELS (\d+)", text).group(1)) == core.RENDER_MAX_LABELS
    assert int(re.search(r"#define IS_RENDER_MAX_CLASSES (\d+)", text).group(1)) == core.RENDER_MAX_CLASSES
    # the ctypes mirror of is_render_args: same fields in the same order
    body = re.search(r"typedef struct is_render_args \{(.*?)\} is_render_args;", text, re.S).group(1)
    fields = re.findall(r"\b([a-z_]+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f for f, _ in core.RenderArgs._fields_]
    assert hasattr(host.Stixels, "RenderBatch")


def _args(**kw):
    base = dict(d_sections=FAKE, n_images=1, realcols=8, max_sections=16, rows=64, cols=72)
    base.update(kw)
    return core.RenderArgs(**base)


@pytest.mark.parametrize("kw, why", [
    (dict(d_sections=None), "null sections"),
    (dict(cols=7), "cols < realcols"),
    (dict(rows=0), "rows < 1"),
    (dict(n_images=0), "n_images < 1"),
    (dict(max_sections=0), "max_sections < 1"),
    (dict(d_sections=FAKE + 8), "misaligned sections"),
    (dict(d_gt_label=FAKE, d_confusion=FAKE, n_labels=0), "n_labels < 1"),
    (dict(d_gt_label=FAKE, d_confusion=FAKE, n_labels=65), "n_labels > 64"),
    (dict(d_confusion=FAKE, n_labels=34), "confusion without gt labels"),
    (dict(d_gt_label=FAKE, n_labels=34), "gt labels without confusion"),
    (dict(d_gt_disparity=FAKE, d_disp_abs_sum=FAKE), "deviation sum without a count"),
    (dict(d_gt_disparity=FAKE, d_disp_count=FAKE), "deviation count without a sum"),
    (dict(d_disp_abs_sum=FAKE, d_disp_count=FAKE), "deviation without gt disparity"),
    (dict(d_gt_disparity=FAKE), "gt disparity without sum and count"),
])
def test_render_sections_refuses_bad_arguments_without_a_gpu(kw, why):
    L = core.lib()
    assert L.is_render_sections(ctypes.byref(_args(**kw)), None) == -1, why
    assert b"invalid argument" in L.is_last_error()


def test_render_sections_refuses_bad_class_tables_and_null_args():
    L = core.lib()
    assert L.is_render_sections(None, None) == -1
    table = np.arange(300, dtype=np.uint8)
    for n_classes in (0, -1, 257):
        a = _args(h_class_to_label=table.ctypes.data, n_classes=n_classes)
        assert L.is_render_sections(ctypes.byref(a), None) == -1, n_classes
    ib = (core.InstanceBuffers * 1)()
    assert L.is_section_instance_labels(ib, 1, 8, 16, FAKE, None) == -1          # arrays missing
    assert L.is_section_instance_labels(ib, 1, 8, 16, None, None) == -1
    assert L.is_section_instance_labels(None, 1, 8, 16, FAKE, None) == -1
    ib[0].d_indices = ib[0].d_labels = ib[0].d_instances_per_class = FAKE
    assert L.is_section_instance_labels(ib, 0, 8, 16, FAKE, None) == -1          # empty batch


def test_render_batch_before_any_compute_raises():
    st = host.Stixels()
    with pytest.raises(ValueError, match="none"):
        st.RenderBatch(1)
    with pytest.raises(ValueError, match="none"):
        st.RenderBatch(1, label=FAKE, gt_label=FAKE, confusion=FAKE)
    st.close()


def _sec(rows):
    s = np.zeros(len(rows), SECTION_DTYPE)
    for k, (t, vb, vt, d, c) in enumerate(rows):
        s[k]["type"], s[k]["vB"], s[k]["vT"], s[k]["disparity"], s[k]["semantic_class"] = t, vb, vt, d, c
    return s


def test_restatement_two_columns_one_row_stixel_early_terminator_and_width_quirk():
    """rows 4, cols 5, 2 stixel columns: w = 5 // 2 = 2, so x = 4 is no stixel's.  Column 0: a one-row ground
    stixel at the bottom (vB = vT = 0), an object above it up to the top.  Column 1: a sky stixel on the two
    bottom rows, then an early terminator -- the rows above stay 0."""
    sec = np.zeros((1, 2, 4), SECTION_DTYPE)
    sec["type"] = -1
    sec[0, 0, :3] = _sec([(0, 0, 0, 1.5, 0), (1, 1, 3, 7.25, 11), (-1, 0, 0, 0, 0)])
    sec[0, 1, :2] = _sec([(2, 0, 1, 0.5, 10), (-1, 0, 0, 0, 0)])
    label, disp, inst, count = rr.render(sec, 4, 5, instances=[{(0, 1): 3, (1, 0): 2}])
    want_label = np.array([[24, 24, 0, 0, 0],
                           [24, 24, 0, 0, 0],
                           [24, 24, 23, 23, 0],
                           [7, 7, 23, 23, 0]], np.uint8)
    want_disp = np.array([[7.25, 7.25, 0, 0, 0],
                          [7.25, 7.25, 0, 0, 0],
                          [7.25, 7.25, 0.5, 0.5, 0],
                          [1.5, 1.5, 0.5, 0.5, 0]], np.float32)
    want_inst = np.array([[11003, 11003, 0, 0, 0],
                          [11003, 11003, 0, 0, 0],
                          [11003, 11003, 10002, 10002, 0],
                          [0, 0, 10002, 10002, 0]], np.int32)
    np.testing.assert_array_equal(label[0], want_label)
    np.testing.assert_array_equal(disp[0], want_disp)
    np.testing.assert_array_equal(inst[0], want_inst)
    assert count.tolist() == [3]
    # the deviation and the confusion of that frame against a hand-made ground truth
    gt = np.array([[24, 0, 0, 255, 7]] * 4, np.uint8)
    conf = rr.confusion(label, gt[None], 34)
    assert conf[24, 24] == 3 and conf[0, 24] == 3 and conf[24, 7] == 1 and conf[0, 7] == 1
    assert conf[0, 0] == 2 and conf[0, 23] == 2 and conf[7, 0] == 4
    assert int(conf.sum()) == 20 - 4       # the 255 column is skipped
    gtd = np.full((1, 4, 5), 2.0, np.float32)
    gtd[0, 0, 0] = 0.0
    s, n = rr.deviation(disp, gtd)
    assert n.tolist() == [11] and s[0] == pytest.approx(5 * 5.25 + 2 * 0.5 + 4 * 1.5)


def test_restatement_instance_id_rule():
    """class*1000 + l for 0 <= l < 1000 only: label -1 (noise), label >= 1000 and no candidate give 0."""
    sec = np.zeros((1, 5, 2), SECTION_DTYPE)
    sec["type"] = -1
    for c in range(5):
        sec[0, c, 0] = _sec([(1, 0, 1, 3.0, 11 + c)])[0]
    m = {(0, 0): -1, (1, 0): 1000, (2, 0): 999, (3, 0): 0}
    _, _, inst, _ = rr.render(sec, 2, 5, instances=[m])
    assert inst[0, 0].tolist() == [0, 0, 13999, 14000, 0]
    _, _, none, _ = rr.render(sec, 2, 5)
    assert not none.any()
    # a class outside the table gives label 0
    sec[0, 4, 0]["semantic_class"] = 19
    label, _, _, _ = rr.render(sec, 2, 5)
    assert label[0, 0].tolist() == [24, 25, 26, 27, 0]


def test_cityscapes_iou_hand_computed():
    ev = evaluation.CITYSCAPES_EVAL_LABELIDS
    assert len(ev) == 19 and evaluation.CITYSCAPES_TRAINID_TO_LABELID.tolist() == rr.CITYSCAPES.tolist()
    # perfect on two classes, the others absent: NaN, mean over the two
    conf = np.zeros((34, 34), np.uint64)
    conf[7, 7], conf[26, 26] = 100, 50
    iou, mean = evaluation.cityscapes_iou(conf)
    assert iou[ev.index(7)] == 1.0 and iou[ev.index(26)] == 1.0
    assert np.isnan(iou).sum() == 17 and mean == 1.0
    # fn takes every prediction of the row (ignored labels too); fp only rows of evaluated labels
    conf[7, 26] = 10      # road predicted as car: fn of 7, fp of 26
    conf[7, 0] = 5        # road predicted as unlabelled: fn of 7
    conf[0, 26] = 1000    # ignored gt predicted as car: no fp
    conf[3, 7] = 1000     # ignored gt predicted as road: no fp
    conf[8, 7] = 20       # sidewalk predicted as road: fp of 7, fn of 8
    iou, mean = evaluation.cityscapes_iou(conf)
    assert iou[ev.index(7)] == pytest.approx(100 / (100 + 20 + 15))
    assert iou[ev.index(26)] == pytest.approx(50 / (50 + 10))
    assert iou[ev.index(8)] == 0.0
    assert mean == pytest.approx((100 / 135 + 50 / 60 + 0) / 3)
    _, mean = evaluation.cityscapes_iou(np.zeros((34, 34)))
    assert np.isnan(mean)
    with pytest.raises(ValueError):
        evaluation.cityscapes_iou(np.zeros((34, 33)))


def test_mean_disparity_deviation():
    m = evaluation.mean_disparity_deviation([6.0, 0.0, 1.5], [3, 0, 1])
    assert m[0] == 2.0 and np.isnan(m[1]) and m[2] == 1.5
