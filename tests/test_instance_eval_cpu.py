"""CPU tests of f6 (instance overlap tables on the device, Cityscapes AP on the host): the C-ABI and host entry
points are declared, exported and bound and refuse bad arguments before they touch a device; the table-based
evaluator (evaluation.CityscapesInstanceEval) gives hand-worked APs and agrees with the literal per-mask
restatement of tests/instance_eval_reference.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import instance_eval_reference as ir
from instance_stixels_amd import core, evaluation, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OVERLAP_CORE = ["is_instance_overlap", "is_pack_overlap_records"]
OVERLAP_HOST = ["ish_instance_overlap_batch", "ish_instance_overlap_records", "ish_set_instance_overlap_capacity"]
FAKE = 1 << 20   # an aligned, never dereferenced "device" address: every call below fails its checks first


def test_overlap_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "instance_stixels_core.h")).read()
    declared = set(re.findall(r"\b(is_[a-z0-9_]+)\s*\(", text))
    L, H = core.lib(), host.lib()
    for name in OVERLAP_CORE:
        assert name in declared, f"{name} is not declared in instance_stixels_core.h"
        assert name in core.EXPORTS
        assert hasattr(L, name), f"libis_core.so does not export {name}"
    for name in OVERLAP_HOST:
        assert name in host.EXPORTS
        assert hasattr(H, name), f"libInstanceStixels.so does not export {name}"
    assert int(re.search(r"#define IS_OVERLAP_MAX_CAPACITY \(1 << (\d+)\)", text).group(1)) == \
        core.OVERLAP_MAX_CAPACITY.bit_length() - 1
    body = re.search(r"typedef struct is_instance_overlap_args \{(.*?)\} is_instance_overlap_args;", text, re.S).group(1)
    fields = re.findall(r"\b([a-z_]+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f for f, _ in core.InstanceOverlapArgs._fields_]
    rec = re.search(r"typedef struct is_overlap_record \{(.*?)\} is_overlap_record;", text, re.S).group(1)
    assert re.findall(r"\b([a-z_]+)\s*;", rec) == list(core.OVERLAP_DTYPE.names)
    assert core.OVERLAP_DTYPE.itemsize == 16
    assert hasattr(host.Stixels, "InstanceOverlapBatch") and hasattr(host.Stixels, "SetInstanceOverlapCapacity")


def _args(**kw):
    base = dict(d_sections=FAKE, n_images=1, realcols=8, max_sections=16, rows=64, cols=72, d_gt_instance=FAKE,
                capacity=64, d_records=FAKE, d_n_records=FAKE, d_overflow=FAKE)
    base.update(kw)
    return core.InstanceOverlapArgs(**base)


@pytest.mark.parametrize("kw, why", [
    (dict(d_sections=None), "null sections"),
    (dict(d_gt_instance=None), "null gt"),
    (dict(d_records=None), "null records"),
    (dict(d_n_records=None), "null n_records"),
    (dict(d_overflow=None), "null overflow"),
    (dict(cols=7), "cols < realcols"),
    (dict(rows=0), "rows < 1"),
    (dict(n_images=0), "n_images < 1"),
    (dict(n_images=65536), "n_images > 65535"),
    (dict(max_sections=0), "max_sections < 1"),
    (dict(capacity=0), "capacity < 1"),
    (dict(capacity=(1 << 28) + 1), "capacity too large"),
    (dict(rows=1 << 15, cols=1 << 14), "frame too large"),
    (dict(d_sections=FAKE + 8), "misaligned sections"),
    (dict(d_gt_instance=FAKE + 2), "misaligned gt"),
    (dict(d_records=FAKE + 4), "misaligned records"),
    (dict(d_section_instance=FAKE + 1), "misaligned map"),
])
def test_instance_overlap_refuses_bad_arguments_without_a_gpu(kw, why):
    L = core.lib()
    assert L.is_instance_overlap(ctypes.byref(_args(**kw)), None) == -1, why
    assert b"invalid argument" in L.is_last_error()


def test_pack_refuses_bad_arguments_and_null_args():
    L = core.lib()
    assert L.is_instance_overlap(None, None) == -1
    assert L.is_pack_overlap_records(None, FAKE, 1, 4, FAKE, None) == -1
    assert L.is_pack_overlap_records(FAKE, FAKE, 0, 4, FAKE, None) == -1
    assert L.is_pack_overlap_records(FAKE, FAKE, 1, 0, FAKE, None) == -1
    assert L.is_pack_overlap_records(FAKE + 4, FAKE, 1, 4, FAKE, None) == -1


def test_instance_overlap_batch_before_any_compute_raises():
    st = host.Stixels()
    with pytest.raises(ValueError, match="none"):
        st.InstanceOverlapBatch(1, FAKE)
    with pytest.raises(ValueError, match="records"):
        st.SetInstanceOverlapCapacity(0)
    st.close()


# ---- hand-worked APs ---------------------------------------------------------------------------------------------
CAR = 13 * 1000        # trainId 13 -> labelId 26 (car)
PERSON = 11 * 1000     # trainId 11 -> labelId 24 (person)
I_CAR = evaluation.CITYSCAPES_INSTANCE_LABELIDS.index(26)
I_PERSON = evaluation.CITYSCAPES_INSTANCE_LABELIDS.index(24)


def _eval(*frames, confidences=None):
    ev = evaluation.CityscapesInstanceEval()
    ev.add([ir.joint_histogram(i, g) for i, g in frames], confidences)
    return ev.result()


def _frame(rows=40, cols=40, bg=7):
    return np.zeros((rows, cols), np.int32), np.full((rows, cols), bg, np.int32)


def test_one_exact_match_is_ap_1():
    inst, gt = _frame()
    inst[5:25, 5:25] = CAR + 1
    gt[5:25, 5:25] = 26001
    r = _eval((inst, gt))
    assert (r["ap"][I_CAR] == 1.0).all()
    assert np.isnan(np.delete(r["ap"], I_CAR, 0)).all()
    assert r["AP"] == 1.0 and r["AP50"] == 1.0


def test_two_gt_one_match_one_false_positive_is_0375():
    inst, gt = _frame(60, 60)
    gt[0:20, 0:20] = 26001          # matched
    gt[30:50, 0:20] = 26002         # missed: a hard false negative
    inst[0:20, 0:20] = CAR + 1
    inst[30:50, 30:50] = CAR + 2    # on background: a false positive
    r = _eval((inst, gt))
    np.testing.assert_allclose(r["ap"][I_CAR], 0.375)   # r = 1/2, p = 1/2: r (p + 1) / 2
    assert r["AP"] == pytest.approx(0.375)


def test_small_gt_under_a_pred_is_nan_and_no_false_positive():
    inst, gt = _frame()
    gt[0:9, 0:9] = 26001            # 81 px < 100: not counted
    inst[0:9, 0:9] = CAR + 1
    r = _eval((inst, gt))
    assert np.isnan(r["ap"][I_CAR]).all() and np.isnan(r["AP"])
    # with a counted gt elsewhere, the pred over the small one is no false positive: AP 1 at every threshold
    gt[20:40, 20:40] = 26002
    inst[20:40, 20:40] = CAR + 2
    r = _eval((inst, gt))
    assert (r["ap"][I_CAR] == 1.0).all()


def test_void_or_group_dominated_unmatched_pred_is_no_false_positive():
    inst, gt = _frame(60, 60)
    gt[0:20, 0:20] = 26001
    inst[0:20, 0:20] = CAR + 1
    gt[30:50, 30:50] = 0            # void (unlabeled)
    inst[30:50, 30:50] = CAR + 2
    r = _eval((inst, gt))
    assert (r["ap"][I_CAR] == 1.0).all()
    gt[30:50, 30:50] = 26           # a car group
    r = _eval((inst, gt))
    assert (r["ap"][I_CAR] == 1.0).all()
    # only 60 % void: ignored share 0.6 is above 0.5 .. 0.55 but not above 0.6 .. 0.95
    gt[30:50, 30:50] = 7
    gt[30:42, 30:50] = 0
    r = _eval((inst, gt))
    # from the third threshold (0.6000000000000001) on, 240/400 = 0.6 is not above it: a false positive,
    # r = 1, p = 1/2, AP = r (p + 1) / 2 = 0.75
    want = np.where(evaluation.CITYSCAPES_OVERLAPS < 0.59, 1.0, 0.75)
    np.testing.assert_allclose(r["ap"][I_CAR], want)


def test_class_with_gt_but_no_prediction_is_0():
    inst, gt = _frame()
    gt[0:20, 0:20] = 24001
    inst[20:40, 20:40] = CAR + 1
    gt[20:40, 20:40] = 26001
    r = _eval((inst, gt))
    assert (r["ap"][I_PERSON] == 0.0).all() and (r["ap"][I_CAR] == 1.0).all()
    assert r["AP"] == 0.5


def test_two_batches_equal_one_batch_of_both():
    rng = np.random.default_rng(1)
    frames = [_random_frame(rng) for _ in range(4)]
    tables = [ir.joint_histogram(i, g) for i, g in frames]
    a = evaluation.CityscapesInstanceEval()
    a.add(tables[:2])
    a.add(tables[2:])
    b = evaluation.CityscapesInstanceEval()
    b.add(tables)
    ra, rb = a.result(), b.result()
    np.testing.assert_array_equal(ra["ap"], rb["ap"])
    assert ra["AP"] == rb["AP"] or (np.isnan(ra["AP"]) and np.isnan(rb["AP"]))


def test_joint_histogram_sums_and_order():
    rng = np.random.default_rng(0)
    inst, gt = _random_frame(rng)
    t = ir.joint_histogram(inst, gt)
    assert int(t["count"].sum()) == inst.size and (t["count"] > 0).all()
    k = t["pred"].astype(np.int64) * 2**32 + t["gt"].astype(np.int64)
    assert (np.diff(k) > 0).all()


def _random_frame(rng, rows=96, cols=128):
    """Blocky pred instances of random classes; a gt built from them (tests/instance_eval_reference.synth_gt)."""
    inst = np.zeros((rows, cols), np.int32)
    for _ in range(int(rng.integers(4, 14))):
        y, x = int(rng.integers(0, rows - 8)), int(rng.integers(0, cols - 8))
        h, w = int(rng.integers(6, 40)), int(rng.integers(6, 40))
        inst[y:y + h, x:x + w] = int(rng.choice([11, 12, 13, 14, 15, 16, 17, 18, 0, 5])) * 1000 + \
            int(rng.integers(0, 4))
    return inst, ir.synth_gt(inst[None], int(rng.integers(0, 1 << 30)))[0]


@pytest.mark.parametrize("seed", range(6))
def test_table_evaluator_equals_per_mask_restatement(seed):
    rng = np.random.default_rng(100 + seed)
    frames = [_random_frame(rng) for _ in range(3)]
    conf = None
    if seed % 2:
        conf = [{int(p): float(rng.choice([0.3, 0.6, 0.9])) for p in np.unique(i)} for i, _ in frames]
    want = ir.masks_ap(frames, conf)
    got = _eval(*frames, confidences=conf)
    np.testing.assert_array_equal(np.isnan(got["ap"]), np.isnan(want))
    np.testing.assert_allclose(got["ap"][~np.isnan(want)], want[~np.isnan(want)], rtol=0, atol=1e-12)
    assert (~np.isnan(want)).any()
