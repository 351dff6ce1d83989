"""CPU tests of f11 (ground-truth offset targets): the numpy restatement of tests/gt_targets_reference.py against the
reference's own Python (tests/golden/reference_python_targets), the surface of the new entry points (declared,
exported, bound), and the refusals that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import gt_targets_reference as gr
from instance_stixels_amd import core, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_python_targets", "gt_targets_reference_python.npz")
CORE_SYMBOLS = ["is_mode_downsample", "is_gt_targets_scratch_bytes", "is_gt_instance_targets"]
HOST_SYMBOLS = ["ish_ground_truth_offsets_batch"]
FAKE = 0x10000   # a "device pointer" that is never dereferenced: every call below is refused before any device call


def fixture_case(z, k):
    """(gt int32 [rows][cols], disparity uint16, ids8 int32, disparity8 uint16, targets3 float32 [3][Hs][Ws]) of case k
    as the reference's Python gave them."""
    return (z[f"c{k}_gt"].astype(np.int32), z[f"c{k}_disparity"], z[f"c{k}_ids8"].astype(np.int32),
            z[f"c{k}_disparity8"], z[f"c{k}_targets3"])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_fixture_holds_every_corner_case():
    z = np.load(GOLDEN)
    names = bytes(z["stat_names"]).decode().split(",")
    assert {"tie2", "tie3", "stuff_beats_id", "id1000", "id1001", "two_parts", "one_cell", "n3_integer",
            "negative_fraction", "even_median", "no_disparity"} <= set(names)
    assert int(z["n_cases"]) == 3
    for k in range(3):
        assert (z[f"c{k}_stats"] >= 1).all(), dict(zip(names, z[f"c{k}_stats"].tolist()))


@pytest.mark.parametrize("k", [0, 1, 2])
def test_restatement_equals_the_reference_bit_for_bit(k):
    gt, disp, ids8, d8, t3 = fixture_case(np.load(GOLDEN), k)
    np.testing.assert_array_equal(gr.mode_downsample(gt), ids8)
    got_d8 = gr.mode_downsample(disp)
    assert got_d8.dtype == np.uint16
    np.testing.assert_array_equal(got_d8, d8)
    np.testing.assert_array_equal(bits(gr.offsets(ids8)), bits(t3[1:]))
    np.testing.assert_array_equal(bits(gr.disparity_plane(ids8, d8)), bits(t3[0]))
    t, i8 = gr.targets(gt[None], disp[None])
    np.testing.assert_array_equal(bits(t[0]), bits(t3))
    np.testing.assert_array_equal(i8[0], ids8)
    t2, _ = gr.targets(gt[None])
    np.testing.assert_array_equal(bits(t2[0]), bits(t3[1:]))


def test_restatement_mode_by_brute_force_on_all_three_types():
    """np.bincount(..).argmax() block by block, as the reference's loop, on random blocks of few values; uint8 too, and
    negative int32 values compared as signed."""
    rng = np.random.default_rng(5)
    for dtype, lo, hi in ((np.uint8, 0, 256), (np.uint16, 0, 65536), (np.int32, 0, 40000)):
        pool = rng.integers(lo, hi, 6).astype(dtype)
        img = pool[rng.integers(0, 6, (2, 24, 40))]
        got = gr.mode_downsample(img)
        assert got.dtype == dtype and got.shape == (2, 3, 5)
        for f in range(2):
            for y in range(3):
                for x in range(5):
                    block = img[f, 8 * y:8 * y + 8, 8 * x:8 * x + 8].astype(np.int64)
                    assert got[f, y, x] == np.bincount(block.ravel()).argmax()
    img = np.full((8, 8), -5, np.int32)
    img[:4] = -(2 ** 31)
    assert gr.mode_downsample(img)[0, 0] == -(2 ** 31)          # a tie: the smaller signed value
    with pytest.raises(ValueError):
        gr.mode_downsample(np.zeros((12, 16), np.int32))


def test_restatement_as_prediction_layout_and_truncation():
    off = np.zeros((1, 2, 2, 3), np.float32)
    off[0, 0, 0, 1] = -0.3125     # 8 * off = -2.5 -> -2 (toward zero)
    off[0, 1, 1, 2] = 0.99        # 7.92 -> 7
    seg = np.full((1, 3, 21, 4), 77, np.int32)
    out = gr.as_prediction(seg, off)
    assert (out[:, :, :19] == 77).all() and (seg == 77).all()
    assert out[0, 1, 19, 2 - 1 - 0] == -2 and out[0, 2, 20, 2 - 1 - 1] == 7
    assert (out[:, :, 19:, 2:] == 0).all()
    assert np.abs(out[:, :, 19:]).sum() == 9


def test_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "instance_stixels_core.h")).read()
    declared = set(re.findall(r"\b(is_[a-z0-9_]+)\s*\(", text))
    L, H = core.lib(), host.lib()
    for name in CORE_SYMBOLS:
        assert name in declared, f"{name} is not declared in instance_stixels_core.h"
        assert name in core.EXPORTS
        assert hasattr(L, name), f"libis_core.so does not export {name}"
    for name in HOST_SYMBOLS:
        assert name in host.EXPORTS
        assert hasattr(H, name), f"libInstanceStixels.so does not export {name}"
    assert int(re.search(r"#define IS_GT_TARGETS_MAX_CAPACITY (\d+)", text).group(1)) == core.GT_TARGETS_MAX_CAPACITY
    for name, value in (("UINT8", core.DTYPE_UINT8), ("UINT16", core.DTYPE_UINT16), ("INT32", core.DTYPE_INT32)):
        assert int(re.search(rf"#define IS_DTYPE_{name} (\d+)", text).group(1)) == value
    # the struct of the binding has the size the header's declaration gives on this ABI
    assert ctypes.sizeof(core.GtTargetsArgs) == 104
    assert hasattr(host.Stixels, "GroundTruthOffsetsBatch") and hasattr(core, "gt_instance_targets")
    from instance_stixels_amd import evaluation
    assert hasattr(evaluation, "gt_offset_scores")


def _refused(match, **fields):
    base = dict(d_gt_instance=FAKE, n_images=1, rows=64, cols=128, d_ids8=FAKE, d_scratch=FAKE, scratch_bytes=1 << 40)
    base.update(fields)
    assert core.gt_instance_targets_ptr(**base) == -1, fields
    err = core.lib().is_last_error().decode()
    assert "invalid argument" in err and re.search(match, err), (fields, err)


def test_gt_instance_targets_refuses_bad_arguments_without_a_gpu():
    L = core.lib()
    assert L.is_gt_instance_targets(None, None) == -1
    _refused("null d_gt_instance", d_gt_instance=None)
    _refused("no output", d_ids8=None)
    _refused("target_planes", d_targets=FAKE, target_planes=4)
    _refused("target_planes", d_targets=FAKE, target_planes=0)
    _refused("target_planes", target_planes=2)                                  # planes without d_targets
    _refused("d_disparity_u16", d_targets=FAKE, target_planes=3)                # 3 planes without a disparity image
    for rows, cols in ((60, 128), (64, 100), (0, 128), (64, 0), (-8, 128)):
        _refused("multiples of 8", rows=rows, cols=cols)
    _refused("n_images", n_images=0)
    _refused("n_images", n_images=65536)
    for p2s in (8, 4, 12, 0, -16):                                              # Hs = 8: a power of two > 8
        _refused("power of two", d_segmentation=FAKE, rows_power2_segmentation=p2s, channels=21)
    _refused("channels", d_segmentation=FAKE, rows_power2_segmentation=16, channels=19)
    _refused("without d_segmentation", rows_power2_segmentation=16)
    _refused("capacity", capacity=-1)
    _refused("capacity", capacity=8 * 16 + 1)                                   # more histograms than cells
    _refused("capacity", capacity=8193, rows=1024, cols=2048)
    _refused("null d_scratch", d_scratch=None)
    _refused("16-byte aligned", d_scratch=FAKE + 8)
    _refused("4-byte aligned", d_gt_instance=FAKE + 2)
    _refused("4-byte aligned", d_key_count=FAKE + 1)
    _refused("2-byte aligned", d_disparity_u16=FAKE + 1)
    need = core.gt_targets_scratch_bytes(1, 64, 128, False, 0)
    assert need > 0 and need % 16 == 0
    _refused("scratch_bytes", scratch_bytes=need - 1)
    _refused("scratch_bytes", scratch_bytes=need, d_disparity_u16=FAKE)         # the histograms need more


def test_scratch_query_and_mode_downsample_refusals_without_a_gpu():
    q = core.gt_targets_scratch_bytes
    assert q(0, 64, 128) == 0 and q(1, 60, 128) == 0 and q(1, 64, 4) == 0 and q(65536, 64, 128) == 0
    assert q(1, 64, 128, True, 129) == 0 and q(1, 64, 128, True, -1) == 0 and q(1, 1024, 2048, True, 8193) == 0
    assert q(1, 64, 128, True, 128) == q(1, 64, 128, True, 0) > q(1, 64, 128, False, 0)   # 0: min(256, cells)
    assert q(1, 1024, 2048, True, 0) == q(1, 1024, 2048, True, 256) > q(1, 1024, 2048, False, 0)
    assert q(2, 1024, 2048) > q(1, 1024, 2048) > 0
    # the table: 2 * pow2(cells) slots of 32 bytes per frame
    assert q(1, 64, 128) >= 2 * 128 * 32 and q(1, 72, 520) >= 2 * 1024 * 32
    m = core.mode_downsample_ptr
    assert m(None, core.DTYPE_INT32, 1, 64, 128, FAKE) == -1
    assert m(FAKE, core.DTYPE_INT32, 1, 64, 128, None) == -1
    assert m(FAKE, 3, 1, 64, 128, FAKE) == -1 and m(FAKE, -1, 1, 64, 128, FAKE) == -1
    assert m(FAKE, core.DTYPE_UINT8, 1, 63, 128, FAKE) == -1 and m(FAKE, core.DTYPE_UINT8, 1, 64, 129, FAKE) == -1
    assert m(FAKE, core.DTYPE_UINT16, 0, 64, 128, FAKE) == -1
    assert m(FAKE + 2, core.DTYPE_INT32, 1, 64, 128, FAKE) == -1      # misaligned for its element
    assert m(FAKE, core.DTYPE_UINT16, 1, 64, 128, FAKE + 1) == -1
    assert b"invalid argument" in core.lib().is_last_error()
