"""CPU tests of the batched road estimation's surface: the C-ABI (is_road_*) and host (ire_*) entry points are
declared, exported and bound, and they refuse bad arguments before they touch a device."""
import ctypes
import os
import re

import pytest

from instance_stixels_amd import core, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROAD_CORE = ["is_road_ctx_create", "is_road_ctx_destroy", "is_road_ctx_device", "is_road_ctx_binary",
             "is_road_vdisparity_batch", "is_road_hough_batch"]
ROAD_HOST = ["ire_compute_batch", "ire_set_batch_limits", "ire_batch_fallbacks", "ire_choose_line"]


def test_road_batch_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "instance_stixels_core.h")).read()
    declared = set(re.findall(r"\b(is_[a-z0-9_]+)\s*\(", text))
    L, H = core.lib(), host.lib()
    for name in ROAD_CORE:
        assert name in declared, f"{name} is not declared in instance_stixels_core.h"
        assert name in core.EXPORTS
        assert hasattr(L, name), f"libis_core.so does not export {name}"
    for name in ROAD_HOST:
        assert name in host.EXPORTS
        assert hasattr(H, name), f"libInstanceStixels.so does not export {name}"
    assert int(re.search(r"#define IS_ROAD_MAX_CANDIDATES (\d+)", text).group(1)) == 8192
    assert host.ROAD_PARAMETERS_DTYPE.itemsize == 16   # Stixels::RoadParameters


def test_road_batch_entry_points_reject_bad_arguments_without_a_gpu():
    L = core.lib()
    ctx = ctypes.c_void_p()
    assert L.is_road_ctx_create(None, 64, 64, 32, 1, -1) == -1
    for rows, cols, D, batch in ((0, 64, 32, 1), (32768, 64, 32, 1), (64, 0, 32, 1), (64, 64, 0, 1),
                                 (64, 64, 16385, 1), (64, 64, 32, 0)):
        assert L.is_road_ctx_create(ctypes.byref(ctx), rows, cols, D, batch, -1) == -1
        assert b"invalid argument" in L.is_last_error()
        assert not ctx.value
    assert L.is_road_vdisparity_batch(None, None, 1, ctypes.c_float(0.2), None, None, None, None) == -1
    assert L.is_road_hough_batch(None, 1, 25, 8, 8, None, None, None, None, None) == -1
    assert L.is_road_ctx_destroy(None) == 0
    assert L.is_road_ctx_device(None) == -1
    assert not L.is_road_ctx_binary(None)


def test_road_estimation_batch_refuses_calls_before_initialize():
    re_ = host.RoadEstimation()
    with pytest.raises(ValueError, match="before Initialize"):
        re_.ComputeBatch(0, 1)
    with pytest.raises(ValueError, match="max_candidates"):
        re_.SetBatchLimits(8, 8193)
    with pytest.raises(ValueError, match="max_lines"):
        re_.SetBatchLimits(0, 16)
    re_.SetBatchLimits(8, 16)
    assert re_.GetBatchFallbacks() == 0
    re_.close()
    with pytest.raises(ValueError, match="closed"):
        re_.GetBatchFallbacks()
