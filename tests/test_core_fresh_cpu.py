"""core._Fresh, the allocator of an entry point's fresh tensors and their guards, on torch.device("cpu"), with
tests/guards.py as the check the GPU tests use; and core._ARGS_ENTRY with the `_ptr` functions made from it."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from guards import check_guards
from instance_stixels_amd import core

CPU = torch.device("cpu")
SHAPE = (2, 3, 5)
NUMEL = 30
# dtype: the pattern of a guard element, as guards() returns it
PATTERNS = {torch.float32: np.float32(-12345.0), torch.float16: np.uint16(0x5A5A), torch.bfloat16: np.uint16(0x5A5A),
            torch.int32: np.int32(0x5A5A5A5A), torch.int64: np.int64(0x5A5A5A5A5A5A5A5A), torch.uint8: np.uint8(0xA5)}
DTYPES = list(PATTERNS)
IDS = [str(d)[6:] for d in DTYPES]
GENERATED = ["gt_instance_targets_ptr", "offset_loss_ptr", "segmentation_head_ptr", "conv3x3_bn_relu_ptr", "conv_bn_ptr",
             "conv_bn_stride_ptr", "stem_ptr", "segmentation_head_backward_ptr", "conv_bn_backward_ptr",
             "conv_bn_stride_backward_ptr", "stem_backward_ptr", "semantic_nll_ptr", "semantic_nll_up_ptr"]


def _element_at(t, offset):
    """The one element of t's allocation `offset` elements from t's first."""
    return torch.as_strided(t, (1,), (1,), t.storage_offset() + offset)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_without_canary_a_plain_tensor_and_no_guards(dtype):
    fresh = core._Fresh(CPU, 0)
    t = fresh.new("out", SHAPE, dtype)
    scratch = fresh.scratch(100)
    assert tuple(t.shape) == SHAPE and t.dtype == dtype and t.is_contiguous() and t.storage_offset() == 0
    assert t.untyped_storage().nbytes() == NUMEL * t.element_size()          # no hidden guard
    assert scratch.dtype == torch.uint8 and scratch.untyped_storage().nbytes() == 100
    assert fresh.guards() == {}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_with_canary_the_view_lies_between_guards_of_the_pattern(dtype):
    fresh = core._Fresh(CPU, 5)
    t = fresh.new("out", SHAPE, dtype)
    assert tuple(t.shape) == SHAPE and t.dtype == dtype and t.is_contiguous()
    assert t.storage_offset() == 5 and t.untyped_storage().nbytes() == (NUMEL + 10) * t.element_size()
    front, back, pattern = fresh.guards()["out"]
    want = PATTERNS[dtype]
    assert pattern == want and pattern.dtype == want.dtype and front.dtype == want.dtype == back.dtype
    assert front.tolist() == [want] * 5 == back.tolist()
    t.copy_(torch.arange(NUMEL).reshape(SHAPE))                              # every element of the view
    check_guards(fresh.guards(), 5, {"out"})
    assert t.flatten().tolist() == list(range(NUMEL))


@pytest.mark.parametrize("offset", [-1, NUMEL], ids=["before", "after"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_write_next_to_the_view_is_reported_with_the_name(dtype, offset):
    fresh = core._Fresh(CPU, 5)
    fresh.new("other", (4,), dtype)
    t = fresh.new("victim", SHAPE, dtype)
    _element_at(t, offset).fill_(1)
    with pytest.raises(AssertionError, match="victim"):
        check_guards(fresh.guards(), 5)
    with pytest.raises(AssertionError, match="victim"):                      # ... and a missing entry by the key set
        check_guards(fresh.guards(), 5, {"other"})


@pytest.mark.parametrize("canary, guard", [(5, 16), (16, 16), (17, 32)])
def test_scratch_guard_is_whole_16_bytes(canary, guard):
    fresh = core._Fresh(CPU, canary)
    scratch = fresh.scratch(100)
    assert scratch.dtype == torch.uint8 and tuple(scratch.shape) == (100,)
    whole = scratch.untyped_storage()
    assert whole.nbytes() == 100 + 2 * guard
    assert (scratch.data_ptr() - whole.data_ptr()) % 16 == 0 and scratch.data_ptr() - whole.data_ptr() == guard
    front, back, pattern = fresh.guards()["scratch"]
    assert front.size == back.size == guard and pattern == np.uint8(0xA5) and pattern.dtype == np.uint8
    scratch.fill_(0)
    check_guards(fresh.guards(), canary, {"scratch"})
    _element_at(scratch, 100).fill_(0)
    with pytest.raises(AssertionError, match="scratch"):
        check_guards(fresh.guards(), canary)


@pytest.mark.parametrize("canary", [0, 5])
def test_rows_give_the_wanted_tensors_and_their_pointers(canary):
    fresh = core._Fresh(CPU, canary)
    out, ptr = fresh.rows((("a", True, SHAPE, torch.float32), ("b", False, (7,), torch.float32),
                           ("c", 1, (7,), torch.bfloat16), ("d", None, SHAPE, torch.uint8)))
    assert list(out) == ["a", "c"] and list(ptr) == ["a", "b", "c", "d"]
    assert ptr["b"] is None and ptr["d"] is None
    assert ptr["a"] == out["a"].data_ptr() and ptr["c"] == out["c"].data_ptr()
    assert tuple(out["a"].shape) == SHAPE and out["c"].dtype == torch.bfloat16
    assert set(fresh.guards()) == ({"a", "c"} if canary else set())
    check_guards(fresh.guards(), canary)


def test_every_table_entry_is_an_export_with_its_argtypes():
    assert len(core._ARGS_ENTRY) == 20 and set(core._ARGS_ENTRY) <= set(core.EXPORTS)
    for entry, cls in core._ARGS_ENTRY.items():
        assert issubclass(cls, ctypes.Structure), entry
        assert getattr(core.lib(), entry).argtypes == [ctypes.POINTER(cls), ctypes.c_void_p], entry


@pytest.mark.parametrize("name", GENERATED)
def test_generated_ptr_functions(name):
    fn = getattr(core, name)
    entry = "is_" + name[:-4]
    assert str(inspect.signature(fn)) == "(stream=0, **fields)"
    assert fn.__name__ == name == fn.__qualname__
    assert entry in fn.__doc__ and core._ARGS_ENTRY[entry].__name__ in fn.__doc__
    assert fn() != 0                                                         # null pointers: refused, nothing raised
    if hasattr(core._ARGS_ENTRY[entry], "reserved"):
        assert fn(reserved=(1, 0, 0, 0)) != 0
