"""k_road_histogram / k_road_binarize (is_k_road.hip; the binarise without and with its point list)
at their edges: NaN (bin 0, stated in the kernels), +-inf, values in (-1, 0), values <= -1, |d| >= 2^31, exact
zeros, row lengths that are no multiple of the 256 threads and max_dis that is no multiple of 64, against
frontend_reference.vdisparity -- exactly, through the single-frame entry and the batched one.  The CPU half
pins the restatement to the numpy twin it replaces in tests/test_road_batch_gpu.py and to the oracle."""
import ctypes
import functools

import numpy as np
import pytest

import frontend_reference as fr
from oracle import oracle
from test_render_gpu import Out

THR = 0.2   # road_vdisparity_threshold of RoadEstimation::Initialize
# (rows, cols, max_dis)
SHAPES = [(8, 1, 2), (16, 255, 48), (16, 257, 64), (24, 1000, 100), (8, 513, 1024)]
SPECIALS = (np.nan, np.inf, -np.inf, -0.5, -1.0, -3.7, 3e9, -3e9)
BATCHES = ((0, 1, 2), (3, 4, 5))      # frames of _frames in the two batched calls
ALL_NAN, ALL_ZERO = 1, 3


@functools.lru_cache(maxsize=None)
def _frames(shape):
    """[6][rows][cols] (read-only): four mixed frames -- random values in [0, max_dis + 10), 10 % exact zeros,
    2 % of each special value -- one frame of NaN only and one of zeros only."""
    rows, cols, D = shape
    rng = np.random.default_rng(rows * 7919 + cols * 31 + D)
    d = (rng.random((6, rows, cols), dtype=np.float32) * np.float32(D + 10)).astype(np.float32)
    r = rng.random(d.shape)
    d[r < 0.10] = 0.0
    for k, s in enumerate(SPECIALS):
        d[(r >= 0.10 + 0.02 * k) & (r < 0.12 + 0.02 * k)] = s
    d[ALL_NAN] = np.nan
    d[ALL_ZERO] = 0.0
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _want(shape):
    return [fr.vdisparity(f, shape[2], THR) for f in _frames(shape)]


def _twin_astype(d, D, thr):
    """The numpy twin tests/test_road_batch_gpu.py had before it called the restatement: the bin by astype,
    which is defined for finite |d| < 2^31 only."""
    col = d.astype(np.int32)
    keep = (d != 0) & (col >= 0) & (col < D)
    r = np.nonzero(keep)[0]
    v = np.bincount(r * D + col[keep], minlength=d.shape[0] * D).astype(np.int32).reshape(d.shape[0], D)
    m = int(v.max())
    b = np.where(v.astype(np.float32) > np.float32(m) * np.float32(thr), 255, 0).astype(np.uint8)
    return v, b, m


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


# ---- CPU half ---------------------------------------------------------------------------------------------
def test_restatement_rules_by_hand():
    d = np.array([[0.0, -0.0, np.nan, np.inf, -np.inf, -0.5, -0.999, -1.0, -3.7, 3e9, -3e9, 2.0 ** 31,
                   0.5, 1.0, 1.999, 2.0, 2.5, 3.0, 1e-30, -1e-30]], np.float32)
    bins = fr.vdisparity_bins(d, 3)
    assert bins.tolist() == [[-1, -1, 0, -1, -1, 0, 0, -1, -1, -1, -1, -1, 0, 1, 1, 2, 2, -1, 0, 0]]
    v, b, m = fr.vdisparity(d, 3, 0.5)
    assert v.tolist() == [[6, 2, 2]] and m == 6 and b.tolist() == [[255, 0, 0]]
    v, b, m = fr.vdisparity(np.zeros((2, 5), np.float32), 4, THR)
    assert m == 0 and not v.any() and not b.any()
    v, b, m = fr.vdisparity(np.full((2, 5), np.nan, np.float32), 4, THR)
    assert m == 5 and v.tolist() == [[5, 0, 0, 0]] * 2


def test_restatement_equals_the_twin_it_replaces_and_the_oracle():
    """On the inputs of tests/test_road_batch_gpu.py (no NaN, inf, negative or huge values) the restatement is
    the astype twin, and the oracle where every value lies in the reference's domain."""
    from test_road_batch_gpu import _batch, _oracle_safe, _vdisparity_np
    for rows, cols, D, seed in ((256, 512, 64, 320), (256, 512, 64, 832)):     # its seeds at this shape
        disp, _ = _batch(rows, cols, D, 8, seed=seed)
        assert np.isfinite(disp).all() and (disp >= 0).all() and (disp < 2.0 ** 31).all()
        safe = 0
        for f in disp:
            want = _twin_astype(f, D, THR)
            assert _same(fr.vdisparity(f, D, THR), want)
            assert _same(_vdisparity_np(f, D, THR), want)
            if _oracle_safe(f, D):
                safe += 1
                assert _same(oracle.road_vdisparity(f, D, THR), want)
        assert safe >= 6
    # the edge frames without the values astype is undefined for: the same again, at the ragged shapes
    for shape in SHAPES:
        for f in _frames(shape):
            g = np.where(np.isfinite(f) & (np.abs(f) < 2.0 ** 31), f, np.float32(0.25)).astype(np.float32)
            assert _same(fr.vdisparity(g, shape[2], THR), _twin_astype(g, shape[2], THR))


@pytest.mark.parametrize("shape", SHAPES)
def test_edge_frames_hold_what_they_are_for(shape):
    rows, cols, D = shape
    d = _frames(shape)
    assert np.isnan(d[ALL_NAN]).all() and not d[ALL_ZERO].any()
    want = _want(shape)
    v, b, m = want[ALL_NAN]
    assert m == cols and (v[:, 0] == cols).all() and not v[:, 1:].any()
    v, b, m = want[ALL_ZERO]
    assert m == 0 and not v.any() and not b.any()
    if rows * cols >= 4000:
        mixed = np.delete(d, (ALL_NAN, ALL_ZERO), axis=0)
        for s in SPECIALS:
            assert (np.isnan(mixed) if s != s else mixed == np.float32(s)).any(), s
        assert (mixed == 0).any() and (mixed >= D).any()


# ---- GPU half ---------------------------------------------------------------------------------------------
def _device(a):
    import torch
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))    # (a copy: the frames are read-only)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_both_entries_equal_the_restatement(shape):
    import torch
    from instance_stixels_amd import core
    rows, cols, D = shape
    frames, want = _frames(shape), _want(shape)
    L = core.lib()
    single = []
    for i, f in enumerate(frames):                                   # is_road_vdisparity, frame by frame
        d = _device(f)
        vd, mx, bn = Out((rows, D), np.int32), Out((1,), np.int32), Out((rows, D), np.uint8)
        assert L.is_road_vdisparity(d.data_ptr(), rows, cols, D, ctypes.c_float(THR), vd.ptr, mx.ptr, bn.ptr,
                                    None) == 0, L.is_last_error()
        torch.cuda.synchronize()
        got = (vd.get(), bn.get(), int(mx.get()[0]))
        print(f"{shape} frame {i}: maximum {got[2]} (restatement {want[i][2]}), bin 0 holds {int(got[0][:, 0].sum())}"
              f" (restatement {int(want[i][0][:, 0].sum())})")
        assert np.array_equal(got[0], want[i][0]), i
        assert got[2] == want[i][2], i
        assert np.array_equal(got[1], want[i][1]), i
        single.append(got)
    n = len(BATCHES[0])
    ctx = ctypes.c_void_p()
    assert L.is_road_ctx_create(ctypes.byref(ctx), rows, cols, D, n, -1) == 0, L.is_last_error()
    try:
        for batch in BATCHES:                                        # is_road_vdisparity_batch, three frames
            d = _device(frames[list(batch)])
            vd, mx, bn = Out((n, rows, D), np.int32), Out((n,), np.int32), Out((n, rows, D), np.uint8)
            assert L.is_road_vdisparity_batch(ctx, d.data_ptr(), n, ctypes.c_float(THR), vd.ptr, mx.ptr, bn.ptr,
                                              None) == 0, L.is_last_error()
            torch.cuda.synchronize()
            vd, mx, bn = vd.get(), mx.get(), bn.get()
            for k, i in enumerate(batch):
                assert np.array_equal(vd[k], want[i][0]) and np.array_equal(vd[k], single[i][0]), i
                assert int(mx[k]) == want[i][2] == single[i][2], i
                assert np.array_equal(bn[k], want[i][1]) and np.array_equal(bn[k], single[i][1]), i
    finally:
        assert L.is_road_ctx_destroy(ctx) == 0


TALL = (32768 + 8, 1, 2)    # more rows than the 15 bits the batched point list's (row << 16) | column holds


@pytest.mark.gpu
def test_single_frame_entry_takes_more_rows_than_the_point_list_packs():
    """is_road_vdisparity builds no point list, so the row limit of is_road_ctx_create is not its own: a mixed
    frame of _frames at TALL, with counted pixels in the rows past 32767, exactly against the restatement."""
    import torch
    from instance_stixels_amd import core
    rows, cols, D = TALL
    frame, want = _frames(TALL)[0], _want(TALL)[0]
    assert np.isnan(frame).any() and np.isinf(frame).any() and (frame == 0).any()
    assert want[0][32768:].any() and want[1][32768:].any() and not want[1][32768:].all()
    L = core.lib()
    ctx = ctypes.c_void_p()
    assert L.is_road_ctx_create(ctypes.byref(ctx), rows, cols, D, 1, -1) != 0 and not ctx.value
    d = _device(frame)
    vd, mx, bn = Out((rows, D), np.int32), Out((1,), np.int32), Out((rows, D), np.uint8)
    assert L.is_road_vdisparity(d.data_ptr(), rows, cols, D, ctypes.c_float(THR), vd.ptr, mx.ptr, bn.ptr,
                                None) == 0, L.is_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(vd.get(), want[0])
    assert int(mx.get()[0]) == want[2]
    assert np.array_equal(bn.get(), want[1])
