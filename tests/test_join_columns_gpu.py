"""k_join_columns / join_one (is_k_frontend.hip) at their edges on the MI355X: is_join_columns against
frontend_reference.join_columns, bit for bit (NaN equals NaN), on the inputs of tests/test_join_columns_cpu.py.
Widths and margins that are no multiple of 4 send some or all groups of a wave through the scalar load path
instead of the two 16-byte loads; the test computes the groups' source addresses itself and says how many took
which."""
import numpy as np
import pytest

import frontend_reference as fr
import helpers
from oracle import oracle
from test_join_columns_cpu import (CASES, D, INVALIDS, N_IMAGES, PRESET, STEP, config, make_input, restatement)
from test_render_gpu import Out

pytestmark = pytest.mark.gpu


def _device_input(big, shift):
    """The input on the device; shift: floats by which the base pointer is moved off its allocation."""
    import torch
    flat = torch.zeros(big.size + shift, dtype=torch.float32, device=torch.device("cuda", 0))
    t = flat[shift:]
    t.copy_(torch.from_numpy(np.array(big)).reshape(-1))             # (a copy: the input is read-only)
    assert t.data_ptr() == flat.data_ptr() + 4 * shift and flat.data_ptr() % 256 == 0
    return flat, t


def _aligned_groups(name, ptr):
    """(aligned, unaligned) groups: join_one takes the two 16-byte loads iff the group's address is a multiple
    of 16."""
    rows, full_cols, margin, realcols = CASES[name]
    img, row, c = np.meshgrid(np.arange(N_IMAGES), np.arange(rows), np.arange(realcols), indexing="ij")
    addr = ptr + 4 * ((img * rows + row) * full_cols + c * STEP + margin)
    aligned = int((addr % 16 == 0).sum())
    return aligned, addr.size - aligned


@pytest.mark.parametrize("invalid", INVALIDS)
@pytest.mark.parametrize("name,shift", [(n, 0) for n in CASES] + [("aligned", 1)])
def test_join_columns_equals_the_restatement(name, shift, invalid):
    import torch
    from instance_stixels_amd.core import Core
    rows, full_cols, margin, realcols = CASES[name]
    big = make_input(name, invalid)
    flat, d_big = _device_input(big, shift)
    aligned, unaligned = _aligned_groups(name, d_big.data_ptr())
    print(f"join {name} shift {shift} invalid {invalid}: {aligned} groups on the 16-byte path, "
          f"{unaligned} on the scalar path")
    if name in ("width67", "margin3", "tiles"):
        assert aligned > 0 and unaligned > 0
    elif name == "aligned":
        assert (aligned == 0) if shift else (unaligned == 0)
    params, lut, odr = oracle.host_initialize(config(name, invalid, False))
    core = Core(params, lut, odr, max_batch=N_IMAGES)
    try:
        for median in (False, True):
            out = Out((N_IMAGES, realcols, rows), np.float32)
            core.join_columns_ptr(d_big.data_ptr(), full_cols, median, out.ptr, N_IMAGES,
                                  torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            got, want = out.get(), restatement(name, invalid, median)
            bad = ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))
            assert fr.same_floats(got, want), (median, int(bad.sum()), np.argwhere(bad)[:5].tolist(),
                                               got[bad][:5], want[bad][:5])
    finally:
        core.close()


def test_unaligned_width_frame_through_the_dp():
    """Case width67 (invalid 0.0, mean, no non-finite or negative values) on through is_compute, unary: the
    Sections of a frame whose groups are mostly unaligned equal the oracle's on the restatement's join."""
    name, invalid = "width67", 0.0
    rows, full_cols, margin, realcols = CASES[name]
    case = helpers.build_case(PRESET, rows, full_cols, D, seed=29, n_images=N_IMAGES, width_margin=margin,
                              invalid_disparity=invalid)
    cfg = case["cfg"]
    assert cfg.realcols == realcols and not cfg.pairwise and not cfg.median_join
    case["disparity"] = np.array(make_input(name, invalid, sprinkle=False))
    want_joined = restatement(name, invalid, False, sprinkle=False)
    assert np.isfinite(want_joined).all() and (want_joined >= 0).all() and (want_joined < D).all()
    got = helpers.run_core(case, want_tables=False)
    for i in range(N_IMAGES):
        ref = helpers.run_oracle(case, image=i, joined=np.array(want_joined[i]))
        errs = helpers.compare(ref, got, i, cfg, check_tables=False)
        assert not errs, (i, errs[:5])
