"""The CNN label maps (f15) without a GPU: the symbols and bindings, the struct layout, the refusals of
is_cnn_label_maps (all made before the device is touched), the host class's refusals, the reference of
tests/cnn_labels_reference.py pinned against torch on the CPU, and evaluation.cnn_scores on a hand-made table."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cnn_labels_reference as cr
from instance_stixels_amd import core, evaluation, host, make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "instance_stixels_core.h")).read()
    assert "is_cnn_label_maps(" in header
    assert "is_cnn_label_maps" in core.EXPORTS and hasattr(core.lib(), "is_cnn_label_maps")
    assert "ish_cnn_label_batch" in host.EXPORTS and hasattr(host.lib(), "ish_cnn_label_batch")
    assert callable(host.Stixels.CnnLabelBatch)
    assert callable(core.cnn_label_maps) and callable(core.cnn_label_maps_ptr) and callable(evaluation.cnn_scores)
    for name, value in (("NEAREST", core.CNN_UP_NEAREST), ("DECONV", core.CNN_UP_DECONV)):
        assert int(re.search(rf"#define IS_CNN_UP_{name}\s+(\d+)", header).group(1)) == value
    for cite in ("run_cityscapes.py:353-365", "train.py:559-605", "DRNSeg.py:35-44", "inference.py:286-292"):
        assert cite in header, cite
    hpp = open(os.path.join(ROOT, "include", "InstanceStixels", "Stixels.hpp")).read()
    assert "struct CnnLabelTargets" in hpp
    assert "void CnnLabelBatch(int n_images, const float* d_cnn_out, int mode" in hpp


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "instance_stixels_core.h"
#define F(f) printf(#f " %zu %zu\n", offsetof(is_cnn_label_args, f), sizeof(((is_cnn_label_args*)0)->f));
int main() {
    printf(". %zu 0\n", sizeof(is_cnn_label_args));
    FIELDS
    return 0;
}
"""


def test_args_layout_matches_the_header(tmp_path):
    src = PROBE.replace("FIELDS", "".join(f"F({n})" for n, _ in core.CnnLabelArgs._fields_))
    (tmp_path / "probe.cpp").write_text(src)
    exe = str(tmp_path / "probe")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "probe.cpp"), "-o", exe],
                   check=True)
    got = {f: (int(off), int(size)) for f, off, size in
           (l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())}
    assert got["."][0] == ctypes.sizeof(core.CnnLabelArgs)
    for name, _ in core.CnnLabelArgs._fields_:
        field = getattr(core.CnnLabelArgs, name)
        assert got[name] == (field.offset, field.size), name


# A call that would be accepted (the pointers are never dereferenced on the host: every case below is refused before
# the device is touched, so this file needs no GPU).
GOOD = dict(d_cnn_out=0x1000, n_images=2, channels=21, n_classes=19, rows8=5, cols8=7, mode=core.CNN_UP_DECONV,
            rows=40, cols=56, d_class8=0x2000, d_label=0x3000, d_gt_label=0x4000, n_labels=34, d_confusion=0x5000)


@pytest.mark.parametrize("change, message", [
    (dict(d_cnn_out=None), "null d_cnn_out"),
    (dict(d_class8=None, d_label=None, d_gt_label=None, d_confusion=None), "no output"),
    (dict(d_gt_label=None), "go together"),
    (dict(d_confusion=None), "go together"),
    (dict(mode=2), "mode"),
    (dict(mode=-1), "mode"),
    (dict(rows=41), "8 \\* rows8"),
    (dict(rows=32), "8 \\* rows8"),
    (dict(cols=55), "8 \\* cols8"),
    (dict(rows8=0, rows=0), "rows8"),
    (dict(cols8=0), "cols8"),
    (dict(n_classes=0), "n_classes"),
    (dict(n_classes=33, channels=40), "IS_HEAD_MAX_CHANNELS"),
    (dict(channels=18), "channels"),
    (dict(n_labels=0), "n_labels"),
    (dict(n_labels=65), "IS_RENDER_MAX_LABELS"),
    (dict(n_images=0), "n_images"),
    (dict(n_images=65536), "n_images"),
    (dict(rows8=8192, rows=65536, cols8=1, cols=32768), "rows \\* cols"),            # 2^31 pixels
    (dict(rows8=1024, rows=8192, cols8=16384, cols=131072, channels=128), "channels \\* rows8 \\* cols8"),  # 2^31
    (dict(d_cnn_out=0x1002), "d_cnn_out must be 4-byte aligned"),
    (dict(d_confusion=0x5004), "d_confusion must be 8-byte aligned"),
    (dict(reserved=(0, 0, 0, 1)), "reserved"),
])
def test_refusals_need_no_device(change, message):
    rc = core.cnn_label_maps_ptr(**dict(GOOD, **change))
    assert rc == -1                                                          # IS_EINVAL
    assert re.search(message, core.lib().is_last_error().decode()), core.lib().is_last_error()


def test_null_args_are_refused():
    assert core.lib().is_cnn_label_maps(None, None) == -1
    assert b"null args" in core.lib().is_last_error()


def test_host_class_refuses_before_initialize():
    cfg = make_config("drn_d_22_unary", 128, 256, 32)
    st = host.Stixels()
    st.SetConfig(cfg)
    with pytest.raises(ValueError, match="not initialised"):
        st.CnnLabelBatch(1, 0x1000, core.CNN_UP_NEAREST, d_label=0x2000)


# ---- the reference against torch ----

def _torch_deconv64(planes):
    """The reference's `up` layer (DRNSeg.py:35-44, 64-79) in float64 on [n][C][Hs][Ws]: ConvTranspose2d(C, C, 16,
    stride=8, padding=4, groups=C) with the bilinear weights W[ky] W[kx]."""
    import torch
    C = planes.shape[1]
    w1 = torch.from_numpy(cr.weights().astype(np.float64))
    w = (w1[:, None] * w1[None, :]).expand(C, 1, 16, 16).contiguous()
    return torch.nn.functional.conv_transpose2d(torch.from_numpy(planes.astype(np.float64)), w, stride=8, padding=4,
                                                groups=C).numpy()


def test_weights_are_the_bilinear_kernel():
    """fill_up_weights' formula for a 16-tap kernel, f = 8, c = 15 / 16: (1 - |k / 8 - c|), squared into 2-D."""
    k = np.arange(16)
    assert np.array_equal(cr.weights().astype(np.float64), 1 - np.abs(k / 8.0 - 15.0 / 16.0))


CASES = [(5, 7, 3.0, 11), (5, 7, 1.0, 12), (13, 9, 3.0, 13), (13, 9, 1.0, 14)]


@pytest.mark.parametrize("Hs, Ws, sigma, seed", CASES)
def test_nearest_mode_is_interpolate_and_argmin(Hs, Ws, sigma, seed):
    import torch
    x = cr.random_costs(2, 21, Hs, Ws, seed, sigma=sigma)
    c8, cls = cr.classes(x, 19, "nearest")
    t = torch.from_numpy(x[:, :19])
    srt = np.sort(x[:, :19], axis=1)
    assert (srt[:, 1] > srt[:, 0]).all()                                     # (no exact ties in these planes)
    up = torch.nn.functional.interpolate(t, scale_factor=8, mode="nearest")
    assert np.array_equal(cls, up.argmin(dim=1).numpy().astype(np.uint8))
    assert np.array_equal(c8, t.argmin(dim=1).numpy().astype(np.uint8))


@pytest.mark.parametrize("Hs, Ws, sigma, seed", CASES)
def test_deconv_mode_stays_within_the_chain_bound_of_conv_transpose2d(Hs, Ws, sigma, seed):
    """Four roundings of at most half an ulp each, of partial sums that sum w |v| bounds: B = 4 * 2^-24 * sum w |v|.
    Where the float64 gap between the best class and the runner-up exceeds 2 B (B the largest of the pixel's
    classes), fp32 cannot change the order, and the labels must be equal."""
    x = cr.random_costs(2, 21, Hs, Ws, seed, sigma=sigma)
    _, cls, up = cr.classes(x, 19, "deconv", want_values=True)
    exact = _torch_deconv64(x[:, :19])
    B = 4 * 2.0 ** -24 * _torch_deconv64(np.abs(x[:, :19]))
    err = np.abs(up.astype(np.float64) - exact)
    print("max err / B", float((err / B).max()), "max err", float(err.max()))
    assert (err <= B).all()
    assert (up.astype(np.float64) != exact).any()                            # (fp32 does round here)
    srt = np.sort(exact, axis=1)
    safe = srt[:, 1] - srt[:, 0] > 2 * B.max(axis=1)
    print("pixels under the gap", int((~safe).sum()), "of", safe.size)
    assert (~safe).sum() <= 0.001 * safe.size
    assert np.array_equal(cls[safe], exact.argmin(axis=1).astype(np.uint8)[safe])


def test_exact_inputs_give_true_ties_and_the_first_class_wins():
    """Planes that are multiples of 1/8 below 32: every product is a multiple of 2^-11 below 2^5 and every partial sum
    one below 2^7 (the weights sum to 1), exact in fp32.  The chain IS the float64 convolution, ties are true ties, and
    numpy's argmin (the first minimum) gives the class everywhere."""
    rng = np.random.default_rng(5)
    x = (rng.integers(0, 256, (2, 19, 6, 5)) / 8.0).astype(np.float32)
    x[0, 7] = x[0, 2]                                                        # two equal planes
    x[1, :, 2, 3] = 4.0                                                      # a cell whose classes are all equal
    for mode in ("nearest", "deconv"):
        c8, cls, up = cr.classes(x, 19, mode, want_values=True)
        exact = _torch_deconv64(x) if mode == "deconv" else np.repeat(np.repeat(x, 8, axis=2), 8, axis=3)
        assert np.array_equal(up.astype(np.float64), exact)
        assert np.array_equal(cls, exact.argmin(axis=1).astype(np.uint8))
        assert np.array_equal(c8, x.argmin(axis=1).astype(np.uint8))
        assert not (cls[0] == 7).any() and c8[1, 2, 3] == 0
        srt = np.sort(exact, axis=1)
        assert (srt[:, 0] == srt[:, 1]).mean() > 0.01                         # (ties do occur)


def test_reference_skips_missing_taps_and_follows_the_nan_rule():
    x = np.full((1, 3, 2, 2), 5.0, np.float32)
    x[0, 1, 0, 0] = np.inf                                                   # a corner cell of class 1
    x[0, 0] = 6.0
    _, cls, up = cr.classes(x, 3, "deconv", want_values=True)
    assert not np.isnan(up).any() and np.isinf(up[0, 1, 0, 0])
    assert cls[0, 0, 0] == 2 and cls[0, 15, 15] == 1                          # 5 (class 1 first) where no inf reaches
    y = np.full((1, 3, 1, 2), np.nan, np.float32)
    y[0, 2, 0, 1] = 1.0
    c8, cls = cr.classes(y, 3, "nearest")
    assert c8.tolist() == [[[0, 0]]] and not cls.any()                       # NaN never replaces; all-NaN gives 0


def test_label_table_and_confusion_reference():
    x = cr.random_costs(1, 19, 2, 3, 1)
    c8, label = cr.label_maps(x, 19, "nearest", cols=30)
    assert label.shape == (1, 16, 30) and not label[:, :, 24:].any()
    assert np.array_equal(label[0, ::8, :24:8], evaluation.CITYSCAPES_TRAINID_TO_LABELID[c8[0]])
    gt = np.full((1, 16, 30), 7, np.uint8)
    gt[0, 0, 0] = 200
    conf = cr.confusion(label, gt, 34, 24)
    assert conf.sum() == 16 * 24 - 1 and conf[7].sum() == conf.sum()
    assert np.array_equal(cr.table(4, [9, 8, 7, 6]), [9, 8, 7, 6]) and cr.table(32)[19:].max() == 0


def test_cnn_scores_on_a_table_equals_cityscapes_iou():
    rng = np.random.default_rng(0)
    conf = rng.integers(0, 1000, (34, 34)).astype(np.uint64)
    got = evaluation.cnn_scores(None, None, confusion=conf)
    iou, mean = evaluation.cityscapes_iou(conf)
    assert np.array_equal(got["iou"], iou, equal_nan=True) and got["mean_iou"] == mean
    assert got["confusion"] is conf
    hand = np.zeros((34, 34), np.uint64)
    hand[7, 7], hand[7, 8], hand[8, 7], hand[0, 7] = 6, 2, 1, 5               # road: tp 6, fn 2, fp 1 (void gt ignored)
    got = evaluation.cnn_scores(None, None, confusion=hand)
    assert got["iou"][0] == 6 / 9 and got["iou"][1] == 0.0 and got["mean_iou"] == (6 / 9) / 2
    with pytest.raises(ValueError):
        evaluation.cnn_scores(None, None)
