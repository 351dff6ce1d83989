"""f9 without a GPU: the layout of is_instance_object / is_contour_point / is_instance_objects_args as g++ compiles the
header against the numpy dtypes and the ctypes struct, the numpy restatement (tests/objects_reference.py) against the
pinned render restatement (render_reference.render's instance image is what draw_instance_masks masks), on a
hand-built frame and on a frame of tests/golden/reference_python_gt, world.instance_objects on a case worked by hand,
and the refusals that need no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import assign_gt_reference as ag
import objects_reference as orf
import render_reference as rr
from instance_stixels_amd import core, host, world
from instance_stixels_amd.config import SECTION_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_python_gt", "assign_gt_reference_python.npz")


def test_symbols_are_exported():
    assert hasattr(core.lib(), "is_instance_objects") and "is_instance_objects" in core.EXPORTS
    for name in ("ish_instance_objects_batch", "ish_instance_objects_records", "ish_set_instance_object_capacity"):
        assert hasattr(host.lib(), name) and name in host.EXPORTS, name
    assert host.OBJECT_DTYPE is core.OBJECT_DTYPE and host.CONTOUR_DTYPE is core.CONTOUR_DTYPE


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "instance_stixels_core.h"
#define F(S, f) printf(#S " " #f " %zu %zu\n", offsetof(S, f), sizeof(((S*)0)->f));
int main() {
    printf("is_instance_object . %zu 0\n", sizeof(is_instance_object));
    printf("is_contour_point . %zu 0\n", sizeof(is_contour_point));
    printf("is_instance_objects_args . %zu 0\n", sizeof(is_instance_objects_args));
    OBJECT_FIELDS
    POINT_FIELDS
    ARGS_FIELDS
    return 0;
}
"""


def test_struct_sizes_and_offsets(tmp_path):
    """The header as a C++ compiler lays it out against OBJECT_DTYPE, CONTOUR_DTYPE and InstanceObjectsArgs."""
    src = PROBE
    src = src.replace("OBJECT_FIELDS", "".join(f"F(is_instance_object, {n})" for n in core.OBJECT_DTYPE.names))
    src = src.replace("POINT_FIELDS", "".join(f"F(is_contour_point, {n})" for n in core.CONTOUR_DTYPE.names))
    src = src.replace("ARGS_FIELDS", "".join(f"F(is_instance_objects_args, {n})"
                                             for n, _ in core.InstanceObjectsArgs._fields_))
    (tmp_path / "probe.cpp").write_text(src)
    exe = str(tmp_path / "probe")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "probe.cpp"), "-o", exe],
                   check=True)
    lines = [l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    got = {(s, f): (int(off), int(size)) for s, f, off, size in lines}
    assert got[("is_instance_object", ".")][0] == 64 == core.OBJECT_DTYPE.itemsize
    assert got[("is_contour_point", ".")][0] == 32 == core.CONTOUR_DTYPE.itemsize
    assert got[("is_instance_objects_args", ".")][0] == ctypes.sizeof(core.InstanceObjectsArgs)
    for struct, dtype in (("is_instance_object", core.OBJECT_DTYPE), ("is_contour_point", core.CONTOUR_DTYPE)):
        assert len([k for k in got if k[0] == struct]) == len(dtype.names) + 1
        for name in dtype.names:
            assert got[(struct, name)] == (dtype.fields[name][1], dtype.fields[name][0].itemsize), (struct, name)
    for name, _ in core.InstanceObjectsArgs._fields_:
        field = getattr(core.InstanceObjectsArgs, name)
        assert got[("is_instance_objects_args", name)] == (field.offset, field.size), name
    # the four 16-byte chunks of the issue's table
    assert [core.OBJECT_DTYPE.fields[n][1] for n in ("frame", "n_columns", "col_max", "disparity_min")] == [0, 16, 32, 48]
    assert core.OBJECT_DTYPE.fields["disparity_q16_sum"][1] == 56 and core.CONTOUR_DTYPE.fields["vT"][1] == 16


def _check_against_render(secs, inst_map, rows, cols):
    """Every object of the restatement against the instance image of render_reference.render: pixels = the count of
    instance == c*1000 + l, the image box = its bounding box, the member columns = the stixel columns it touches."""
    n, C, S = secs.shape
    w = cols // C
    mappings = [{(c, i): int(inst_map[f, c, i]) for c in range(C) for i in range(S)} for f in range(n)]
    _, _, image, _ = rr.render(secs, rows, cols, instances=mappings)
    obj, pts, frame_objects, frame_points = orf.objects_and_points(secs, inst_map, rows, cols)
    assert frame_objects.sum() == len(obj) and frame_points.sum() == len(pts) == obj["n_columns"].sum()
    ids = set()
    for o in obj:
        value = int(o["semantic_class"]) * 1000 + int(o["label"])
        ids.add((int(o["frame"]), value))
        ys, xs = np.nonzero(image[o["frame"]] == value)
        assert len(ys) == o["pixels"], value
        assert (xs.min(), xs.max(), ys.min(), ys.max()) == (o["col_min"] * w, o["col_max"] * w + w - 1, o["top"],
                                                            o["bottom"]), value
        mine = pts[o["first_point"]:o["first_point"] + o["n_columns"]]
        assert np.array_equal(mine["column"], np.unique(xs // w)) and (mine["object"] == len(ids) - 1).all()
        for p in mine:  # the column's share of the mask, and a member of it
            assert p["column_pixels"] == np.count_nonzero(xs // w == p["column"])
            assert mappings[o["frame"]][(int(p["column"]), int(p["section"]))] == o["label"]
            s = secs[o["frame"], p["column"], p["section"]]
            assert (s["vB"], s["vT"], s["semantic_class"]) == (p["vB"], p["vT"], o["semantic_class"])
            assert s["disparity"] == p["disparity"]
    # and no instance of the image is missing among the objects (the render restatement also paints a labelled
    # section of another class, which no cluster label or vote produces: the instance classes are 11..18)
    for f in range(n):
        assert {(f, int(v)) for v in np.unique(image[f]) if 11000 <= v < 19000} == {k for k in ids if k[0] == f}
    assert list(map(tuple, obj[["frame", "semantic_class", "label"]].tolist())) == sorted(
        map(tuple, obj[["frame", "semantic_class", "label"]].tolist()))
    return obj, pts


def test_restatement_against_render_hand_built():
    """A partition of every column (what is_compute leaves): instance 13/4 over columns 1..3 with two stixels in
    column 2, 13/5 in column 3, a class-10 and a class-19 section with labels, a label of 1000 and one of -1."""
    rows, cols, C, S = 32, 40, 5, 6
    secs = np.zeros((1, C, S), SECTION_DTYPE)
    secs["type"] = -1
    inst = np.full((1, C, S), -1, np.int32)
    cut = [0, 8, 14, 20, 32]
    plan = {0: [(10, 2), (19, 2), (13, 1000), (13, -1)],
            1: [(0, -1), (13, 4), (13, 4), (12, 4)],
            2: [(0, -1), (13, 4), (14, 4), (13, 4)],
            3: [(13, 5), (13, 4), (13, 5), (2, 7)],
            4: [(0, -1), (1, -1), (2, -1), (3, -1)]}
    for c, column in plan.items():
        for i, (cls, l) in enumerate(column):
            secs[0, c, i] = (1, cut[i], cut[i + 1] - 1, 3.0 + c + 0.5 * i, cls, 0, 0, 0)
            inst[0, c, i] = l
    obj, pts = _check_against_render(secs, inst, rows, cols)
    assert [(o["semantic_class"], o["label"]) for o in obj] == [(12, 4), (13, 4), (13, 5), (14, 4)]
    car = obj[1]
    assert (car["n_stixels"], car["n_columns"], car["col_min"], car["col_max"]) == (5, 3, 1, 3)
    assert (car["disparity_min"], car["disparity_max"]) == (4.5, 6.5)
    # column 2 holds sections 1 (d = 5.5) and 3 (d = 6.5) of the car: the larger disparity is the closer one
    assert pts[car["first_point"] + 1]["section"] == 3 and pts[car["first_point"] + 1]["disparity"] == 6.5
    q16 = sum(h * int(d * 65536) for h, d in ((6, 4.5), (6, 5.0), (6, 5.5), (12, 6.5), (6, 6.5)))
    assert car["disparity_q16_sum"] == q16 and car["pixels"] == 8 * (6 + 6 + 6 + 12 + 6)


def test_restatement_against_render_on_a_reference_fixture():
    """Case 0 of the committed ground-truth fixture: the Sections of a real compute call, the map the pinned vote
    gives them.  Cannot pass empty: at least two objects, one of them over two columns or more."""
    g = np.load(GOLDEN)
    raw = g["c0_sections"]
    secs = np.ascontiguousarray(raw).view(SECTION_DTYPE).reshape((1,) + raw.shape[:2])
    gt = g["c0_gt"].astype(np.int32)
    labels, _ = ag.assign(secs, gt[None])
    rows, cols = gt.shape
    obj, pts = _check_against_render(secs, labels.astype(np.int32), rows, cols)
    assert len(obj) >= 2 and (obj["n_columns"] >= 2).any()
    assert (obj["n_stixels"] >= obj["n_columns"]).all() and (obj["reserved"] == 0).all()


def test_world_instance_objects_by_hand():
    """Two objects; every number of the first worked by hand in float64 with compute3d's operand order."""
    rows, cols, realcols = 100, 80, 10   # w = 8
    obj = np.zeros(2, core.OBJECT_DTYPE)
    pts = np.zeros(3, core.CONTOUR_DTYPE)
    obj[0] = (0, 13, 2, 3, 2, 0, 8 * 30, 4, 5, 60, 79, 0, 8.0, 16.0, (20 * 8 + 10 * 16) * 65536)
    obj[1] = (0, 14, 0, 1, 1, 2, 0, 7, 7, 100, -1, 0, 4.0, 4.0, 0)
    pts[0] = (0, 4, 1, 20, 39, 8 * 20, 8.0, 0)     # rows 60..79
    pts[1] = (0, 5, 2, 25, 34, 8 * 10, 16.0, 0)    # rows 65..74
    pts[2] = (1, 7, 0, 200, 150, 0, 4.0, 0)        # an empty rectangle: no pixels
    cam = {"intrinsic": {"fx": 100.0, "fy": 50.0, "u0": 40.0, "v0": 50.0}, "extrinsic": {"baseline": 0.5}}
    out = world.instance_objects(obj, pts, (rows, cols), realcols, cam)
    assert out["mean_disparity"][0] == (20 * 8.0 + 10 * 16.0) / 30 and np.isnan(out["mean_disparity"][1])
    assert out["box"].tolist() == [[32, 60, 47, 79], [56, 100, 63, -1]]
    assert out["contour_offsets"].tolist() == [0, 2, 3]
    # point 0: x = (32 + 39 + 1) / 2 = 36, y = (60 + 79) / 2 = 69.5, z = 100 * 0.5 / 8 = 6.25
    z0, z1 = 100.0 * 0.5 / 8.0, 100.0 * 0.5 / 16.0
    want0 = [-(z0 / 100.0) * (40.0 - 36.0), -(z0 / 50.0) * (50.0 - 69.5), z0]
    want1 = [-(z1 / 100.0) * (40.0 - 44.0), -(z1 / 50.0) * (50.0 - 69.5), z1]
    assert out["contour"][:2].tolist() == [[36.0, 69.5, 8.0], [44.0, 69.5, 16.0]]
    assert out["contour3d"][0].tolist() == want0 and out["contour3d"][1].tolist() == want1
    assert want0 == [-0.25, 2.4375, 6.25]
    d0, d1 = np.sqrt(np.sum(np.square(want0))), np.sqrt(np.sum(np.square(want1)))
    assert out["closest_distance"][0] == min(d0, d1) == d1
    assert out["contour3d"].dtype == np.float64 and out["box"].dtype == np.int64
    # raises where compute3d raises, and on arrays that do not belong together
    bad = pts.copy()
    bad["disparity"][1] = 0.0
    with pytest.raises(ValueError, match="Disparity should not be 0"):
        world.instance_objects(obj, bad, (rows, cols), realcols, cam)
    with pytest.raises(ValueError, match="Camera parameters"):
        world.instance_objects(obj, pts, (rows, cols), realcols, None)
    with pytest.raises(ValueError, match="not those of the objects"):
        world.instance_objects(obj, pts[:2], (rows, cols), realcols, cam)
    with pytest.raises(ValueError, match="realcols"):
        world.instance_objects(obj, pts, (rows, cols), 7, cam)
    empty = world.instance_objects(obj[:0], pts[:0], (rows, cols), realcols, cam)
    assert len(empty["box"]) == 0 and empty["contour_offsets"].tolist() == [0]


def _args(**over):
    """Arguments that pass every check (fake, aligned device addresses: nothing is launched on a refusal)."""
    fields = dict(d_sections=0x10000, d_section_instance=0x20000, n_images=2, realcols=4, max_sections=8, rows=64,
                  cols=32, object_capacity=4, point_capacity=8, d_objects=0x30000, d_points=0x40000,
                  d_frame_objects=0x50000, d_frame_points=0x60000, d_totals=0x70000)
    fields.update(over)
    return core.InstanceObjectsArgs(**fields)


@pytest.mark.parametrize("over, text", [
    (dict(d_sections=0), "null sections"),
    (dict(n_images=0), "n_images"),
    (dict(n_images=70000), "n_images"),
    (dict(rows=0), "rows"),
    (dict(cols=3), "cols"),
    (dict(max_sections=0), "max_sections"),
    (dict(max_sections=40000), "max_sections"),
    (dict(n_images=65535, realcols=40000, cols=40000, max_sections=8), "31 bits"),
    (dict(object_capacity=-1), "capacity"),
    (dict(point_capacity=-1), "capacity"),
    (dict(d_objects=0), "d_objects"),
    (dict(d_points=0), "d_points"),
    (dict(d_totals=0), "null output"),
    (dict(d_frame_objects=0), "null output"),
    (dict(d_sections=0x10008), "16-byte"),
    (dict(d_objects=0x30008), "16-byte"),
    (dict(d_points=0x40004), "16-byte"),
    (dict(d_section_instance=0x20002), "4-byte"),
    (dict(d_totals=0x70001), "4-byte"),
])
def test_argument_refusals_need_no_device(over, text):
    L = core.lib()
    a = _args(**over)
    assert L.is_instance_objects(ctypes.byref(a), None) == -1  # IS_EINVAL
    assert text in L.is_last_error().decode()
    assert L.is_instance_objects(None, None) == -1 and "null" in L.is_last_error().decode()


def test_host_class_refuses_before_any_compute():
    st = host.Stixels()
    with pytest.raises(ValueError, match="there are none"):
        st.InstanceObjectsBatch(1)
    for bad in (0, -3, 8001):
        with pytest.raises(ValueError, match="SetInstanceObjectCapacity"):
            st.SetInstanceObjectCapacity(bad)
    st.SetInstanceObjectCapacity(1)
    st.SetInstanceObjectCapacity(8000)
    st.close()
