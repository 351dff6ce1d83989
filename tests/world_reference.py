"""Plain numpy restatement of the stixel world (is_stixel_world / Stixels::WorldBatch): the records of one
frame from its Sections and its instance mapping, with the fp32 vertices of Stixels::Get3DVertices
(reference Stixels.cu:683-742) -- every operation on float32 arrays, in that function's operand order."""
import numpy as np

from instance_stixels_amd.core import WORLD_DTYPE


def used(sections):
    """(column, section) index arrays of the sections is_pack_sections packs: in front of each column's
    terminator, max_sections - 1 of a column without one."""
    C, S = sections.shape
    term = sections["type"] == -1
    n = np.where(term.any(axis=1), term.argmax(axis=1), S - 1)
    cols = np.repeat(np.arange(C), n)
    idx = np.concatenate([np.arange(k) for k in n]) if C else np.zeros(0, np.int64)
    return cols.astype(np.int64), idx.astype(np.int64)


def vertices(sec, column, rows, column_step, focal, baseline, cx, cy, alpha_ground, vhor):
    """[n][12] float32 for the Sections `sec` [n] of stixel columns `column` [n]."""
    f32 = np.float32
    focal, baseline, cx, cy, alpha = f32(focal), f32(baseline), f32(cx), f32(cy), f32(alpha_ground)
    x_l = (column * int(column_step)).astype(f32)
    x_r = x_l + f32(column_step)
    y_t = (int(rows) - sec["vT"].astype(np.int64) - 1).astype(f32)
    y_b = (int(rows) - sec["vB"].astype(np.int64)).astype(f32)
    bf = baseline * focal
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        obj = bf / sec["disparity"].astype(f32)
        g_top = bf / (alpha * (int(vhor) - sec["vT"].astype(np.int64)).astype(f32))
        g_bot = bf / (alpha * (int(vhor) - sec["vB"].astype(np.int64)).astype(f32))
        zero = np.zeros(len(sec), f32)  # sky stays at depth 0
        top = np.where(sec["type"] == 1, obj, np.where(sec["type"] == 0, g_top, zero)).astype(f32)
        bot = np.where(sec["type"] == 1, obj, np.where(sec["type"] == 0, g_bot, zero)).astype(f32)
        out = np.empty((len(sec), 12), f32)
        for k, (x, y, z) in enumerate(((x_l, y_t, top), (x_r, y_t, top), (x_r, y_b, bot), (x_l, y_b, bot))):
            out[:, 3 * k] = -z / focal * (cx - x)
            out[:, 3 * k + 1] = -z / focal * (cy - y)
            out[:, 3 * k + 2] = z
    return out


def records(sections, mapping, rows, column_step, focal, baseline, cx, cy, alpha_ground, vhor):
    """sections [realcols][max_sections] SECTION_DTYPE, mapping {(column, section): label} or None ->
    WORLD_DTYPE records in (column, section) order."""
    col, idx = used(sections)
    sec = sections[col, idx]
    out = np.zeros(len(sec), WORLD_DTYPE)
    out["column"], out["section"] = col, idx
    for name in ("type", "vB", "vT", "semantic_class", "disparity", "cost", "instance_meanx", "instance_meany"):
        out[name] = sec[name]
    mapping = mapping or {}
    out["instance_id"] = [mapping.get((int(c), int(i)), -1) for c, i in zip(col, idx)]
    out["vertices"] = vertices(sec, col, rows, column_step, focal, baseline, cx, cy, alpha_ground, vhor)
    return out


def records_of(cfg, data, mapping):
    """The records of one host.StixelsData of configuration `cfg`."""
    return records(data.sections, mapping, cfg.rows, cfg.column_step, cfg.focal, cfg.baseline,
                   cfg.camera_center_x, cfg.camera_center_y, data.alpha_ground, data.vhor)


def same_floats(got, want):
    """The vertex rule: identical bits, except that a NaN on one side must be a NaN on the other (any payload)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and
                np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


def assert_records_equal(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.shape, want.shape)
    for name in got.dtype.names:
        if name == "vertices":
            assert same_floats(got[name], want[name]), "vertices differ"
        elif got.dtype[name].kind == "f":
            assert np.array_equal(got[name].view(np.uint32), want[name].view(np.uint32)), name
        else:
            assert np.array_equal(got[name], want[name]), name
